// C ABI of librevo (include/revo.h), except the gallery and the searches (gallery.hip, search.hip, candidate_search.hip):
// error state, the per-kernel-class profiler, the model handle with its embed forward schedule, and the single-kernel ops.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/revo.h"
#include "api_internal.h"
#include "kernels.h"

// ------------------------------------------------------------ error state --
static thread_local std::string g_err;
void revo_set_error(const std::string& msg) { g_err = msg; }
extern "C" const char* revo_last_error(void) { return g_err.c_str(); }
extern "C" int32_t revo_version(void) { return 100; }

extern "C" int32_t revo_sync(void* stream) {
    REVO_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

// --------------------------------------------------------------- profiler --
namespace {
struct Profiler {
    int on = 0;      // 0 off, 1 every kernel class, 2 only the body GEMMs (gemm_qkv / out / fc1 / fc2), 3 every 4th of those
    unsigned sample[4] = {0, 0, 0, 0};
    std::mutex mu;
    std::vector<ProfRec> recs;
    std::vector<hipEvent_t> pool;
    std::map<std::string, std::pair<long, double>> acc;
    hipEvent_t get() {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e; (void)hipEventCreate(&e); return e;
    }
    void drain() {
        for (auto& r : recs) {
            float ms = 0.f;
            if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
                auto& s = acc[r.cls];
                s.first += 1; s.second += ms;
            }
            pool.push_back(r.a); pool.push_back(r.b);
        }
        recs.clear();
    }
} g_prof;
}  // namespace

ProfScope::ProfScope(const char* cls, hipStream_t s) : active(g_prof.on != 0), st(s) {
    if (active && g_prof.on >= 2) {
        const int which = !strcmp(cls, "gemm_qkv") ? 0 : !strcmp(cls, "gemm_out") ? 1 : !strcmp(cls, "gemm_fc1") ? 2 :
                          !strcmp(cls, "gemm_fc2") ? 3 : -1;
        active = which >= 0;
        // mode 3: every fourth launch of each class (all layers have the same shapes): a quarter of the event cost
        if (active && g_prof.on == 3) active = (g_prof.sample[which]++ & 3) == 0;
    }
    if (!active) return;
    std::lock_guard<std::mutex> lk(g_prof.mu);
    rec.cls = cls; rec.a = g_prof.get(); rec.b = g_prof.get();
    (void)hipEventRecord(rec.a, st);
}
ProfScope::~ProfScope() {
    if (!active) return;
    (void)hipEventRecord(rec.b, st);
    std::lock_guard<std::mutex> lk(g_prof.mu);
    g_prof.recs.push_back(rec);
}

extern "C" int32_t revo_prof_enable(int32_t on) {
    g_prof.on = on < 0 ? 0 : (on > 3 ? 1 : on);
    for (auto& x : g_prof.sample) x = 0;
    return 0;
}
extern "C" int32_t revo_prof_reset(void) {
    std::lock_guard<std::mutex> lk(g_prof.mu);
    g_prof.drain();
    g_prof.acc.clear();
    return 0;
}
extern "C" int32_t revo_prof_report(char* buf, int32_t capacity) {
    std::lock_guard<std::mutex> lk(g_prof.mu);
    g_prof.drain();
    std::string s = "{";
    bool first = true;
    for (auto& kv : g_prof.acc) {
        if (!first) s += ", ";
        first = false;
        s += "\"" + kv.first + "\": {\"launches\": " + std::to_string(kv.second.first) +
             ", \"ms\": " + std::to_string(kv.second.second) + "}";
    }
    s += "}";
    if ((int)s.size() + 1 > capacity) { revo_set_error("prof_report: buffer too small"); return -2; }
    memcpy(buf, s.c_str(), s.size() + 1);
    return 0;
}

// ------------------------------------------------------------- small ops ---
namespace revo {
// q[o] = scale * (bias[o] + sum_i w[o][i] * probe[i])   -- the pool head's query is input independent
__global__ __launch_bounds__(256) void probe_q_kernel(const float* __restrict__ w, const float* __restrict__ bias,
                                                      const float* __restrict__ probe, int W, float scale,
                                                      float* __restrict__ q) {
    const int lane = threadIdx.x & 63;
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= W) return;
    float acc = 0.f;
    for (int i = lane; i < W; i += 64) acc = fmaf(w[(long)o * W + i], probe[i], acc);
    acc = wave_sum(acc);
    if (lane == 0) q[o] = (acc + bias[o]) * scale;
}
}  // namespace revo

// ------------------------------------------------------------ the model ----
// (LayerW, the weight upload helpers, the gemm() wrapper and the block loop that both towers run: api_internal.h)
struct revo_vit {
    revo_vit_cfg cfg;
    int device = 0, max_batch = 0, S = 0, G2 = 0, Kp = 0, hd = 0, phd = 0, PM = 0, debug_layers = -1;
    std::vector<void*> owned;
    // weights
    bf16_t* w_patch = nullptr; float *cls = nullptr, *pos = nullptr, *lnpre_w = nullptr, *lnpre_b = nullptr,
            *lnpost_w = nullptr, *lnpost_b = nullptr;
    std::vector<LayerW> layers;
    // attention-pool head, all fp32 (head.hip): probe query folded into the key projection (qk, ck), value / out / MLP /
    // proj weights as uploaded
    float *q_probe = nullptr, *qk = nullptr, *ck = nullptr, *w_v = nullptr, *b_v = nullptr, *w_po = nullptr, *b_po = nullptr;
    float *pln_w = nullptr, *pln_b = nullptr, *w_pfc1 = nullptr, *b_pfc1 = nullptr, *w_pfc2 = nullptr, *b_pfc2 = nullptr,
          *w_projT = nullptr;
    float2* rope_cs = nullptr;
    // workspace
    bf16_t *patches = nullptr, *h = nullptr, *qkv = nullptr, *att = nullptr, *mlp = nullptr;
    bf16_t* xlo = nullptr;             // low plane of the residual stream while it is kept as (h, xlo) = (bf16(x), bf16(x - hi))
    float *x = nullptr, *pool_logits = nullptr, *pool_u = nullptr, *pool_att = nullptr, *pool_o = nullptr, *pool_h = nullptr,
          *pool_m = nullptr, *feat = nullptr;
    float* splitk_ws = nullptr;        // fp32 partial planes of the split-K residual GEMMs
    float2* ln_stats = nullptr;        // [rows][width / 256] (mean, M2) per 256-column slice: the folded LayerNorm's row statistics
    int ln_parts = 0;                  // width / 256 when the fold applies (width % 256 == 0, <= 6 slices), else 0
    unsigned long long* ln_tele = nullptr;   // [4] telemetry of the folded LayerNorm's consumers (kernels.h GemmArgs::lnc_tele; revo_vit_stats)
    // region head (revo_vit_forward_regions): allocated by the first call with regions, a fixed size whatever n_regions is.
    // REGION_CHUNK rows of the head's buffers; image indices and bitmaps of REGION_STAGE regions on the device, filled
    // through one pinned host buffer (rg_ev: the last copy out of it)
    float *rg_u = nullptr, *rg_att = nullptr, *rg_o = nullptr, *rg_h = nullptr, *rg_m = nullptr, *rg_feat = nullptr;
    int32_t* rg_img = nullptr; uint32_t* rg_bits = nullptr;
    uint32_t* rg_pin = nullptr; hipEvent_t rg_ev = nullptr; bool rg_ev_pending = false;

    template <class T> int dalloc(T** out, size_t count) {
        void* p = nullptr;
        REVO_HIP_CHECK(hipMalloc(&p, count * sizeof(T) + 256));
        owned.push_back(p);
        *out = (T*)p;
        return 0;
    }
    ~revo_vit() {
        for (void* p : owned) (void)hipFree(p);
        if (rg_pin) (void)hipHostFree(rg_pin);
        if (rg_ev) (void)hipEventDestroy(rg_ev);
    }
};

extern "C" int32_t revo_vit_create(const revo_vit_cfg* cfg, const revo_tensor* weights, int32_t n_weights,
                                   int32_t device, int32_t max_batch, revo_vit** out) {
    API_BEGIN
    REVO_REQUIRE(cfg && weights && out, "vit_create: null argument");
    REVO_REQUIRE(max_batch >= 1, "vit_create: max_batch must be >= 1");
    const revo_vit_cfg& c = *cfg;
    REVO_REQUIRE(c.image_size % c.patch_size == 0, "vit_create: image_size must be a multiple of patch_size");
    REVO_REQUIRE(c.width % c.heads == 0 && c.width % c.pool_heads == 0, "vit_create: width must divide into heads");
    REVO_REQUIRE(c.width % 64 == 0 && c.mlp_dim % 64 == 0, "vit_create: width and mlp_dim must be multiples of 64");
    REVO_REQUIRE(c.out_dim % 4 == 0, "vit_create: out_dim must be a multiple of 4");
    REVO_REQUIRE(c.width / c.heads == 64 || c.width / c.heads == 96,
                 "vit_create: body head_dim must be 64 (PE-Core B16 / L14) or 96 (G14)");
    REVO_REQUIRE(c.image_size > 0 && c.patch_size > 0 && c.layers >= 1 && c.heads >= 1 && c.pool_heads >= 1 && n_weights >= 0,
                 "vit_create: sizes must be positive");
    std::unique_ptr<revo_vit> v(new revo_vit());
    v->cfg = c; v->device = device; v->max_batch = max_batch;
#ifdef REVO_EXPERIMENTS
    if (const char* e = getenv("REVO_LN_FOLD")) revo::gemm_set_ln_fold(atoi(e));     // A/B runs of bench.py (scripts/): 0, 1 or 2
#endif
    const int W = c.width, M = c.mlp_dim, D = c.out_dim, P = c.patch_size, G = c.image_size / P;
    v->G2 = G * G; v->S = v->G2 + (c.use_cls ? 1 : 0);
    v->hd = W / c.heads; v->phd = W / c.pool_heads;
    // the pool head's MLP has its own width (upstream AttentionPooling: mlp_ratio 4), not the tower's mlp_dim
    const int PM = c.pool_mlp_dim > 0 ? c.pool_mlp_dim : 4 * W;
    REVO_REQUIRE(PM % 64 == 0, "vit_create: pool_mlp_dim must be a multiple of 64");
    v->PM = PM;
    const int Kreal = 3 * P * P;
    v->Kp = (Kreal + 63) / 64 * 64;
    const int S = v->S;

    // The checkpoint is validated as a whole before the device is touched: every tensor the architecture needs must
    // be present with the right element count (a checkpoint of another variant fails here, by name, not half-way
    // through the upload).
    WeightMap wm;
    for (int i = 0; i < n_weights; ++i) {
        REVO_REQUIRE(weights[i].name && weights[i].data, "vit_create: weight entry with a null name or data pointer");
        wm.m[weights[i].name] = &weights[i];
    }
    {
        std::vector<std::pair<std::string, int64_t>> need = {
            {"visual.conv1.weight", (int64_t)W * Kreal}, {"visual.positional_embedding", (int64_t)S * W},
            {"visual.ln_pre.weight", W}, {"visual.ln_pre.bias", W}, {"visual.ln_post.weight", W}, {"visual.ln_post.bias", W},
            {"visual.attn_pool.probe", W}, {"visual.attn_pool.attn.in_proj_weight", (int64_t)3 * W * W},
            {"visual.attn_pool.attn.in_proj_bias", 3 * W}, {"visual.attn_pool.attn.out_proj.weight", (int64_t)W * W},
            {"visual.attn_pool.attn.out_proj.bias", W}, {"visual.attn_pool.layernorm.weight", W},
            {"visual.attn_pool.layernorm.bias", W}, {"visual.attn_pool.mlp.c_fc.weight", (int64_t)PM * W},
            {"visual.attn_pool.mlp.c_fc.bias", PM}, {"visual.attn_pool.mlp.c_proj.weight", (int64_t)W * PM},
            {"visual.attn_pool.mlp.c_proj.bias", W}, {"visual.proj", (int64_t)W * D}};
        if (c.use_cls) need.push_back({"visual.class_embedding", W});
        for (int i = 0; i < c.layers; ++i) {
            const std::string p = "visual.transformer.resblocks." + std::to_string(i) + ".";
            for (const char* n : {"ln_1.weight", "ln_1.bias", "ln_2.weight", "ln_2.bias", "attn.out_proj.bias", "mlp.c_proj.bias"})
                need.push_back({p + n, W});
            need.push_back({p + "attn.in_proj_weight", (int64_t)3 * W * W});
            need.push_back({p + "attn.in_proj_bias", 3 * W});
            need.push_back({p + "attn.out_proj.weight", (int64_t)W * W});
            need.push_back({p + "mlp.c_fc.weight", (int64_t)M * W});
            need.push_back({p + "mlp.c_fc.bias", M});
            need.push_back({p + "mlp.c_proj.weight", (int64_t)W * M});
            if (c.use_ls) { need.push_back({p + "ls_1.gamma", W}); need.push_back({p + "ls_2.gamma", W}); }
        }
        for (auto& kv : need)
            if (!wm.get(kv.first, kv.second)) return -2;
        // ... and nothing else: a tensor the forward would not read (LayerScale gains handed to a handle created with
        // use_ls = 0, a tensor of another architecture) means a different model, not one to run without it
        if (wm.m.size() != need.size()) {
            std::map<std::string, int64_t> want(need.begin(), need.end());
            for (auto& kv : wm.m)
                if (!want.count(kv.first)) {
                    revo_set_error("unexpected weight tensor: " + kv.first + " (not read by this architecture" +
                                   (c.use_ls ? ")" : "; LayerScale needs cfg.use_ls = 1)"));
                    return -2;
                }
        }
    }
    REVO_ON_DEVICE(device);

    // staging buffer for fp32 -> bf16 conversion: the largest matrix
    size_t stage_elems = (size_t)std::max({(long)3 * W * W, (long)M * W, (long)PM * W, (long)W * Kreal, (long)W * D});
    float* stage = nullptr;
    REVO_HIP_CHECK(hipMalloc((void**)&stage, stage_elems * 4));
    struct StageGuard { float* p; ~StageGuard() { (void)hipFree(p); } } sg{stage};
    float* gb = nullptr;               // gain | shift | bias of the layer being folded
    REVO_HIP_CHECK(hipMalloc((void**)&gb, (size_t)(2 * W + std::max(3 * W, M)) * 4));
    StageGuard sg2{gb};

    const revo_tensor* t;
    if (!(t = wm.get("visual.conv1.weight", (int64_t)W * Kreal))) return -2;
    // split-precision patch embedding: rows ( hi | lo | hi ) of w / 255 (elementwise.hip patchify_kernel)
    CHECK_RC(v->dalloc(&v->w_patch, (size_t)W * 3 * v->Kp));
    REVO_HIP_CHECK(hipMemcpy(stage, t->data, (size_t)W * Kreal * 4, hipMemcpyDefault));
    CHECK_RC(revo::launch_split_hi_lo_hi(stage, W, Kreal, 1.0f / 255.0f, v->w_patch, v->Kp, 0));
    REVO_HIP_CHECK(hipStreamSynchronize(0));
    if (c.use_cls) CHECK_RC(up_f32(v.get(), wm, "visual.class_embedding", W, &v->cls));
    CHECK_RC(up_f32(v.get(), wm, "visual.positional_embedding", (int64_t)S * W, &v->pos));
    CHECK_RC(up_f32(v.get(), wm, "visual.ln_pre.weight", W, &v->lnpre_w));
    CHECK_RC(up_f32(v.get(), wm, "visual.ln_pre.bias", W, &v->lnpre_b));
    CHECK_RC(up_f32(v.get(), wm, "visual.ln_post.weight", W, &v->lnpost_w));
    CHECK_RC(up_f32(v.get(), wm, "visual.ln_post.bias", W, &v->lnpost_b));
    v->layers.resize(c.layers);
    for (int i = 0; i < c.layers; ++i) {
        const std::string p = "visual.transformer.resblocks." + std::to_string(i) + ".";
        LayerW& L = v->layers[i];
        memset(&L, 0, sizeof(L));
        CHECK_RC(up_folded(v.get(), wm, stage, gb, p + "attn.in_proj_weight", p + "attn.in_proj_bias", p + "ln_1", 3 * W, W,
                           &L.w_qkv, &L.c_qkv, &L.b_qkv));
        if (!(t = wm.get(p + "attn.out_proj.weight", (int64_t)W * W))) return -2;
        CHECK_RC(up_bf16(v.get(), stage, t->data, W, W, W, &L.w_o));
        CHECK_RC(up_f32(v.get(), wm, p + "attn.out_proj.bias", W, &L.b_o));
        CHECK_RC(up_folded(v.get(), wm, stage, gb, p + "mlp.c_fc.weight", p + "mlp.c_fc.bias", p + "ln_2", M, W,
                           &L.w_fc1, &L.c_fc1, &L.b_fc1));
        if (!(t = wm.get(p + "mlp.c_proj.weight", (int64_t)W * M))) return -2;
        CHECK_RC(up_bf16(v.get(), stage, t->data, W, M, M, &L.w_fc2));
        CHECK_RC(up_f32(v.get(), wm, p + "mlp.c_proj.bias", W, &L.b_fc2));
        if (c.use_ls) {
            CHECK_RC(up_f32(v.get(), wm, p + "ls_1.gamma", W, &L.ls1));
            CHECK_RC(up_f32(v.get(), wm, p + "ls_2.gamma", W, &L.ls2));
        }
    }
    // attention-pool head: fp32 weights; the probe's query and the key projection folded into qk / ck (head.hip)
    {
        const std::string p = "visual.attn_pool.";
        float *probe = nullptr, *wi = nullptr, *bi = nullptr;
        CHECK_RC(up_f32(v.get(), wm, p + "probe", W, &probe));
        CHECK_RC(up_f32(v.get(), wm, p + "attn.in_proj_weight", (int64_t)3 * W * W, &wi));
        CHECK_RC(up_f32(v.get(), wm, p + "attn.in_proj_bias", 3 * W, &bi));
        CHECK_RC(v->dalloc(&v->q_probe, (size_t)W));
        hipLaunchKernelGGL(revo::probe_q_kernel, dim3((W + 3) / 4), dim3(256), 0, 0, wi, bi, probe, W,
                           1.0f / sqrtf((float)v->phd), v->q_probe);
        REVO_HIP_CHECK(hipGetLastError());
        CHECK_RC(v->dalloc(&v->qk, (size_t)c.pool_heads * W));
        CHECK_RC(v->dalloc(&v->ck, (size_t)c.pool_heads));
        CHECK_RC(revo::launch_probe_qk(v->q_probe, wi + (size_t)W * W, bi + W, W, c.pool_heads, v->qk, v->ck, 0));
        v->w_v = wi + (size_t)2 * W * W;
        v->b_v = bi + 2 * W;
        REVO_HIP_CHECK(hipStreamSynchronize(0));
        CHECK_RC(up_f32(v.get(), wm, p + "attn.out_proj.weight", (int64_t)W * W, &v->w_po));
        CHECK_RC(up_f32(v.get(), wm, p + "attn.out_proj.bias", W, &v->b_po));
        CHECK_RC(up_f32(v.get(), wm, p + "layernorm.weight", W, &v->pln_w));
        CHECK_RC(up_f32(v.get(), wm, p + "layernorm.bias", W, &v->pln_b));
        CHECK_RC(up_f32(v.get(), wm, p + "mlp.c_fc.weight", (int64_t)PM * W, &v->w_pfc1));
        CHECK_RC(up_f32(v.get(), wm, p + "mlp.c_fc.bias", PM, &v->b_pfc1));
        CHECK_RC(up_f32(v.get(), wm, p + "mlp.c_proj.weight", (int64_t)W * PM, &v->w_pfc2));
        CHECK_RC(up_f32(v.get(), wm, p + "mlp.c_proj.bias", W, &v->b_pfc2));
    }
    if (!(t = wm.get("visual.proj", (int64_t)W * D))) return -2;
    CHECK_RC(v->dalloc(&v->w_projT, (size_t)D * W));
    REVO_HIP_CHECK(hipMemcpy(stage, t->data, (size_t)W * D * 4, hipMemcpyDefault));
    CHECK_RC(revo::launch_transpose_f32(stage, W, D, v->w_projT, 0));
    REVO_HIP_CHECK(hipStreamSynchronize(0));

    // 2-D rope table: [S][hd/2] (cos, sin); x-axis pairs first, then y-axis; cls row unrotated
    {
        const int hd = v->hd, d = hd / 2, nf = d / 2;
        std::vector<float2> cs((size_t)S * (hd / 2));
        const int start = c.use_cls ? 1 : 0;
        for (int s = 0; s < S; ++s) {
            for (int pi = 0; pi < hd / 2; ++pi) {
                double ang = 0.0;
                if (!(c.use_cls && s == 0)) {
                    const int g = s - (c.use_cls ? 1 : 0);
                    const int gy = g / G, gx = g % G;
                    const bool xaxis = pi < nf;
                    const int f = xaxis ? pi : pi - nf;
                    const double freq = 1.0 / pow((double)c.rope_theta, (double)(2 * f) / (double)d);
                    ang = (double)((xaxis ? gx : gy) + start) * freq;
                }
                cs[(size_t)s * (hd / 2) + pi] = make_float2((float)cos(ang), (float)sin(ang));
            }
        }
        CHECK_RC(v->dalloc(&v->rope_cs, cs.size()));
        REVO_HIP_CHECK(hipMemcpy(v->rope_cs, cs.data(), cs.size() * sizeof(float2), hipMemcpyHostToDevice));
    }

    // workspace for max_batch images
    const size_t rows = (size_t)max_batch * S, B = (size_t)max_batch;
    CHECK_RC(v->dalloc(&v->patches, (size_t)max_batch * v->G2 * 3 * v->Kp));
    CHECK_RC(v->dalloc(&v->x, rows * W));
    CHECK_RC(v->dalloc(&v->h, rows * W));
    CHECK_RC(v->dalloc(&v->qkv, rows * 3 * W));
    CHECK_RC(v->dalloc(&v->att, rows * W));
    CHECK_RC(v->dalloc(&v->mlp, rows * M));
    CHECK_RC(v->dalloc(&v->pool_logits, B * c.pool_heads * S));
    CHECK_RC(v->dalloc(&v->pool_u, B * c.pool_heads * W));
    CHECK_RC(v->dalloc(&v->pool_att, B * W));
    CHECK_RC(v->dalloc(&v->pool_o, B * W));
    CHECK_RC(v->dalloc(&v->pool_h, B * W));
    CHECK_RC(v->dalloc(&v->pool_m, B * PM));
    CHECK_RC(v->dalloc(&v->feat, B * D));
    CHECK_RC(v->dalloc(&v->splitk_ws, SPLITK_WS_ELEMS));
    v->ln_parts = (W % 256 == 0 && W / 256 <= 6) ? W / 256 : 0;
    if (v->ln_parts) CHECK_RC(v->dalloc(&v->ln_stats, rows * (size_t)v->ln_parts));
    if (v->ln_parts) CHECK_RC(v->dalloc(&v->xlo, rows * W));
    CHECK_RC(v->dalloc(&v->ln_tele, 4));
    REVO_HIP_CHECK(hipMemset(v->ln_tele, 0, 4 * sizeof(unsigned long long)));
    REVO_HIP_CHECK(hipDeviceSynchronize());
    *out = v.release();
    return 0;
    API_END
}

extern "C" int32_t revo_vit_destroy(revo_vit* vit) {
    API_BEGIN
    if (vit) { DeviceGuard dg(vit->device); delete vit; }
    return 0;
    API_END
}
extern "C" int32_t revo_vit_seq_len(const revo_vit* vit) { return vit ? vit->S : -1; }
extern "C" int32_t revo_vit_stats(revo_vit* vit, double* out4, int32_t reset, void* stream) {
    API_BEGIN
    REVO_REQUIRE(vit && out4, "vit_stats: null argument");
    REVO_ON_DEVICE(vit->device);
    unsigned long long c[4] = {0, 0, 0, 0};
    REVO_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    REVO_HIP_CHECK(hipMemcpy(c, vit->ln_tele, sizeof(c), hipMemcpyDeviceToHost));
    if (reset) REVO_HIP_CHECK(hipMemset(vit->ln_tele, 0, sizeof(c)));
    out4[0] = (double)c[0]; out4[1] = (double)c[1]; out4[2] = (double)c[2]; out4[3] = (double)revo::LNC_TELE_RATIO;
    return 0;
    API_END
}
#ifdef REVO_EXPERIMENTS   // parity-test hooks: librevo_exp.so only (include/revo.h)
extern "C" int32_t revo_vit_set_debug_layers(revo_vit* vit, int32_t n) {
    REVO_REQUIRE(vit, "null handle");
    vit->debug_layers = n;
    return 0;
}
extern "C" int32_t revo_vit_read_residual(revo_vit* vit, int32_t batch, float* dst, void* stream) {
    REVO_REQUIRE(vit && dst && batch >= 1 && batch <= vit->max_batch, "read_residual: bad arguments");
    REVO_ON_DEVICE(vit->device);
    REVO_HIP_CHECK(hipMemcpyAsync(dst, vit->x, (size_t)batch * vit->S * vit->cfg.width * 4, hipMemcpyDeviceToDevice,
                                  (hipStream_t)stream));
    return 0;
}

extern "C" int32_t revo_vit_read_tap(revo_vit* vit, int32_t which, int32_t batch, void* dst, void* stream) {
    REVO_REQUIRE(vit && dst && batch >= 1 && batch <= vit->max_batch, "read_tap: bad arguments");
    REVO_ON_DEVICE(vit->device);
    const size_t rows = (size_t)batch * vit->S, W = vit->cfg.width;
    const void* src = nullptr;
    size_t bytes = 0;
    switch (which) {
        case 0: src = vit->x; bytes = rows * W * 4; break;                  // fp32 residual stream
        case 1: src = vit->x; bytes = rows * W * 4; break;                  // fp32 ln_post output (in place in the residual buffer; after a whole forward)
        case 2: src = vit->pool_o; bytes = (size_t)batch * W * 4; break;    // fp32 attention-pool output (after its MLP residual, before proj)
        default: REVO_REQUIRE(false, "read_tap: which must be 0 (residual), 1 (ln_post output) or 2 (pooled)");
    }
    REVO_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}
#endif

// The head behind the pooled rows u [R][pool_heads][W]: value and output projection, the pool's LayerNorm and MLP, proj, L2 --
// for the R images of a forward or for R regions (revo_vit_forward_regions).  A row's result does not depend on R or on
// the other rows (head.hip: the skinny GEMM cuts K the same way whatever M is).
static int pool_head_tail(revo_vit* v, int R, const float* u, float* att, float* o, float* h, float* m, float* feat_ws,
                          float* out, int32_t normalize, hipStream_t st) {
    using namespace revo;
    const revo_vit_cfg& c = v->cfg;
    const int W = c.width, D = c.out_dim, PM = v->PM, PH = c.pool_heads;
    { ProfScope ps("gemm_pool", st);
      // values: head h's output columns from head h's pooled row
      CHECK_RC(launch_gemm_f32_skinny(0, u, (long)PH * W, W, v->phd, v->w_v, W, v->b_v, R, W, W, att, W, st));
      CHECK_RC(launch_gemm_f32_skinny(0, att, W, 0, 0, v->w_po, W, v->b_po, R, W, W, o, W, st)); }
    { ProfScope ps("layernorm", st);
      CHECK_RC(launch_layernorm(o, W, v->pln_w, v->pln_b, c.ln_eps, R, W, h, W, 0, st)); }
    float* feat = normalize ? feat_ws : out;
    { ProfScope ps("gemm_pool", st);
      CHECK_RC(launch_gemm_f32_skinny(1, h, W, 0, 0, v->w_pfc1, W, v->b_pfc1, R, PM, W, m, PM, st));
      CHECK_RC(launch_gemm_f32_skinny(2, m, PM, 0, 0, v->w_pfc2, PM, v->b_pfc2, R, W, PM, o, W, st));
      CHECK_RC(launch_gemm_f32_skinny(0, o, W, 0, 0, v->w_projT, W, nullptr, R, D, W, feat, D, st)); }
    if (normalize) {
        ProfScope ps("l2norm", st);
        CHECK_RC(launch_l2norm_rows(feat_ws, D, out, D, nullptr, 0, R, D, st));
    }
    return 0;
}

// Forward of images [b0, b0 + B) of the call's batch on stream st; every workspace buffer is
// addressed at the rows of those images.
static int vit_forward_range(revo_vit* vv, const void* images_all, int32_t image_dtype, int b0, int B, float* out_all,
                             int32_t normalize, hipStream_t st, bool with_head = true) {
    const revo_vit_cfg& c = vv->cfg;
    const int W = c.width, Md = c.mlp_dim, D = c.out_dim, S = vv->S, PM = vv->PM;
    const int rows = B * S;
    using namespace revo;
    // views of the workspace at this range
    struct View {
        bf16_t *patches, *h, *qkv, *att, *mlp;
        float *x, *pool_logits, *pool_u, *pool_att, *pool_o, *pool_h, *pool_m, *feat;
    } w;
    const size_t r0 = (size_t)b0 * S;
    const int PH = c.pool_heads;
    w.patches = vv->patches + (size_t)b0 * vv->G2 * 3 * vv->Kp;
    w.x = vv->x + r0 * W; w.h = vv->h + r0 * W; w.qkv = vv->qkv + r0 * 3 * W; w.att = vv->att + r0 * W;
    w.mlp = vv->mlp + r0 * Md;
    w.pool_logits = vv->pool_logits + (size_t)b0 * PH * S; w.pool_u = vv->pool_u + (size_t)b0 * PH * W;
    w.pool_att = vv->pool_att + (size_t)b0 * W; w.pool_o = vv->pool_o + (size_t)b0 * W;
    w.pool_h = vv->pool_h + (size_t)b0 * W; w.pool_m = vv->pool_m + (size_t)b0 * PM;
    w.feat = vv->feat + (size_t)b0 * D;
    const size_t img_elems = (size_t)3 * c.image_size * c.image_size;
    const void* images = (const char*)images_all + (size_t)b0 * img_elems * (image_dtype == 1 ? 1 : 4);
    float* out = out_all ? out_all + (size_t)b0 * D : nullptr;
    struct FW {
        // names used by the schedule below: workspace from the view, everything else from the handle
        bf16_t *patches, *h, *qkv, *att, *mlp;
        float *x, *pool_logits, *pool_u, *pool_att, *pool_o, *pool_h, *pool_m, *feat;
        int Kp, G2, hd, phd, debug_layers;
        bf16_t* w_patch; float *pos, *cls, *lnpre_w, *lnpre_b, *lnpost_w, *lnpost_b;
        const std::vector<LayerW>& layers;
        float *qk, *ck, *w_v, *b_v, *w_po, *b_po, *pln_w, *pln_b, *w_pfc1, *b_pfc1, *w_pfc2, *b_pfc2, *w_projT;
        float2* rope_cs;
    } fw{w.patches, w.h, w.qkv, w.att, w.mlp, w.x, w.pool_logits, w.pool_u, w.pool_att, w.pool_o, w.pool_h, w.pool_m, w.feat,
         vv->Kp, vv->G2, vv->hd, vv->phd, vv->debug_layers, vv->w_patch, vv->pos, vv->cls, vv->lnpre_w, vv->lnpre_b,
         vv->lnpost_w, vv->lnpost_b, vv->layers, vv->qk, vv->ck, vv->w_v, vv->b_v, vv->w_po, vv->b_po, vv->pln_w,
         vv->pln_b, vv->w_pfc1, vv->b_pfc1, vv->w_pfc2, vv->b_pfc2, vv->w_projT, vv->rope_cs};
    const FW* v = &fw;

    {   // K1 + K2: patch embed GEMM in split precision (patchify_kernel: the row of a patch holds its values twice --
        // exact integers for u8 images -- or as hi | hi | lo; the weight rows are hi | lo | hi of w / 255), position add, cls row
        const int parts = image_dtype == 1 ? 2 : 3;
        { ProfScope ps("patchify", st);
          CHECK_RC(launch_patchify(images, image_dtype == 1, B, c.image_size, c.patch_size, v->patches, v->Kp, st)); }
        GemmArgs a{};
        a.A = v->patches; a.lda = (long)parts * v->Kp; a.B = v->w_patch; a.ldb = 3l * v->Kp; a.M = B * v->G2; a.N = W;
        a.K = parts * v->Kp;
        a.C = v->x; a.ldc = W; a.pos = v->pos; a.S = S; a.G2 = v->G2; a.cls = c.use_cls ? 1 : 0;
        { ProfScope ps("gemm_patch", st); CHECK_RC(launch_gemm(EPI_PATCH, a, st)); }
        if (c.use_cls) { ProfScope ps("elementwise", st); CHECK_RC(launch_cls_rows(v->x, W, v->cls, v->pos, B, S, W, st)); }
    }
    if (v->debug_layers == -2) return 0;   // parity hook: the embedded tokens (patch embed + position + class token), before ln_pre
    { ProfScope ps("layernorm", st);
      CHECK_RC(launch_layernorm(v->x, W, v->lnpre_w, v->lnpre_b, c.ln_eps, rows, W, v->x, W, 0, st)); }

    // The block loop both towers run (api_internal.h body_blocks).  This tower's two pieces of it: K4 + K5, bias and the 2-D
    // rotary embedding of q and k in the qkv GEMM's epilogue (every tile shape), and attention over all keys
    BodyCtx bc{};
    bc.who = "vit_forward"; bc.layers = &v->layers;
    bc.nl = v->debug_layers < 0 ? c.layers : std::min(v->debug_layers, c.layers);
    bc.W = W; bc.Md = Md; bc.rows = rows; bc.eps = c.ln_eps;
    bc.x = v->x; bc.h = v->h; bc.qkv = v->qkv; bc.att = v->att; bc.mlp = v->mlp;
    bc.xlo = vv->xlo ? vv->xlo + r0 * W : nullptr;
    bc.stats = vv->ln_parts ? vv->ln_stats + r0 * vv->ln_parts : nullptr;
    bc.ln_parts = vv->ln_parts; bc.ln_tele = vv->ln_tele; bc.splitk_ws = vv->splitk_ws;
    CHECK_RC(body_blocks(
        bc, st,
        [&](GemmArgs& a) {
            a.rope_cs = v->rope_cs; a.rope_S = S; a.rope_hd = v->hd; a.rope_cols = 2 * W;
            return (int)EPI_BF16_ROPE;
        },
        [&]() { return launch_attention_ex(v->qkv, 3 * W, v->att, W, B, S, c.heads, v->hd, c.use_cls, st); }));
    if (v->debug_layers >= 0) return 0;   // parity hook: residual stream only

    // ln_post (fp32, in place) -> attention pool -> proj -> normalise: all fp32 (head.hip says why)
    { ProfScope ps("layernorm", st);
      // (the pool's logits come out of the same kernel: the normalised row is in registers there)
      const LnLogits lg{v->qk, v->ck, v->pool_logits, PH, S};
      CHECK_RC(launch_layernorm(v->x, W, v->lnpost_w, v->lnpost_b, c.ln_eps, rows, W, v->x, W, 0, st, &lg)); }
    if (!with_head) return 0;             // revo_vit_forward_regions without out_global: the rows and the logits are all it needs
    { ProfScope ps("pool_attention", st);
      CHECK_RC(launch_pool_head_rows(v->x, W, B, S, W, PH, v->pool_logits, v->pool_u, st)); }
    CHECK_RC(pool_head_tail(vv, B, v->pool_u, v->pool_att, v->pool_o, v->pool_h, v->pool_m, v->feat, out, normalize, st));
    return 0;
}

extern "C" int32_t revo_vit_forward(revo_vit* v, const void* images, int32_t image_dtype, int32_t batch, float* out,
                                    int32_t normalize, void* stream) {
    API_BEGIN
    REVO_REQUIRE(v && images && out, "vit_forward: null argument");
    REVO_REQUIRE(batch >= 1 && batch <= v->max_batch, "vit_forward: batch exceeds max_batch of the handle");
    REVO_REQUIRE(image_dtype == 0 || image_dtype == 1, "vit_forward: image_dtype must be 0 (f32) or 1 (u8)");
    REVO_ON_DEVICE(v->device);
    hipStream_t st = (hipStream_t)stream;
    return vit_forward_range(v, images, image_dtype, 0, batch, out, normalize, st);
    API_END
}

// ------------------------------------------------------- region embeddings ----
constexpr int REGION_CHUNK = 512;      // regions per pass of the head (its buffers: 16 MiB of pooled rows for L14)
constexpr int REGION_STAGE = 4096;     // regions whose image indices and bitmaps are on the device at a time

static int region_workspace(revo_vit* v) {
    if (v->rg_u) return 0;
    const revo_vit_cfg& c = v->cfg;
    const size_t W = c.width, R = REGION_CHUNK, words = ((size_t)v->S + 31) / 32;
    CHECK_RC(v->dalloc(&v->rg_img, (size_t)REGION_STAGE));
    CHECK_RC(v->dalloc(&v->rg_bits, (size_t)REGION_STAGE * words));
    CHECK_RC(v->dalloc(&v->rg_att, R * W));
    CHECK_RC(v->dalloc(&v->rg_o, R * W));
    CHECK_RC(v->dalloc(&v->rg_h, R * W));
    CHECK_RC(v->dalloc(&v->rg_m, R * (size_t)v->PM));
    CHECK_RC(v->dalloc(&v->rg_feat, R * (size_t)c.out_dim));
    REVO_HIP_CHECK(hipHostMalloc((void**)&v->rg_pin, (size_t)REGION_STAGE * (1 + words) * 4, hipHostMallocDefault));
    REVO_HIP_CHECK(hipEventCreateWithFlags(&v->rg_ev, hipEventDisableTiming));
    CHECK_RC(v->dalloc(&v->rg_u, R * (size_t)c.pool_heads * W));      // last: marks the workspace complete
    return 0;
}

extern "C" int32_t revo_vit_forward_regions(revo_vit* v, const void* images, int32_t image_dtype, int32_t batch,
                                            const int32_t* region_image, const uint32_t* region_bits, int32_t bits_on_device,
                                            int32_t n_regions, float* out_global, float* out_regions, int32_t normalize,
                                            void* stream) {
    API_BEGIN
    // everything that can be refused is refused before the device is touched
    REVO_REQUIRE(batch >= 0 && n_regions >= 0, "vit_forward_regions: negative batch or region count");
    REVO_REQUIRE(n_regions == 0 || (region_image && region_bits && out_regions),
                 "vit_forward_regions: null region_image, region_bits or out_regions with n_regions > 0");
    for (int32_t r = 0; r < n_regions; ++r)
        if (region_image[r] < 0 || region_image[r] >= batch) {
            revo_set_error("requirement failed: vit_forward_regions: region " + std::to_string(r) + " names image " +
                           std::to_string(region_image[r]) + ", outside [0, batch = " + std::to_string(batch) + ")");
            return -2;
        }
    REVO_REQUIRE(v && images, "vit_forward_regions: null handle or images");
    REVO_REQUIRE(out_global || n_regions > 0, "vit_forward_regions: null out_global with no regions: nothing to compute");
    REVO_REQUIRE(batch >= 1 && batch <= v->max_batch, "vit_forward_regions: batch exceeds max_batch of the handle");
    REVO_REQUIRE(image_dtype == 0 || image_dtype == 1, "vit_forward_regions: image_dtype must be 0 (f32) or 1 (u8)");
    REVO_ON_DEVICE(v->device);
    hipStream_t st = (hipStream_t)stream;
    using namespace revo;
    if (n_regions > 0) CHECK_RC(region_workspace(v));
    // one body forward; the global head exactly as revo_vit_forward runs it, or none
    CHECK_RC(vit_forward_range(v, images, image_dtype, 0, batch, out_global, normalize, st, out_global != nullptr));
    if (n_regions == 0 || v->debug_layers != -1) return 0;
    const revo_vit_cfg& c = v->cfg;
    const int W = c.width, D = c.out_dim, S = v->S, PH = c.pool_heads;
    const size_t words = ((size_t)S + 31) / 32;
    for (int64_t s0 = 0; s0 < n_regions; s0 += REGION_STAGE) {
        const int ns = (int)std::min<int64_t>(REGION_STAGE, n_regions - s0);
        // image indices (and host bitmaps) go through the pinned buffer: the caller's arrays are read before the call returns
        if (v->rg_ev_pending) REVO_HIP_CHECK(hipEventSynchronize(v->rg_ev));     // the previous copy out of it
        memcpy(v->rg_pin, region_image + s0, (size_t)ns * 4);
        REVO_HIP_CHECK(hipMemcpyAsync(v->rg_img, v->rg_pin, (size_t)ns * 4, hipMemcpyHostToDevice, st));
        const uint32_t* bits = region_bits + (size_t)s0 * words;
        if (!bits_on_device) {
            memcpy(v->rg_pin + REGION_STAGE, bits, (size_t)ns * words * 4);
            REVO_HIP_CHECK(hipMemcpyAsync(v->rg_bits, v->rg_pin + REGION_STAGE, (size_t)ns * words * 4, hipMemcpyHostToDevice, st));
            bits = v->rg_bits;
        }
        REVO_HIP_CHECK(hipEventRecord(v->rg_ev, st));
        v->rg_ev_pending = true;
        for (int r0 = 0; r0 < ns; r0 += REGION_CHUNK) {
            const int R = std::min(REGION_CHUNK, ns - r0);
            const uint32_t* cb = bits + (size_t)r0 * words;
            float* out = out_regions + (size_t)(s0 + r0) * D;
            { ProfScope ps("pool_regions", st);
              CHECK_RC(launch_pool_head_rows_masked(v->x, W, batch, S, W, PH, v->pool_logits, v->rg_img + r0, cb, R, v->rg_u, st)); }
            CHECK_RC(pool_head_tail(v, R, v->rg_u, v->rg_att, v->rg_o, v->rg_h, v->rg_m, v->rg_feat, out, normalize, st));
            { ProfScope ps("pool_regions", st);
              CHECK_RC(launch_zero_empty_regions(cb, R, S, D, out, st)); }
        }
    }
    return 0;
    API_END
}

// ------------------------------------------------------- single kernels ----
extern "C" int32_t revo_op_gemm(int32_t epi, const void* a, int64_t lda, const void* b, int64_t ldb, int32_t m,
                                int32_t n, int32_t k, void* c, int64_t ldc, const float* bias, const float* gamma,
                                void* stream) {
    API_BEGIN
    REVO_REQUIRE(epi >= 0 && epi <= 3, "op_gemm: epilogue must be 0..3");
    // the residual epilogue may cut the K range of its last, partly filled round of tiles (split-K tail): give it
    // the scratch the ViT forward would, for the duration of this call (stream-ordered allocation: nothing is kept
    // by the library between calls, nothing waits)
    constexpr long OP_WS_ELEMS = 16l << 20;
    hipStream_t st = (hipStream_t)stream;
    float* ws = nullptr;
    if (epi == revo::EPI_RESID_F32) REVO_HIP_CHECK(hipMallocAsync((void**)&ws, OP_WS_ELEMS * 4, st));
    const int rc = gemm("gemm_op", epi, (const bf16_t*)a, lda, (const bf16_t*)b, ldb, m, n, k, c, ldc, bias, gamma, st, ws,
                        ws ? OP_WS_ELEMS : 0);
    if (ws) REVO_HIP_CHECK(hipFreeAsync(ws, st));
    return rc;
    API_END
}
// The two halves of a LayerNorm folded into the GEMMs around it (kernels.h GemmArgs::lnf_* / lnc_*), one kernel each
extern "C" int32_t revo_op_gemm_resid_ln(const void* a, int64_t lda, const void* b, int64_t ldb, int32_t m, int32_t n, int32_t k,
                                         float* c, int64_t ldc, const float* bias, const float* gamma, void* xb, int64_t ldxb,
                                         void* stats, int32_t* done, void* xlo, int32_t x_in_planes, int32_t planes_out,
                                         void* stream) {
    API_BEGIN
    REVO_REQUIRE(a && b && c && xb && done, "op_gemm_resid_ln: null argument");
    REVO_REQUIRE(stats || (xlo && x_in_planes && !planes_out), "op_gemm_resid_ln: stats may be NULL only for planes in, fp32 out");
    REVO_REQUIRE(xlo || (!x_in_planes && !planes_out), "op_gemm_resid_ln: planes need the low plane");
    constexpr long OP_WS_ELEMS = 16l << 20;
    hipStream_t st = (hipStream_t)stream;
    float* ws = nullptr;
    REVO_HIP_CHECK(hipMallocAsync((void**)&ws, OP_WS_ELEMS * 4, st));
    revo::GemmArgs g{};
    g.A = (const bf16_t*)a; g.lda = lda; g.B = (const bf16_t*)b; g.ldb = ldb; g.M = m; g.N = n; g.K = k; g.C = c; g.ldc = ldc;
    g.bias = bias; g.gamma = gamma; g.ws = ws; g.ws_elems = OP_WS_ELEMS;
    int flag = 0;
    if (stats) { g.lnf_xb = (bf16_t*)xb; g.lnf_ldxb = ldxb; g.lnf_stats = (float2*)stats; g.lnf_done = &flag; }
    if (xlo) { g.xp_hi = (bf16_t*)xb; g.xp_lo = (bf16_t*)xlo; g.xp_ld = ldxb; g.xp_in = x_in_planes != 0; g.xp_out = planes_out != 0; }
    const int rc = revo::launch_gemm(revo::EPI_RESID_F32, g, st);
    REVO_HIP_CHECK(hipFreeAsync(ws, st));
    *done = flag;
    return rc;
    API_END
}
extern "C" int32_t revo_op_gemm_ln_in(int32_t epi, const void* a, int64_t lda, const void* b, int64_t ldb, int32_t m, int32_t n,
                                      int32_t k, void* c, int64_t ldc, const float* bias, const float* csum, const void* stats,
                                      int32_t parts, float eps, void* tele, void* stream) {
    API_BEGIN
    REVO_REQUIRE(epi == revo::EPI_BF16 || epi == revo::EPI_BF16_GELU, "op_gemm_ln_in: epilogue must be 0 (bf16) or 1 (bf16 + GELU)");
    REVO_REQUIRE(a && b && c && csum && stats, "op_gemm_ln_in: null argument");
    revo::GemmArgs g{};
    g.A = (const bf16_t*)a; g.lda = lda; g.B = (const bf16_t*)b; g.ldb = ldb; g.M = m; g.N = n; g.K = k; g.C = c; g.ldc = ldc;
    g.bias = bias; g.lnc_stats = (const float2*)stats; g.lnc_parts = parts; g.lnc_c = csum; g.lnc_eps = eps;
    g.lnc_tele = (unsigned long long*)tele;
    return revo::launch_gemm(epi, g, (hipStream_t)stream);
    API_END
}
extern "C" int32_t revo_op_gemm_rope(const void* a, int64_t lda, const void* b, int64_t ldb, int32_t m, int32_t n,
                                     int32_t k, void* c, int64_t ldc, const float* bias, const float* cos_sin,
                                     int32_t seq, int32_t head_dim, int32_t rope_cols, void* stream) {
    API_BEGIN
    revo::GemmArgs g{};
    g.A = (const bf16_t*)a; g.lda = lda; g.B = (const bf16_t*)b; g.ldb = ldb; g.M = m; g.N = n; g.K = k; g.C = c; g.ldc = ldc;
    g.bias = bias; g.rope_cs = (const float2*)cos_sin; g.rope_S = seq; g.rope_hd = head_dim; g.rope_cols = rope_cols;
    return revo::launch_gemm(revo::EPI_BF16_ROPE, g, (hipStream_t)stream);
    API_END
}
// The qkv launch of a batch-sized forward: the folded LayerNorm's consumer and the fused RoPE in one epilogue (vit_forward_range)
extern "C" int32_t revo_op_gemm_ln_in_rope(const void* a, int64_t lda, const void* b, int64_t ldb, int32_t m, int32_t n, int32_t k,
                                           void* c, int64_t ldc, const float* bias, const float* csum, const void* stats,
                                           int32_t parts, float eps, const float* cos_sin, int32_t seq, int32_t head_dim,
                                           int32_t rope_cols, void* stream) {
    API_BEGIN
    REVO_REQUIRE(a && b && c && csum && stats && cos_sin, "op_gemm_ln_in_rope: null argument");
    revo::GemmArgs g{};
    g.A = (const bf16_t*)a; g.lda = lda; g.B = (const bf16_t*)b; g.ldb = ldb; g.M = m; g.N = n; g.K = k; g.C = c; g.ldc = ldc;
    g.bias = bias; g.rope_cs = (const float2*)cos_sin; g.rope_S = seq; g.rope_hd = head_dim; g.rope_cols = rope_cols;
    g.lnc_stats = (const float2*)stats; g.lnc_parts = parts; g.lnc_c = csum; g.lnc_eps = eps;
    return revo::launch_gemm(revo::EPI_BF16_ROPE, g, (hipStream_t)stream);
    API_END
}
// A residual GEMM with the LayerNorm behind it offered to the launcher the way a one-image forward offers it (gemm() with an
// LnAfter of `fused` only): the split-K form with the LayerNorm in its reduce normalises the new rows into ln_out (no affine)
extern "C" int32_t revo_op_gemm_resid_norm(const void* a, int64_t lda, const void* b, int64_t ldb, int32_t m, int32_t n, int32_t k,
                                           float* c, int64_t ldc, const float* bias, const float* gamma, void* ln_out,
                                           int64_t ln_ldo, float eps, int32_t* fused, void* stream) {
    API_BEGIN
    REVO_REQUIRE(a && b && c && ln_out && fused, "op_gemm_resid_norm: null argument");
    constexpr long OP_WS_ELEMS = 16l << 20;
    hipStream_t st = (hipStream_t)stream;
    float* ws = nullptr;
    REVO_HIP_CHECK(hipMallocAsync((void**)&ws, OP_WS_ELEMS * 4, st));
    int flag = 0;
    const LnAfter ln{eps, (bf16_t*)ln_out, ln_ldo, &flag, nullptr, nullptr, nullptr, 0, 0};
    const int rc = gemm("gemm_op", revo::EPI_RESID_F32, (const bf16_t*)a, lda, (const bf16_t*)b, ldb, m, n, k, c, ldc, bias, gamma,
                        st, ws, OP_WS_ELEMS, &ln);
    REVO_HIP_CHECK(hipFreeAsync(ws, st));
    *fused = flag;
    return rc;
    API_END
}
#ifdef REVO_EXPERIMENTS
// result-preserving kernel-variant switches (librevo_exp.so only; see revo.h)
extern "C" int32_t revo_op_set_variant(int32_t flags) {
    revo::gemm_force_gy((flags >> 4) & 15);
    revo::attention_force_nw((flags >> 8) & 15);
    revo::gemm_set_tail_split(((flags >> 12) & 1) ? 0 : 1);
    revo::gemm_set_persistent(((flags >> 16) & 1) ? 0 : 1);
    revo::gemm_set_splitk(((flags >> 17) & 1) ? 0 : 1);
    revo::gemm_set_min_tiles256(((flags >> 18) & 1) ? 0 : 100);
    revo::gemm_set_ring(((flags >> 19) & 1) ? 0 : 1, 0);
    revo::gemm_set_rows192(((flags >> 3) & 1) ? 0 : 1);
    revo::attention_set_shape16((flags >> 20) & 1);
    return 0;
}
// 0: every ln_1 / ln_2 runs as its own LayerNorm kernel (A/B timing and parity of the folded form against it); 1: default
extern "C" int32_t revo_op_set_ln_fold(int32_t on) {
    REVO_REQUIRE(on >= 0 && on <= 2, "set_ln_fold: 0 (LayerNorm kernels), 1 (folded, stream in planes: default) or 2 (folded, fp32 stream + bf16 copy)");
    revo::gemm_set_ln_fold(on);
    return 0;
}
// 0: the bf16 epilogues on gemm256p_kernel (a tile's stores drained before the next main loop: the round-5 kernels); 1: default,
// gemm256q_kernel (stores left in flight through the next tile's first K-tile).  Same results either way.
extern "C" int32_t revo_op_set_qstores(int32_t on) {
    revo::gemm_set_qstores(on);          // (2: queued, stores dropped -- timing experiment, WRONG RESULTS)
    return 0;
}
// phase groups of the persistent 256 x 256 GEMM (gemm.hip gemm256pp_kernel): 0 = the launcher's choice, 1 = off, 2..4 forced
extern "C" int32_t revo_op_set_phase_groups(int32_t groups) {
    REVO_REQUIRE(groups >= 0 && groups <= 4, "set_phase_groups: 0 (heuristic), 1 (off) or 2..4");
    revo::gemm_set_phase_groups(groups);
    return 0;
}
// diagnostic: device array [workgroups][2] of u64 the body attention kernel fills with (shader-clock ticks, 100 MHz ticks) per workgroup
extern "C" int32_t revo_debug_attention_clock(void* buf) {
    revo::attention_set_clock_buffer((unsigned long long*)buf);
    return 0;
}
// diagnostic: buf = device array [workgroups][items][4] of u64 (100 MHz stamps: main loop begin, main loop end, epilogue
// issued, rows of the piece) that the phased persistent kernel fills for its first `items` pieces; NULL = off
extern "C" int32_t revo_debug_gemm_stamps(void* buf, int32_t items) {
    revo::gemm_set_stamps((unsigned long long*)buf, buf ? items : 0);
    return 0;
}
// the GEMM launch forms issued since the last reset (kernels.h GemmForm bits); reset != 0 clears the record
extern "C" int32_t revo_debug_gemm_forms(int32_t reset) { return (int32_t)revo::gemm_debug_forms(reset); }
extern "C" int32_t revo_op_set_gemm_tile(int32_t tile) {
    REVO_REQUIRE(tile == 0 || tile == 128 || tile == 256, "set_gemm_tile: 0, 128 or 256");
    revo::gemm_force_tile(tile);
    return 0;
}
// timing experiments (librevo_exp.so only): the variant bits plus the switches that skip work
extern "C" int32_t revo_op_set_gemm_debug(int32_t flags) {
    revo::gemm_set_debug(flags & 3);
    revo::gemm_set_stagger(((flags >> 28) & 15) * 200, 2 + ((flags >> 2) & 3));   // bits 28-31: stagger in 2 us steps (100 MHz clock), bits 2-3: groups - 2
    revo::topk_scan256_set_debug(((flags >> 13) & 7) | (((flags >> 20) & 255) << 3));
    return revo_op_set_variant(flags);
}
// the scan launch's phases for Q queries over `rows` scanned rows: host logic only, no device needed (CPU-tier tests)
extern "C" int64_t revo_debug_scan_plan(int32_t Q, int64_t rows, int64_t* out, int32_t cap) {
    if (Q < 1 || rows < 1 || !out || cap < 2) return -1;
    return (int64_t)revo::topk_scan256_plan_dump(Q, (long)rows, (long*)out, cap);
}
// the plan launch_gemm would execute for a problem under the library's current switches: host logic only, no device needed
// (CPU-tier tests; kernels.h gemm_debug_plan has the layout of `out`)
extern "C" int64_t revo_debug_gemm_plan(int32_t epi, int32_t m, int32_t n, int32_t k, int64_t lda, int64_t ldb, int64_t ldc,
                                        int64_t ws_elems, int32_t offers, int32_t rope_seq, int32_t rope_head_dim, int32_t rope_cols,
                                        int64_t* out, int32_t cap) {
    if (epi < 0 || epi > 5 || !out) return -2;
    return (int64_t)revo::gemm_debug_plan(epi, m, n, k, (long)lda, (long)ldb, (long)ldc, (long)ws_elems, (unsigned)offers, rope_seq,
                                          rope_head_dim, rope_cols, (long*)out, cap);
}
// whether the forward keeps the residual stream in planes for this many rows of this tower (reporting / tests)
extern "C" int32_t revo_debug_stream_in_planes(const revo_vit* v, int32_t batch) {
    if (!v || !v->xlo) return 0;
    const int W = v->cfg.width, Md = v->cfg.mlp_dim, rows = batch * v->S;
    return revo::gemm_ln_planes_enabled() && revo::gemm_resid_folds(rows, W, W, W, W, W) && revo::gemm_resid_folds(rows, W, Md, Md, Md, W);
}
#endif
extern "C" int32_t revo_op_layernorm(const float* x, int64_t ldx, const float* w, const float* b, float eps,
                                     int32_t rows, int32_t width, void* out, int64_t ldo, int32_t out_is_bf16,
                                     void* stream) {
    API_BEGIN
    return revo::launch_layernorm(x, ldx, w, b, eps, rows, width, out, ldo, out_is_bf16, (hipStream_t)stream);
    API_END
}
extern "C" int32_t revo_op_layernorm_logits(const float* x, int64_t ldx, const float* w, const float* b, float eps, int32_t rows,
                                            int32_t width, float* out, int64_t ldo, const float* qk, const float* ck,
                                            int32_t heads, int32_t seq, float* logits, void* stream) {
    API_BEGIN
    REVO_REQUIRE(x && out && qk && ck && logits && rows >= 1 && seq >= 1 && rows % seq == 0, "op_layernorm_logits: bad arguments");
    const revo::LnLogits lg{qk, ck, logits, heads, seq};
    return revo::launch_layernorm(x, ldx, w, b, eps, rows, width, out, ldo, 0, (hipStream_t)stream, &lg);
    API_END
}
extern "C" int32_t revo_op_linear_f32(int32_t epi, const float* A, int64_t lda, const float* Wt, int64_t ldw, const float* bias,
                                      int32_t M, int32_t N, int32_t K, float* C, int64_t ldc, void* stream) {
    API_BEGIN
    REVO_REQUIRE(A && Wt && C && M >= 1 && N >= 1 && K >= 16 && lda >= K && ldw >= K && ldc >= N, "op_linear_f32: bad arguments");
    return revo::launch_gemm_f32_skinny(epi, A, lda, 0, 0, Wt, ldw, bias, M, N, K, C, ldc, (hipStream_t)stream);
    API_END
}
extern "C" int32_t revo_op_pool_rows(const float* x, int64_t ldx, const float* logits, int32_t batch, int32_t seq, int32_t width,
                                     int32_t heads, float* u, void* stream) {
    API_BEGIN
    REVO_REQUIRE(x && logits && u && batch >= 1 && seq >= 1 && width >= 4 && ldx >= width, "op_pool_rows: bad arguments");
    return revo::launch_pool_head_rows(x, ldx, batch, seq, width, heads, logits, u, (hipStream_t)stream);
    API_END
}
extern "C" int32_t revo_op_pool_rows_masked(const float* x, int64_t ldx, const float* logits, const int32_t* region_image,
                                            const uint32_t* region_bits, int32_t n_regions, int32_t batch, int32_t seq,
                                            int32_t width, int32_t heads, float* u, void* stream) {
    API_BEGIN
    REVO_REQUIRE(n_regions >= 0 && batch >= 1 && seq >= 1 && width >= 4 && heads >= 1 && ldx >= width,
                 "op_pool_rows_masked: sizes must be positive, ldx at least width");
    REVO_REQUIRE(n_regions == 0 || (x && logits && region_image && region_bits && u), "op_pool_rows_masked: null argument");
    for (int32_t r0 = 0; r0 < n_regions; r0 += 32768) {
        const int R = std::min(32768, n_regions - r0);
        CHECK_RC(revo::launch_pool_head_rows_masked(x, ldx, batch, seq, width, heads, logits, region_image + r0,
                                                    region_bits + (size_t)r0 * (((size_t)seq + 31) / 32), R,
                                                    u + (size_t)r0 * heads * width, (hipStream_t)stream));
    }
    return 0;
    API_END
}

extern "C" int32_t revo_op_rope(void* qkv, int64_t ld, const float* cs, int32_t rows, int32_t seq, int32_t width,
                                int32_t heads, void* stream) {
    API_BEGIN
    return revo::launch_rope((bf16_t*)qkv, ld, (const float2*)cs, rows, seq, width, heads, (hipStream_t)stream);
    API_END
}
extern "C" int32_t revo_op_attention(const void* qkv, int64_t ld, void* out, int64_t ldo, int32_t batch, int32_t seq,
                                     int32_t heads, int32_t head_dim, void* stream) {
    API_BEGIN
    ProfScope ps("attention", (hipStream_t)stream);
    return revo::launch_attention((const bf16_t*)qkv, ld, (bf16_t*)out, ldo, batch, seq, heads, head_dim,
                                  (hipStream_t)stream);
    API_END
}
extern "C" int32_t revo_op_f32_to_bf16(const float* src, int64_t ld_src, void* dst, int64_t ld_dst, int64_t rows,
                                       int32_t cols, void* stream) {
    API_BEGIN
    return revo::launch_f32_to_bf16(src, ld_src, (bf16_t*)dst, ld_dst, rows, cols, (hipStream_t)stream);
    API_END
}
