// The image tower of the C ABI (include/revo.h): its handle, the embed forward schedule, the region embeddings, the dense token
// vectors and the text-prompted regions built on them (kernels: detect.hip).  The blocks
// are tower.h body_blocks with the 2-D rotary embedding in the qkv epilogue and attention over all keys; the head (ln_post,
// attention pool, proj, normalisation) is fp32 (head.hip says why).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/revo.h"
#include "kernels.h"
#include "tower.h"

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
// (the blocks' weights, the body workspace, the allocations and their release: tower.h TowerCore)
struct revo_vit : TowerCore {
    revo_vit_cfg cfg;
    int S = 0, G2 = 0, Kp = 0, hd = 0, phd = 0, PM = 0;
    // weights
    bf16_t* w_patch = nullptr; float *cls = nullptr, *pos = nullptr, *lnpre_w = nullptr, *lnpre_b = nullptr,
            *lnpost_w = nullptr, *lnpost_b = nullptr;
    // attention-pool head, all fp32 (head.hip): probe query folded into the key projection (qk, ck), value / out / MLP /
    // proj weights as uploaded
    float *q_probe = nullptr, *qk = nullptr, *ck = nullptr, *w_v = nullptr, *b_v = nullptr, *w_po = nullptr, *b_po = nullptr;
    float *pln_w = nullptr, *pln_b = nullptr, *w_pfc1 = nullptr, *b_pfc1 = nullptr, *w_pfc2 = nullptr, *b_pfc2 = nullptr,
          *w_projT = nullptr;
    float2* rope_cs = nullptr;
    // grid shapes (revo_vit_set_grid): the token grid a forward runs on, with its position and rotary tables, built on first
    // use.  Entry 0 is the native G x G grid and aliases pos / rope_cs above; S and G2 above stay the native (largest) sizes
    // every workspace is allocated for, and the forwards read the ACTIVE shape (shape()) where they need the call's.
    struct GridShape { int gh, gw, S, G2; float* pos; float2* rope_cs; };
    static constexpr int MAX_SHAPES = 64;
    std::vector<GridShape> shapes;
    int active = 0;
    const GridShape& shape() const { return shapes[active]; }
    // workspace beside the body's
    bf16_t* patches = nullptr;
    float *pool_logits = nullptr, *pool_u = nullptr, *pool_att = nullptr, *pool_o = nullptr, *pool_h = nullptr,
          *pool_m = nullptr, *feat = nullptr;
    // region head (revo_vit_forward_regions): allocated by the first call with regions, a fixed size whatever n_regions is.
    // REGION_CHUNK rows of the head's buffers; image indices and bitmaps of REGION_STAGE regions on the device, filled
    // through one pinned host buffer
    float *rg_u = nullptr, *rg_att = nullptr, *rg_o = nullptr, *rg_h = nullptr, *rg_m = nullptr, *rg_feat = nullptr;
    int32_t* rg_img = nullptr; uint32_t* rg_bits = nullptr;
    PinnedStage rg_pin;
    // text-prompted regions (revo_vit_detect): allocated by the first call, sized for max_batch images, 64 prompts and g * g
    // regions per image; the region vectors grow with the largest result
    struct Detect {
        float *tok = nullptr, *scores = nullptr, *prompts = nullptr, *thr = nullptr;
        int32_t *labels = nullptr, *counts = nullptr;                 // counts[max_batch]: the region kernel's error word
        uint32_t* stage = nullptr;
        int32_t *r_img = nullptr, *r_prompt = nullptr, *r_box = nullptr, *r_cells = nullptr;
        float* r_conf = nullptr; uint32_t* r_bits = nullptr;
        float* r_vec = nullptr; size_t r_vec_rows = 0;
        bool valid = false, has_vec = false;
        int64_t n = 0; int batch = 0, P = 0;
    } det;
    ~revo_vit() { if (det.r_vec) (void)hipFree(det.r_vec); }
};

// 2-D rope table of a gh x gw grid: [S][hd/2] (cos, sin); x-axis pairs first, then y-axis; cls row unrotated.  Integer
// coordinates gx + cls, gy + cls whatever the grid: not rescaled to the native range.
static std::vector<float2> rope_table(const revo_vit_cfg& c, int hd, int gh, int gw) {
    const int d = hd / 2, nf = d / 2;
    const int start = c.use_cls ? 1 : 0;
    const int S = gh * gw + start;
    std::vector<float2> cs((size_t)S * (hd / 2));
    for (int s = 0; s < S; ++s) {
        for (int pi = 0; pi < hd / 2; ++pi) {
            double ang = 0.0;
            if (!(c.use_cls && s == 0)) {
                const int g = s - start;
                const int gy = g / gw, gx = g % gw;
                const bool xaxis = pi < nf;
                const int f = xaxis ? pi : pi - nf;
                const double freq = 1.0 / pow((double)c.rope_theta, (double)(2 * f) / (double)d);
                ang = (double)((xaxis ? gx : gy) + start) * freq;
            }
            cs[(size_t)s * (hd / 2) + pi] = make_float2((float)cos(ang), (float)sin(ang));
        }
    }
    return cs;
}

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
    v->W = c.width; v->Md = c.mlp_dim; v->ln_eps = c.ln_eps;
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

    // the checkpoint is validated as a whole before the device is touched (tower.h check_checkpoint)
    const std::string blocks = "visual.transformer.resblocks.";
    WeightMap wm;
    CHECK_RC(wm.fill("vit_create", weights, n_weights));
    {
        NeedList need = {
            {"visual.conv1.weight", (int64_t)W * Kreal}, {"visual.positional_embedding", (int64_t)S * W},
            {"visual.ln_pre.weight", W}, {"visual.ln_pre.bias", W}, {"visual.ln_post.weight", W}, {"visual.ln_post.bias", W},
            {"visual.attn_pool.probe", W}, {"visual.attn_pool.attn.in_proj_weight", (int64_t)3 * W * W},
            {"visual.attn_pool.attn.in_proj_bias", 3 * W}, {"visual.attn_pool.attn.out_proj.weight", (int64_t)W * W},
            {"visual.attn_pool.attn.out_proj.bias", W}, {"visual.attn_pool.layernorm.weight", W},
            {"visual.attn_pool.layernorm.bias", W}, {"visual.attn_pool.mlp.c_fc.weight", (int64_t)PM * W},
            {"visual.attn_pool.mlp.c_fc.bias", PM}, {"visual.attn_pool.mlp.c_proj.weight", (int64_t)W * PM},
            {"visual.attn_pool.mlp.c_proj.bias", W}, {"visual.proj", (int64_t)W * D}};
        if (c.use_cls) need.push_back({"visual.class_embedding", W});
        need_blocks(need, blocks, c.layers, W, M, c.use_ls);
        CHECK_RC(check_checkpoint(wm, need, "this architecture", c.use_ls));
    }
    REVO_ON_DEVICE(device);

    Staging sg;
    CHECK_RC(sg.alloc(W, M, std::max({(long)PM * W, (long)W * Kreal, (long)W * D})));

    const revo_tensor* t;
    if (!(t = wm.get("visual.conv1.weight", (int64_t)W * Kreal))) return -2;
    // split-precision patch embedding: rows ( hi | lo | hi ) of w / 255 (elementwise.hip patchify_kernel)
    CHECK_RC(v->dalloc(&v->w_patch, (size_t)W * 3 * v->Kp));
    REVO_HIP_CHECK(hipMemcpy(sg.stage, t->data, (size_t)W * Kreal * 4, hipMemcpyDefault));
    CHECK_RC(revo::launch_split_hi_lo_hi(sg.stage, W, Kreal, 1.0f / 255.0f, v->w_patch, v->Kp, 0));
    REVO_HIP_CHECK(hipStreamSynchronize(0));
    if (c.use_cls) CHECK_RC(up_f32(v.get(), wm, "visual.class_embedding", W, &v->cls));
    CHECK_RC(up_f32(v.get(), wm, "visual.positional_embedding", (int64_t)S * W, &v->pos));
    CHECK_RC(up_f32(v.get(), wm, "visual.ln_pre.weight", W, &v->lnpre_w));
    CHECK_RC(up_f32(v.get(), wm, "visual.ln_pre.bias", W, &v->lnpre_b));
    CHECK_RC(up_f32(v.get(), wm, "visual.ln_post.weight", W, &v->lnpost_w));
    CHECK_RC(up_f32(v.get(), wm, "visual.ln_post.bias", W, &v->lnpost_b));
    CHECK_RC(upload_blocks(v.get(), wm, sg, blocks, c.layers, c.use_ls));
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
    CHECK_RC(upload_projT(v.get(), wm, sg, "visual.proj", D, &v->w_projT));

    // 2-D rope table of the native grid, and the native shape: entry 0 of the grid cache
    {
        const std::vector<float2> cs = rope_table(c, v->hd, G, G);
        CHECK_RC(v->dalloc(&v->rope_cs, cs.size()));
        REVO_HIP_CHECK(hipMemcpy(v->rope_cs, cs.data(), cs.size() * sizeof(float2), hipMemcpyHostToDevice));
        v->shapes.reserve(revo_vit::MAX_SHAPES);
        v->shapes.push_back({G, G, v->S, v->G2, v->pos, v->rope_cs});
    }

    // workspace for max_batch images
    const size_t B = (size_t)max_batch;
    CHECK_RC(v->dalloc(&v->patches, (size_t)max_batch * v->G2 * 3 * v->Kp));
    CHECK_RC(alloc_body(v.get(), B * S));
    CHECK_RC(v->dalloc(&v->pool_logits, B * c.pool_heads * S));
    CHECK_RC(v->dalloc(&v->pool_u, B * c.pool_heads * W));
    CHECK_RC(v->dalloc(&v->pool_att, B * W));
    CHECK_RC(v->dalloc(&v->pool_o, B * W));
    CHECK_RC(v->dalloc(&v->pool_h, B * W));
    CHECK_RC(v->dalloc(&v->pool_m, B * PM));
    CHECK_RC(v->dalloc(&v->feat, B * D));
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
extern "C" int32_t revo_vit_seq_len(const revo_vit* vit) { return vit ? vit->shape().S : -1; }

// The grid of the forwards that follow (include/revo.h GRIDS).  Everything that can be refused is refused before the device is
// touched; a shape's tables are built on `stream` by the first call that names it and kept for the life of the handle.
extern "C" int32_t revo_vit_set_grid(revo_vit* v, int32_t grid_h, int32_t grid_w, void* stream) {
    API_BEGIN
    REVO_REQUIRE(v, "vit_set_grid: null handle");
    const revo_vit_cfg& c = v->cfg;
    const int P = c.patch_size, G = c.image_size / P, cls = c.use_cls ? 1 : 0;
    if (grid_h == 0 && grid_w == 0) grid_h = grid_w = G;
    const std::string name = "(" + std::to_string(grid_h) + ", " + std::to_string(grid_w) + ")";
    REVO_REQUIRE(grid_h >= 1 && grid_w >= 1, "vit_set_grid: grid " + name + " must have positive sides ((0, 0) restores the native grid)");
    REVO_REQUIRE((int64_t)grid_h * grid_w <= (int64_t)v->G2, "vit_set_grid: grid " + name + " has more than the native " +
                 std::to_string(G) + " * " + std::to_string(G) + " = " + std::to_string(v->G2) + " cells");
    REVO_REQUIRE((int64_t)grid_h * P <= 65535 && (int64_t)grid_w * P <= 65535,
                 "vit_set_grid: grid " + name + " makes a band of more than 65535 pixels");
    for (size_t i = 0; i < v->shapes.size(); ++i)
        if (v->shapes[i].gh == grid_h && v->shapes[i].gw == grid_w) {
            if ((int)i != v->active) v->det.valid = false;        // a detect result belongs to the grid it was made on
            v->active = (int)i;
            return 0;
        }
    REVO_REQUIRE((int)v->shapes.size() < revo_vit::MAX_SHAPES, "vit_set_grid: the handle already holds " +
                 std::to_string(revo_vit::MAX_SHAPES) + " grid shapes; grid " + name + " would be one more");
    REVO_ON_DEVICE(v->device);
    hipStream_t st = (hipStream_t)stream;
    revo_vit::GridShape sh{grid_h, grid_w, grid_h * grid_w + cls, grid_h * grid_w, nullptr, nullptr};
    const std::vector<float2> cs = rope_table(c, v->hd, grid_h, grid_w);
    CHECK_RC(v->dalloc(&sh.pos, (size_t)sh.S * c.width));
    CHECK_RC(v->dalloc(&sh.rope_cs, cs.size()));
    CHECK_RC(revo::launch_pos_resample(v->pos, G, cls, grid_h, grid_w, c.width, sh.pos, st));
    REVO_HIP_CHECK(hipMemcpyAsync(sh.rope_cs, cs.data(), cs.size() * sizeof(float2), hipMemcpyHostToDevice, st));
    REVO_HIP_CHECK(hipStreamSynchronize(st));                     // (cs is this frame's; once per grid and handle)
    v->shapes.push_back(sh);
    v->active = (int)v->shapes.size() - 1;
    v->det.valid = false;
    return 0;
    API_END
}

extern "C" int32_t revo_vit_stats(revo_vit* vit, double* out4, int32_t reset, void* stream) {
    API_BEGIN
    REVO_REQUIRE(vit && out4, "vit_stats: null argument");
    REVO_ON_DEVICE(vit->device);
    unsigned long long c[4] = {0, 0, 0, 0};
    // read and reset ON `stream`, behind the forwards that count and ahead of the next one, then the documented wait
    hipStream_t st = (hipStream_t)stream;
    REVO_HIP_CHECK(hipMemcpyAsync(c, vit->ln_tele, sizeof(c), hipMemcpyDeviceToHost, st));
    if (reset) REVO_HIP_CHECK(hipMemsetAsync(vit->ln_tele, 0, sizeof(c), st));
    REVO_HIP_CHECK(hipStreamSynchronize(st));
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
    REVO_HIP_CHECK(hipMemcpyAsync(dst, vit->x, (size_t)batch * vit->shape().S * vit->cfg.width * 4, hipMemcpyDeviceToDevice,
                                  (hipStream_t)stream));
    return 0;
}

extern "C" int32_t revo_vit_read_tap(revo_vit* vit, int32_t which, int32_t batch, void* dst, void* stream) {
    REVO_REQUIRE(vit && dst && batch >= 1 && batch <= vit->max_batch, "read_tap: bad arguments");
    REVO_ON_DEVICE(vit->device);
    const size_t rows = (size_t)batch * vit->shape().S, W = vit->cfg.width;
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
// whether the forward keeps the residual stream in planes for this many rows of this tower (reporting / tests)
extern "C" int32_t revo_debug_stream_in_planes(const revo_vit* v, int32_t batch) { return v && stream_in_planes(*v, batch * v->shape().S); }
// the active grid shape's tables: pos [S'][W] fp32 and rope [S'][head_dim / 2] (cos, sin) fp32 pairs (tests)
extern "C" int32_t revo_vit_read_grid_tables(revo_vit* vit, float* pos_dst, float* rope_dst, void* stream) {
    REVO_REQUIRE(vit && pos_dst && rope_dst, "read_grid_tables: null argument");
    REVO_ON_DEVICE(vit->device);
    const revo_vit::GridShape& sh = vit->shape();
    REVO_HIP_CHECK(hipMemcpyAsync(pos_dst, sh.pos, (size_t)sh.S * vit->cfg.width * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    REVO_HIP_CHECK(hipMemcpyAsync(rope_dst, sh.rope_cs, (size_t)sh.S * (vit->hd / 2) * sizeof(float2), hipMemcpyDeviceToDevice,
                                  (hipStream_t)stream));
    return 0;
}
#endif

// The head behind the pooled rows u [R][pool_heads][W]: value and output projection, the pool's LayerNorm and MLP, proj, L2 --
// for the R images of a forward or for R regions (revo_vit_forward_regions).  A row's result does not depend on R or on
// the other rows (head.hip: the skinny GEMM cuts K the same way whatever M is).
// (u_ld / u_group: the distance between two rows of u and between two heads' rows; a one-token region's pooled row is its ln_post
//  row for every head -- a softmax over one token is exactly 1 -- so the token vectors read the rows themselves: W and 0)
static int pool_head_tail(revo_vit* v, int R, const float* u, long u_ld, long u_group, float* att, float* o, float* h, float* m,
                          float* feat_ws, float* out, int32_t normalize, hipStream_t st) {
    using namespace revo;
    const revo_vit_cfg& c = v->cfg;
    const int W = c.width, D = c.out_dim, PM = v->PM;
    { ProfScope ps("gemm_pool", st);
      // values: head h's output columns from head h's pooled row
      CHECK_RC(launch_gemm_f32_skinny(0, u, u_ld, u_group, v->phd, v->w_v, W, v->b_v, R, W, W, att, W, st));
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

// Forward of the call's B images (B <= max_batch) on stream st.
static int vit_forward(revo_vit* v, const void* images, int32_t image_dtype, int B, float* out, int32_t normalize,
                       hipStream_t st, bool with_head = true) {
    const revo_vit_cfg& c = v->cfg;
    const revo_vit::GridShape& sh = v->shape();        // the call's grid: gh x gw patches, S tokens per image
    const int W = c.width, S = sh.S, PH = c.pool_heads;
    const int rows = B * S;
    using namespace revo;
    v->det.valid = false;                 // a detect result lives until the next forward of any kind

    {   // K1 + K2: patch embed GEMM in split precision (patchify_kernel: the row of a patch holds its values twice --
        // exact integers for u8 images -- or as hi | hi | lo; the weight rows are hi | lo | hi of w / 255), position add, cls row
        const int parts = image_dtype == 1 ? 2 : 3;
        { ProfScope ps("patchify", st);
          CHECK_RC(launch_patchify(images, image_dtype == 1, B, sh.gh * c.patch_size, sh.gw * c.patch_size, c.patch_size, v->patches,
                                   v->Kp, st)); }
        GemmArgs a{};
        a.A = v->patches; a.lda = (long)parts * v->Kp; a.B = v->w_patch; a.ldb = 3l * v->Kp; a.M = B * sh.G2; a.N = W;
        a.K = parts * v->Kp;
        a.C = v->x; a.ldc = W; a.pos = sh.pos; a.S = S; a.G2 = sh.G2; a.cls = c.use_cls ? 1 : 0;
        { ProfScope ps("gemm_patch", st); CHECK_RC(launch_gemm(EPI_PATCH, a, st)); }
        if (c.use_cls) { ProfScope ps("elementwise", st); CHECK_RC(launch_cls_rows(v->x, W, v->cls, sh.pos, B, S, W, st)); }
    }
    if (v->debug_layers == -2) return 0;   // parity hook: the embedded tokens (patch embed + position + class token), before ln_pre
    { ProfScope ps("layernorm", st);
      CHECK_RC(launch_layernorm(v->x, W, v->lnpre_w, v->lnpre_b, c.ln_eps, rows, W, v->x, W, 0, st)); }

    // The block loop both towers run (tower.h body_blocks).  This tower's two pieces of it: K4 + K5, bias and the 2-D
    // rotary embedding of q and k in the qkv GEMM's epilogue (every tile shape), and attention over all keys
    CHECK_RC(body_blocks(
        *v, "vit_forward", rows, v->debug_layers < 0 ? c.layers : std::min(v->debug_layers, c.layers), st,
        [&](GemmArgs& a) {
            a.rope_cs = sh.rope_cs; a.rope_S = S; a.rope_hd = v->hd; a.rope_cols = 2 * W;
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
    CHECK_RC(pool_head_tail(v, B, v->pool_u, (long)PH * W, W, v->pool_att, v->pool_o, v->pool_h, v->pool_m, v->feat, out, normalize, st));
    return 0;
}

extern "C" int32_t revo_vit_forward(revo_vit* v, const void* images, int32_t image_dtype, int32_t batch, float* out,
                                    int32_t normalize, void* stream) {
    API_BEGIN
    REVO_REQUIRE(v && images && out, "vit_forward: null argument");
    REVO_REQUIRE(batch >= 1 && batch <= v->max_batch, "vit_forward: batch exceeds max_batch of the handle");
    REVO_REQUIRE(image_dtype == 0 || image_dtype == 1, "vit_forward: image_dtype must be 0 (f32) or 1 (u8)");
    REVO_ON_DEVICE(v->device);
    return vit_forward(v, images, image_dtype, batch, out, normalize, (hipStream_t)stream);
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
    CHECK_RC(v->rg_pin.alloc((size_t)REGION_STAGE * (1 + words) * 4));     // image indices, then bitmaps
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
    CHECK_RC(vit_forward(v, images, image_dtype, batch, out_global, normalize, st, out_global != nullptr));
    if (n_regions == 0 || v->debug_layers != -1) return 0;
    const revo_vit_cfg& c = v->cfg;
    const int W = c.width, D = c.out_dim, S = v->shape().S, PH = c.pool_heads;     // (the workspace is sized for the native S)
    const size_t words = ((size_t)S + 31) / 32;
    uint32_t* pin = (uint32_t*)v->rg_pin.p;
    for (int64_t s0 = 0; s0 < n_regions; s0 += REGION_STAGE) {
        const int ns = (int)std::min<int64_t>(REGION_STAGE, n_regions - s0);
        // image indices (and host bitmaps) go through the pinned buffer: the caller's arrays are read before the call returns
        CHECK_RC(v->rg_pin.wait());
        memcpy(pin, region_image + s0, (size_t)ns * 4);
        REVO_HIP_CHECK(hipMemcpyAsync(v->rg_img, pin, (size_t)ns * 4, hipMemcpyHostToDevice, st));
        const uint32_t* bits = region_bits + (size_t)s0 * words;
        if (!bits_on_device) {
            memcpy(pin + REGION_STAGE, bits, (size_t)ns * words * 4);
            REVO_HIP_CHECK(hipMemcpyAsync(v->rg_bits, pin + REGION_STAGE, (size_t)ns * words * 4, hipMemcpyHostToDevice, st));
            bits = v->rg_bits;
        }
        CHECK_RC(v->rg_pin.record(st));
        for (int r0 = 0; r0 < ns; r0 += REGION_CHUNK) {
            const int R = std::min(REGION_CHUNK, ns - r0);
            const uint32_t* cb = bits + (size_t)r0 * words;
            float* out = out_regions + (size_t)(s0 + r0) * D;
            { ProfScope ps("pool_regions", st);
              CHECK_RC(launch_pool_head_rows_masked(v->x, W, batch, S, W, PH, v->pool_logits, v->rg_img + r0, cb, R, v->rg_u, st)); }
            CHECK_RC(pool_head_tail(v, R, v->rg_u, (long)PH * W, W, v->rg_att, v->rg_o, v->rg_h, v->rg_m, v->rg_feat, out, normalize, st));
            { ProfScope ps("pool_regions", st);
              CHECK_RC(launch_zero_empty_regions(cb, R, S, D, out, st)); }
        }
    }
    return 0;
    API_END
}

// ---------------------------------------------------------- dense token vectors ----
// The head of `rows` consecutive ln_post rows of the last body forward, each as the one-token region it is: pool_head_tail reads
// v->x itself, REGION_CHUNK rows at a time through the region workspace.
static int token_head(revo_vit* v, long rows, float* out, int32_t normalize, hipStream_t st) {
    const int W = v->cfg.width, D = v->cfg.out_dim;
    for (long r0 = 0; r0 < rows; r0 += REGION_CHUNK) {
        const int R = (int)std::min<long>(REGION_CHUNK, rows - r0);
        CHECK_RC(pool_head_tail(v, R, v->x + (size_t)r0 * W, W, 0, v->rg_att, v->rg_o, v->rg_h, v->rg_m, v->rg_feat,
                                out + (size_t)r0 * D, normalize, st));
    }
    return 0;
}

extern "C" int32_t revo_vit_forward_tokens(revo_vit* v, const void* images, int32_t image_dtype, int32_t batch, float* out_global,
                                           float* out_tokens, int32_t normalize, void* stream) {
    API_BEGIN
    REVO_REQUIRE(v && images, "vit_forward_tokens: null handle or images");
    REVO_REQUIRE(out_tokens, "vit_forward_tokens: null out_tokens");
    REVO_REQUIRE(batch >= 1 && batch <= v->max_batch, "vit_forward_tokens: batch exceeds max_batch of the handle");
    REVO_REQUIRE(image_dtype == 0 || image_dtype == 1, "vit_forward_tokens: image_dtype must be 0 (f32) or 1 (u8)");
    REVO_ON_DEVICE(v->device);
    hipStream_t st = (hipStream_t)stream;
    CHECK_RC(region_workspace(v));
    CHECK_RC(vit_forward(v, images, image_dtype, batch, out_global, normalize, st, out_global != nullptr));
    if (v->debug_layers != -1) return 0;
    ProfScope ps("token_head", st);
    return token_head(v, (long)batch * v->shape().S, out_tokens, normalize, st);
    API_END
}

// ------------------------------------------------------- text-prompted regions ----
static int detect_workspace(revo_vit* v) {
    revo_vit::Detect& d = v->det;
    if (d.r_bits) return 0;
    const size_t B = (size_t)v->max_batch, G2 = (size_t)v->G2, D = (size_t)v->cfg.out_dim, words = ((size_t)v->S + 31) / 32;
    const size_t Rmax = B * G2;
    CHECK_RC(v->dalloc(&d.tok, B * v->S * D));
    CHECK_RC(v->dalloc(&d.scores, B * revo::DETECT_MAX_PROMPTS * G2));
    CHECK_RC(v->dalloc(&d.prompts, (size_t)revo::DETECT_MAX_PROMPTS * D));
    CHECK_RC(v->dalloc(&d.thr, (size_t)revo::DETECT_MAX_PROMPTS));
    CHECK_RC(v->dalloc(&d.labels, Rmax));
    CHECK_RC(v->dalloc(&d.counts, B + 1));
    CHECK_RC(v->dalloc(&d.stage, revo::detect_stage_words((int)B, (int)G2, (int)words)));
    CHECK_RC(v->dalloc(&d.r_img, Rmax));
    CHECK_RC(v->dalloc(&d.r_prompt, Rmax));
    CHECK_RC(v->dalloc(&d.r_box, Rmax * 4));
    CHECK_RC(v->dalloc(&d.r_cells, Rmax));
    CHECK_RC(v->dalloc(&d.r_conf, Rmax));
    CHECK_RC(v->dalloc(&d.r_bits, Rmax * words));           // last: marks the workspace complete
    return 0;
}

extern "C" int32_t revo_vit_detect(revo_vit* v, const void* images, int32_t image_dtype, int32_t batch, const float* prompts,
                                   int32_t n_prompts, const float* thresholds, int32_t n_background, int32_t min_cells,
                                   int32_t max_regions, float* out_global, int32_t with_vectors, int32_t normalize,
                                   int64_t* n_regions, void* stream) {
    API_BEGIN
    // everything that can be refused is refused before the device is touched
    REVO_REQUIRE(v && images, "vit_detect: null handle or images");
    REVO_REQUIRE(prompts, "vit_detect: null prompts");
    REVO_REQUIRE(thresholds, "vit_detect: null thresholds");
    REVO_REQUIRE(n_regions, "vit_detect: null n_regions");
    REVO_REQUIRE(batch >= 1 && batch <= v->max_batch, "vit_detect: batch must be in [1, max_batch of the handle]");
    REVO_REQUIRE(image_dtype == 0 || image_dtype == 1, "vit_detect: image_dtype must be 0 (f32) or 1 (u8)");
    REVO_REQUIRE(n_prompts >= 1 && n_prompts <= revo::DETECT_MAX_PROMPTS, "vit_detect: n_prompts must be in [1, 64]");
    REVO_REQUIRE(n_background >= 0 && n_background < n_prompts, "vit_detect: n_background must be in [0, n_prompts)");
    REVO_REQUIRE(min_cells >= 1, "vit_detect: min_cells must be at least 1");
    REVO_REQUIRE(v->active == 0, "vit_detect: the handle is set to grid (" + std::to_string(v->shape().gh) + ", " +
                 std::to_string(v->shape().gw) + "); text-prompted regions run on the native grid only (revo_vit_set_grid(0, 0))");
    REVO_REQUIRE(v->G2 <= revo::DETECT_MAX_CELLS, "vit_detect: a grid of more than 1024 cells is not supported");
    REVO_REQUIRE(max_regions >= 1 && max_regions <= v->G2, "vit_detect: max_regions must be in [1, g * g = " + std::to_string(v->G2) + "]");
    for (int32_t p = 0; p < n_prompts; ++p)
        REVO_REQUIRE(!std::isnan(thresholds[p]), "vit_detect: thresholds[" + std::to_string(p) + "] is NaN");
    REVO_REQUIRE(v->debug_layers == -1, "vit_detect: the handle is set to stop its forward early (debug layers)");
    REVO_ON_DEVICE(v->device);
    hipStream_t st = (hipStream_t)stream;
    using namespace revo;
    revo_vit::Detect& d = v->det;
    d.valid = false;
    CHECK_RC(region_workspace(v));
    CHECK_RC(detect_workspace(v));
    const revo_vit_cfg& c = v->cfg;
    const int W = c.width, D = c.out_dim, S = v->S, G2 = v->G2, PH = c.pool_heads, cls = c.use_cls ? 1 : 0;
    const int words = (S + 31) / 32;
    // the call's one body forward (the global head as revo_vit_forward runs it, or none), then the normalised token vectors
    CHECK_RC(vit_forward(v, images, image_dtype, batch, out_global, normalize, st, out_global != nullptr));
    { ProfScope ps("token_head", st);
      CHECK_RC(token_head(v, (long)batch * S, d.tok, 1, st)); }
    // prompts through the query normalisation of every search; thresholds to the device (the call is synchronous)
    { ProfScope ps("detect_scores", st);
      CHECK_RC(launch_l2norm_rows(prompts, D, d.prompts, D, nullptr, 0, n_prompts, D, st));
      REVO_HIP_CHECK(hipMemcpyAsync(d.thr, thresholds, (size_t)n_prompts * 4, hipMemcpyHostToDevice, st));
      CHECK_RC(launch_detect_scores(d.tok, D, S, cls, G2, (long)batch * G2, d.prompts, n_prompts, D, d.scores, st)); }
    std::vector<int32_t> h((size_t)batch + 1);
    { ProfScope ps("detect_regions", st);
      REVO_HIP_CHECK(hipMemsetAsync(d.counts + v->max_batch, 0, 4, st));
      DetectRegionArgs a{};
      a.scores = d.scores; a.batch = batch; a.P = n_prompts; a.g = c.image_size / c.patch_size; a.cls = cls; a.thr = d.thr;
      a.nbg = n_background; a.min_cells = min_cells; a.max_regions = max_regions; a.labels = d.labels; a.counts = d.counts;
      a.stage = d.stage; a.err = d.counts + v->max_batch;
      CHECK_RC(launch_detect_regions(a, st));
      CHECK_RC(launch_detect_compact(d.counts, d.stage, batch, max_regions, words, d.r_img, d.r_prompt, d.r_box, d.r_cells,
                                     d.r_conf, d.r_bits, st)); }
    REVO_HIP_CHECK(hipMemcpyAsync(h.data(), d.counts, (size_t)batch * 4, hipMemcpyDeviceToHost, st));
    REVO_HIP_CHECK(hipMemcpyAsync(h.data() + batch, d.counts + v->max_batch, 4, hipMemcpyDeviceToHost, st));
    REVO_HIP_CHECK(hipStreamSynchronize(st));
    if (h[batch] != 0) {
        revo_set_error("vit_detect: connected components did not converge");
        return -4;
    }
    int64_t total = 0;
    for (int b = 0; b < batch; ++b) {
        REVO_REQUIRE(h[b] >= 0 && h[b] <= max_regions, "vit_detect: internal: inconsistent region counts");
        total += h[b];
    }
    if (with_vectors && total > 0) {
        // the regions' vectors from the rows and logits of the same forward: the masked pool over the device bitmaps
        if (d.r_vec_rows < (size_t)total) {
            if (d.r_vec) REVO_HIP_CHECK(hipFree(d.r_vec));
            d.r_vec = nullptr; d.r_vec_rows = 0;
            REVO_HIP_CHECK(hipMalloc((void**)&d.r_vec, (size_t)total * D * 4));
            d.r_vec_rows = (size_t)total;
        }
        for (int64_t r0 = 0; r0 < total; r0 += REGION_CHUNK) {
            const int R = (int)std::min<int64_t>(REGION_CHUNK, total - r0);
            { ProfScope ps("pool_regions", st);
              CHECK_RC(launch_pool_head_rows_masked(v->x, W, batch, S, W, PH, v->pool_logits, d.r_img + r0,
                                                    d.r_bits + (size_t)r0 * words, R, v->rg_u, st)); }
            CHECK_RC(pool_head_tail(v, R, v->rg_u, (long)PH * W, W, v->rg_att, v->rg_o, v->rg_h, v->rg_m, v->rg_feat,
                                    d.r_vec + (size_t)r0 * D, normalize, st));
        }
        REVO_HIP_CHECK(hipStreamSynchronize(st));
    }
    d.n = total; d.batch = batch; d.P = n_prompts; d.has_vec = with_vectors != 0;
    d.valid = true;
    *n_regions = total;
    return 0;
    API_END
}

template <class T> static int detect_copy(void* dst, const T* src, size_t count, int dst_on_device) {
    if (!dst || count == 0) return 0;
    REVO_HIP_CHECK(hipMemcpy(dst, src, count * sizeof(T), dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    if (dst_on_device) REVO_HIP_CHECK(hipStreamSynchronize(nullptr));   // (complete on return, whatever stream the caller is on)
    return 0;
}

extern "C" int32_t revo_vit_detect_read(revo_vit* v, int64_t start, int64_t n, int32_t* region_image, int32_t* region_prompt,
                                        int32_t* boxes, int32_t* cells, float* confidence, uint32_t* bits, float* vectors,
                                        int32_t dst_on_device) {
    API_BEGIN
    REVO_REQUIRE(v, "vit_detect_read: null handle");
    REVO_REQUIRE(start >= 0 && n >= 0, "vit_detect_read: negative start or count");
    const revo_vit::Detect& d = v->det;
    REVO_REQUIRE(d.valid, "vit_detect_read: no result (call revo_vit_detect again after another forward)");
    REVO_REQUIRE(start + n <= d.n, "vit_detect_read: range past the result's " + std::to_string(d.n) + " regions");
    REVO_REQUIRE(!vectors || d.has_vec, "vit_detect_read: the result was computed without vectors");
    if (n == 0) return 0;
    REVO_ON_DEVICE(v->device);
    const size_t words = ((size_t)v->S + 31) / 32, D = (size_t)v->cfg.out_dim, s = (size_t)start, m = (size_t)n;
    CHECK_RC(detect_copy(region_image, d.r_img + s, m, dst_on_device));
    CHECK_RC(detect_copy(region_prompt, d.r_prompt + s, m, dst_on_device));
    CHECK_RC(detect_copy(boxes, d.r_box + s * 4, m * 4, dst_on_device));
    CHECK_RC(detect_copy(cells, d.r_cells + s, m, dst_on_device));
    CHECK_RC(detect_copy(confidence, d.r_conf + s, m, dst_on_device));
    CHECK_RC(detect_copy(bits, d.r_bits + s * words, m * words, dst_on_device));
    if (vectors) CHECK_RC(detect_copy(vectors, d.r_vec + s * D, m * D, dst_on_device));
    return 0;
    API_END
}

extern "C" int32_t revo_vit_detect_maps(revo_vit* v, float* scores, int32_t* labels, int32_t dst_on_device) {
    API_BEGIN
    REVO_REQUIRE(v, "vit_detect_maps: null handle");
    const revo_vit::Detect& d = v->det;
    REVO_REQUIRE(d.valid, "vit_detect_maps: no result (call revo_vit_detect again after another forward)");
    if (!scores && !labels) return 0;
    REVO_ON_DEVICE(v->device);
    CHECK_RC(detect_copy(scores, d.scores, (size_t)d.batch * d.P * v->G2, dst_on_device));
    return detect_copy(labels, d.labels, (size_t)d.batch * v->G2, dst_on_device);
    API_END
}
