// What the two towers (vit.hip: image, text.hip: text) share (not part of the C ABI): a block's weights, the checkpoint map with
// its check and its upload helpers, the core of a tower handle (allocations, block weights, body workspace), the pinned host
// staging buffer, the gemm() wrapper and the block loop.  api.hip sees it for gemm() alone (the single-kernel GEMM ops).
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "api_internal.h"
#include "kernels.h"

// ln_1 / ln_2 are folded into the weights of the GEMM that follows them: w_qkv = bf16(ln_1.weight . W),
// b_qkv = b + W ln_1.bias, c_qkv[j] = sum_k w_qkv[j][k]; the same for fc1 with ln_2.  The forward feeds those GEMMs either
// bf16(x) with the row statistics (folded form) or the normalised row without gain and shift (LayerNorm kernel).
struct LayerW {
    bf16_t *w_qkv, *w_o, *w_fc1, *w_fc2;
    float *b_qkv, *b_o, *b_fc1, *b_fc2, *c_qkv, *c_fc1, *ls1, *ls2;
};

constexpr size_t SPLITK_WS_ELEMS = 16u << 20;     // 64 MiB of fp32

// ------------------------------------------------------------ the checkpoint ----
using NeedList = std::vector<std::pair<std::string, int64_t>>;     // a tensor's name and its element count

struct WeightMap {
    std::map<std::string, const revo_tensor*> m;
    // `who`: the entry point's name in the message
    int fill(const char* who, const revo_tensor* weights, int n_weights) {
        for (int i = 0; i < n_weights; ++i) {
            REVO_REQUIRE(weights[i].name && weights[i].data, std::string(who) + ": weight entry with a null name or data pointer");
            m[weights[i].name] = &weights[i];
        }
        return 0;
    }
    const revo_tensor* get(const std::string& name, int64_t numel) {
        auto it = m.find(name);
        if (it == m.end()) { revo_set_error("missing weight tensor: " + name); return nullptr; }
        if (it->second->numel != numel) {
            revo_set_error("weight " + name + ": expected " + std::to_string(numel) + " elements, got " +
                           std::to_string(it->second->numel));
            return nullptr;
        }
        return it->second;
    }
};

// the tensors of a tower's blocks, `prefix` = "...transformer.resblocks."
static inline void need_blocks(NeedList& need, const std::string& prefix, int layers, int W, int M, int use_ls) {
    for (int i = 0; i < layers; ++i) {
        const std::string p = prefix + std::to_string(i) + ".";
        for (const char* n : {"ln_1.weight", "ln_1.bias", "ln_2.weight", "ln_2.bias", "attn.out_proj.bias", "mlp.c_proj.bias"})
            need.push_back({p + n, W});
        need.push_back({p + "attn.in_proj_weight", (int64_t)3 * W * W});
        need.push_back({p + "attn.in_proj_bias", 3 * W});
        need.push_back({p + "attn.out_proj.weight", (int64_t)W * W});
        need.push_back({p + "mlp.c_fc.weight", (int64_t)M * W});
        need.push_back({p + "mlp.c_fc.bias", M});
        need.push_back({p + "mlp.c_proj.weight", (int64_t)W * M});
        if (use_ls) { need.push_back({p + "ls_1.gamma", W}); need.push_back({p + "ls_2.gamma", W}); }
    }
}

// The checkpoint is validated as a whole before the device is touched: every tensor the architecture needs must be present
// with the right element count (a checkpoint of another variant fails here, by name, not half-way through the upload) ...
// and nothing else: a tensor the forward would not read (LayerScale gains handed to a handle created with use_ls = 0, a
// tensor of another architecture) means a different model, not one to run without it.  `reader`: who does not read it.
static inline int check_checkpoint(WeightMap& wm, const NeedList& need, const char* reader, int use_ls) {
    for (auto& kv : need)
        if (!wm.get(kv.first, kv.second)) return -2;
    if (wm.m.size() != need.size()) {
        std::map<std::string, int64_t> want(need.begin(), need.end());
        for (auto& kv : wm.m)
            if (!want.count(kv.first)) {
                revo_set_error("unexpected weight tensor: " + kv.first + " (not read by " + reader +
                               (use_ls ? ")" : "; LayerScale needs cfg.use_ls = 1)"));
                return -2;
            }
    }
    return 0;
}

// ------------------------------------------------------------ the tower core ----
// What a tower handle (revo_vit, revo_text) is made of whichever tower it is: its device allocations, the blocks' weights and
// the workspace of the block loop for max_batch inputs.
struct TowerCore {
    int device = 0, max_batch = 0, debug_layers = -1;
    int W = 0, Md = 0; float ln_eps = 0.f;
    std::vector<LayerW> layers;
    // body workspace
    float* x = nullptr;
    bf16_t *h = nullptr, *qkv = nullptr, *att = nullptr, *mlp = nullptr;
    bf16_t* xlo = nullptr;             // low plane of the residual stream while it is kept as (h, xlo) = (bf16(x), bf16(x - hi))
    float2* ln_stats = nullptr;        // [rows][width / 256] (mean, M2) per 256-column slice: the folded LayerNorm's row statistics
    int ln_parts = 0;                  // width / 256 when the fold applies (width % 256 == 0, <= 6 slices), else 0
    unsigned long long* ln_tele = nullptr;   // [4] telemetry of the folded LayerNorm's consumers (kernels.h GemmArgs::lnc_tele; revo_vit_stats)
    float* splitk_ws = nullptr;        // fp32 partial planes of the split-K residual GEMMs
    std::vector<void*> owned;

    template <class T> int dalloc(T** out, size_t count) {
        void* p = nullptr;
        REVO_HIP_CHECK(hipMalloc(&p, count * sizeof(T) + 256));
        owned.push_back(p);
        *out = (T*)p;
        return 0;
    }
    ~TowerCore() { for (void* p : owned) (void)hipFree(p); }
};

// Staging of a create: `stage` for fp32 -> bf16 conversion, sized for the largest matrix (the blocks' or `largest_other`, the
// caller's largest outside the blocks); `gb` for gain | shift | bias of the layer being folded.  Freed on scope exit.
struct Staging {
    float *stage = nullptr, *gb = nullptr;
    int alloc(int W, int M, long largest_other) {
        const size_t stage_elems = (size_t)std::max({(long)3 * W * W, (long)M * W, largest_other});
        REVO_HIP_CHECK(hipMalloc((void**)&stage, stage_elems * 4));
        REVO_HIP_CHECK(hipMalloc((void**)&gb, (size_t)(2 * W + std::max(3 * W, M)) * 4));
        return 0;
    }
    ~Staging() { (void)hipFree(stage); (void)hipFree(gb); }
};

// fp32 (host or device) -> device fp32
static inline int up_f32(TowerCore* v, WeightMap& wm, const std::string& name, int64_t numel, float** out) {
    const revo_tensor* t = wm.get(name, numel);
    if (!t) return -2;
    CHECK_RC(v->dalloc(out, (size_t)numel));
    REVO_HIP_CHECK(hipMemcpy(*out, t->data, (size_t)numel * 4, hipMemcpyDefault));
    return 0;
}
// linear layer behind a LayerNorm: fp32 [rows][cols] weights, [cols] gain / shift, [rows] bias (host or device) ->
// bf16(gamma . W), column sums of the rounded weights, bias + W beta
static inline int up_folded(TowerCore* v, WeightMap& wm, const Staging& s, const std::string& wname, const std::string& bname,
                            const std::string& ln, int64_t rows, int64_t cols, bf16_t** w_out, float** c_out, float** b_out) {
    const revo_tensor *tw = wm.get(wname, rows * cols), *tb = wm.get(bname, rows), *tg = wm.get(ln + ".weight", cols),
                      *te = wm.get(ln + ".bias", cols);
    if (!tw || !tb || !tg || !te) return -2;
    float *stage = s.stage, *gb = s.gb;
    CHECK_RC(v->dalloc(w_out, (size_t)(rows * cols)));
    CHECK_RC(v->dalloc(c_out, (size_t)rows));
    CHECK_RC(v->dalloc(b_out, (size_t)rows));
    REVO_HIP_CHECK(hipMemcpy(stage, tw->data, (size_t)(rows * cols) * 4, hipMemcpyDefault));
    REVO_HIP_CHECK(hipMemcpy(gb, tg->data, (size_t)cols * 4, hipMemcpyDefault));
    REVO_HIP_CHECK(hipMemcpy(gb + cols, te->data, (size_t)cols * 4, hipMemcpyDefault));
    REVO_HIP_CHECK(hipMemcpy(gb + 2 * cols, tb->data, (size_t)rows * 4, hipMemcpyDefault));
    CHECK_RC(revo::launch_fold_ln_linear(stage, gb, gb + cols, gb + 2 * cols, (int)rows, (int)cols, *w_out, cols, *c_out, *b_out, 0));
    REVO_HIP_CHECK(hipStreamSynchronize(0));
    return 0;
}
// fp32 [rows][cols] (host or device) -> device bf16 [rows][cols]
static inline int up_bf16(TowerCore* v, WeightMap& wm, const Staging& s, const std::string& name, int64_t rows, int64_t cols,
                          bf16_t** out) {
    const revo_tensor* t = wm.get(name, rows * cols);
    if (!t) return -2;
    CHECK_RC(v->dalloc(out, (size_t)(rows * cols)));
    REVO_HIP_CHECK(hipMemcpy(s.stage, t->data, (size_t)(rows * cols) * 4, hipMemcpyDefault));
    CHECK_RC(revo::launch_f32_to_bf16(s.stage, cols, *out, cols, rows, (int)cols, 0));
    REVO_HIP_CHECK(hipStreamSynchronize(0));
    return 0;
}
// every block of the tower (v->W, v->Md set), `prefix` as in need_blocks
static inline int upload_blocks(TowerCore* v, WeightMap& wm, const Staging& s, const std::string& prefix, int layers, int use_ls) {
    const int W = v->W, M = v->Md;
    v->layers.resize(layers);
    for (int i = 0; i < layers; ++i) {
        const std::string p = prefix + std::to_string(i) + ".";
        LayerW& L = v->layers[i];
        memset(&L, 0, sizeof(L));
        CHECK_RC(up_folded(v, wm, s, p + "attn.in_proj_weight", p + "attn.in_proj_bias", p + "ln_1", 3 * W, W, &L.w_qkv, &L.c_qkv,
                           &L.b_qkv));
        CHECK_RC(up_bf16(v, wm, s, p + "attn.out_proj.weight", W, W, &L.w_o));
        CHECK_RC(up_f32(v, wm, p + "attn.out_proj.bias", W, &L.b_o));
        CHECK_RC(up_folded(v, wm, s, p + "mlp.c_fc.weight", p + "mlp.c_fc.bias", p + "ln_2", M, W, &L.w_fc1, &L.c_fc1, &L.b_fc1));
        CHECK_RC(up_bf16(v, wm, s, p + "mlp.c_proj.weight", W, M, &L.w_fc2));
        CHECK_RC(up_f32(v, wm, p + "mlp.c_proj.bias", W, &L.b_fc2));
        if (use_ls) {
            CHECK_RC(up_f32(v, wm, p + "ls_1.gamma", W, &L.ls1));
            CHECK_RC(up_f32(v, wm, p + "ls_2.gamma", W, &L.ls2));
        }
    }
    return 0;
}
// the output projection is stored [W][D]; the fp32 GEMM wants [D][W]
static inline int upload_projT(TowerCore* v, WeightMap& wm, const Staging& s, const std::string& name, int D, float** out) {
    const int W = v->W;
    const revo_tensor* t = wm.get(name, (int64_t)W * D);
    if (!t) return -2;
    CHECK_RC(v->dalloc(out, (size_t)D * W));
    REVO_HIP_CHECK(hipMemcpy(s.stage, t->data, (size_t)W * D * 4, hipMemcpyDefault));
    CHECK_RC(revo::launch_transpose_f32(s.stage, W, D, *out, 0));
    REVO_HIP_CHECK(hipStreamSynchronize(0));
    return 0;
}
// the block loop's workspace for `rows` rows of the residual stream
static inline int alloc_body(TowerCore* v, size_t rows) {
    const size_t W = (size_t)v->W;
    CHECK_RC(v->dalloc(&v->x, rows * W));
    CHECK_RC(v->dalloc(&v->h, rows * W));
    CHECK_RC(v->dalloc(&v->qkv, rows * 3 * W));
    CHECK_RC(v->dalloc(&v->att, rows * W));
    CHECK_RC(v->dalloc(&v->mlp, rows * (size_t)v->Md));
    CHECK_RC(v->dalloc(&v->splitk_ws, SPLITK_WS_ELEMS));
    v->ln_parts = (W % 256 == 0 && W / 256 <= 6) ? (int)(W / 256) : 0;
    if (v->ln_parts) CHECK_RC(v->dalloc(&v->ln_stats, rows * (size_t)v->ln_parts));
    if (v->ln_parts) CHECK_RC(v->dalloc(&v->xlo, rows * W));
    CHECK_RC(v->dalloc(&v->ln_tele, 4));
    REVO_HIP_CHECK(hipMemset(v->ln_tele, 0, 4 * sizeof(unsigned long long)));
    return 0;
}

// A pinned host buffer through which a caller's host array reaches the device: the array is read before the call returns, the
// copy out of the buffer is stream-ordered.  wait() before the buffer is written again, record(st) behind the last copy out of it.
struct PinnedStage {
    void* p = nullptr; hipEvent_t ev = nullptr; bool pending = false;
    int alloc(size_t bytes) {
        REVO_HIP_CHECK(hipHostMalloc(&p, bytes, hipHostMallocDefault));
        REVO_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        return 0;
    }
    int wait() {
        if (pending) REVO_HIP_CHECK(hipEventSynchronize(ev));     // the previous copy out of it
        return 0;
    }
    int record(hipStream_t st) {
        REVO_HIP_CHECK(hipEventRecord(ev, st));
        pending = true;
        return 0;
    }
    ~PinnedStage() {
        if (p) (void)hipHostFree(p);
        if (ev) (void)hipEventDestroy(ev);
    }
};

// ------------------------------------------------------------------- GEMMs ----
// the operands, the shape and the result of a GEMM: the nine fields every launch fills
static inline revo::GemmArgs gemm_args(const void* A, long lda, const void* B, long ldb, int M, int N, int K, void* C, long ldc) {
    revo::GemmArgs a{};
    a.A = (const bf16_t*)A; a.lda = lda; a.B = (const bf16_t*)B; a.ldb = ldb; a.M = M; a.N = N; a.K = K; a.C = C; a.ldc = ldc;
    return a;
}

// ln (optional, residual epilogue): the LayerNorm that follows; *ln_fused = 1 if the GEMM's launch form did it (kernels.h)
// The LayerNorm behind a residual GEMM, without gain and shift (those live in the next GEMM's weights).  Whichever the
// launch form can do: *fused = 1: `out` holds the normalised rows (one-image forms: the split-K reduce does it);
// *folded = 1: `out` holds bf16(x) and `stats` the rows' partial statistics (folded form, kernels.h GemmArgs::lnf_*);
// neither: the caller runs the LayerNorm kernel.
// planes: keep the residual stream as (out, lo) = (bf16(x), bf16(x - bf16(x))) from here on (kernels.h GemmArgs::xp_*)
struct LnAfter { float eps; bf16_t* out; long ldo; int* fused; float2* stats; int* folded; bf16_t* lo; int x_in_planes, planes_out; };
static inline int gemm(const char* cls, int epi, const bf16_t* A, long lda, const bf16_t* B, long ldb, int M, int N, int K, void* C,
                       long ldc, const float* bias, const float* gamma, hipStream_t st, float* ws = nullptr, long ws_elems = 0,
                       const LnAfter* ln = nullptr) {
    revo::GemmArgs a = gemm_args(A, lda, B, ldb, M, N, K, C, ldc);
    a.bias = bias; a.gamma = gamma; a.ws = ws; a.ws_elems = ws_elems;
    if (ln) {
        a.ln_eps = ln->eps; a.ln_ldo = ln->ldo; a.ln_fused = ln->fused;
        if (ln->fused) a.ln_out = ln->out;
        if (ln->stats) { a.lnf_xb = ln->out; a.lnf_ldxb = ln->ldo; a.lnf_stats = ln->stats; a.lnf_done = ln->folded; }
        if (ln->lo) { a.xp_hi = ln->out; a.xp_lo = ln->lo; a.xp_ld = ln->ldo; a.xp_in = ln->x_in_planes; a.xp_out = ln->planes_out; }
    }
    ProfScope ps(cls, st);
    return revo::launch_gemm(epi, a, st);
}

// Between folded residual GEMMs the stream itself lives in two bf16 planes, (h, xlo) = (bf16(x), bf16(x - bf16(x))):
// the high plane IS the next GEMM's A operand, so the residual epilogues move 4 + 4 bytes per element instead of fp32
// rows plus a bf16 copy (4 + 4 + 2).  Entered by the first folding out-proj (fp32 in, planes out), left by the last
// fc2 (planes in, fp32 out: what follows the blocks reads fp32); only when both residual GEMMs of a block fold.
static inline bool stream_in_planes(const TowerCore& t, int rows) {
    const int W = t.W, Md = t.Md;
    return t.xlo && revo::gemm_ln_planes_enabled() && revo::gemm_resid_folds(rows, W, W, W, W, W) &&
           revo::gemm_resid_folds(rows, W, Md, Md, Md, W);
}

// The first `nl` transformer blocks of tower `t` over `rows` rows of its residual stream t.x (fp32 [rows][W], LayerNorm of
// block 0 not yet applied: ln_pre's output for the image tower, the embedded tokens for the text tower).  `who`: the entry
// point's name in messages.  The two towers differ in two launches of a block, given as callables: qkv_args(GemmArgs&) adds
// what the tower's qkv epilogue needs and returns the epilogue (image: the RoPE tables, EPI_BF16_ROPE; text: EPI_BF16);
// attention() launches the tower's attention from qkv into att (image: all keys; text: causal).
template <class QkvArgs, class Attention>
int body_blocks(const TowerCore& t, const char* who, int rows, int nl, hipStream_t st, QkvArgs&& qkv_args, Attention&& attention) {
    using namespace revo;
    const int W = t.W, Md = t.Md;
    // ln_1 / ln_2 live in the weights of qkv / fc1 (LayerW): what those GEMMs read from `h` is, depending on what the
    // residual GEMM in front of them could do,
    //   H_XB    bf16(x) + the rows' partial statistics in ln_stats: the folded form (batch-sized forwards: the residual
    //           epilogue that holds the new row writes both; the consuming epilogue applies rstd (acc - mean c) + b'),
    //   H_NORM  the normalised rows (one-image forwards: the split-K reduce of the residual GEMM normalises its rows;
    //           otherwise the LayerNorm kernel, which is also what block 0's ln_1 takes).
    enum { H_NONE = 0, H_NORM = 1, H_XB = 2 };
    int h_state = H_NONE;
    float2* stats = t.ln_stats;        // (null with ln_parts = 0: no fold)
    bf16_t* xlo = stream_in_planes(t, rows) ? t.xlo : nullptr;
    bool x_planes = false;
    auto ln_before = [&](const float* csum, GemmArgs& a) {
        if (h_state == H_XB) { a.lnc_stats = stats; a.lnc_parts = t.ln_parts; a.lnc_c = csum; a.lnc_eps = t.ln_eps; a.lnc_tele = t.ln_tele; }
    };
    auto normalise_if_needed = [&]() -> int {
        if (h_state != H_NONE) return 0;
        if (x_planes) { revo_set_error(std::string(who) + ": internal: a LayerNorm kernel was asked for while the stream is in planes"); return -3; }
        ProfScope ps("layernorm", st);
        CHECK_RC(launch_layernorm(t.x, W, nullptr, nullptr, t.ln_eps, rows, W, t.h, W, 1, st));
        h_state = H_NORM;
        return 0;
    };
    for (int i = 0; i < nl; ++i) {
        const LayerW& L = t.layers[i];
        CHECK_RC(normalise_if_needed());
        {
            GemmArgs a{};
            a.A = t.h; a.lda = W; a.B = L.w_qkv; a.ldb = W; a.M = rows; a.N = 3 * W; a.K = W; a.C = t.qkv;
            a.ldc = 3 * W; a.bias = L.b_qkv;
            const int epi = qkv_args(a);
            ln_before(L.c_qkv, a);
            ProfScope ps("gemm_qkv", st);
            CHECK_RC(launch_gemm(epi, a, st));
        }
        { ProfScope ps("attention", st);
          CHECK_RC(attention()); }
        int fused = 0, folded = 0;
        const LnAfter ln2{t.ln_eps, t.h, W, &fused, stats, &folded, xlo, x_planes ? 1 : 0, xlo ? 1 : 0};
        CHECK_RC(gemm("gemm_out", EPI_RESID_F32, t.att, W, L.w_o, W, rows, W, W, t.x, W, L.b_o, L.ls1, st, t.splitk_ws,
                      (long)SPLITK_WS_ELEMS, &ln2));
        h_state = folded ? H_XB : (fused ? H_NORM : H_NONE);
        x_planes = xlo && folded;
#ifdef REVO_EXPERIMENTS
        // cache-state experiment: re-touch bf16(x) (a device copy into the dead qkv buffer) before the GEMM that streams it
        if (folded && getenv("REVO_LNFOLD_TOUCH")) {
            ProfScope ps("touch", st);
            REVO_HIP_CHECK(hipMemcpyAsync(t.qkv, t.h, (size_t)rows * W * 2, hipMemcpyDeviceToDevice, st));
        }
#endif
        CHECK_RC(normalise_if_needed());
        {
            GemmArgs a{};
            a.A = t.h; a.lda = W; a.B = L.w_fc1; a.ldb = W; a.M = rows; a.N = Md; a.K = W; a.C = t.mlp; a.ldc = Md;
            a.bias = L.b_fc1;
            ln_before(L.c_fc1, a);
            ProfScope ps("gemm_fc1", st);
            CHECK_RC(launch_gemm(EPI_BF16_GELU, a, st));
        }
        // (splitk_ws: scratch for the split-K forms of fc2 -- leftover rows at large batch, the whole GEMM at small batch)
        fused = 0; folded = 0;
        const bool last = i + 1 >= nl;
        // the last fc2 has no LayerNorm of the body behind it: it brings the stream back to fp32 rows (ln_post / ln_final, the taps)
        const LnAfter ln1n{t.ln_eps, t.h, W, last ? nullptr : &fused, last ? nullptr : stats, last ? nullptr : &folded, xlo,
                           x_planes ? 1 : 0, (xlo && !last) ? 1 : 0};
        CHECK_RC(gemm("gemm_fc2", EPI_RESID_F32, t.mlp, Md, L.w_fc2, Md, rows, W, Md, t.x, W, L.b_fc2, L.ls2, st,
                      t.splitk_ws, (long)SPLITK_WS_ELEMS, (!last || x_planes) ? &ln1n : nullptr));
        h_state = last ? H_NONE : (folded ? H_XB : (fused ? H_NORM : H_NONE));
        x_planes = !last && xlo && folded;
#ifdef REVO_EXPERIMENTS
        if (folded && !last && getenv("REVO_LNFOLD_TOUCH")) {
            ProfScope ps("touch", st);
            REVO_HIP_CHECK(hipMemcpyAsync(t.qkv, t.h, (size_t)rows * W * 2, hipMemcpyDeviceToDevice, st));
        }
#endif
    }
    return 0;
}
