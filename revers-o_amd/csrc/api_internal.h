// Plumbing shared by api.hip, text.hip, gallery.hip, search.hip and candidate_search.hip (not part of the C ABI): status guards,
// device guard, profiler scope; and what the two towers (api.hip: image, text.hip: text) share: a block's weights, the
// checkpoint map and its upload helpers, the gemm() wrapper and the block loop.
#pragma once
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "../../include/revo.h"
#include "common.h"
#include "kernels.h"

#define API_BEGIN try {
#define API_END                                            \
    }                                                      \
    catch (const std::exception& e) {                      \
        revo_set_error(std::string("exception: ") + e.what()); \
        return -3;                                         \
    }                                                      \
    catch (...) {                                          \
        revo_set_error("unknown exception");               \
        return -3;                                         \
    }
#define CHECK_RC(expr)            \
    do {                          \
        int _rc = (expr);         \
        if (_rc) return _rc;      \
    } while (0)

// A handle is bound to the device it was created on: every entry point that takes one makes that
// device current for the duration of the call (allocations, kernel attributes and launches all go
// to the current device) and puts the caller's device back afterwards.
struct DeviceGuard {
    int prev = -1; bool switched = false; hipError_t err = hipSuccess;
    explicit DeviceGuard(int device) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != device) { err = hipSetDevice(device); switched = err == hipSuccess; }
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};
#define REVO_ON_DEVICE(dev)                 \
    DeviceGuard dg_(dev);                   \
    REVO_HIP_CHECK(dg_.err)

// times what is enqueued on `s` during its lifetime as kernel class `cls` (revo_prof_enable; the state lives in api.hip)
struct ProfRec { std::string cls; hipEvent_t a, b; };
struct ProfScope {
    bool active; hipStream_t st; ProfRec rec;
    ProfScope(const char* cls, hipStream_t s);
    ~ProfScope();
};

// ------------------------------------------------- shared by the two towers ----
// ln_1 / ln_2 are folded into the weights of the GEMM that follows them: w_qkv = bf16(ln_1.weight . W),
// b_qkv = b + W ln_1.bias, c_qkv[j] = sum_k w_qkv[j][k]; the same for fc1 with ln_2.  The forward feeds those GEMMs either
// bf16(x) with the row statistics (folded form) or the normalised row without gain and shift (LayerNorm kernel).
struct LayerW {
    bf16_t *w_qkv, *w_o, *w_fc1, *w_fc2;
    float *b_qkv, *b_o, *b_fc1, *b_fc2, *c_qkv, *c_fc1, *ls1, *ls2;
};

constexpr size_t SPLITK_WS_ELEMS = 16u << 20;     // 64 MiB of fp32

struct WeightMap {
    std::map<std::string, const revo_tensor*> m;
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

// The upload helpers take the handle (revo_vit, revo_text) for its dalloc() only.
// fp32 (host or device) -> device fp32
template <class H>
int up_f32(H* v, WeightMap& wm, const std::string& name, int64_t numel, float** out) {
    const revo_tensor* t = wm.get(name, numel);
    if (!t) return -2;
    CHECK_RC(v->dalloc(out, (size_t)numel));
    REVO_HIP_CHECK(hipMemcpy(*out, t->data, (size_t)numel * 4, hipMemcpyDefault));
    return 0;
}
// linear layer behind a LayerNorm: fp32 [rows][cols] weights, [cols] gain / shift, [rows] bias (host or device) ->
// bf16(gamma . W), column sums of the rounded weights, bias + W beta
template <class H>
int up_folded(H* v, WeightMap& wm, float* stage, float* gb, const std::string& wname, const std::string& bname,
              const std::string& ln, int64_t rows, int64_t cols, bf16_t** w_out, float** c_out, float** b_out) {
    const revo_tensor *tw = wm.get(wname, rows * cols), *tb = wm.get(bname, rows), *tg = wm.get(ln + ".weight", cols),
                      *te = wm.get(ln + ".bias", cols);
    if (!tw || !tb || !tg || !te) return -2;
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
// fp32 [rows][cols] (host or device) -> device bf16 [rows][ld] zero padded
template <class H>
int up_bf16(H* v, float* stage, const float* src, int64_t rows, int64_t cols, int64_t ld, bf16_t** out) {
    CHECK_RC(v->dalloc(out, (size_t)(rows * ld)));
    REVO_HIP_CHECK(hipMemcpy(stage, src, (size_t)(rows * cols) * 4, hipMemcpyDefault));
    CHECK_RC(revo::launch_f32_to_bf16(stage, cols, *out, ld, rows, (int)cols, 0));
    REVO_HIP_CHECK(hipStreamSynchronize(0));
    return 0;
}

// ln (optional, residual epilogue): the LayerNorm that follows; *ln_fused = 1 if the GEMM's launch form did it (kernels.h)
// The LayerNorm behind a residual GEMM, without gain and shift (those live in the next GEMM's weights).  Whichever the
// launch form can do: *fused = 1: `out` holds the normalised rows (one-image forms: the split-K reduce does it);
// *folded = 1: `out` holds bf16(x) and `stats` the rows' partial statistics (folded form, kernels.h GemmArgs::lnf_*);
// neither: the caller runs the LayerNorm kernel.
// planes: keep the residual stream as (out, lo) = (bf16(x), bf16(x - bf16(x))) from here on (kernels.h GemmArgs::xp_*)
struct LnAfter { float eps; bf16_t* out; long ldo; int* fused; float2* stats; int* folded; bf16_t* lo; int x_in_planes, planes_out; };
// consumer side of the folded form: A = bf16(x), the epilogue applies rstd (acc - mean c) + bias
struct LnBefore { const float2* stats; int parts; const float* c; float eps; };
static inline int gemm(const char* cls, int epi, const bf16_t* A, long lda, const bf16_t* B, long ldb, int M, int N, int K, void* C,
                       long ldc, const float* bias, const float* gamma, hipStream_t st, float* ws = nullptr, long ws_elems = 0,
                       const LnAfter* ln = nullptr) {
    revo::GemmArgs a{};
    a.A = A; a.lda = lda; a.B = B; a.ldb = ldb; a.M = M; a.N = N; a.K = K; a.C = C; a.ldc = ldc;
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

// The transformer blocks of a forward over `rows` rows of the residual stream x (fp32 [rows][W], LayerNorm of block 0 not yet
// applied: ln_pre's output for the image tower, the embedded tokens for the text tower).  All buffers are the caller's views.
struct BodyCtx {
    const char* who;                   // the entry point's name in messages
    const std::vector<LayerW>* layers; int nl;     // blocks [0, nl) run
    int W, Md, rows; float eps;
    float* x; bf16_t *h, *qkv, *att, *mlp;
    bf16_t* xlo;                       // low plane of the residual stream at these rows, null: the handle keeps none
    float2* stats; int ln_parts; unsigned long long* ln_tele;      // the folded LayerNorm's statistics at these rows (null / 0: no fold)
    float* splitk_ws;
};
// The two towers differ in two launches of a block, given as callables: qkv_args(GemmArgs&) adds what the tower's qkv epilogue
// needs and returns the epilogue (image: the RoPE tables, EPI_BF16_ROPE; text: EPI_BF16); attention() launches the tower's
// attention from qkv into att (image: all keys; text: causal).
template <class QkvArgs, class Attention>
int body_blocks(const BodyCtx& b, hipStream_t st, QkvArgs&& qkv_args, Attention&& attention) {
    using namespace revo;
    const int W = b.W, Md = b.Md, rows = b.rows, nl = b.nl;
    // ln_1 / ln_2 live in the weights of qkv / fc1 (LayerW): what those GEMMs read from `h` is, depending on what the
    // residual GEMM in front of them could do,
    //   H_XB    bf16(x) + the rows' partial statistics in ln_stats: the folded form (batch-sized forwards: the residual
    //           epilogue that holds the new row writes both; the consuming epilogue applies rstd (acc - mean c) + b'),
    //   H_NORM  the normalised rows (one-image forwards: the split-K reduce of the residual GEMM normalises its rows;
    //           otherwise the LayerNorm kernel, which is also what block 0's ln_1 takes).
    enum { H_NONE = 0, H_NORM = 1, H_XB = 2 };
    int h_state = H_NONE;
    float2* stats = b.stats;
    // Between folded residual GEMMs the stream itself lives in two bf16 planes, (h, xlo) = (bf16(x), bf16(x - bf16(x))):
    // the high plane IS the next GEMM's A operand, so the residual epilogues move 4 + 4 bytes per element instead of fp32
    // rows plus a bf16 copy (4 + 4 + 2).  Entered by the first folding out-proj (fp32 in, planes out), left by the last
    // fc2 (planes in, fp32 out: what follows the blocks reads fp32); only when both residual GEMMs of a block fold.
    bf16_t* xlo = (b.xlo && gemm_ln_planes_enabled() && gemm_resid_folds(rows, W, W, W, W, W) && gemm_resid_folds(rows, W, Md, Md, Md, W))
                      ? b.xlo : nullptr;
    bool x_planes = false;
    auto ln_before = [&](const float* csum, GemmArgs& a) {
        if (h_state == H_XB) { a.lnc_stats = stats; a.lnc_parts = b.ln_parts; a.lnc_c = csum; a.lnc_eps = b.eps; a.lnc_tele = b.ln_tele; }
    };
    auto normalise_if_needed = [&]() -> int {
        if (h_state != H_NONE) return 0;
        if (x_planes) { revo_set_error(std::string(b.who) + ": internal: a LayerNorm kernel was asked for while the stream is in planes"); return -3; }
        ProfScope ps("layernorm", st);
        CHECK_RC(launch_layernorm(b.x, W, nullptr, nullptr, b.eps, rows, W, b.h, W, 1, st));
        h_state = H_NORM;
        return 0;
    };
    for (int i = 0; i < nl; ++i) {
        const LayerW& L = (*b.layers)[i];
        CHECK_RC(normalise_if_needed());
        {
            GemmArgs a{};
            a.A = b.h; a.lda = W; a.B = L.w_qkv; a.ldb = W; a.M = rows; a.N = 3 * W; a.K = W; a.C = b.qkv;
            a.ldc = 3 * W; a.bias = L.b_qkv;
            const int epi = qkv_args(a);
            ln_before(L.c_qkv, a);
            ProfScope ps("gemm_qkv", st);
            CHECK_RC(launch_gemm(epi, a, st));
        }
        { ProfScope ps("attention", st);
          CHECK_RC(attention()); }
        int fused = 0, folded = 0;
        const LnAfter ln2{b.eps, b.h, W, &fused, stats, &folded, xlo, x_planes ? 1 : 0, xlo ? 1 : 0};
        CHECK_RC(gemm("gemm_out", EPI_RESID_F32, b.att, W, L.w_o, W, rows, W, W, b.x, W, L.b_o, L.ls1, st, b.splitk_ws,
                      (long)SPLITK_WS_ELEMS, &ln2));
        h_state = folded ? H_XB : (fused ? H_NORM : H_NONE);
        x_planes = xlo && folded;
#ifdef REVO_EXPERIMENTS
        // cache-state experiment: re-touch bf16(x) (a device copy into the dead qkv buffer) before the GEMM that streams it
        if (folded && getenv("REVO_LNFOLD_TOUCH")) {
            ProfScope ps("touch", st);
            REVO_HIP_CHECK(hipMemcpyAsync(b.qkv, b.h, (size_t)rows * W * 2, hipMemcpyDeviceToDevice, st));
        }
#endif
        CHECK_RC(normalise_if_needed());
        {
            GemmArgs a{};
            a.A = b.h; a.lda = W; a.B = L.w_fc1; a.ldb = W; a.M = rows; a.N = Md; a.K = W; a.C = b.mlp; a.ldc = Md;
            a.bias = L.b_fc1;
            ln_before(L.c_fc1, a);
            ProfScope ps("gemm_fc1", st);
            CHECK_RC(launch_gemm(EPI_BF16_GELU, a, st));
        }
        // (splitk_ws: scratch for the split-K forms of fc2 -- leftover rows at large batch, the whole GEMM at small batch)
        fused = 0; folded = 0;
        const bool last = i + 1 >= nl;
        // the last fc2 has no LayerNorm of the body behind it: it brings the stream back to fp32 rows (ln_post / ln_final, the taps)
        const LnAfter ln1n{b.eps, b.h, W, last ? nullptr : &fused, last ? nullptr : stats, last ? nullptr : &folded, xlo,
                           x_planes ? 1 : 0, (xlo && !last) ? 1 : 0};
        CHECK_RC(gemm("gemm_fc2", EPI_RESID_F32, b.mlp, Md, L.w_fc2, Md, rows, W, Md, b.x, W, L.b_fc2, L.ls2, st,
                      b.splitk_ws, (long)SPLITK_WS_ELEMS, (!last || x_planes) ? &ln1n : nullptr));
        h_state = last ? H_NONE : (folded ? H_XB : (fused ? H_NORM : H_NONE));
        x_planes = !last && xlo && folded;
#ifdef REVO_EXPERIMENTS
        if (folded && !last && getenv("REVO_LNFOLD_TOUCH")) {
            ProfScope ps("touch", st);
            REVO_HIP_CHECK(hipMemcpyAsync(b.qkv, b.h, (size_t)rows * W * 2, hipMemcpyDeviceToDevice, st));
        }
#endif
    }
    return 0;
}
