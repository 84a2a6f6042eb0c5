// C ABI of librevo (include/revo.h), except the two towers (vit.hip, text.hip), the gallery and the searches (gallery.hip,
// search.hip, candidate_search.hip): error state, the per-kernel-class profiler, and the single-kernel ops.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/revo.h"
#include "api_internal.h"
#include "kernels.h"
#include "tower.h"      // gemm(), gemm_args(), LnAfter: the single-kernel GEMM ops launch the way a forward does

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

// ------------------------------------------------------- single kernels ----
// The residual epilogue may cut the K range of its last, partly filled round of tiles (split-K tail): an op gives it the
// scratch a forward would, for the duration of the call (stream-ordered allocation: nothing is kept by the library between
// calls, nothing waits).  Allocated on construction unless `wanted` is false, freed on scope exit.
namespace {
constexpr long OP_WS_ELEMS = 16l << 20;
struct OpScratch {
    float* p = nullptr; hipStream_t st; hipError_t err = hipSuccess;
    explicit OpScratch(hipStream_t s, bool wanted = true) : st(s) {
        if (wanted) err = hipMallocAsync((void**)&p, OP_WS_ELEMS * 4, st);
    }
    OpScratch(const OpScratch&) = delete;
    ~OpScratch() { if (p) (void)hipFreeAsync(p, st); }
    long elems() const { return p ? OP_WS_ELEMS : 0; }
    int status() const {
        if (err == hipSuccess) return 0;
        revo_set_error(std::string("hipMallocAsync((void**)&ws, OP_WS_ELEMS * 4, st): ") + hipGetErrorString(err));
        return -1;
    }
};
}  // namespace

extern "C" int32_t revo_op_gemm(int32_t epi, const void* a, int64_t lda, const void* b, int64_t ldb, int32_t m,
                                int32_t n, int32_t k, void* c, int64_t ldc, const float* bias, const float* gamma,
                                void* stream) {
    API_BEGIN
    REVO_REQUIRE(epi >= 0 && epi <= 3, "op_gemm: epilogue must be 0..3");
    hipStream_t st = (hipStream_t)stream;
    OpScratch ws(st, epi == revo::EPI_RESID_F32);        // only the residual epilogue takes scratch
    CHECK_RC(ws.status());
    return gemm("gemm_op", epi, (const bf16_t*)a, lda, (const bf16_t*)b, ldb, m, n, k, c, ldc, bias, gamma, st, ws.p, ws.elems());
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
    hipStream_t st = (hipStream_t)stream;
    OpScratch ws(st);
    CHECK_RC(ws.status());
    revo::GemmArgs g = gemm_args(a, lda, b, ldb, m, n, k, c, ldc);
    g.bias = bias; g.gamma = gamma; g.ws = ws.p; g.ws_elems = OP_WS_ELEMS;
    int flag = 0;
    if (stats) { g.lnf_xb = (bf16_t*)xb; g.lnf_ldxb = ldxb; g.lnf_stats = (float2*)stats; g.lnf_done = &flag; }
    if (xlo) { g.xp_hi = (bf16_t*)xb; g.xp_lo = (bf16_t*)xlo; g.xp_ld = ldxb; g.xp_in = x_in_planes != 0; g.xp_out = planes_out != 0; }
    const int rc = revo::launch_gemm(revo::EPI_RESID_F32, g, st);
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
    revo::GemmArgs g = gemm_args(a, lda, b, ldb, m, n, k, c, ldc);
    g.bias = bias; g.lnc_stats = (const float2*)stats; g.lnc_parts = parts; g.lnc_c = csum; g.lnc_eps = eps;
    g.lnc_tele = (unsigned long long*)tele;
    return revo::launch_gemm(epi, g, (hipStream_t)stream);
    API_END
}
extern "C" int32_t revo_op_gemm_rope(const void* a, int64_t lda, const void* b, int64_t ldb, int32_t m, int32_t n,
                                     int32_t k, void* c, int64_t ldc, const float* bias, const float* cos_sin,
                                     int32_t seq, int32_t head_dim, int32_t rope_cols, void* stream) {
    API_BEGIN
    revo::GemmArgs g = gemm_args(a, lda, b, ldb, m, n, k, c, ldc);
    g.bias = bias; g.rope_cs = (const float2*)cos_sin; g.rope_S = seq; g.rope_hd = head_dim; g.rope_cols = rope_cols;
    return revo::launch_gemm(revo::EPI_BF16_ROPE, g, (hipStream_t)stream);
    API_END
}
// The qkv launch of a batch-sized forward: the folded LayerNorm's consumer and the fused RoPE in one epilogue (vit.hip vit_forward)
extern "C" int32_t revo_op_gemm_ln_in_rope(const void* a, int64_t lda, const void* b, int64_t ldb, int32_t m, int32_t n, int32_t k,
                                           void* c, int64_t ldc, const float* bias, const float* csum, const void* stats,
                                           int32_t parts, float eps, const float* cos_sin, int32_t seq, int32_t head_dim,
                                           int32_t rope_cols, void* stream) {
    API_BEGIN
    REVO_REQUIRE(a && b && c && csum && stats && cos_sin, "op_gemm_ln_in_rope: null argument");
    revo::GemmArgs g = gemm_args(a, lda, b, ldb, m, n, k, c, ldc);
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
    hipStream_t st = (hipStream_t)stream;
    OpScratch ws(st);
    CHECK_RC(ws.status());
    int flag = 0;
    const LnAfter ln{eps, (bf16_t*)ln_out, ln_ldo, &flag, nullptr, nullptr, nullptr, 0, 0};
    const int rc = gemm("gemm_op", revo::EPI_RESID_F32, (const bf16_t*)a, lda, (const bf16_t*)b, ldb, m, n, k, c, ldc, bias, gamma,
                        st, ws.p, OP_WS_ELEMS, &ln);
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
// The same kernel with grouped A rows, the way the pool's value projection launches it (vit.hip): output columns
// [g * group_cols, (g + 1) * group_cols) read their A rows at A + g * a_group_stride.  The launcher's own grouping refusals
// (group_cols % 16, a_group_stride % 4) pass through.
extern "C" int32_t revo_op_linear_f32_grouped(int32_t epi, const float* A, int64_t lda, int64_t a_group_stride, int32_t group_cols,
                                              const float* Wt, int64_t ldw, const float* bias, int32_t M, int32_t N, int32_t K,
                                              float* C, int64_t ldc, void* stream) {
    API_BEGIN
    REVO_REQUIRE(A && Wt && C && M >= 1 && N >= 1 && K >= 16 && lda >= K && ldw >= K && ldc >= N && group_cols >= 0 &&
                 a_group_stride >= 0, "op_linear_f32_grouped: bad arguments");
    return revo::launch_gemm_f32_skinny(epi, A, lda, a_group_stride, group_cols, Wt, ldw, bias, M, N, K, C, ldc, (hipStream_t)stream);
    API_END
}
// The probe's keys folded into one [heads, width] matrix at load time (head.hip probe_qk_kernel): qk[h][i] = sum over the
// head's rows o of q[o] Wk[o][i], ck[h] = sum of q[o] bk[o]
extern "C" int32_t revo_op_probe_qk(const float* q, const float* Wk, const float* bk, int32_t width, int32_t heads, float* qk,
                                    float* ck, void* stream) {
    API_BEGIN
    REVO_REQUIRE(q && Wk && bk && qk && ck, "op_probe_qk: null argument");
    REVO_REQUIRE(width >= 1 && heads >= 1 && width % heads == 0, "op_probe_qk: width must be a positive multiple of heads");
    return revo::launch_probe_qk(q, Wk, bk, width, heads, qk, ck, (hipStream_t)stream);
    API_END
}
// The row normaliser whole (elementwise.hip l2norm_rows_kernel: every gallery row, every query; its row_stats and max_stats
// are the only inputs of the exactness certificate).  Every refusal comes before the device is touched.
extern "C" int32_t revo_op_l2norm_rows(const float* src, int64_t ld_src, float* dst_f32, int64_t ld_f32, uint16_t* dst_bf16,
                                       int64_t ld_bf16, int64_t rows, int32_t dim, int32_t normalize, float* row_stats,
                                       float* max_stats, uint32_t* zero_a, int64_t zero_a_words, uint32_t* zero_b,
                                       int64_t zero_b_words, const int64_t* dst_rows, void* stream) {
    API_BEGIN
    REVO_REQUIRE(src, "op_l2norm_rows: null src");
    REVO_REQUIRE(rows >= 0, "op_l2norm_rows: negative rows");
    REVO_REQUIRE(dim >= 1, "op_l2norm_rows: dim must be at least 1");
    REVO_REQUIRE(ld_src >= dim && (!dst_f32 || ld_f32 >= dim) && (!dst_bf16 || ld_bf16 >= dim),
                 "op_l2norm_rows: a row stride is below dim");
    REVO_REQUIRE(zero_a_words >= 0 && zero_b_words >= 0 && (zero_a || zero_a_words == 0) && (zero_b || zero_b_words == 0),
                 "op_l2norm_rows: a null array to clear with a positive word count");
    static_assert(sizeof(long long) == sizeof(int64_t), "dst_rows is passed through as it is");
    return revo::launch_l2norm_rows(src, ld_src, dst_f32, ld_f32, dst_bf16, ld_bf16, rows, dim, (hipStream_t)stream, normalize ? 1 : 0,
                                    row_stats, (uint32_t*)max_stats, zero_a, zero_a_words, zero_b, zero_b_words,
                                    (const long long*)dst_rows);
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

// ---- the kernels of revo_vit_detect without a tower (detect.hip)
extern "C" int32_t revo_op_detect_scores(const float* tokens, int64_t rows, const float* prompts, int32_t n_prompts, int32_t dim,
                                         float* prompts_norm, float* scores, void* stream) {
    API_BEGIN
    REVO_REQUIRE(rows >= 0 && rows < (1ll << 31), "op_detect_scores: rows must be in [0, 2^31)");
    REVO_REQUIRE(n_prompts >= 1 && n_prompts <= revo::DETECT_MAX_PROMPTS, "op_detect_scores: n_prompts must be in [1, 64]");
    REVO_REQUIRE(dim >= 4 && dim % 4 == 0, "op_detect_scores: dim must be a positive multiple of 4");
    REVO_REQUIRE(prompts && prompts_norm && (rows == 0 || (tokens && scores)), "op_detect_scores: null argument");
    hipStream_t st = (hipStream_t)stream;
    CHECK_RC(revo::launch_l2norm_rows(prompts, dim, prompts_norm, dim, nullptr, 0, n_prompts, dim, st));
    return revo::launch_detect_scores(tokens, dim, (int)rows, 0, (int)rows, rows, prompts_norm, n_prompts, dim, scores, st);
    API_END
}
extern "C" int32_t revo_op_detect_regions(const float* scores, int32_t batch, int32_t n_prompts, int32_t g, int32_t use_cls,
                                          const float* thresholds, int32_t n_background, int32_t min_cells, int32_t max_regions,
                                          int32_t* region_image, int32_t* region_prompt, int32_t* boxes, int32_t* cells,
                                          float* confidence, uint32_t* bits, int32_t* labels, int32_t* counts, void* stream) {
    API_BEGIN
    REVO_REQUIRE(batch >= 0, "op_detect_regions: negative batch");
    REVO_REQUIRE(g >= 1 && (int64_t)g * g <= revo::DETECT_MAX_CELLS, "op_detect_regions: g * g must be in [1, 1024]");
    REVO_REQUIRE(n_prompts >= 1 && n_prompts <= revo::DETECT_MAX_PROMPTS, "op_detect_regions: n_prompts must be in [1, 64]");
    REVO_REQUIRE(n_background >= 0 && n_background < n_prompts, "op_detect_regions: n_background must be in [0, n_prompts)");
    REVO_REQUIRE(min_cells >= 1, "op_detect_regions: min_cells must be at least 1");
    REVO_REQUIRE(max_regions >= 1 && max_regions <= g * g, "op_detect_regions: max_regions must be in [1, g * g]");
    REVO_REQUIRE(use_cls == 0 || use_cls == 1, "op_detect_regions: use_cls must be 0 or 1");
    REVO_REQUIRE(thresholds && counts && (batch == 0 || scores), "op_detect_regions: null scores, thresholds or counts");
    if (batch == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int words = (g * g + use_cls + 31) / 32;
    // the images' slots and the error word: a buffer for the length of the call, which ends synchronised
    uint32_t* ws = nullptr;
    const size_t stage_words = revo::detect_stage_words(batch, max_regions, words);
    REVO_HIP_CHECK(hipMalloc((void**)&ws, (stage_words + 1) * 4));
    int32_t err = 0;
    auto run = [&]() -> int {
        REVO_HIP_CHECK(hipMemsetAsync(ws + stage_words, 0, 4, st));
        revo::DetectRegionArgs a{};
        a.scores = scores; a.batch = batch; a.P = n_prompts; a.g = g; a.cls = use_cls; a.thr = thresholds; a.nbg = n_background;
        a.min_cells = min_cells; a.max_regions = max_regions; a.labels = labels; a.counts = counts; a.stage = ws;
        a.err = (int*)(ws + stage_words);
        CHECK_RC(revo::launch_detect_regions(a, st));
        CHECK_RC(revo::launch_detect_compact(counts, ws, batch, max_regions, words, region_image, region_prompt, boxes, cells,
                                             confidence, bits, st));
        REVO_HIP_CHECK(hipMemcpyAsync(&err, ws + stage_words, 4, hipMemcpyDeviceToHost, st));
        REVO_HIP_CHECK(hipStreamSynchronize(st));
        return 0;
    };
    const int rc = run();
    (void)hipFree(ws);
    if (rc) return rc;
    if (err != 0) {
        revo_set_error("op_detect_regions: connected components did not converge");
        return -4;
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
