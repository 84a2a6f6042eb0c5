// launch_gemm: executes the plan gemm_plan.h makes of a problem with the kernels of gemm_kernels.h.  Nothing here decides a
// launch form: the plan names each step's kernel, rows and grid, and run_step launches it.
#include <cstdlib>
#include "gemm_kernels.h"
#include "gemm_plan.h"

namespace revo {

static GemmKnobs g_knobs;
void gemm_force_tile(int t) { g_knobs.force_tile = t; }
void gemm_force_gy(int gy) { g_knobs.force_gy = gy; }
void gemm_set_min_tiles256(int n) { g_knobs.min_tiles256 = n; }
void gemm_set_persistent(int on) { g_knobs.persistent = on; }
void gemm_set_qstores(int on) { g_knobs.qstores = on & 31; g_knobs.qtail = !(on & 32); }      // (+ 32: no fused leftover rows)
void gemm_set_ring(int on, int max_tiles) { g_knobs.ring = on; if (max_tiles > 0) g_knobs.ring_max_tiles = max_tiles; }
void gemm_set_tail_split(int on) { g_knobs.tail_split = on; }
void gemm_set_splitk(int on) { g_knobs.splitk = on; }
void gemm_set_rows192(int on) { g_knobs.rows192 = on; }
void gemm_set_ln_fold(int on) { g_knobs.lnf = on != 0; g_knobs.ln_planes = on != 2; }
bool gemm_ln_planes_enabled() { return g_knobs.lnf && g_knobs.ln_planes; }
#ifdef REVO_EXPERIMENTS
void gemm_set_debug(int d) { g_knobs.dbg = d; }
void gemm_set_stagger(int cycles, int groups) { g_knobs.stagger_cycles = cycles; g_knobs.stagger_groups = groups < 1 ? 1 : groups; }
void gemm_set_phase_groups(int g) { g_knobs.phase_groups = g < 0 ? 0 : (g > 4 ? 4 : g); }
static unsigned long long* g_stamps = nullptr; static int g_stamp_items = 0;
void gemm_set_stamps(unsigned long long* buf, int items) { g_stamps = buf; g_stamp_items = items; }
// Which launch forms ran (librevo_exp.so only, revo_debug_gemm_forms): the plans' form bits, nothing on the device.
static unsigned g_forms = 0;
unsigned gemm_debug_forms(int reset) { const unsigned f = g_forms; if (reset) g_forms = 0; return f; }
#endif

static const char* check_args(const GemmArgs& a) {
    if (const char* e = gemm_shape_error(a.M, a.N, a.K, a.lda, a.ldb, a.ldc)) return e;
    if (((uintptr_t)a.A | (uintptr_t)a.B | (uintptr_t)a.C) & 15) return "gemm: operands must be 16-byte aligned";
    return nullptr;
}

bool gemm_resid_folds(int M, int N, int K, long lda, long ldb, long ldc) {
    GemmProblem p{};
    p.epi = EPI_RESID_F32; p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
    p.fold_offered = true;
    const GemmPlan pl = gemm_plan(p, g_knobs);
    return !pl.error && pl.step[0].fold;
}

// the persistent kernels (gemm256p_kernel: 256- or 192-row tiles, one instantiation per plane format pair XP)
template <int EPI, int BMR>
static int launch_256p(GemmArgs& b, const GemmStep& s, hipStream_t st) {
    int nslot = s.nslot;
#ifdef REVO_EXPERIMENTS
    b.stagger_cycles = g_knobs.stagger_cycles; b.stagger_groups = g_knobs.stagger_groups;
    b.stamps = g_stamps; b.stamp_items = g_stamp_items;
    // (burst-size study, scripts/experiments/r5_gemm_half_chip.py: fewer persistent workgroups per XCD)
    if (const char* e = getenv("REVO_GEMM_NSLOT")) { const int v = atoi(e); if (v >= 1 && v < nslot) nslot = v; }
    {
        // phase groups (gemm256pp_kernel), forced by scripts/gemm_phase_ab.py only; the stamps live in that kernel too
        // (one group = every workgroup in step)
        int groups = g_knobs.phase_groups > 1 ? g_knobs.phase_groups : 1;
        if (BMR != 256 && groups > 3) groups = 3;
        if (groups > 1 || b.stamps != nullptr) {
            REVO_FUNC_LDS((gemm256pp_kernel<EPI, BMR>), G256P_LDS);
            hipLaunchKernelGGL((gemm256pp_kernel<EPI, BMR>), dim3(8 * nslot), dim3(G256_THREADS), G256P_LDS, st, b, nslot, groups);
            return 0;
        }
    }
#endif
    if constexpr (EPI == EPI_RESID_F32) {
        // the residual stream in planes: one kernel instantiation per format pair (gemm256_epilogue, XP)
#define REVO_LAUNCH_XP(X)                                                                                              \
    case X:                                                                                                             \
        REVO_FUNC_LDS((gemm256p_kernel<EPI, BMR, X>), G256P_LDS);                                                       \
        hipLaunchKernelGGL((gemm256p_kernel<EPI, BMR, X>), dim3(8 * nslot), dim3(G256_THREADS), G256P_LDS, st, b, nslot); \
        return 0;
        switch (s.xp) { REVO_LAUNCH_XP(1) REVO_LAUNCH_XP(2) REVO_LAUNCH_XP(3) default: break; }
#undef REVO_LAUNCH_XP
    }
    REVO_FUNC_LDS((gemm256p_kernel<EPI, BMR>), G256P_LDS);
    hipLaunchKernelGGL((gemm256p_kernel<EPI, BMR>), dim3(8 * nslot), dim3(G256_THREADS), G256P_LDS, st, b, nslot);
    return 0;
}

template <int EPI, int DBG>
static int launch_256d(const GemmArgs& b, const GemmStep& s, hipStream_t st) {
    REVO_FUNC_LDS((gemm256_kernel<EPI, DBG>), G256_LDS_LN);
    hipLaunchKernelGGL((gemm256_kernel<EPI, DBG>), dim3(s.grid_x), dim3(G256_THREADS), G256_LDS_LN, st, b);
    return 0;
}

// The split-K forms (EPI_RESID_F32): the ring kernel or the 256 x 256 kernel on S parts of K into fp32 planes of the
// workspace, then the reduce -- which also normalises the new rows when the step says so.
static int launch_splitk(const GemmArgs& b, const GemmStep& s, hipStream_t st) {
    const long plane = (long)b.M * b.N;
    GemmArgs c = b;
    c.C = b.ws; c.ldc = b.N; c.bias = nullptr; c.gamma = nullptr;
    c.ksplit = s.S; c.c_split_stride = plane;
    if (s.form == GF_SPLITK_256) {
        REVO_FUNC_LDS((gemm256_kernel<EPI_F32, 4>), G256_LDS);
        hipLaunchKernelGGL((gemm256_kernel<EPI_F32, 4>), dim3(s.grid_x, s.grid_y), dim3(G256_THREADS), G256_LDS, st, c);
    } else {
        constexpr int LDS = G128R_NST * (128 + 64) * 128;
        REVO_FUNC_LDS((gemm128r_kernel<EPI_F32>), LDS);
        hipLaunchKernelGGL((gemm128r_kernel<EPI_F32>), dim3(s.grid_x, s.grid_y), dim3(GEMM_THREADS), LDS, st, c);
    }
    REVO_HIP_CHECK(hipGetLastError());
    if (s.reduce_ln) {
        const dim3 grid((unsigned)((b.M + 3) / 4));
        const int groups = (b.N / 8 + 63) / 64;
#define RLN_LAUNCH(G) hipLaunchKernelGGL((splitk_reduce_resid_ln_kernel<G>), grid, dim3(256), 0, st, b.ws, s.S, plane, b.M, b.N, b.bias, \
                                         b.gamma, (float*)b.C, b.ldc, b.ln_w, b.ln_b, b.ln_eps, b.ln_out, b.ln_ldo)
        if (groups <= 1) RLN_LAUNCH(1);
        else if (groups <= 2) RLN_LAUNCH(2);
        else if (groups <= 3) RLN_LAUNCH(3);
        else RLN_LAUNCH(4);
#undef RLN_LAUNCH
        return 0;
    }
    const long quads = plane / 4;
    hipLaunchKernelGGL(splitk_reduce_resid_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, st, b.ws, s.S, plane,
                       b.M, b.N, b.bias, b.gamma, (float*)b.C, b.ldc);
    return 0;
}

// One step of a plan: the caller's arguments on the step's rows, the fields the launcher owns filled from the step.  The
// folded producer's outputs and the planes reach only the step that carries them.
template <int EPI>
static int run_step(const GemmArgs& a, const GemmStep& s, hipStream_t st) {
    constexpr bool BF16 = EPI == EPI_BF16 || EPI == EPI_BF16_GELU;
    GemmArgs b = a;
    b.M = s.rows;
    b.A = a.A + (long)s.row0 * a.lda;
    b.C = (char*)a.C + (long)s.row0 * a.ldc * (BF16 ? 2 : 4);
    if (b.lnc_stats) b.lnc_stats += (long)s.row0 * a.lnc_parts;
    b.gy = s.gy; b.t192_tiles = s.t192_tiles; b.t192_tall = s.t192_tall; b.qtail_rows = s.qtail_rows;
    if (!s.fold) { b.lnf_xb = nullptr; b.lnf_stats = nullptr; }
    if (!s.xp) b.xp_in = b.xp_out = 0;
    switch (s.form) {
        case GF_SKINNY_444:
        case GF_SKINNY_411:
            if (s.form == GF_SKINNY_444) hipLaunchKernelGGL((gemm_skinny_kernel<EPI, 4, 4, 4>), dim3(s.grid_x, s.grid_y), dim3(256), 0, st, b);
            else hipLaunchKernelGGL((gemm_skinny_kernel<EPI, 4, 1, 1>), dim3(s.grid_x), dim3(256), 0, st, b);
            break;
        case GF_128_128:
            REVO_FUNC_LDS((gemm128_kernel<EPI, 128>), 2 * (128 + 128) * 128);
            hipLaunchKernelGGL((gemm128_kernel<EPI, 128>), dim3(s.grid_x), dim3(GEMM_THREADS), 2 * (128 + 128) * 128, st, b);
            break;
        case GF_128_64:
            hipLaunchKernelGGL((gemm128_kernel<EPI, 64>), dim3(s.grid_x), dim3(GEMM_THREADS), 2 * (128 + 64) * 128, st, b);
            break;
        case GF_128R: {
            constexpr int LDS = G128R_NST * (128 + 64) * 128;
            REVO_FUNC_LDS((gemm128r_kernel<EPI>), LDS);
            hipLaunchKernelGGL((gemm128r_kernel<EPI>), dim3(s.grid_x), dim3(GEMM_THREADS), LDS, st, b);
            break;
        }
        case GF_256_TILE:
#ifdef REVO_EXPERIMENTS
            if constexpr (EPI == EPI_BF16) {
                if (s.dbg == 1) return launch_256d<EPI_BF16, 1>(b, s, st);
                if (s.dbg == 2) return launch_256d<EPI_BF16, 2>(b, s, st);
                if (s.dbg) return launch_256d<EPI_BF16, 3>(b, s, st);
            }
#endif
            return launch_256d<EPI, 0>(b, s, st);
        case GF_256P:
            return launch_256p<EPI, 256>(b, s, st);
        case GF_256P_192:
            if constexpr (EPI == EPI_RESID_F32) return launch_256p<EPI, 192>(b, s, st);
            return -3;
        case GF_256Q:
        case GF_256Q_QTAIL:
            if constexpr (BF16 || (EPI == EPI_BF16_ROPE && G256Q_ROPE_BUILT)) {
#ifdef REVO_EXPERIMENTS
                b.stamps = g_stamps; b.stamp_items = g_stamp_items;
                b.stagger_cycles = 0;
                b.stagger_groups = ((g_knobs.qstores & 7) == 2 ? 0x100 : 0)        // 2: the stores are issued but dropped (timing only)
                                   | ((g_knobs.qstores & 8) ? 0x200 : 0);          // + 8: stamp item 2 = shader-clock cycles of the main loop (its clock)
#endif
                REVO_FUNC_LDS((gemm256q_kernel<EPI>), G256Q_LDS);
                hipLaunchKernelGGL((gemm256q_kernel<EPI>), dim3(8 * s.nslot), dim3(G256_THREADS), G256Q_LDS, st, b, s.nslot);
                break;
            }
            return -3;
        case GF_SPLITK_RING:
        case GF_SPLITK_RING_LN:
        case GF_SPLITK_256:
            if constexpr (EPI == EPI_RESID_F32) return launch_splitk(b, s, st);
            return -3;
        default:
            return -3;
    }
    return 0;
}

template <int EPI>
static int run_plan(const GemmArgs& a, const GemmPlan& pl, hipStream_t st) {
    for (int i = 0; i < pl.nsteps; ++i) {
        const int rc = run_step<EPI>(a, pl.step[i], st);
        if (rc == -3) revo_set_error("gemm: internal: the plan names a form this epilogue does not have");
        if (rc) return rc;
        REVO_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

// Few rows against very many columns with a plain fp32 output (the search pre-pass of up to 128 queries): 128 x 64 tiles
// on the six-deep ring, a round or two of workgroups whose K loops keep five steps of loads in flight (one 256 x 256 tile
// per CU is a chain of sixteen DMA latencies).
int launch_gemm_f32_ring(const GemmArgs& a, hipStream_t st) {
    if (const char* e = check_args(a)) {
        revo_set_error(e);
        return -2;
    }
    REVO_REQUIRE(a.N % 64 == 0 && a.K % 64 == 0, "gemm ring: N and K must be multiples of 64");
    const int tiles64 = ((a.M + 127) / 128) * ((a.N + 63) / 64);
    constexpr int LDS = G128R_NST * (128 + 64) * 128;
    REVO_FUNC_LDS((gemm128r_kernel<EPI_F32>), LDS);
    GemmArgs b = a;
    b.ksplit = 1;
    hipLaunchKernelGGL((gemm128r_kernel<EPI_F32>), dim3(tiles64), dim3(GEMM_THREADS), LDS, st, b);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_gemm(int epi, const GemmArgs& a, hipStream_t st) {
    if (const char* e = check_args(a)) {
        revo_set_error(e);
        return -2;
    }
    if (a.lnc_stats && (!a.lnc_c || a.lnc_parts < 1 || a.lnc_parts > 6 || (epi != EPI_BF16 && epi != EPI_BF16_GELU && epi != EPI_BF16_ROPE))) {
        revo_set_error("gemm: a folded LayerNorm (lnc_*) needs a bf16 epilogue, the column sums and 1..6 statistics slots per row");
        return -2;
    }
    if (epi == EPI_BF16_ROPE && (!a.rope_cs || a.rope_S <= 0 || a.rope_hd <= 0 || a.rope_hd % 8 || a.rope_cols % a.rope_hd || a.rope_cols > a.N)) {
        revo_set_error("gemm: the RoPE epilogue needs a table, rope_hd % 8 == 0 and rope_cols a multiple of rope_hd");
        return -2;
    }
    const GemmPlan pl = gemm_plan(gemm_problem(epi, a), g_knobs);
    if (pl.error) {
        revo_set_error(pl.error);
        return -2;
    }
    int rc;
    switch (epi) {
        case EPI_BF16: rc = run_plan<EPI_BF16>(a, pl, st); break;
        case EPI_BF16_GELU: rc = run_plan<EPI_BF16_GELU>(a, pl, st); break;
        case EPI_RESID_F32: rc = run_plan<EPI_RESID_F32>(a, pl, st); break;
        case EPI_F32: rc = run_plan<EPI_F32>(a, pl, st); break;
        case EPI_PATCH: rc = run_plan<EPI_PATCH>(a, pl, st); break;
        case EPI_BF16_ROPE: rc = run_plan<EPI_BF16_ROPE>(a, pl, st); break;
        default: revo_set_error("gemm: unknown epilogue"); return -2;
    }
    if (rc) return rc;
    // what the plan did for the caller, only once every launch was accepted
    if (pl.step[0].fold) *a.lnf_done = 1;
    if (pl.step[0].reduce_ln) *a.ln_fused = 1;
#ifdef REVO_EXPERIMENTS
    g_forms |= pl.forms;
#endif
    return 0;
}

#ifdef REVO_EXPERIMENTS
long gemm_debug_plan(int epi, int M, int N, int K, long lda, long ldb, long ldc, long ws_elems, unsigned offers, int rope_S,
                     int rope_hd, int rope_cols, long* out, int cap) {
    GemmProblem p{};
    p.epi = epi; p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc; p.ws_elems = ws_elems;
    p.ln_offered = offers & 1; p.ln_ldo = ldc;
    p.fold_offered = offers & 2; p.lnf_ldxb = ldc;
    p.xp_in = (offers >> 2) & 1; p.xp_out = (offers >> 3) & 1; p.planes_valid = true;
    p.lnc = offers & 16; p.prefer256 = (offers >> 5) & 1;
    p.rope_S = rope_S; p.rope_hd = rope_hd; p.rope_cols = rope_cols;
    const GemmPlan pl = gemm_plan(p, g_knobs);
    constexpr int PER_STEP = 14;
    if (cap < 2 + 2 * PER_STEP) return -2;
    out[0] = pl.error ? -1 : (long)pl.forms;
    out[1] = pl.error ? 0 : pl.nsteps;
    for (int i = 0; i < out[1]; ++i) {
        const GemmStep& s = pl.step[i];
        const long v[PER_STEP] = {(long)s.form, s.row0, s.rows, s.gy, s.nslot, s.grid_x, s.grid_y, s.t192_tiles, s.t192_tall, s.qtail_rows,
                                  s.S, s.reduce_ln, s.xp, s.fold};
        for (int j = 0; j < PER_STEP; ++j) out[2 + i * PER_STEP + j] = v[j];
    }
    return out[0];
}
#endif

}  // namespace revo
