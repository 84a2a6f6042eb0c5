// Body of topk_scan256_kernel (S256_FILTER 0) and topk_scan256_filtered_kernel (S256_FILTER 1), topk256.hip.  Included
// inside the kernels' braces rather than shared as an inlined __device__ function: the plain forms sit at the 256-VGPR limit,
// and an inlined body is optimised in a different order -- it moved their spill counts (tests/test_kernel_register_budget.py).
// This way the plain kernels compile from exactly the code they had before the filtered form existed.

    constexpr int SEG = 2 * KSEL;
    // up to 128 queries the loop runs at the HBM rate: operands are requested a K-tile and a half ahead (gemm256_core.h)
    constexpr bool DEEP = ROWS == 64 || ROWS == 128;
    // ROWS != 0: the whole search is ONE query tile, so every gallery row is read by one workgroup, once: non-temporal DMA
    // (measured, 1 M x 1024, whole search: 1 query 0.416-0.427 -> 0.400-0.401 ms, 64 queries 0.441-0.451 -> 0.427-0.431,
    //  128 queries 0.521 -> 0.493-0.499; the bytes no longer push the queries, bounds and segments out of L2 / the Infinity Cache).
    //  With several query tiles the workgroups of an XCD that hold the same slice re-read it from L2: default policy.
#ifndef S256_ONE_TILE_AUX
#define S256_ONE_TILE_AUX 2
#endif
    constexpr int BAUX = ROWS != 0 ? S256_ONE_TILE_AUX : 0;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    S256Lds L;
    L.queue = (uint64_t*)(smem + G256_LDS);
    L.stage = (uint64_t*)(smem + S256_STG_OFF);
    L.tau = (float*)(smem + S256_TAU_OFF);
    L.base = (uint32_t*)(L.tau + 256);
    L.start = (int*)(L.base + 256);
    L.end = L.start + 256;
    L.cnt = L.end + 256;
    L.ctrl = L.cnt + 256;
    L.scratch = (uint64_t*)(L.ctrl + 16);
    L.wkey = L.scratch + 8 * 128;
    static_assert(S256_CNT_OFF == S256_TAU_OFF + (256 + 256 + 256 + 256) * 4, "cnt follows tau, base, start, end");
    static_assert(S256_WKEY_OFF + 256 * 8 == S256_LDS, "wkey is the last block");

#ifndef REVO_EXPERIMENTS
    // the product build has no timing switches and no counters: these fold to constants
    p.dbg = 0;
    p.stats = nullptr;
#endif
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int lane = tid & 63;
    // 1-D grid in phases: block b of phase i (scalar compares against the phases' first blocks) -> local j = b - first[i],
    // query tile q0[i] + j % qn[i], slice j / qn[i] of ns[i].  Blocks are dealt to the 8 XCDs round-robin and every phase
    // starts at a multiple of 8, so in a phase of 8 a query tiles all slices of a query tile run on one XCD (shared L2:
    // histograms, query rows) and the a workgroups that hold the same slice of the XCD's a query tiles stream the same
    // gallery rows side by side.
    // (constant indices only: a run-time index into the by-value argument block makes hipcc copy it to scratch)
    int ph_first = p.ph_first[0], ph_q0 = p.ph_q0[0], ph_qn = p.ph_qn[0], nsl = p.ph_ns[0];
#pragma unroll
    for (int i = 1; i < S256_PHASES; ++i)
        if (i < p.nph && (int)blockIdx.x >= p.ph_first[i]) { ph_first = p.ph_first[i]; ph_q0 = p.ph_q0[i]; ph_qn = p.ph_qn[i]; nsl = p.ph_ns[i]; }
    const int jloc = (int)blockIdx.x - ph_first;
    // (an integer division is a vector-unit sequence: its wave-uniform results are moved to scalar registers here, or the
    //  slice bounds derived from them sit in vector registers across the main loop -- at the 256-register limit, in scratch)
    const int sp = __builtin_amdgcn_readfirstlane(jloc / ph_qn);
    const int qtile = ph_q0 + (jloc - sp * ph_qn);
    const int q0 = qtile * 256;
    if (q0 >= p.Q) return;
    const int qvalid = (p.Q - q0) < 256 ? (p.Q - q0) : 256;

    // slices: the tiles are dealt out as evenly as possible (the first `rem` slices take one more)
    const long span = p.N - p.n_begin;
    const long tiles = (span + 255) / 256;
    // (32-bit and scalar: tiles < 2^24; the hardware has no scalar 64-bit order compare, so as `long` these bounds lived in
    //  vector registers across the main loop)
    const int per = __builtin_amdgcn_readfirstlane((int)tiles / nsl), rem = (int)tiles - per * nsl;
    const int t0 = sp * per + (sp < rem ? sp : rem);
    const int t1 = t0 + per + (sp < rem ? 1 : 0);
    const long row_begin = p.n_begin + (long)t0 * 256;            // first gallery row of this slice
    const uint32_t idx_base = (uint32_t)row_begin;
    const long seg_row_stride = (long)p.splits * SEG;
    uint64_t* myseg = p.seg + ((long)q0 * p.splits + sp) * SEG;      // row r of the tile: + r * seg_row_stride
    uint32_t* myhist = p.hist + (long)q0 * S256_NB;

    if (tid < 256) {
        const uint32_t b0 = tid < qvalid ? p.tau_base[q0 + tid] : 0u;
        float t0_ = tid < qvalid ? orderable_f32(p.tau_g[q0 + tid]) : INFINITY;
        if constexpr (MARGIN) { if (tid < qvalid) t0_ = s256_admit(t0_, b0, p.marg[q0 + tid]); }
        L.tau[tid] = t0_;
        L.base[tid] = b0;
        L.wkey[tid] = 0ull;
        L.cnt[tid] = 0;
    }
    if (tid == 0) { L.ctrl[0] = 0; L.ctrl[1] = 0; }
    __syncthreads();
    // (phases differ in their slice counts: a query's slots beyond its phase's slices are closed by slice 0)
    if (sp == 0 && tid < qvalid)
        for (int s2 = nsl; s2 < p.splits; ++s2) p.seg_cnt[(long)(q0 + tid) * p.splits + s2] = 0;
    if (t0 >= t1) {
        if (tid < qvalid) p.seg_cnt[(long)(q0 + tid) * p.splits + sp] = 0;
        return;
    }

    G256Operand A, B;
    g256_operand_init(A, p.Qb, p.ldq, p.Q, q0, wave, lane);
    g256_operand_init(B, p.Gb + row_begin * p.ldg, p.ldg, p.N - row_begin, 0, wave, lane);
    if constexpr (DEEP) g256_issue_prologue_deep<BAUX>(A, B, smem, p.D, wave); else g256_issue_prologue<BAUX>(A, B, smem, p.D, wave);
    // FILTER: the allow-bits of the tile whose operands were requested last (fm_pend) and of the tile being selected (fm_cur)
#if S256_FILTER
    uint64_t fm_pend = 0ull;
#endif
#if S256_FILTER
    fm_pend = s256_allow_word(p.allow, row_begin + (wave & 3) * 64);
#endif
    // Slices that start after others have run (later rounds of workgroups on this CU) begin with what those have
    // learnt, not with the pre-pass bound: one refresh while the first operands are in flight.  (Without it every
    // slice's first tile admitted about one score per row: at 24 tiles per slice a third of all slow fragments.)
    if (!(p.dbg & 17)) {
        if (p.stats && tid == 0) atomicAdd(p.stats + 5, 1ull);
        s256_refresh_hist<KSEL, MARGIN>(L, p.hist, p.tau_g, q0, qvalid, tid, MARGIN ? p.marg : nullptr);
    }

    // Normal mode: one pass per tile (groups == 1).  If a pass pushes more entries to the overflow queue than
    // it holds, or stages more survivors than the staging buffer holds (an adversarially ordered gallery), the tile
    // is recomputed in 2, 4, ... 64 column groups, one pass and one drain per group; at 64 groups a pass can
    // admit at most 256 x 4 = 1024 entries, so the retry always terminates.  Entries found twice are dropped when lists are merged (drain, final reduce).
    int t = t0;
    int groups = 1, grp = 0;
    uint32_t staged_before = 0;            // survivors staged by earlier passes (the LDS total is never reset)
    while (t < t1) {
        const long n0 = p.n_begin + (long)t * 256;
#if S256_FILTER
        const uint64_t fm_cur = fm_pend;
#endif
        {
            f32x4 acc[8][4];
#pragma unroll
            for (int m = 0; m < 8; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
            // few queries: most of the tile's MFMA work would multiply zero rows (separate kernel
            // instantiations: inside one kernel a second main loop costs the main path its register allocation)
            gemm256_mainloop<ROWS, false, DEEP, 0, BAUX>(A, B, smem, p.D, wave, lane, acc);

            if (groups == 1 && t + 1 < t1) {
                // next gallery tile: rebased descriptors (any gallery size), DMA in flight during the selection
                g256_operand_init(B, p.Gb + (n0 + 256) * p.ldg, p.ldg, p.N - (n0 + 256), 0, wave, lane);
                if constexpr (DEEP) g256_issue_prologue_deep<BAUX>(A, B, smem, p.D, wave); else g256_issue_prologue<BAUX>(A, B, smem, p.D, wave);
#if S256_FILTER
                fm_pend = s256_allow_word(p.allow, n0 + 256 + (wave & 3) * 64);
#endif
            }
            asm volatile("" : "+v"(lane) :: "memory");
            const int lr = lane & 15, lq = lane >> 4;
            const int rbase = (wave >> 2) * 128 + lr;            // + m * 16
            const int cbase = (wave & 3) * 64 + lq * 4;          // + n * 16 + j
            const long left = p.N - n0;
            const uint32_t rel0 = (uint32_t)(n0 - row_begin);
            float taum[8];
            unsigned hitm = 0;             // bit m: some lane of this wave has a candidate in row fragment m
            if (left < 256) {
                // the gallery's last, ragged tile: columns past the end become NaN (never admitted, ignored by
                // fmaxf).  One uniform branch per tile; inside the loops below the same test cost two scalar
                // instructions and a branch per score.
#pragma unroll
                for (int n = 0; n < 4; ++n)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool past = cbase + n * 16 + j >= left;
#pragma unroll
                        for (int m = 0; m < 8; ++m) acc[m][n][j] = past ? __builtin_nanf("") : acc[m][n][j];
                    }
            }
#if S256_FILTER
            s256_apply_allow(acc, fm_cur, lq);
#endif
            if (p.dbg & 1) {
                asm volatile("" :: "v"(acc[0][0]), "v"(acc[7][3]));
            } else {
#pragma unroll
                for (int m = 0; m < 8; ++m) taum[m] = s256_lds_f32(S256_TAU_OFF + (rbase + m * 16) * 4);
#pragma unroll
                for (int m = 0; m < 8; ++m) {
                    float mx = -INFINITY;
#pragma unroll
                    for (int n = 0; n < 4; ++n)
#pragma unroll
                        for (int j = 0; j < 4; ++j) mx = fmaxf(mx, acc[m][n][j]);
                    if (__ballot(mx >= taum[m]) != 0ull) hitm |= 1u << m;
                }
            }
            if (hitm && !(p.dbg & 4)) {
#pragma unroll
                for (int m = 0; m < 8; ++m) {
                    if (!(hitm & (1u << m))) continue;          // wave-uniform
                    if (p.stats && lane == 0) atomicAdd(p.stats + 3, 1ull);
                    const int row = rbase + m * 16;
                    // the row's KSEL-th best as of its last drain, as (score, index); none yet admits everything
                    const uint64_t wk = s256_lds_u64(S256_WKEY_OFF + row * 8);
                    const float ws = wk ? key_score(wk) : -INFINITY;
                    const uint32_t widx = wk ? key_index(wk) : 0xffffffffu;
#pragma unroll
                    for (int n = 0; n < 4; ++n)
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float v = acc[m][n][j];
                            const int col = cbase + n * 16 + j;
                            // admission score (shared across slices) first, then the strict test against the
                            // row's own KSEL-th entry: an equal score enters only with a smaller index, so a
                            // huge tie group cannot keep the queue full forever.  Survivors are rare: each lane
                            // stages its own (row | score | index) in LDS under a mostly empty exec mask; nothing
                            // here touches global memory.
                            const bool pass = v >= taum[m];
                            if (__ballot(pass) == 0ull) continue;       // wave-uniform: most elements of a hit fragment fail too
                            if (pass && (col & (groups - 1)) == grp &&
                                (v > ws || (v == ws && idx_base + rel0 + col < widx))) {
                                const uint32_t pos = (uint32_t)s256_lds_inc(S256_CTRL_OFF + 4) - staged_before;
                                if (pos < (uint32_t)S256_STG) s256_lds_store64(S256_STG_OFF + pos * 8, s256_entry(row, v, rel0 + col));
                            }
                        }
                }
            }
        }
        // the accumulators are dead from here on (refresh and drain are real calls)
        s256_barrier_lds();
        // Flush.  The pass's survivors sit in the staging buffer; thread i moves entry i to its row's segment in
        // global memory (slot from the row's LDS counter) and counts it in the query's histogram.  A tile has a few
        // dozen survivors, so a wave issues at most ONE store and ONE atomic instruction per tile, and those fit
        // inside the four vector-memory operations the next main loop's first wait leaves outstanding anyway.
        // (Placed by the lane that found them, 2 x 7 operations per wave and tile were in flight at that wait, and it
        //  -- and then the whole workgroup at the barrier behind it -- sat there until they had been acknowledged.)
        const uint32_t staged_total = s256_lds_u32(S256_CTRL_OFF + 4);
        const uint32_t staged = staged_total - staged_before;
        staged_before = staged_total;
        {
            const uint32_t nst = staged < (uint32_t)S256_STG ? staged : (uint32_t)S256_STG;
            for (uint32_t i = tid; i < nst; i += 512) {
                const uint64_t e = s256_lds_u64(S256_STG_OFF + i * 8);
                const int row = (int)(e >> 56);
                const int slot = s256_lds_inc(S256_CNT_OFF + row * 4);
                if (slot < SEG) {
                    if (!(p.dbg & 8)) {
                        myseg[(long)row * seg_row_stride + slot] = s256_entry_to_key(e, idx_base);
                        const uint32_t so = (uint32_t)(e >> 24), bo = s256_lds_u32(S256_BASE_OFF + row * 4);
                        if (groups == 1 && (!MARGIN || so >= bo)) {   // a recomputed tile must not be counted twice; a score
                                                               // admitted by the margin only may lie below the histogram's origin
                            uint32_t b = (so - bo) >> S256_SH;
                            b = b < (uint32_t)(S256_NB - 1) ? b : (uint32_t)(S256_NB - 1);
                            (void)__hip_atomic_fetch_add(myhist + (long)row * S256_NB + b, 1u, __ATOMIC_RELAXED, S256_HIST_SCOPE);
                        }
                    }
                    if (p.stats) atomicAdd(p.stats + 4, 1ull);
                } else {
                    const int pos = s256_lds_inc(S256_CTRL_OFF);
                    if (pos < S256_QCAP) s256_lds_store64(G256_LDS + pos * 8, e);
                }
            }
        }
        s256_barrier_lds();
        const int qc = (int)s256_lds_u32(S256_CTRL_OFF);
        const bool overflow = qc > S256_QCAP || staged > (uint32_t)S256_STG;
        if (p.stats && tid == 0) {
            if (overflow || groups > 1) atomicAdd(p.stats + 2, 1ull);
            if (overflow || groups > 1 || qc >= S256_DRAIN || (t + 1 >= t1 && qc > 0)) { atomicAdd(p.stats + 0, 1ull); atomicAdd(p.stats + 1, (unsigned long long)qc); }
        }
        if (groups == 1 && !overflow) {
            if (qc >= S256_DRAIN || (t + 1 >= t1 && qc > 0))
                s256_drain<KSEL, MARGIN>(L, myseg, seg_row_stride, q0, qvalid, idx_base, tid, p.tau_g, MARGIN ? p.marg : nullptr, MARGIN ? p.dropflag : nullptr);
            // what all slices of these queries have learnt meanwhile: after the first two tiles (the bound moves
            // fastest early on: it follows KSEL / rows seen), then every fourth tile, every 16th from tile 32 on
            // (each refresh is an L2 round trip plus ~3 us of wave scans)
            const int tl = t - t0;
            if (t + 1 < t1 && !(p.dbg & 17) && (tl < 2 || ((tl & 3) == 3 && tl < 32) || (tl & 15) == 15)) {
                if (p.stats && tid == 0) atomicAdd(p.stats + 5, 1ull);
                s256_refresh_hist<KSEL, MARGIN>(L, p.hist, p.tau_g, q0, qvalid, tid, MARGIN ? p.marg : nullptr);
            }
            ++t;
            continue;
        }
        // retry mode (or entering it): merge what was queued, then recompute this tile / its next column group
        s256_drain<KSEL, MARGIN>(L, myseg, seg_row_stride, q0, qvalid, idx_base, tid, p.tau_g, MARGIN ? p.marg : nullptr, MARGIN ? p.dropflag : nullptr);
        // a recomputed tile appends its survivors a second time: these queries' segments may hold repeated keys
        if constexpr (MARGIN) { if (tid < qvalid) p.dropflag[q0 + tid] = 1; }
        if (overflow) {
            groups = groups < S256_MAXGROUPS ? groups * 2 : S256_MAXGROUPS;
            grp = 0;
        } else if (++grp == groups) {
            groups = 1;
            grp = 0;
            ++t;                                                  // tile complete
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // a DMA issued for another tile must not land on top
        __syncthreads();
        if (t < t1) {
            const long nn = p.n_begin + (long)t * 256;
            g256_operand_init(B, p.Gb + nn * p.ldg, p.ldg, p.N - nn, 0, wave, lane);
            if constexpr (DEEP) g256_issue_prologue_deep<BAUX>(A, B, smem, p.D, wave); else g256_issue_prologue<BAUX>(A, B, smem, p.D, wave);
#if S256_FILTER
            fm_pend = s256_allow_word(p.allow, nn + (wave & 3) * 64);
#endif
        }
    }
    if (tid < qvalid) {
        const int c = L.cnt[tid];
        p.seg_cnt[(long)(q0 + tid) * p.splits + sp] = c < SEG ? c : SEG;
    }
