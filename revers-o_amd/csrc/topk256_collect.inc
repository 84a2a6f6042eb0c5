// Body of topk_collect256_kernel (C256_FILTER 0) and topk_collect256_filtered_kernel (C256_FILTER 1), topk256.hip:
// included inside the kernels' braces, so that the plain kernels compile from exactly the code they had before (the same
// reason as topk256_scan.inc).

    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* tau = (float*)(smem + C256_TAU_OFF);
    uint32_t* ctrl = (uint32_t*)(smem + C256_CTRL_OFF);
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int lane = tid & 63;
    const int nq = *p.n_q;
    // three instantiations are launched when the search has more than 64 queries; the entry count picks the one that
    // works: <= 64 entries run at the HBM rate (ROWS = 64), <= 128 nearly (ROWS = 128), more at the MFMA rate
    if (ROWS == 64 ? nq > 64 : (ROWS == 128 ? (nq <= 64 || nq > 128) : (nq <= 128 && p.small_modes))) return;
    const int sp = blockIdx.x;                              // one workgroup per gallery slice; it walks the query tiles
    const long tiles = (p.N + 255) / 256;
    const long per = tiles / p.splits, rem = tiles - per * p.splits;
    const long t0 = sp * per + (sp < rem ? sp : rem);
    const long t1 = t0 + per + (sp < rem ? 1 : 0);
    if (t0 >= t1) return;
    const long row_begin = t0 * 256;
    const uint32_t idx_base = (uint32_t)row_begin;
    for (int q0 = 0; q0 < nq; q0 += 256) {
    const int qvalid = (nq - q0) < 256 ? (nq - q0) : 256;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                        // the previous query tile's last reads of tau / the stage
    if (tid < 256) tau[tid] = tid < qvalid ? p.lb[q0 + tid] : INFINITY;
    if (tid == 0) ctrl[0] = 0u;
    __syncthreads();

    G256Operand A, B;
    g256_operand_init(A, p.Qb, p.ldq, nq, q0, wave, lane);
    g256_operand_init(B, p.Gb + row_begin * p.ldg, p.ldg, p.N - row_begin, 0, wave, lane);
    g256_issue_prologue(A, B, smem, p.D, wave);
#if C256_FILTER
    uint64_t fm_pend = 0ull;
#endif
#if C256_FILTER
    fm_pend = s256_allow_word(p.allow, row_begin + (wave & 3) * 64);
#endif

    long t = t0;
    int groups = 1, grp = 0;
    // column classes (col & 63: the finest level of the ladder) of the CURRENT tile whose survivors are already in the
    // lists.  A pass that did not overflow appends at once; when a later group of the same tile overflows and the
    // ladder deepens, the classes of the passes before it must not be appended again (the exact finish re-scores
    // every list entry and assumes each row appears once: a repeated row would take two places of a result).
    uint64_t done = 0;
    uint32_t staged_before = 0;
    while (t < t1) {
        const long n0 = t * 256;
#if C256_FILTER
        const uint64_t fm_cur = fm_pend;
#endif
        {
            f32x4 acc[8][4];
#pragma unroll
            for (int m = 0; m < 8; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
            gemm256_mainloop<ROWS>(A, B, smem, p.D, wave, lane, acc);
            if (groups == 1 && t + 1 < t1) {
                g256_operand_init(B, p.Gb + (n0 + 256) * p.ldg, p.ldg, p.N - (n0 + 256), 0, wave, lane);
                g256_issue_prologue(A, B, smem, p.D, wave);
#if C256_FILTER
                fm_pend = s256_allow_word(p.allow, n0 + 256 + (wave & 3) * 64);
#endif
            }
            asm volatile("" : "+v"(lane) :: "memory");
            const int lr = lane & 15, lq = lane >> 4;
            const int rbase = (wave >> 2) * 128 + lr;
            const int cbase = (wave & 3) * 64 + lq * 4;
            const long left = p.N - n0;
            const uint32_t rel0 = (uint32_t)(n0 - row_begin);
            if (left < 256) {
#pragma unroll
                for (int n = 0; n < 4; ++n)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool past = cbase + n * 16 + j >= left;
#pragma unroll
                        for (int m = 0; m < 8; ++m) acc[m][n][j] = past ? __builtin_nanf("") : acc[m][n][j];
                    }
            }
#if C256_FILTER
            s256_apply_allow(acc, fm_cur, lq);
#endif
            float taum[8];
            unsigned hitm = 0;
#pragma unroll
            for (int m = 0; m < 8; ++m) taum[m] = s256_lds_f32(C256_TAU_OFF + (rbase + m * 16) * 4);
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                float mx = -INFINITY;
#pragma unroll
                for (int n = 0; n < 4; ++n)
#pragma unroll
                    for (int j = 0; j < 4; ++j) mx = fmaxf(mx, acc[m][n][j]);
                if (__ballot(mx >= taum[m]) != 0ull) hitm |= 1u << m;
            }
            if (hitm) {
#pragma unroll
                for (int m = 0; m < 8; ++m) {
                    if (!(hitm & (1u << m))) continue;          // wave-uniform
                    const int row = rbase + m * 16;
#pragma unroll
                    for (int n = 0; n < 4; ++n)
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float v = acc[m][n][j];
                            const int col = cbase + n * 16 + j;
                            const bool pass = v >= taum[m];
                            if (__ballot(pass) == 0ull) continue;
                            if (pass && (col & (groups - 1)) == grp && !((done >> (col & 63)) & 1ull)) {
                                const uint32_t pos = (uint32_t)s256_lds_inc(C256_CTRL_OFF) - staged_before;
                                if (pos < (uint32_t)S256_STG) s256_lds_store64(C256_STG_OFF + pos * 8, s256_entry(row, v, rel0 + col));
                            }
                        }
                }
            }
        }
        s256_barrier_lds();
        const uint32_t staged_total = s256_lds_u32(C256_CTRL_OFF);
        const uint32_t staged = staged_total - staged_before;
        staged_before = staged_total;
        const bool overflow = staged > (uint32_t)S256_STG;
        if (!overflow) {
            for (uint32_t i = tid; i < staged; i += 512) {
                const uint64_t e = s256_lds_u64(C256_STG_OFF + i * 8);
                const int row = (int)(e >> 56);
                const int slot = atomicAdd(p.cnt + q0 + row, 1);
                if (slot < p.cap) p.col[(long)(q0 + row) * p.cap + slot] = s256_entry_to_key(e, idx_base);
            }
        }
        s256_barrier_lds();
        if (groups == 1 && !overflow) { ++t; continue; }
        if (overflow) {
            groups = groups < S256_MAXGROUPS ? groups * 2 : S256_MAXGROUPS;
            grp = 0;
        } else {
            done |= c256_class_mask(groups, grp);            // this pass's columns are in the lists now
            ++grp;
        }
        // the next group of the (possibly deeper) ladder that still has columns to append
        while (grp < groups && (c256_class_mask(groups, grp) & ~done) == 0ull) ++grp;
        if (grp == groups) {
            groups = 1;
            grp = 0;
            done = 0;
            ++t;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t < t1) {
            const long nn = t * 256;
            g256_operand_init(B, p.Gb + nn * p.ldg, p.ldg, p.N - nn, 0, wave, lane);
            g256_issue_prologue(A, B, smem, p.D, wave);
#if C256_FILTER
            fm_pend = s256_allow_word(p.allow, nn + (wave & 3) * 64);
#endif
        }
    }
    }
