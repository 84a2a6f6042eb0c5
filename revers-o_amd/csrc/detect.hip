// Text-prompted regions (revo_vit_detect, include/revo.h DETECT): the kernels behind the token vectors.
//
//   scores   one wave per (cell, four prompts): the fp32 chain of every re-score in this library (topk_util.h exact_dot4) over
//            the cell's token vector and the normalised prompt -> s[b][p][c]
//   regions  one workgroup per image, the g x g <= 1024 cells in LDS: the label of every cell (best prompt, ties to the lowest,
//            NaN never wins, background and threshold cut), connected components by min-label propagation with pointer
//            jumping (every loop has a trip limit; one that is hit sets the error word), the components' attributes reduced with
//            LDS atomics, the kept components ranked by a count of comparisons, the best max_regions emitted with their bitmaps
//            into the image's slots of a staging area, the image's count
//   compact  the images' slots -> consecutive result rows, images ascending
#include "kernels.h"
#include "topk_util.h"

namespace revo {

// ------------------------------------------------------------------------ scores ----
// Item i = (row r, prompt group q): r = i / groups, q = i % groups.  Row r is cell r % cells of image r / cells, token
// cls + r % cells of the image's S token rows.  A lane u < m leaves with prompt 4 q + u's score (loads past m repeat the last
// prompt).  fmaf's product commutes: the bits revo_search_range gives prompt p against a gallery row equal to the token row.
__global__ __launch_bounds__(256) void detect_scores_kernel(const float* __restrict__ tok, long ldt, int S, int cls, int cells,
                                                            long rows, const float* __restrict__ prompts, int P, int D,
                                                            float* __restrict__ scores) {
    const int lane = threadIdx.x & 63;
    const long groups = (P + 3) / 4, items = rows * groups, waves = (long)gridDim.x * 4;
    for (long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6); i < items; i += waves) {
        const long r = i / groups;
        const int q0 = (int)(i - r * groups) * 4;
        const int m = P - q0 < 4 ? P - q0 : 4;
        const long b = r / cells;
        const int c = (int)(r - b * cells);
        const float* tr = tok + (b * S + cls + c) * ldt;
        const float* gr[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) gr[u] = prompts + (long)(q0 + (u < m ? u : m - 1)) * D;
        float t[4];
        exact_dot4(tr, gr, D, lane, t);
        const float v = lane == 0 ? t[0] : (lane == 1 ? t[1] : (lane == 2 ? t[2] : t[3]));
        if (lane < m) scores[(b * P + q0 + lane) * cells + c] = v;
    }
}

int launch_detect_scores(const float* tok, long ldt, int S, int cls, int cells, long rows, const float* prompts, int P, int D,
                         float* scores, hipStream_t st) {
    REVO_REQUIRE(D >= 4 && D % 4 == 0 && ldt % 4 == 0, "detect_scores: dim must be a multiple of 4, rows 16-byte aligned");
    REVO_REQUIRE(P >= 1 && P <= DETECT_MAX_PROMPTS, "detect_scores: n_prompts must be in [1, 64]");
    if (rows <= 0) return 0;
    const long items = rows * ((P + 3) / 4), blocks = (items + 3) / 4;
    hipLaunchKernelGGL(detect_scores_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, st, tok, ldt, S, cls,
                       cells, rows, prompts, P, D, scores);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}

// ----------------------------------------------------------------------- regions ----
constexpr int DET_THREADS = 256;
constexpr int DET_JUMPS = 11;                 // pointer jumps of a cell per round (a chain of 1024 cells halves ten times)
// the kernel's LDS (static): labels, scores, parents, five attribute arrays, the confidences, the slots, the ranking keys
constexpr size_t DET_LDS = (size_t)DETECT_MAX_CELLS * (2 + 4 + 4 + 5 * 4 + 4 + 4 + 8) + 16;
static_assert(DET_LDS <= 64 * 1024, "the region kernel's LDS is static: under the 64 KiB a launch gets without opting in");
static_assert(DET_LDS <= 160 * 1024, "a CU has 160 KiB of LDS");

__device__ __forceinline__ int lds_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__global__ __launch_bounds__(DET_THREADS) void detect_regions_kernel(DetectRegionArgs p) {
    __shared__ short lab[DETECT_MAX_CELLS];
    __shared__ float sc[DETECT_MAX_CELLS];
    __shared__ int parent[DETECT_MAX_CELLS];
    __shared__ int cnt[DETECT_MAX_CELLS], bx0[DETECT_MAX_CELLS], by0[DETECT_MAX_CELLS], bx1[DETECT_MAX_CELLS], by1[DETECT_MAX_CELLS];
    __shared__ uint32_t conf[DETECT_MAX_CELLS];
    __shared__ int slot[DETECT_MAX_CELLS];
    __shared__ uint64_t keys[DETECT_MAX_CELLS];
    __shared__ int s_changed, s_nk;
    const int tid = threadIdx.x, b = blockIdx.x, g = p.g, G2 = g * g, P = p.P;
    const float* sb = p.scores + (long)b * P * G2;

    // labels: the prompt with the largest score (ties: the lowest prompt; -0 == +0; NaN never wins), cut by background and threshold
    for (int c = tid; c < G2; c += DET_THREADS) {
        int w = -1;
        float best = 0.f;
        for (int q = 0; q < P; ++q) {
            const float s = sb[(long)q * G2 + c];
            if (s == s && (w < 0 || s > best)) { w = q; best = s; }
        }
        int l = -1;
        if (w >= 0 && w < P - p.nbg && best >= p.thr[w]) l = w;
        lab[c] = (short)l; sc[c] = best; parent[c] = c;
        cnt[c] = 0; bx0[c] = g; by0[c] = g; bx1[c] = -1; by1[c] = -1; conf[c] = 0u; slot[c] = -1;
        if (p.labels) p.labels[(long)b * G2 + c] = l;
    }
    if (tid == 0) { s_changed = 0; s_nk = 0; }
    __syncthreads();

    // connected components: parent[c] <= c, always a cell of c's component.  A round lowers a cell (and the cell it points to)
    // to the smallest parent among its equal-label 4-neighbours, then jumps every pointer towards its root.  After round k a
    // cell's parent is at most the lowest cell within k steps of it, so G2 rounds always suffice; hooking and jumping make it
    // a few.  At the fixed point every cell of a component points to the component's lowest cell.
    bool done = false;
    for (int round = 0; round < G2 + 2; ++round) {
        bool ch = false;
        for (int c = tid; c < G2; c += DET_THREADS) {
            const int l = lab[c];
            if (l < 0) continue;
            const int y = c / g, x = c - y * g;
            const int pc = lds_load(&parent[c]);
            int m = pc, t;
            if (x > 0 && lab[c - 1] == l && (t = lds_load(&parent[c - 1])) < m) m = t;
            if (x + 1 < g && lab[c + 1] == l && (t = lds_load(&parent[c + 1])) < m) m = t;
            if (y > 0 && lab[c - g] == l && (t = lds_load(&parent[c - g])) < m) m = t;
            if (y + 1 < g && lab[c + g] == l && (t = lds_load(&parent[c + g])) < m) m = t;
            if (m < pc) { atomicMin(&parent[pc], m); atomicMin(&parent[c], m); ch = true; }
        }
        __syncthreads();
        for (int c = tid; c < G2; c += DET_THREADS) {
            if (lab[c] < 0) continue;
            const int p0 = lds_load(&parent[c]);
            int pc = p0;
            for (int j = 0; j < DET_JUMPS; ++j) {
                const int pp = lds_load(&parent[pc]);
                if (pp >= pc) break;
                pc = pp;
            }
            if (pc < p0) { atomicMin(&parent[c], pc); ch = true; }
        }
        if (ch) atomicOr(&s_changed, 1);
        __syncthreads();
        const int any = s_changed;
        __syncthreads();
        if (tid == 0) s_changed = 0;          // (read again only behind the next round's two barriers)
        if (!any) { done = true; break; }
    }
    if (!done) {                               // workgroup-uniform: the trip limit was hit
        if (tid == 0) { atomicOr(p.err, 1); p.counts[b] = 0; }
        return;
    }

    // attributes of a component, at its root (= its lowest cell)
    for (int c = tid; c < G2; c += DET_THREADS) {
        if (lab[c] < 0) continue;
        const int r = parent[c], y = c / g, x = c - y * g;
        atomicAdd(&cnt[r], 1);
        atomicMin(&bx0[r], x); atomicMin(&by0[r], y); atomicMax(&bx1[r], x); atomicMax(&by1[r], y);
        atomicMax(&conf[r], f32_orderable(sc[c]));
    }
    __syncthreads();
    // the kept components' keys: (confidence desc, -0 as +0; first cell asc) = larger key first
    for (int c = tid; c < G2; c += DET_THREADS) {
        if (lab[c] < 0 || parent[c] != c || cnt[c] < p.min_cells) continue;
        const float cf = orderable_f32(conf[c]);
        const int i = atomicAdd(&s_nk, 1);
        keys[i] = ((uint64_t)f32_orderable(cf == 0.f ? 0.f : cf) << 32) | (uint64_t)(uint32_t)(~(uint32_t)c);
    }
    __syncthreads();
    const int nk = s_nk, maxR = p.max_regions, words = (G2 + p.cls + 31) / 32;
    const int nout = nk < maxR ? nk : maxR;
    const long s0 = (long)b * maxR, total = (long)p.batch * maxR;
    int* st_prompt = (int*)p.stage;
    int* st_cells = st_prompt + total;
    uint32_t* st_conf = (uint32_t*)(st_cells + total);
    int* st_box = (int*)(st_conf + total);
    uint32_t* st_bits = (uint32_t*)(st_box + 4 * total);
    // a component's place = the number of kept components in front of it (nk comparisons each, whatever the data)
    for (int i = tid; i < nk; i += DET_THREADS) {
        const uint64_t k = keys[i];
        int rank = 0;
        for (int j = 0; j < nk; ++j) rank += keys[j] > k ? 1 : 0;
        if (rank >= maxR) continue;
        const int r = (int)(~(uint32_t)k);
        slot[r] = rank;
        st_prompt[s0 + rank] = lab[r];
        st_cells[s0 + rank] = cnt[r];
        st_conf[s0 + rank] = __float_as_uint(orderable_f32(conf[r]));
        st_box[(s0 + rank) * 4 + 0] = bx0[r]; st_box[(s0 + rank) * 4 + 1] = by0[r];
        st_box[(s0 + rank) * 4 + 2] = bx1[r]; st_box[(s0 + rank) * 4 + 3] = by1[r];
    }
    __syncthreads();
    // bitmaps: word wi of slot k holds tokens 32 wi .. 32 wi + 31; cell c is token cls + c
    for (int e = tid; e < nout * words; e += DET_THREADS) {
        const int k = e / words, wi = e - k * words;
        uint32_t word = 0u;
        for (int j = 0; j < 32; ++j) {
            const int c = wi * 32 + j - p.cls;
            if (c >= 0 && c < G2 && lab[c] >= 0 && slot[parent[c]] == k) word |= 1u << j;
        }
        st_bits[(s0 + k) * words + wi] = word;
    }
    if (tid == 0) p.counts[b] = nout;
}

// image b's regions go to rows off .. off + counts[b], off = the counts in front of it
__global__ __launch_bounds__(256) void detect_compact_kernel(const int* __restrict__ counts, const uint32_t* __restrict__ stage,
                                                             int batch, int maxR, int words, int* __restrict__ r_img,
                                                             int* __restrict__ r_prompt, int* __restrict__ r_box,
                                                             int* __restrict__ r_cells, uint32_t* __restrict__ r_conf,
                                                             uint32_t* __restrict__ r_bits) {
    __shared__ long s_off;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        long off = 0;
        for (int i = 0; i < b; ++i) off += counts[i];
        s_off = off;
    }
    __syncthreads();
    const long off = s_off, s0 = (long)b * maxR, total = (long)batch * maxR;
    const int n = counts[b];
    const int* st_prompt = (const int*)stage;
    const int* st_cells = st_prompt + total;
    const uint32_t* st_conf = (const uint32_t*)(st_cells + total);
    const int* st_box = (const int*)(st_conf + total);
    const uint32_t* st_bits = (const uint32_t*)(st_box + 4 * total);
    for (int k = tid; k < n; k += 256) {
        if (r_img) r_img[off + k] = b;
        if (r_prompt) r_prompt[off + k] = st_prompt[s0 + k];
        if (r_cells) r_cells[off + k] = st_cells[s0 + k];
        if (r_conf) r_conf[off + k] = st_conf[s0 + k];
    }
    if (r_box) for (long e = tid; e < (long)n * 4; e += 256) r_box[off * 4 + e] = st_box[s0 * 4 + e];
    if (r_bits) for (long e = tid; e < (long)n * words; e += 256) r_bits[off * words + e] = st_bits[s0 * words + e];
}

size_t detect_stage_words(int batch, int max_regions, int words) { return (size_t)batch * max_regions * (7 + (size_t)words); }

int launch_detect_regions(const DetectRegionArgs& a, hipStream_t st) {
    REVO_REQUIRE(a.g >= 1 && a.g * a.g <= DETECT_MAX_CELLS, "detect_regions: the grid must hold 1 .. 1024 cells");
    REVO_REQUIRE(a.P >= 1 && a.P <= DETECT_MAX_PROMPTS, "detect_regions: n_prompts must be in [1, 64]");
    REVO_REQUIRE(a.nbg >= 0 && a.nbg < a.P, "detect_regions: n_background must be in [0, n_prompts)");
    REVO_REQUIRE(a.min_cells >= 1, "detect_regions: min_cells must be at least 1");
    REVO_REQUIRE(a.max_regions >= 1 && a.max_regions <= a.g * a.g, "detect_regions: max_regions must be in [1, g * g]");
    REVO_REQUIRE(a.cls == 0 || a.cls == 1, "detect_regions: use_cls must be 0 or 1");
    if (a.batch <= 0) return 0;
    hipLaunchKernelGGL(detect_regions_kernel, dim3((unsigned)a.batch), dim3(DET_THREADS), 0, st, a);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_detect_compact(const int* counts, const uint32_t* stage, int batch, int max_regions, int words, int* r_img, int* r_prompt,
                          int* r_box, int* r_cells, float* r_conf, uint32_t* r_bits, hipStream_t st) {
    if (batch <= 0) return 0;
    hipLaunchKernelGGL(detect_compact_kernel, dim3((unsigned)batch), dim3(256), 0, st, counts, stage, batch, max_regions, words, r_img,
                       r_prompt, r_box, r_cells, (uint32_t*)r_conf, r_bits);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace revo
