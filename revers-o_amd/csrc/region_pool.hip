// Region embeddings from one forward: the attention-pool head of head.hip with its softmax restricted
// to the tokens of a region.  The body's forward, ln_post and the probe's logits are shared by all regions of an image; a
// region costs one masked pooling of the rows it covers and one row of the head's five skinny GEMMs.
//   u[r, h, c] = sum_{s allowed} softmax_{s allowed}(logits[b, h, :])[s] * x[b * S + s][c],   b = region_image[r]
// region_bits[r][ceil(S / 32)]: token s is allowed iff bit s & 31 of word s >> 5 is set (the layout of revo_search_set_filter);
// bits at or past S are ignored.
#include "kernels.h"

namespace revo {

constexpr int RP_WAVES = 16;      // as pool_accumulate_kernel (head.hip): the summation order below is that kernel's
constexpr int RP_HC = 4;
constexpr int RP_MAXH = LN_MAXH;

// Masked sibling of pool_accumulate_kernel<CPL>, grid (W / (64 CPL), regions).  The order of every sum is that kernel's,
// restricted to the allowed tokens: lane-strided max and sum over s for the softmax; wave w takes the rows s = w (mod 16)
// ascending in one fma chain per column; the sixteen partial sums are added in wave order.  So a region with every token
// allowed has the bits of launch_pool_head_rows for its image, and the two column forms agree bit for bit.
// Disallowed tokens are skipped, not weighted by zero: their logits enter neither the max nor the sum and their rows are
// never loaded (each wave compacts the rows it owns into a list in LDS first: the main loop walks that list with
// wave-uniform row numbers, eight loads in flight as in the unmasked kernel).  NaN or Inf outside the region changes
// nothing; a region of 20 tokens reads 20 rows.  A region without an allowed token (or with an image index outside the
// batch) writes zeros.
template <int CPL>
__global__ __launch_bounds__(RP_WAVES * 64) void pool_accumulate_masked_kernel(const float* __restrict__ x, long ldx,
                                                                     const float* __restrict__ logits,
                                                                     const int* __restrict__ region_image,
                                                                     const uint32_t* __restrict__ region_bits, int B, int S,
                                                                     int W, int H, float* __restrict__ u) {
    extern __shared__ float psm[];                    // [H][S] probabilities, then [RP_WAVES][RP_HC][64 CPL] partial sums,
    constexpr int NC = 64 * CPL;                      // then the bitmap, the waves' row lists and a flag
    float* red = psm + (((long)H * S + 3) & ~3l);
    const int words = (S + 31) >> 5, cap = (S + RP_WAVES - 1) / RP_WAVES;
    uint32_t* lbits = (uint32_t*)(red + RP_WAVES * RP_HC * NC);
    int* rowlist = (int*)(lbits + words);             // [RP_WAVES][cap]
    int* any = rowlist + RP_WAVES * cap;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = blockIdx.y, c = (blockIdx.x * 64 + lane) * CPL;
    const int b = region_image[r];
    const bool image_ok = b >= 0 && b < B;

    if (threadIdx.x == 0) *any = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < words; i += RP_WAVES * 64) {
        uint32_t v = image_ok ? region_bits[(long)r * words + i] : 0u;
        if (i == words - 1 && (S & 31)) v &= (1u << (S & 31)) - 1u;      // bits at or past S
        lbits[i] = v;
        if (v) *any = 1;
    }
    __syncthreads();
    if (*any == 0) {                                  // empty region: zeros, nothing divided
        for (int t = threadIdx.x; t < H * NC; t += RP_WAVES * 64) {
            const int h = t / NC, col = blockIdx.x * NC + (t - h * NC);
            if (col < W) u[((long)r * H + h) * W + col] = 0.f;
        }
        return;
    }
    auto allowed = [&](int s) { return (lbits[s >> 5] >> (s & 31)) & 1u; };

    for (int h = w; h < H; h += RP_WAVES) {
        const float* lg = logits + ((long)b * H + h) * S;
        float m = -INFINITY;
        for (int s = lane; s < S; s += 64)
            if (allowed(s)) m = fmaxf(m, lg[s]);
        m = wave_max(m);
        float sum = 0.f;
        for (int s = lane; s < S; s += 64)
            if (allowed(s)) {
                const float e = expf(lg[s] - m);
                psm[(long)h * S + s] = e;
                sum += e;
            }
        sum = wave_sum(sum);
        const float inv = 1.0f / sum;                 // (not empty: the term of the largest allowed logit is exp(0) = 1)
        for (int s = lane; s < S; s += 64)
            if (allowed(s)) psm[(long)h * S + s] *= inv;
    }
    // this wave's allowed rows, ascending: s = w + 16 j
    int n_rows = 0;
    {
        int* mine = rowlist + w * cap;
        for (int j0 = 0; j0 < cap; j0 += 64) {
            const int s = w + (j0 + lane) * RP_WAVES;
            const bool on = s < S && allowed(s);
            const unsigned long long bal = __ballot(on);
            if (on) mine[n_rows + __popcll(bal & ((1ull << lane) - 1ull))] = s;
            n_rows += __popcll(bal);
        }
    }
    __syncthreads();

    float acc[RP_MAXH][CPL];
#pragma unroll
    for (int h = 0; h < RP_MAXH; ++h)
#pragma unroll
        for (int j = 0; j < CPL; ++j) acc[h][j] = 0.f;
    if (c < W) {
        const float* xc = x + (long)b * S * ldx + c;
        const int* mine = rowlist + w * cap;
        auto load = [&](int s, float (&v)[CPL]) {
            if constexpr (CPL == 4) {
                const f32x4 t = *(const f32x4*)(xc + (long)s * ldx);
                v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
            } else {
                v[0] = xc[(long)s * ldx];
            }
        };
        int k = 0;
        for (; k + 7 < n_rows; k += 8) {
            int s[8];
            float v[8][CPL];
#pragma unroll
            for (int i = 0; i < 8; ++i) s[i] = __builtin_amdgcn_readfirstlane(mine[k + i]);
#pragma unroll
            for (int i = 0; i < 8; ++i) load(s[i], v[i]);
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int h = 0; h < RP_MAXH; ++h)
                    if (h < H) {
                        const float pr = psm[(long)h * S + s[i]];
#pragma unroll
                        for (int j = 0; j < CPL; ++j) acc[h][j] = fmaf(pr, v[i][j], acc[h][j]);
                    }
        }
        for (; k < n_rows; ++k) {
            const int s = __builtin_amdgcn_readfirstlane(mine[k]);
            float v[CPL];
            load(s, v);
#pragma unroll
            for (int h = 0; h < RP_MAXH; ++h)
                if (h < H) {
                    const float pr = psm[(long)h * S + s];
#pragma unroll
                    for (int j = 0; j < CPL; ++j) acc[h][j] = fmaf(pr, v[j], acc[h][j]);
                }
        }
    }
    // the sixteen waves' partial sums, RP_HC heads at a time, in wave order (pool_accumulate_kernel's reduction)
#pragma unroll
    for (int h0 = 0; h0 < RP_MAXH; h0 += RP_HC) {
        if (h0 >= H) break;
        if (h0) __syncthreads();
#pragma unroll
        for (int hh = 0; hh < RP_HC; ++hh)
#pragma unroll
            for (int j = 0; j < CPL; ++j) red[((long)w * RP_HC + hh) * NC + lane * CPL + j] = acc[h0 + hh][j];
        __syncthreads();
        for (int t = threadIdx.x; t < RP_HC * NC; t += RP_WAVES * 64) {
            const int hh = t / NC, cc = t - hh * NC;
            const int col = blockIdx.x * NC + cc;
            if (h0 + hh < H && col < W) {
                float sum = red[((long)0 * RP_HC + hh) * NC + cc];
#pragma unroll
                for (int o = 1; o < RP_WAVES; ++o) sum += red[((long)o * RP_HC + hh) * NC + cc];
                u[((long)r * H + h0 + hh) * W + col] = sum;
            }
        }
    }
}

int launch_pool_head_rows_masked(const float* x, long ldx, int B, int S, int W, int H, const float* logits,
                                 const int* region_image, const uint32_t* region_bits, int R, float* u, hipStream_t st) {
    REVO_REQUIRE(H >= 1 && H <= RP_MAXH && W % 4 == 0 && ldx % 4 == 0, "masked pool head: at most 16 heads, width a multiple of 4");
    REVO_REQUIRE(B >= 1 && S >= 1 && W >= 4, "masked pool head: batch, sequence and width must be positive");
    REVO_REQUIRE(R <= 65535, "masked pool head: at most 65535 regions per launch");
    if (R <= 0) return 0;
    // as the batch form chooses with B: four columns per lane once that still gives most CUs a workgroup
    const bool wide = (long)R * ((W + 255) / 256) >= 192;
    const int cpl = wide ? 4 : 1;
    const size_t words = (size_t)(S + 31) / 32, cap = (size_t)(S + RP_WAVES - 1) / RP_WAVES;
    const size_t lds = ((((size_t)H * S + 3) & ~(size_t)3) + RP_WAVES * (size_t)RP_HC * 64 * cpl + words + RP_WAVES * cap + 1) * 4;
    REVO_REQUIRE(lds <= 160 * 1024, "masked pool head: sequence too long for the probability table in LDS");
    if (wide) {
        REVO_FUNC_LDS(pool_accumulate_masked_kernel<4>, (int)lds);
        hipLaunchKernelGGL(pool_accumulate_masked_kernel<4>, dim3((W + 255) / 256, R), dim3(RP_WAVES * 64), lds, st, x, ldx, logits,
                           region_image, region_bits, B, S, W, H, u);
    } else {
        REVO_FUNC_LDS(pool_accumulate_masked_kernel<1>, (int)lds);
        hipLaunchKernelGGL(pool_accumulate_masked_kernel<1>, dim3((W + 63) / 64, R), dim3(RP_WAVES * 64), lds, st, x, ldx, logits,
                           region_image, region_bits, B, S, W, H, u);
    }
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}

// Rows of regions without an allowed token become zeros (the head maps a zero pooled row to its biases, not to zero): the
// final vector of an empty region is all zeros and is not normalised.
__global__ __launch_bounds__(256) void zero_empty_regions_kernel(const uint32_t* __restrict__ region_bits, int S, int D,
                                                                 float* __restrict__ out) {
    const int r = blockIdx.x, words = (S + 31) >> 5;
    const uint32_t* bits = region_bits + (long)r * words;
    uint32_t acc = 0;
    for (int i = 0; i < words; ++i) {                 // (uniform: every thread reads the same few words)
        uint32_t v = bits[i];
        if (i == words - 1 && (S & 31)) v &= (1u << (S & 31)) - 1u;
        acc |= v;
    }
    if (acc) return;
    for (int c = threadIdx.x; c < D; c += 256) out[(long)r * D + c] = 0.f;
}
int launch_zero_empty_regions(const uint32_t* region_bits, int R, int S, int D, float* out, hipStream_t st) {
    if (R <= 0) return 0;
    hipLaunchKernelGGL(zero_empty_regions_kernel, dim3(R), dim3(256), 0, st, region_bits, S, D, out);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace revo
