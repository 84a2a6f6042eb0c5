// Stable LSD radix sort of (64-bit key, fp32 value) entries, 8-bit digits, and the one-workgroup prefix sum it is built
// on: the sort step of the candidate pipeline (pairs, range and recommend searches) and the range
// search's CSR offsets.
#include "kernels.h"

namespace revo {

// One LSD pass over digit (key >> shift) & 255: block j of `tile` keys counts its digits (hist), one workgroup turns the
// counts [digit][block] into exclusive offsets (prefix sum), block j scatters its keys in index order (stable).
__global__ __launch_bounds__(256) void radix_hist_kernel(const uint64_t* __restrict__ keys, long n, long tile, int shift,
                                                         uint32_t* __restrict__ cnt, int nblk) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const long e0 = (long)blockIdx.x * tile, e1 = e0 + tile < n ? e0 + tile : n;
    for (long e = e0 + threadIdx.x; e < e1; e += 256) atomicAdd(&h[(keys[e] >> shift) & 255u], 1u);
    __syncthreads();
    cnt[(long)threadIdx.x * nblk + blockIdx.x] = h[threadIdx.x];
}
// prefix sums of c[0 .. M) in place (INCLUSIVE: c[i] counts itself), one workgroup: thread t takes the contiguous chunk t * per ..
template <class T, bool INCLUSIVE>
__global__ __launch_bounds__(1024) void prefix_sum_kernel(T* __restrict__ c, long M) {
    __shared__ T s[1024];
    const int t = threadIdx.x;
    const long per = (M + 1023) / 1024, a = (long)t * per, e = a + per < M ? a + per : M;
    T sum = 0;
    for (long i = a; i < e; ++i) sum += c[i];
    s[t] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {              // inclusive scan of the chunk sums
        const T v = t >= off ? s[t - off] : 0;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    T run = s[t] - sum;
    for (long i = a; i < e; ++i) { const T x = c[i]; c[i] = INCLUSIVE ? run + x : run; run += x; }
}
// Rounds of 256 keys in index order: a key's place = its digit's running offset + the keys of its digit in earlier waves of
// the round + those in earlier lanes of its wave (8 ballots find the lanes with the same digit)
__global__ __launch_bounds__(256) void radix_scatter_kernel(const uint64_t* __restrict__ kin, const float* __restrict__ vin,
                                                            uint64_t* __restrict__ kout, float* __restrict__ vout, long n,
                                                            long tile, int shift, const uint32_t* __restrict__ cnt, int nblk) {
    __shared__ uint32_t run[256], wc[4][256];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    run[t] = cnt[(long)t * nblk + blockIdx.x];
#pragma unroll
    for (int w = 0; w < 4; ++w) wc[w][t] = 0u;
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    const long e0 = (long)blockIdx.x * tile, e1 = e0 + tile < n ? e0 + tile : n;
    for (long r0 = e0; r0 < e1; r0 += 256) {
        const long e = r0 + t;
        const bool valid = e < e1;
        const uint64_t k = valid ? kin[e] : 0ull;
        const float v = valid ? vin[e] : 0.f;
        const uint32_t d = (uint32_t)(k >> shift) & 255u;
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const unsigned long long bb = __ballot((d >> bit) & 1u);
            peers &= ((d >> bit) & 1u) ? bb : ~bb;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & below);
        if (valid && rank == 0u) wc[wave][d] = (uint32_t)__popcll(peers);
        __syncthreads();
        if (valid) {
            uint32_t pos = run[d] + rank;
            for (int w = 0; w < wave; ++w) pos += wc[w][d];
            kout[pos] = k;
            vout[pos] = v;
        }
        __syncthreads();
        run[t] += wc[0][t] + wc[1][t] + wc[2][t] + wc[3][t];
#pragma unroll
        for (int w = 0; w < 4; ++w) wc[w][t] = 0u;
        __syncthreads();
    }
}

// keys per block of a radix pass: at most SORT_MAX_BLOCKS blocks (cnt holds 256 words per block)
static long sort_keys_tile(long n) {
    long tile = (n + SORT_MAX_BLOCKS - 1) / SORT_MAX_BLOCKS;
    tile = (tile + 255) / 256 * 256;
    return tile < 4096 ? 4096 : tile;
}
int launch_sort_keys_u64(uint64_t* keys, float* vals, uint64_t* keys_alt, float* vals_alt, long n, int key_bits, uint32_t* cnt,
                         uint64_t** out_keys, float** out_vals, hipStream_t st) {
    *out_keys = keys; *out_vals = vals;
    if (n <= 1) return 0;
    const long tile = sort_keys_tile(n);
    const int nblk = (int)((n + tile - 1) / tile);
    for (int shift = 0; shift < key_bits; shift += 8) {
        hipLaunchKernelGGL(radix_hist_kernel, dim3((unsigned)nblk), dim3(256), 0, st, keys, n, tile, shift, cnt, nblk);
        hipLaunchKernelGGL((prefix_sum_kernel<uint32_t, false>), dim3(1), dim3(1024), 0, st, cnt, 256l * nblk);
        hipLaunchKernelGGL(radix_scatter_kernel, dim3((unsigned)nblk), dim3(256), 0, st, keys, vals, keys_alt, vals_alt, n, tile,
                           shift, cnt, nblk);
        uint64_t* tk = keys; keys = keys_alt; keys_alt = tk;
        float* tv = vals; vals = vals_alt; vals_alt = tv;
    }
    REVO_HIP_CHECK(hipGetLastError());
    *out_keys = keys; *out_vals = vals;
    return 0;
}
int launch_inclusive_sums_u64(unsigned long long* c, long n, hipStream_t st) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL((prefix_sum_kernel<unsigned long long, true>), dim3(1), dim3(1024), 0, st, c, n);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace revo
