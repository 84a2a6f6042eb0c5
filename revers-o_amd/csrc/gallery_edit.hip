// Row movement of revo_gallery_remove (include/revo.h, EDIT): the surviving rows of one chunk of the
// gallery gathered, in order, into a compact run of rows -- staging memory, or the gallery itself where the chunk's destination
// lies wholly in front of the chunk.  HBM-bound: 16-byte accesses, every lane of a wave busy whatever the row length.
#include "kernels.h"

namespace revo {
namespace {
// the rows of bitmap word w that stay: bit clear and row < N
__device__ __forceinline__ uint32_t keep_word(const uint32_t* __restrict__ bits, long w, long N) {
    const long r0 = w << 5;
    if (r0 >= N) return 0u;
    uint32_t k = ~bits[w];
    if (N - r0 < 32) k &= (1u << (int)(N - r0)) - 1u;
    return k;
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const uint32_t t = (uint32_t)__shfl_xor((int)v, o, 64); v = t < v ? t : v; }
    return v;
}
}  // namespace

// one workgroup per chunk: popcount per word, summed; the first removed row
__global__ __launch_bounds__(256) void remove_count_kernel(const uint32_t* __restrict__ bits, long N, long chunk,
                                                           uint32_t* __restrict__ cnt, uint32_t* __restrict__ first) {
    __shared__ uint32_t s_n[4], s_f[4];
    const long row0 = (long)blockIdx.x * chunk;
    const long len = N - row0 < chunk ? N - row0 : chunk;
    const long w0 = row0 >> 5, nw = (len + 31) >> 5;
    uint32_t n = 0, f = (uint32_t)len;
    for (long i = threadIdx.x; i < nw; i += 256) {
        const uint32_t k = keep_word(bits, w0 + i, N);
        n += __popc(k);
        const long left = N - ((w0 + i) << 5);                       // rows of this word inside the gallery (> 0 here)
        const uint32_t rem = ~k & (left < 32 ? (1u << (int)left) - 1u : 0xffffffffu);
        if (rem) { const uint32_t r = (uint32_t)(i * 32 + __ffs(rem) - 1); f = r < f ? r : f; }
    }
    n = wave_sum_u32(n); f = wave_min_u32(f);
    if ((threadIdx.x & 63) == 0) { s_n[threadIdx.x >> 6] = n; s_f[threadIdx.x >> 6] = f; }
    __syncthreads();
    if (threadIdx.x == 0) {
        cnt[blockIdx.x] = s_n[0] + s_n[1] + s_n[2] + s_n[3];
        uint32_t m = s_f[0];
        for (int i = 1; i < 4; ++i) m = s_f[i] < m ? s_f[i] : m;
        first[blockIdx.x] = m;
    }
}
int launch_remove_count(const uint32_t* bits, long N, long chunk, uint32_t* cnt, uint32_t* first, hipStream_t st) {
    REVO_REQUIRE(chunk >= 32 && chunk % 32 == 0 && chunk <= REMOVE_MAX_CHUNK, "remove_count: bad chunk size");
    if (N <= 0) return 0;
    hipLaunchKernelGGL(remove_count_kernel, dim3((unsigned)((N + chunk - 1) / chunk)), dim3(256), 0, st, bits, N, chunk, cnt,
                       first);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}

// A workgroup takes 256 rows (8 bitmap words) of the chunk, a wave 64 of them.  The destination of a kept row is the number
// of kept rows of the chunk in front of it: the workgroup sums the popcounts of the chunk's words in front of its own (at
// most 2048 words, from L2), a ballot ranks the rows inside the wave.  The wave then copies its kept rows as one flat run of
// 16-byte units, so a short row (64 bf16 = 8 units) keeps all 64 lanes loading.
__global__ __launch_bounds__(256) void remove_gather_kernel(const uint32_t* __restrict__ bits, long N, long row0, long len,
                                                            long j0, const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                            int u4_per_row) {
    __shared__ uint32_t s_part[4], s_cnt[4];
    __shared__ uint8_t s_src[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long w0 = row0 >> 5;                      // the chunk's first word
    const long tw = (long)blockIdx.x * 8;           // this workgroup's first word, counted from the chunk's
    uint32_t n = 0;
    for (long i = threadIdx.x; i < tw; i += 256) n += __popc(keep_word(bits, w0 + i, N));
    n = wave_sum_u32(n);
    const long off = (tw + 2 * wave) * 32 + lane;   // this lane's row, counted from the chunk's first
    const bool keep = off < len && ((keep_word(bits, w0 + tw + 2 * wave + (lane >> 5), N) >> (lane & 31)) & 1u);
    const unsigned long long kept = __ballot(keep);
    const int kw = __popcll(kept);
    if (keep) s_src[wave][__popcll(kept & ((1ull << lane) - 1ull))] = (uint8_t)lane;
    if (lane == 0) { s_part[wave] = n; s_cnt[wave] = (uint32_t)kw; }
    __syncthreads();
    long before = (long)s_part[0] + s_part[1] + s_part[2] + s_part[3];
    for (int i = 0; i < wave; ++i) before += s_cnt[i];
    const long wave_row0 = row0 + (tw + 2 * wave) * 32;
    const long total = (long)kw * u4_per_row;
#pragma unroll 4
    for (long it = lane; it < total; it += 64) {
        const int j = (int)(it / u4_per_row);
        const int c = (int)(it - (long)j * u4_per_row);
        const long jr = before + j;                 // the row's rank among the chunk's kept rows
        if (jr < j0) continue;                      // (in front of the first removed row: already in place)
        dst[jr * u4_per_row + c] = src[(wave_row0 + s_src[wave][j]) * u4_per_row + c];
    }
}
int launch_remove_gather(const uint32_t* bits, long N, long row0, long len, long j0, const uint4* src, uint4* dst,
                         int u4_per_row, hipStream_t st) {
    REVO_REQUIRE(row0 >= 0 && row0 % 32 == 0 && len >= 0 && len <= REMOVE_MAX_CHUNK && row0 + len <= N && u4_per_row >= 1,
                 "remove_gather: bad chunk");
    if (len == 0) return 0;
    hipLaunchKernelGGL(remove_gather_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, st, bits, N, row0, len, j0, src,
                       dst, u4_per_row);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace revo
