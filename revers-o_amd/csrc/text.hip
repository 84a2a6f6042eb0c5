// The text tower of the CLIP checkpoint (include/revo.h, TEXT): its three kernels -- token embedding,
// causal attention, end-of-text pooling -- its handle and its forward.  The blocks are the image tower's (tower.h
// body_blocks) with a plain bf16 qkv epilogue and the causal attention below; the head (ln_final on the pooled rows, the
// projection, the normalisation) is fp32 like the image tower's.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/revo.h"
#include "kernels.h"
#include "tower.h"

namespace revo {

// ---------------------------------------------------------- token embedding --
// one workgroup per row; 16-byte loads and stores, 64-bit row offsets
__global__ __launch_bounds__(256) void embed_tokens_kernel(const int32_t* __restrict__ tokens, const float* __restrict__ table,
                                                           const float* __restrict__ pos, int S, int vocab, int W,
                                                           float* __restrict__ x, long ldx) {
    const long row = blockIdx.x;
    const int tok = tokens[row];
    const int s = (int)(row % S);
    const bool ok = tok >= 0 && tok < vocab;          // (the entry points validate on the host; this keeps a bad id from reading)
    const float4* t = (const float4*)(table + (long)(ok ? tok : 0) * W);
    const float4* p = (const float4*)(pos + (long)s * W);
    float4* o = (float4*)(x + row * ldx);
    const float nan = __uint_as_float(0x7fc00000u);
    for (int c = threadIdx.x; c < W / 4; c += 256) {
        const float4 a = t[c], b = p[c];
        o[c] = ok ? make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w) : make_float4(nan, nan, nan, nan);
    }
}
int launch_embed_tokens(const int32_t* tokens, const float* table, const float* pos, int B, int S, int vocab, int W, float* x,
                        long ldx, hipStream_t st) {
    REVO_REQUIRE(W % 4 == 0 && ldx % 4 == 0 && ldx >= W, "embed_tokens: width and row stride must be multiples of 4, stride at least width");
    REVO_REQUIRE(vocab >= 1 && S >= 1, "embed_tokens: vocab and seq must be positive");
    if (B <= 0) return 0;
    hipLaunchKernelGGL(embed_tokens_kernel, dim3((unsigned)((long)B * S)), dim3(256), 0, st, tokens, table, pos, S, vocab, W, x, ldx);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------- end-of-text pooling --
// one wave per prompt: the first position of the largest id, then that row
__global__ __launch_bounds__(64) void pool_eot_kernel(const int32_t* __restrict__ tokens, const float* __restrict__ x, long ldx,
                                                      int S, int W, float* __restrict__ out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    // (a lane without a position keeps at = S and loses every tie; a lane with one starts from its first, so that a prompt
    //  of nothing but the smallest int32 still names position 0 and never the row after the prompt)
    int best = INT32_MIN, at = S;
    for (int s = lane; s < S; s += 64) {
        const int t = tokens[(long)b * S + s];
        if (t > best || s == lane) { best = t; at = s; }   // ascending s: the first position of the lane's largest id
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int ob = __shfl_xor(best, o, 64), oa = __shfl_xor(at, o, 64);
        if (ob > best || (ob == best && oa < at)) { best = ob; at = oa; }
    }
    const float4* src = (const float4*)(x + ((long)b * S + at) * ldx);
    float4* dst = (float4*)(out + (long)b * W);
    for (int c = lane; c < W / 4; c += 64) dst[c] = src[c];
}
int launch_pool_eot(const int32_t* tokens, const float* x, long ldx, int B, int S, int W, float* out, hipStream_t st) {
    REVO_REQUIRE(W % 4 == 0 && ldx % 4 == 0 && S >= 1, "pool_eot: width and row stride must be multiples of 4");
    if (B <= 0) return 0;
    hipLaunchKernelGGL(pool_eot_kernel, dim3(B), dim3(64), 0, st, tokens, x, ldx, S, W, out);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------- causal attention --
// One workgroup per (sequence, head), one wave per block of 32 query rows.  K [key][d] and V transposed [d][key] of the
// (sequence, head) are staged in LDS once, zero rows past S.  Scores come from the swapped product mfma(K, Q): the 32 x 32
// result has the QUERY on the lane and 16 of the tile's 32 keys in the lane's registers (the other 16 in lane ^ 32), so a row's
// maximum and sum are register loops plus one exchange.  The same registers, rounded to bf16, are the B operand of
// O^T = V^T . P^T in the permuted k order of an accumulator tile: element j of lane half h of k-step s is key
// 16 s + 8 (j >> 2) + 4 h + (j & 3) of the tile, and the V^T fragment is read from those keys.
// Key tiles above the diagonal are not computed; a masked score is -inf before the row maximum, its probability exactly 0,
// and 0 . v = 0 for any finite v: row i is a function of rows 0..i alone, bit for bit.
constexpr int ATTC_KLD = 72;                      // bf16 per K row in LDS (64 + 8: 144-byte rows, 16-byte aligned, off the bank period)
constexpr int ATTC_VLD = ATTC_MAX_S + 8;          // bf16 per V^T row in LDS (272-byte rows, 8-byte aligned)
__global__ __launch_bounds__(256) void attn_causal_kernel(const bf16_t* __restrict__ qkv, long ld, bf16_t* __restrict__ out,
                                                          long ldo, int S, int H, float c) {
    __shared__ __attribute__((aligned(16))) bf16_t Ks[ATTC_MAX_S * ATTC_KLD];
    __shared__ __attribute__((aligned(16))) bf16_t Vt[64 * ATTC_VLD];
    const int b = blockIdx.x / H, hh = blockIdx.x % H;
    const int W = H * 64;
    const int nthreads = blockDim.x;              // 64 x query blocks
    const int SP = (nthreads / 64) * 32;          // S padded to whole key tiles, <= ATTC_MAX_S
    const bf16_t* base = qkv + (long)b * S * ld + hh * 64;
    for (int i = threadIdx.x; i < SP * 8; i += nthreads) {
        const int key = i >> 3, ch = i & 7;
        uint4 kk = make_uint4(0, 0, 0, 0), vv = make_uint4(0, 0, 0, 0);
        if (key < S) {
            kk = *(const uint4*)(base + (long)key * ld + W + ch * 8);
            vv = *(const uint4*)(base + (long)key * ld + 2 * W + ch * 8);
        }
        *(uint4*)(Ks + key * ATTC_KLD + ch * 8) = kk;
        const uint32_t w4[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) Vt[(ch * 8 + j) * ATTC_VLD + key] = (bf16_t)(w4[j >> 1] >> ((j & 1) * 16));
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, qb = threadIdx.x >> 6;
    const int ql = lane & 31, half = lane >> 5;
    const int query = qb * 32 + ql;
    bf16x8 qf[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        uint4 q4 = make_uint4(0, 0, 0, 0);
        if (query < S) q4 = *(const uint4*)(base + (long)query * ld + 16 * t + 8 * half);
        qf[t] = __builtin_bit_cast(bf16x8, q4);
    }
    // pass 1: the scores of key tiles 0..qb, scaled to the exponent of 2, masked; the row's maximum
    f32x16 e[4];
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
        if (kt <= qb) {
            f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const uint4 k4 = *(const uint4*)(Ks + (kt * 32 + ql) * ATTC_KLD + 16 * t + 8 * half);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, k4), qf[t], acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                const float v = key <= query ? acc[r] * c : -INFINITY;
                e[kt][r] = v;
                m = fmaxf(m, v);
            }
        }
    }
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    // pass 2: p = 2^(e - m), the row's sum in fp32, O^T += V^T . bf16(P^T)
    f32x16 o0 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, o1 = o0;
    float l = 0.f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
        if (kt <= qb) {
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                float p[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    p[j] = exp2f(e[kt][8 * s2 + j] - m);
                    l += p[j];
                }
                const uint4 pk = make_uint4(pack_bf16x2(p[0], p[1]), pack_bf16x2(p[2], p[3]), pack_bf16x2(p[4], p[5]),
                                            pack_bf16x2(p[6], p[7]));
                const bf16x8 pb = __builtin_bit_cast(bf16x8, pk);
                const int k0 = kt * 32 + 16 * s2 + 4 * half;      // elements 0..3: keys k0 + j; 4..7: keys k0 + 8 + (j - 4)
                const uint2 a0 = *(const uint2*)(Vt + ql * ATTC_VLD + k0), a1 = *(const uint2*)(Vt + ql * ATTC_VLD + k0 + 8);
                const uint2 b0 = *(const uint2*)(Vt + (32 + ql) * ATTC_VLD + k0), b1 = *(const uint2*)(Vt + (32 + ql) * ATTC_VLD + k0 + 8);
                const uint4 va = make_uint4(a0.x, a0.y, a1.x, a1.y), vb = make_uint4(b0.x, b0.y, b1.x, b1.y);
                o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, va), pb, o0, 0, 0, 0);
                o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, vb), pb, o1, 0, 0, 0);
            }
        }
    }
    l += __shfl_xor(l, 32, 64);
    if (query >= S) return;
    const float inv = 1.0f / l;
    bf16_t* orow = out + ((long)b * S + query) * ldo + hh * 64;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        // registers 4g..4g+3: d = 8 g + 4 half + 0..3 of the 32-wide block
        *(uint2*)(orow + 8 * g + 4 * half) = make_uint2(pack_bf16x2(o0[4 * g] * inv, o0[4 * g + 1] * inv),
                                                        pack_bf16x2(o0[4 * g + 2] * inv, o0[4 * g + 3] * inv));
        *(uint2*)(orow + 32 + 8 * g + 4 * half) = make_uint2(pack_bf16x2(o1[4 * g] * inv, o1[4 * g + 1] * inv),
                                                             pack_bf16x2(o1[4 * g + 2] * inv, o1[4 * g + 3] * inv));
    }
}
int launch_attention_causal(const bf16_t* qkv, long ld, bf16_t* out, long ldo, int B, int S, int H, int hd, hipStream_t st) {
    REVO_REQUIRE(hd == 64, "causal attention: head_dim must be 64");
    REVO_REQUIRE(S <= ATTC_MAX_S, "causal attention: at most 128 positions");
    REVO_REQUIRE(H >= 1 && ld % 8 == 0 && ldo % 4 == 0 && ld >= 3l * H * 64 && ldo >= (long)H * 64,
                 "causal attention: strides must keep 16-byte (qkv) and 8-byte (out) alignment and hold the heads");
    REVO_REQUIRE(qkv && out, "causal attention: null argument");
    REVO_REQUIRE((((uintptr_t)qkv) & 15) == 0 && (((uintptr_t)out) & 7) == 0, "causal attention: misaligned buffer");
    if (B <= 0 || S <= 0) return 0;
    const float c = (1.0f / sqrtf((float)hd)) * 1.44269504088896340736f;
    const int nqb = (S + 31) / 32;
    hipLaunchKernelGGL(attn_causal_kernel, dim3((unsigned)((long)B * H)), dim3(64 * nqb), 0, st, qkv, ld, out, ldo, S, H, c);
    REVO_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace revo

// ------------------------------------------------------------- the handle ----
// (the blocks' weights, the body workspace, the allocations and their release: tower.h TowerCore)
struct revo_text : TowerCore {
    revo_text_cfg cfg;
    int last_seq = 0;
    float *tok_emb = nullptr, *pos = nullptr, *lnf_w = nullptr, *lnf_b = nullptr, *w_projT = nullptr;
    // workspace for max_batch prompts of context_length positions, beside the body's
    int32_t* tokens = nullptr;         // device copy of the call's ids
    float *pooled = nullptr, *pooled_n = nullptr, *feat = nullptr;
    PinnedStage tok_pin;               // the ids reach the device through this pinned buffer
};

extern "C" int32_t revo_text_create(const revo_text_cfg* cfg, const revo_tensor* weights, int32_t n_weights, int32_t device,
                                    int32_t max_batch, revo_text** out) {
    API_BEGIN
    REVO_REQUIRE(cfg && weights && out, "text_create: null argument");
    REVO_REQUIRE(max_batch >= 1, "text_create: max_batch must be >= 1");
    const revo_text_cfg& c = *cfg;
    REVO_REQUIRE(c.context_length >= 1 && c.vocab_size >= 1 && c.width >= 1 && c.layers >= 1 && c.heads >= 1 && c.mlp_dim >= 1 &&
                 c.out_dim >= 1 && n_weights >= 0, "text_create: sizes must be positive");
    REVO_REQUIRE(c.width % c.heads == 0 && c.width / c.heads == 64, "text_create: head_dim must be 64 (every known PE-Core text tower)");
    REVO_REQUIRE(c.context_length <= revo::ATTC_MAX_S, "text_create: context_length above 128 (the causal attention kernel's limit)");
    REVO_REQUIRE(c.width % 64 == 0 && c.mlp_dim % 64 == 0, "text_create: width and mlp_dim must be multiples of 64");
    REVO_REQUIRE(c.out_dim % 4 == 0, "text_create: out_dim must be a multiple of 4");
    REVO_REQUIRE((long)max_batch * c.context_length < (1l << 24), "text_create: max_batch * context_length too large");
    std::unique_ptr<revo_text> v(new revo_text());
    v->cfg = c; v->device = device; v->max_batch = max_batch;
    v->W = c.width; v->Md = c.mlp_dim; v->ln_eps = c.ln_eps;
    const int W = c.width, M = c.mlp_dim, D = c.out_dim, S = c.context_length;

    // the checkpoint is validated as a whole before the device is touched (tower.h check_checkpoint)
    const std::string blocks = "transformer.resblocks.";
    WeightMap wm;
    CHECK_RC(wm.fill("text_create", weights, n_weights));
    {
        NeedList need = {
            {"token_embedding.weight", (int64_t)c.vocab_size * W}, {"positional_embedding", (int64_t)S * W},
            {"ln_final.weight", W}, {"ln_final.bias", W}, {"text_projection", (int64_t)W * D}};
        need_blocks(need, blocks, c.layers, W, M, c.use_ls);
        CHECK_RC(check_checkpoint(wm, need, "the text tower", c.use_ls));
    }
    REVO_ON_DEVICE(device);

    Staging sg;
    CHECK_RC(sg.alloc(W, M, (long)W * D));
    CHECK_RC(up_f32(v.get(), wm, "token_embedding.weight", (int64_t)c.vocab_size * W, &v->tok_emb));
    CHECK_RC(up_f32(v.get(), wm, "positional_embedding", (int64_t)S * W, &v->pos));
    CHECK_RC(up_f32(v.get(), wm, "ln_final.weight", W, &v->lnf_w));
    CHECK_RC(up_f32(v.get(), wm, "ln_final.bias", W, &v->lnf_b));
    CHECK_RC(upload_blocks(v.get(), wm, sg, blocks, c.layers, c.use_ls));
    CHECK_RC(upload_projT(v.get(), wm, sg, "text_projection", D, &v->w_projT));

    const size_t rows = (size_t)max_batch * S, B = (size_t)max_batch;
    CHECK_RC(v->dalloc(&v->tokens, rows));
    CHECK_RC(alloc_body(v.get(), rows));
    CHECK_RC(v->dalloc(&v->pooled, B * W));
    CHECK_RC(v->dalloc(&v->pooled_n, B * W));
    CHECK_RC(v->dalloc(&v->feat, B * D));
    CHECK_RC(v->tok_pin.alloc(rows * 4));
    REVO_HIP_CHECK(hipDeviceSynchronize());
    *out = v.release();
    return 0;
    API_END
}

extern "C" int32_t revo_text_destroy(revo_text* text) {
    API_BEGIN
    if (text) { DeviceGuard dg(text->device); delete text; }
    return 0;
    API_END
}

#ifdef REVO_EXPERIMENTS   // parity-test hooks: librevo_exp.so only (include/revo.h)
extern "C" int32_t revo_text_set_debug_layers(revo_text* text, int32_t n) {
    REVO_REQUIRE(text, "null handle");
    text->debug_layers = n;
    return 0;
}
extern "C" int32_t revo_text_read_residual(revo_text* text, int32_t batch, float* dst, void* stream) {
    REVO_REQUIRE(text && dst && batch >= 1 && batch <= text->max_batch && text->last_seq >= 1, "text_read_residual: bad arguments");
    REVO_ON_DEVICE(text->device);
    REVO_HIP_CHECK(hipMemcpyAsync(dst, text->x, (size_t)batch * text->last_seq * text->cfg.width * 4, hipMemcpyDeviceToDevice,
                                  (hipStream_t)stream));
    return 0;
}
#endif

extern "C" int32_t revo_text_forward(revo_text* v, const int32_t* tokens, int32_t batch, int32_t seq_len, float* out,
                                     int32_t normalize, void* stream) {
    API_BEGIN
    // everything that can be refused is refused before the device is touched
    REVO_REQUIRE(batch >= 1 && seq_len >= 1, "text_forward: batch and seq_len must be at least 1");
    REVO_REQUIRE(v && tokens && out, "text_forward: null argument");
    REVO_REQUIRE(batch <= v->max_batch, "text_forward: batch exceeds max_batch of the handle");
    const revo_text_cfg& c = v->cfg;
    REVO_REQUIRE(seq_len <= c.context_length, "text_forward: seq_len exceeds context_length");
    for (int b = 0; b < batch; ++b)
        for (int s = 0; s < seq_len; ++s) {
            const int32_t id = tokens[(size_t)b * seq_len + s];
            if (id < 0 || id >= c.vocab_size) {
                revo_set_error("requirement failed: text_forward: prompt " + std::to_string(b) + " position " + std::to_string(s) +
                               " holds token id " + std::to_string(id) + ", outside [0, vocab_size = " +
                               std::to_string(c.vocab_size) + ")");
                return -2;
            }
        }
    REVO_ON_DEVICE(v->device);
    hipStream_t st = (hipStream_t)stream;
    using namespace revo;
    const int W = c.width, D = c.out_dim, B = batch, S = seq_len, rows = B * S;
    // the ids go through the pinned buffer: the caller's array is read before the call returns
    CHECK_RC(v->tok_pin.wait());
    memcpy(v->tok_pin.p, tokens, (size_t)rows * 4);
    REVO_HIP_CHECK(hipMemcpyAsync(v->tokens, v->tok_pin.p, (size_t)rows * 4, hipMemcpyHostToDevice, st));
    CHECK_RC(v->tok_pin.record(st));
    v->last_seq = S;

    { ProfScope ps("embed_tokens", st);
      CHECK_RC(launch_embed_tokens(v->tokens, v->tok_emb, v->pos, B, S, c.vocab_size, W, v->x, W, st)); }
    if (v->debug_layers == -2) return 0;   // parity hook: the embedded rows

    // the image tower's blocks (tower.h body_blocks) with a plain bf16 qkv epilogue and the causal attention; block 0
    // has no ln_pre in front of it: its ln_1 normalises the embedded rows
    CHECK_RC(body_blocks(
        *v, "text_forward", rows, v->debug_layers < 0 ? c.layers : std::min(v->debug_layers, c.layers), st,
        [&](GemmArgs&) { return (int)EPI_BF16; },
        [&]() { return launch_attention_causal(v->qkv, 3 * W, v->att, W, B, S, c.heads, 64, st); }));
    if (v->debug_layers >= 0) return 0;    // parity hook: residual stream only

    // the head in fp32 on B rows: the end-of-text row, ln_final, the projection, the normalisation
    { ProfScope ps("pool_eot", st);
      CHECK_RC(launch_pool_eot(v->tokens, v->x, W, B, S, W, v->pooled, st)); }
    { ProfScope ps("layernorm", st);
      CHECK_RC(launch_layernorm(v->pooled, W, v->lnf_w, v->lnf_b, c.ln_eps, B, W, v->pooled_n, W, 0, st)); }
    float* feat = normalize ? v->feat : out;
    { ProfScope ps("gemm_text_proj", st);
      CHECK_RC(launch_gemm_f32_skinny(0, v->pooled_n, W, 0, 0, v->w_projT, W, nullptr, B, D, W, feat, D, st)); }
    if (normalize) {
        ProfScope ps("l2norm", st);
        CHECK_RC(launch_l2norm_rows(v->feat, D, out, D, nullptr, 0, B, D, st));
    }
    return 0;
    API_END
}

// ------------------------------------------------------- single kernels ----
extern "C" int32_t revo_op_attention_causal(const void* qkv, int64_t ld, void* out, int64_t ldo, int32_t batch, int32_t seq,
                                            int32_t heads, int32_t head_dim, void* stream) {
    API_BEGIN
    REVO_REQUIRE(batch >= 0 && seq >= 0, "op_attention_causal: negative batch or seq");
    ProfScope ps("attention", (hipStream_t)stream);
    return revo::launch_attention_causal((const bf16_t*)qkv, ld, (bf16_t*)out, ldo, batch, seq, heads, head_dim, (hipStream_t)stream);
    API_END
}
extern "C" int32_t revo_op_embed_tokens(const int32_t* tokens_dev, const float* table, const float* pos, int32_t batch,
                                        int32_t seq, int32_t vocab, int32_t width, float* x, int64_t ldx, void* stream) {
    API_BEGIN
    REVO_REQUIRE(tokens_dev && table && pos && x, "op_embed_tokens: null argument");
    REVO_REQUIRE(batch >= 0 && seq >= 1 && (long)batch * seq < (1l << 31), "op_embed_tokens: bad batch or seq");
    return revo::launch_embed_tokens(tokens_dev, table, pos, batch, seq, vocab, width, x, ldx, (hipStream_t)stream);
    API_END
}
extern "C" int32_t revo_op_pool_eot(const int32_t* tokens_dev, const float* x, int64_t ldx, int32_t batch, int32_t seq,
                                    int32_t width, float* out, void* stream) {
    API_BEGIN
    REVO_REQUIRE(tokens_dev && x && out, "op_pool_eot: null argument");
    REVO_REQUIRE(batch >= 0 && seq >= 1 && (long)batch * seq < (1l << 31), "op_pool_eot: bad batch or seq");
    REVO_REQUIRE(width >= 4 && ldx >= width, "op_pool_eot: row stride below width");
    return revo::launch_pool_eot(tokens_dev, x, ldx, batch, seq, width, out, (hipStream_t)stream);
    API_END
}
