// Internal launcher interface of librevo (not part of the C ABI; see include/revo.h).
#pragma once
#include "common.h"

namespace revo {

// ---------------------------------------------------------------- GEMM -----
enum GemmEpi {
    EPI_BF16 = 0,       // C bf16 = acc + bias
    EPI_BF16_GELU = 1,  // C bf16 = gelu_erf(acc + bias)
    EPI_RESID_F32 = 2,  // C f32 += gamma * (acc + bias)        (residual stream, in place)
    EPI_F32 = 3,        // C f32 = acc + bias
    EPI_PATCH = 4,      // C f32[(m/G2)*S + cls + m%G2] = acc + pos[cls + m%G2]
    EPI_BF16_ROPE = 5,  // EPI_BF16 + axial 2-D RoPE on columns [0, rope_cols) (q and k thirds of qkv); 256 kernel only
};

struct GemmArgs {
    const bf16_t* A; long lda;   // [M][lda]  activations, K-contiguous
    const bf16_t* B; long ldb;   // [N][ldb]  weights (nn.Linear layout), K-contiguous
    int M, N, K;
    void* C; long ldc;
    const float* bias;           // [N] or null
    const float* gamma;          // [N] LayerScale or null   (EPI_RESID_F32)
    const float* pos;            // [S][N]                    (EPI_PATCH)
    int S, G2, cls;              //                           (EPI_PATCH)
    int gy;                      // XCD arrangement of the 256 x 256 kernel (set by the launcher)
    const float2* rope_cs;       // [rope_S][rope_hd/2] (cos, sin)      (EPI_BF16_ROPE)
    int rope_S, rope_hd, rope_cols;
    int prefer256;               // caller's hint: few rows but very many columns (search pre-pass) -> 256 x 256 tiles
    float* ws; long ws_elems;    // optional scratch for the split-K tail of EPI_RESID_F32 (null = never split K)
    int t192_tiles, t192_tall;         // set by the launcher (192-row form): tile rows, how many of the last are 208 rows tall
    int ksplit; long c_split_stride;   // set by the launcher: K ranges per tile, fp32 elements between partial outputs
    // EPI_RESID_F32 only, optional: the LayerNorm that reads the updated residual rows next (ln_w != null).  If the
    // launcher takes the one-image form -- ring kernel on K parts + one reduce -- the reduce also normalises its rows
    // into ln_out (bf16) and *ln_fused is set to 1: the caller then skips that LayerNorm launch (a 577-row LayerNorm is
    // nothing but its launch: 5 us of a 90-us block).  Any other form leaves *ln_fused alone.
    // (ln_w == null with ln_out set: normalise only, no affine -- the towers' gains and shifts live in the weights of
    //  the GEMM that follows, api.hip "LayerNorm folded")
    const float* ln_w; const float* ln_b; float ln_eps; bf16_t* ln_out; long ln_ldo; int* ln_fused;
    // LayerNorm folded into the two GEMMs around it.  The LayerNorm's gain lives in the next GEMM's
    // weights (W' = bf16(gamma . W), bias b' = b + W beta), so what that GEMM needs from the row is bf16(x) as its A
    // operand and the row's mean and 1/std in its epilogue:   out = rstd * (bf16(x) . W'^T - mean * c) + b',  c_j = sum_k W'_jk.
    //  * producer (EPI_RESID_F32, the GEMM that writes the residual row): lnf_xb (bf16 [M][lnf_ldxb]) receives bf16(x_new),
    //    lnf_stats ([M][N / 256] (mean, M2) of each 256-column slice of the new row: one slot per column tile, fixed
    //    order, merged by the consumer).  Only launch forms that cover ALL rows with the 256 x 256 kernels' row-coalesced
    //    epilogue do this; they set *lnf_done = 1, any other form leaves it alone (the caller then runs the LayerNorm kernel).
    //  * consumer (EPI_BF16 / _GELU / _ROPE): lnc_stats ([M][lnc_parts] as written above; the normalised width is
    //    256 * lnc_parts), lnc_c ([N] column sums of the rounded weights), lnc_eps; `bias` is b'.
    bf16_t* lnf_xb; long lnf_ldxb; float2* lnf_stats; int* lnf_done;
    // Residual stream as two bf16 planes (EPI_RESID_F32, the two whole-rows persistent forms only):
    // between the folded residual GEMMs of one forward the stream is kept as hi = bf16(x), lo = bf16(x - hi) -- x to 2^-17
    // instead of 2^-24, still 256 times finer than the bf16 GEMM operands -- because hi IS the next GEMM's A operand: the
    // epilogue moves 4 + 4 bytes per element where fp32 rows plus their bf16 copy were 4 + 4 + 2.  xp_in: the old
    // values come from (xp_hi, xp_lo) instead of C; xp_out: the new values go there instead of to C (C is then stale;
    // xp_hi must be lnf_xb).  *lnf_done = 1 also says that xp_out was honoured.
    bf16_t* xp_hi; bf16_t* xp_lo; long xp_ld; int xp_in, xp_out;
    const float2* lnc_stats; int lnc_parts; const float* lnc_c; float lnc_eps;
    // Telemetry of the folded consumer (optional; device, 3 x u64): the A operand is bf16(x) UN-CENTRED, so the fold's
    // error against LayerNorm-then-round grows with |mean| / std of a row (tests/test_gpu_ln_fold.py records the curve).
    // The 256 x 256 kernels' column-tile-0 workgroups -- each row of the launch exactly once -- add: [0] rows merged,
    // [1] rows with |mean| * rstd > LNC_TELE_RATIO, [2] rows with |mean| * rstd > 4 * LNC_TELE_RATIO.
    unsigned long long* lnc_tele;
    // Set by the launcher (queued-stores kernel only): rows [M, M + qtail_rows) -- the few rows that whole rounds of 256-row
    // tiles leave over (fc1 of PE-L14 at batch 64: 64) -- are done by the same launch, one 16-column strip per workgroup
    // behind its last tile, instead of by a launch of their own (gemm.hip gemm256q_kernel)
    int qtail_rows;
#ifdef REVO_EXPERIMENTS
    int stagger_cycles, stagger_groups;   // timing experiment (persistent kernel): phase groups, see gemm256p_kernel
    unsigned long long* stamps; int stamp_items;   // diagnostic (gemm256pp_kernel): [workgroup][item][4] 100 MHz time stamps
#endif
};
constexpr float LNC_TELE_RATIO = 8.0f;
constexpr int LNF_SLICE = 256;      // columns per partial of the folded LayerNorm's statistics = one column tile of the 256 x 256 kernel
int launch_gemm(int epi, const GemmArgs& a, hipStream_t st);
// The launch forms launch_gemm can issue (bits of revo_debug_gemm_forms, librevo_exp.so; tests/test_gpu_gemm_bounds.py lists
// them too): kernels, then properties of the launch
enum GemmForm : unsigned {
    GF_SKINNY_444 = 1u << 0,      // gemm_skinny_kernel<., 4, 4, 4>
    GF_SKINNY_411 = 1u << 1,      // gemm_skinny_kernel<., 4, 1, 1>
    GF_128_128 = 1u << 2,         // gemm128_kernel<., 128>
    GF_128_64 = 1u << 3,          // gemm128_kernel<., 64>
    GF_128R = 1u << 4,            // gemm128r_kernel (six-deep ring)
    GF_256_TILE = 1u << 5,        // gemm256_kernel, one workgroup per tile
    GF_256P = 1u << 6,            // gemm256p_kernel, 256-row tiles
    GF_256P_192 = 1u << 7,        // gemm256p_kernel, 192-row tiles
    GF_256Q = 1u << 8,            // gemm256q_kernel
    GF_256Q_QTAIL = 1u << 9,      // gemm256q_kernel with qtail_rows
    GF_SPLITK_RING = 1u << 10,    // split-K on the ring kernel + splitk_reduce_resid_kernel
    GF_SPLITK_RING_LN = 1u << 11, // split-K on the ring kernel + splitk_reduce_resid_ln_kernel
    GF_SPLITK_256 = 1u << 12,     // split-K on gemm256_kernel<EPI_F32, 4> + splitk_reduce_resid_kernel
    GF_LN_FOLDED = 1u << 13,      // producer wrote bf16(x) and the row statistics (*lnf_done)
    GF_LN_CONSUMED = 1u << 14,    // consumer applied row statistics (lnc_*)
    GF_PLANES_IN = 1u << 15,      // old residual values from the two bf16 planes
    GF_PLANES_OUT = 1u << 16,     // new residual values to the two bf16 planes
};
#ifdef REVO_EXPERIMENTS
unsigned gemm_debug_forms(int reset);
// The plan (gemm_plan.h) launch_gemm would execute under the library's current switches, for a problem given as plain values;
// offers: bit 0 a LayerNorm to fuse, 1 the folded producer, 2 planes in, 3 planes out, 4 lnc statistics, 5 prefer256 (the
// output strides of the offered forms are taken as ldc).  Host only.  out: [0] form bits (-1: the launcher refuses),
// [1] steps, then 14 values per step: form, row0, rows, gy, nslot, grid x, grid y, t192 tiles, t192 tall, qtail rows, S,
// reduce does the LayerNorm, XP, folds.  Returns the form bits, -1 for a refusal, -2 when `cap` is too small.
long gemm_debug_plan(int epi, int M, int N, int K, long lda, long ldb, long ldc, long ws_elems, unsigned offers, int rope_S,
                     int rope_hd, int rope_cols, long* out, int cap);
#endif
// EPI_F32 on 128 x 64 ring tiles whatever the tile count (few rows x very many columns: the search pre-pass of few queries)
int launch_gemm_f32_ring(const GemmArgs& a, hipStream_t st);
// true when the plan of launch_gemm(EPI_RESID_F32) (gemm_plan.h) is one of the two that can fold the LayerNorm behind it (and
// keep the residual stream in planes): the persistent 256-row kernel over ALL rows
bool gemm_resid_folds(int M, int N, int K, long lda, long ldb, long ldc);
// residual stream planes <-> fp32 (format changes at the ends of a forward's folded stretch; parity hooks)
int launch_planes_to_f32(const bf16_t* hi, const bf16_t* lo, long ldp, float* x, long ldx, long rows, int W, hipStream_t st);
#ifdef REVO_EXPERIMENTS
void gemm_set_debug(int d);           // timing experiments (results are wrong): librevo_exp.so only
void gemm_set_stagger(int cycles, int groups);
void gemm_set_stamps(unsigned long long* buf, int items);
void gemm_set_phase_groups(int g);    // 0 / 1 = off, 2..4 = forced (scripts/gemm_phase_ab.py)
#endif
void gemm_force_gy(int gy);
void gemm_set_tail_split(int on);
void gemm_force_tile(int t);   // 0 = heuristic, 128 or 256 = forced

// --------------------------------------------------------- elementwise -----
// out = LayerNorm(x) * w + b over rows of width W (fp32 statistics, two-pass).
// logits (optional, fp32 output): also the attention-pool logits of every normalised row (head.hip): row r = token r % S of
// image r / S; logits[(image * H + h) * S + token] = y . qk[h] + ck[h]
constexpr int LN_MAXH = 16;
struct LnLogits { const float* qk; const float* ck; float* logits; int H, S; };
int launch_layernorm(const float* x, long ldx, const float* w, const float* b, float eps, int rows, int W,
                     void* out, long ldo, int out_is_bf16, hipStream_t st, const LnLogits* logits = nullptr);
// (w / b null: normalise only.)  Weights of a linear layer with the LayerNorm in front of it folded in (elementwise.hip):
// out = bf16(gamma . W) [rows][ld], csum[j] = sum_k of the rounded row, bias_out = bias + W beta
int launch_fold_ln_linear(const float* w, const float* gamma, const float* beta, const float* bias, int rows, int cols,
                          bf16_t* out, long ld, float* csum, float* bias_out, hipStream_t st);
// images NCHW (u8 pixel values; f32: already normalised to [-1, 1]) -> im2col matrix for the split-precision patch GEMM:
// rows [B*G*G][parts * Kp] bf16, k = c*P*P + py*P + px zero padded to Kp, parts = 2 (u8: the exact integers 2v - 255,
// twice) or 3 (f32: hi | hi | lo of 255 x); the weights carry the 1/255 (elementwise.hip, head.hip split_hi_lo_hi)
// (img_h x img_w pixels = gh x gw patches of P x P)
int launch_patchify(const void* images, int is_u8, int B, int img_h, int img_w, int P, bf16_t* out, long Kp, hipStream_t st);
// position table [cls + G*G][W] -> [cls + gh*gw][W], bilinear with half-pixel centres (elementwise.hip)
int launch_pos_resample(const float* src, int G, int cls, int gh, int gw, int W, float* dst, hipStream_t st);
// ---- the attention-pool head in fp32 (head.hip)
int launch_probe_qk(const float* q, const float* Wk, const float* bk, int W, int heads, float* qk, float* ck, hipStream_t st);
// u [B][H][W] = softmax-weighted sums of the fp32 ln_post rows x; the logits [B][H][S] of the probe come from the
// ln_post kernel (launch_layernorm's LnLogits)
int launch_pool_head_rows(const float* x, long ldx, int B, int S, int W, int H, const float* logits, float* u, hipStream_t st);
// region_pool.hip: u [R][H][W], region r pooled over the tokens its bitmap allows (region_bits [R][ceil(S / 32)], bit s & 31 of
// word s >> 5) of image region_image[r] (device int32); every token allowed = the bits of launch_pool_head_rows; no token
// allowed = zeros.  At most 65535 regions per launch.
int launch_pool_head_rows_masked(const float* x, long ldx, int B, int S, int W, int H, const float* logits,
                                 const int* region_image, const uint32_t* region_bits, int R, float* u, hipStream_t st);
// out [R][D]: the rows of regions without an allowed token become zeros
int launch_zero_empty_regions(const uint32_t* region_bits, int R, int S, int D, float* out, hipStream_t st);
// C[M][N] (+)= epi(A . Wt^T + bias) in fp32, M small; epi 0 plain, 1 exact-erf GELU, 2 C += ; group_cols > 0: output
// columns [g * group_cols, ...) read A at A + g * a_group_stride
int launch_gemm_f32_skinny(int epi, const float* A, long lda, long a_group_stride, int group_cols, const float* Wt, long ldw,
                           const float* bias, int M, int N, int K, float* C, long ldc, hipStream_t st);
int launch_transpose_f32(const float* src, int rows, int cols, float* dst, hipStream_t st);
int launch_split_hi_lo_hi(const float* src, long rows, int cols, float scale, bf16_t* dst, long ld, hipStream_t st);
// x[b*S + 0][:] = cls + pos[0]
int launch_cls_rows(float* x, long ldx, const float* cls, const float* pos, int B, int S, int W, hipStream_t st);
// in-place interleaved-pair rotation of the q and k thirds of qkv [rows][3W]
int launch_rope(bf16_t* qkv, long ld, const float2* cs, int rows, int S, int W, int heads, hipStream_t st);
// dst[r][0..cols) = bf16(src[r][0..cols)), dst[r][cols..ld_dst) = 0
int launch_f32_to_bf16(const float* src, long ld_src, bf16_t* dst, long ld_dst, long rows, int cols, hipStream_t st);
// row-wise L2 normalise; writes fp32 and/or bf16 copies (either may be null)
// normalize = 0: rows copied unscaled.  row_stats [rows][2] (optional): (||bf16(y) - y||, ||bf16(y)||) per output row;
// max_stats [2] (optional): running maxima (fp32 bit patterns) of ||y|| and ||bf16(y) - y||  -- inputs of the search's
// exactness certificate
// zero_a / zero_b (optional): two word arrays the kernel also clears (a search's counters and histograms: its first kernel
// does what two memset launches did)
int launch_l2norm_rows(const float* src, long ld_src, float* dst_f32, long ld_f32, bf16_t* dst_bf16, long ld_bf16,
                       long rows, int D, hipStream_t st, int normalize = 1, float* row_stats = nullptr,
                       uint32_t* max_stats = nullptr, uint32_t* zero_a = nullptr, long zero_a_words = 0,
                       uint32_t* zero_b = nullptr, long zero_b_words = 0, const long long* dst_rows = nullptr);
// (dst_rows, optional, device [rows]: output row i goes to row dst_rows[i] of dst_f32 / dst_bf16 instead of row i -- the
//  overwrite of gallery rows, revo_gallery_update; row_stats stays indexed by i)

// ------------------------------------------------- gallery edit (gallery_edit.hip) ----
constexpr long REMOVE_MAX_CHUNK = 65536;   // rows per chunk of a removal at most (a workgroup sums the chunk's words in front of its own)
// per chunk c of `chunk` rows (a multiple of 32) of a remove-bitmap over N rows: cnt[c] = rows of the chunk whose bit is clear,
// first[c] = offset in the chunk of its first row whose bit is set (the chunk's row count if none)
int launch_remove_count(const uint32_t* bits, long N, long chunk, uint32_t* cnt, uint32_t* first, hipStream_t st);
// the rows [row0, row0 + len) of src (rows of u4_per_row 16-byte units) whose bit is clear, gathered in order: the row with
// j kept rows of the chunk in front of it goes to row j of dst, for j >= j0.  row0 % 32 == 0, len <= REMOVE_MAX_CHUNK; dst must
// not overlap the source rows
int launch_remove_gather(const uint32_t* bits, long N, long row0, long len, long j0, const uint4* src, uint4* dst,
                         int u4_per_row, hipStream_t st);

// ----------------------------------------------------------- attention -----
// qkv [B*S][ld] bf16 (q | k | v thirds, heads contiguous inside a third) -> out [B*S][ldo] bf16
int launch_attention(const bf16_t* qkv, long ld, bf16_t* out, long ldo, int B, int S, int H, int hd, hipStream_t st);
// has_cls: row 0 is the class token and may be scheduled apart from the patch rows (same result)
int launch_attention_ex(const bf16_t* qkv, long ld, bf16_t* out, long ldo, int B, int S, int H, int hd, int has_cls,
                        hipStream_t st);
// ---- the text tower's kernels (text.hip)
// causal attention on the same qkv layout: 1 <= S <= ATTC_MAX_S, hd 64; output row i depends on rows 0..i alone, bit for bit
constexpr int ATTC_MAX_S = 128;
int launch_attention_causal(const bf16_t* qkv, long ld, bf16_t* out, long ldo, int B, int S, int H, int hd, hipStream_t st);
// x[b * S + s][:] = table[tokens[b * S + s]] + pos[s] (tokens: device; an id outside [0, vocab) gives a row of NaN)
int launch_embed_tokens(const int32_t* tokens, const float* table, const float* pos, int B, int S, int vocab, int W, float* x,
                        long ldx, hipStream_t st);
// out[b][:] = x[b * S + p][:], p = the first position of prompt b's largest token id
int launch_pool_eot(const int32_t* tokens, const float* x, long ldx, int B, int S, int W, float* out, hipStream_t st);
void gemm_set_min_tiles256(int n);  // timing experiments only (default 100)
void gemm_set_ring(int on, int max_tiles);   // timing experiments only (default on, 256 tiles)
void gemm_set_splitk(int on);       // timing experiments only (1 = default)
void gemm_set_persistent(int on);   // timing experiments only (1 = default)
void gemm_set_qstores(int on);      // timing experiments only (1 = default): 0 = the bf16 epilogues on gemm256p_kernel (stores drained before the next main loop)
void gemm_set_rows192(int on);      // timing experiments only (1 = default)
void gemm_set_ln_fold(int on);      // timing experiments only (1 = default): 0 = LayerNorm kernels instead of the folded form, 2 = folded with an fp32 stream
bool gemm_ln_planes_enabled();
void attention_force_nw(int nw);   // timing experiments only (0 = heuristic)
void attention_set_shape16(int on); // head_dim 64: 1 = the v_mfma_f32_16x16x32_bf16 kernel (attn16_fwd_kernel), 0 = the 32x32x16 one
#ifdef REVO_EXPERIMENTS
// diagnostic: every workgroup of the body attention kernel writes (shader-clock ticks, 100 MHz ticks) of its lifetime to
// buf[workgroup][2] (device; null = off): the clock the chip holds under this kernel (MI355X_MICROARCH.md, DVFS item 6)
void attention_set_clock_buffer(unsigned long long* buf);
#endif

// ---------------------------------------------------------------- top-k ----
struct ScanArgs {
    const bf16_t* Qb; long ldq;   // [Q][D] bf16 normalised queries
    const bf16_t* Gb; long ldg;   // [N][D] bf16 normalised gallery rows
    int Q; long N; int D;
    int ksel;                     // candidates kept per query (32 or 64)
    int splits;                   // gallery splits (grid.y); part is [Q][splits][ksel]
    uint64_t* part;               // out: candidate keys, sorted best-first, 0 = empty
    const uint32_t* allow;        // optional allow-bitmap (revo_search_set_filter; padded to whole 256-row tiles)
};
int topk_scan_workspace_splits(int Q, long N);
int launch_topk_scan(const ScanArgs& a, hipStream_t st);
// merge `splits` sorted candidate lists per query into one list of ksel keys (in place into part[q][0])
int launch_topk_reduce(uint64_t* part, int Q, int splits, int ksel, hipStream_t st);
// ---- exactness certificate and its fallback (topk.hip: finish; topk256.hip: collect; topk_exact.hip: the rest) ----
// The scan selects on bf16-input scores; the finish step re-scores its ksel candidates in fp32.  A query is CERTIFIED
// when the score a row needs to enter the result exceeds the best bf16 score any un-re-scored row can have by more
// than eps, a rigorous bound of |bf16-scan score - fp32 score|.  Uncertified queries are handed
// to the collect pass (every row whose bf16 score is within eps of what is needed, re-scored exactly), and queries
// whose collect list overflows to a brute-force fp32 pass over the whole gallery.  All of it is enqueued on the
// stream with device-side counts: no host round trip.
constexpr int EXACT_COL_CAP = 2048;     // collected keys per uncertified query
constexpr int EXACT_L3_SLICES = 32;     // gallery slices of the brute-force pass (their 64-key lists reuse the query's collect buffer)
static_assert(EXACT_L3_SLICES * 64 == EXACT_COL_CAP, "the brute-force partial lists live in the collect buffer");
// the slots of ExactWs::ctr
enum ExactCtr : int {
    CTR_UNCERTIFIED,     // uncertified queries of this search
    CTR_BRUTEFORCE,      // of those: collect list overflowed -> brute force
    CTR_CHECKED,         // queries the certificate was evaluated for
    CTR_COLLECTED,       // rows collected (all lists)
    CTR_MODE3_FAILED,    // mode 3: failed (counted only)
    CTR_FROM_SEGS,       // uncertified queries resolved from the scan's segments (numbered from the back)
    CTR_GROUPED,         // grouped searches: queries sent to the grouped fallback (GroupWs)
    CTR_LARGE_FALLBACK,  // large-k searches: queries sent to the exhaustive fallback (LargeWs)
    CTR_PAIR_PASSES,     // revo_gallery_pairs: join passes run (1, or 2 after a workspace regrow)
    CTR_SLOTS
};
struct ExactWs {
    int* ctr;            // [CTR_SLOTS] counters of the last search (ExactCtr)
    int* unc_q;          // [cap] query index of uncertified entry j (or the output row, see out_compact)
    float* unc_lb;       // [cap] bf16-score bound of entry j's collect pass
    bf16_t* qb_u;        // [cap][ldqb] its bf16 query row (compacted: the collect pass reads whole query tiles)
    long ldqb;
    int* col_cnt;        // [cap] rows appended to entry j's list (may exceed EXACT_COL_CAP: overflow)
    uint64_t* col;       // [cap][EXACT_COL_CAP] keys (bf16 score, row)
    int* over_j;         // [cap] entries that overflowed
    int* orow;           // [cap] out_compact results: the output row of entry j (its place in the caller's list)
    int cap;             // entries the arrays hold.  Entries the finish step fills from the scan's own segments (no gallery
                         // pass needed) are numbered from the BACK: cap - 1, cap - 2, ...; their count is ctr[CTR_FROM_SEGS]
};
// ---- grouped search (revo_search_groups; topk_exact.hip).  The exact top-GROUP_K1 rows of the ungrouped search decide a
// query's groups when they certify it (topk_group_select_kernel); other queries are entries of the grouped fallback:
// pass A (bruteforce_body, group mode) finds the best groups over the whole gallery in fp32, pass B (group_size > 1) the
// best rows of the chosen groups.  Entry count: ExactWs::ctr[CTR_GROUPED]; slice lists: ExactWs::col, as for the brute force.
constexpr int GROUP_K1 = 50;
struct GroupWs {
    const int* group_of_row;   // [N] group of each row, -1 = none
    int* gq;                   // [cap] query of fallback entry i
    int* chosen;               // [cap][64] entry i's best groups after pass A, best first, -1 padded
    int hits;                  // 0: pass A; group_size: pass B
    int has_thr; float thr;
};
struct GroupOut {
    float* scores; long long* idx;   // [Q][limit][group_size]
    int* hit_counts; int* group_ids; // [Q][limit]
    int* group_counts;               // [Q]
    int limit, group_size;
    long idx_offset;
};
int launch_topk_group_select(const float* s1, const long long* i1, const int* c1, int Q, const ExactWs& ws, const GroupWs& gw,
                             int force_fallback, const GroupOut& o, hipStream_t st);
int launch_topk_group_fallback(const ExactWs& ws, GroupWs gw, int max_entries, const float* Qf, long ldqf, const float* Gf,
                               long ldgf, long N, int D, const uint32_t* allow, const GroupOut& o, hipStream_t st);
// The scan's segments of one launch part (queries [q0, q0 + nq) of the search): every survivor the scan appended
struct SegSrc { const uint64_t* seg; const int* cnt; int splits, q0, nq; };
struct CertArgs {
    const float* qstat;      // [Q][2] (||qb - qf||, ||qb||) from the query normalisation
    const uint32_t* gstat;   // [2] fp32 bit patterns: max ||g||, max ||gb - g|| over the gallery's rows
    int mode;                // 0 = certificate + fallback, 1 = every query takes the collect path, 2 = every query takes the
                             // brute-force path, 3 = certificate only (counted, no fallback: the pre-certificate behaviour)
    ExactWs ws;
    const bf16_t* Qb; long ldq;   // the search's bf16 query rows (source of qb_u)
    float* cert_out;         // row-sharded search: [Q] this shard's bound U + eps for the merge step's certificate (then no
                             // local decision is taken); null otherwise
    // Resolving an uncertified query WITHOUT another pass over the gallery (nsegs > 0: the scan ran with an admission
    // margin, launch_topk_scan256): the scan admitted every row scoring at least max(pre-pass bound, bound - marg[q]),
    // where `bound` is any lower bound of the query's ksel-th best scan score it held at the time -- so every row with
    // scan score >= max(base, U - marg[q]), U = the ksel-th best scan score, sits in the query's segments (or, a
    // pre-pass row, in prelist), unless a drain or a recomputed tile touched the query (dropflag).  If the bound the
    // collect pass would use reaches that level, the finish step fills the entry's list from there.
    SegSrc segs[2]; int nsegs;
    int seg_ksel;                // ksel of the scan (segments hold 2 * ksel keys)
    const uint64_t* prelist;     // [Q][ksel] the pre-pass rows' best keys
    const uint32_t* tau_base;    // [Q] the pre-pass bound (order-preserving u32) -- or, `estimated`, the estimate the scan started from
    int estimated;               // the scan's starting admission scores were estimates (a shard of a larger gallery): finish counts
                                 // them as the score an unseen row can have
    const float* marg;           // [Q] admission margins
    const int* dropflag;         // [Q] != 0: the query's segments may be incomplete or hold repeated keys
};
// marg[q] = 2 eps(q) (+ rounding slack), dropflag[q] = 0: the admission margins of a scan whose uncertified queries are
// to be resolved from its segments
int launch_cert_margin(const float* qstat, const uint32_t* gstat, int D, int Q, float* marg, int* dropflag, hipStream_t st);
// exact fp32 re-score of the ksel candidates of each query, final order (score desc, index asc),
// threshold cut, write k results.  Gf may be null: then the bf16-scan scores are returned (and nothing is certified).
// all_bounds (optional): [parts][Q][top_m] order-preserving u32 scores published by every shard of a row-sharded
// gallery; only candidates at or above their ksel-th largest (a lower bound of the global ksel-th best) are re-scored.
// cert (optional): evaluate the exactness certificate and hand uncertified queries to the fallback workspace.
int launch_topk_finish(const uint64_t* part, long part_stride, int ksel, const float* Qf, long ldqf, const float* Gf,
                       long ldgf, int D, int Q, int k, int has_thr, float thr, long idx_offset, const uint32_t* all_bounds,
                       int parts, int top_m, float* out_scores, long long* out_idx, int* out_counts, const CertArgs* cert,
                       hipStream_t st);
// rigorous bound of |bf16-scan score - fp32 re-score| for a query with (e_q, n_qb) against rows with (G, Eg); see DESIGN.md
__host__ __device__ inline float cert_eps(float e_q, float n_qb, float G, float Eg, int D) {
    const float gam1 = (float)D * 1.1920929e-7f;      // D * 2^-23: fp32 accumulation of the MFMA chain (truncation allowed)
    const float gam2 = (float)D * 5.9604645e-8f;      // D * 2^-24: the fp32 fma chain of the re-score
    const float eps = e_q * G + n_qb * Eg + gam1 * n_qb * (G + Eg) + gam2 * (n_qb + e_q) * G;
    return eps * 1.001f + 1e-30f;
}
struct Collect256Args {
    const bf16_t* Qb; long ldq;   // compacted bf16 query rows of the uncertified entries
    const bf16_t* Gb; long ldg;
    long N; int D;
    int splits, small_modes;      // set by the launcher
    const int* n_q;               // device: number of entries (query tiles past it exit)
    const float* lb;              // [entries] bf16-score bound
    int* cnt;                     // [entries] rows appended
    uint64_t* col;                // [entries][cap]
    int cap;
    const uint32_t* allow;        // optional allow-bitmap (revo_search_set_filter; padded to whole 256-row tiles): rows whose bit is clear are skipped
};
int launch_topk_collect256(const Collect256Args& a, int max_queries, hipStream_t st);
int topk_collect256_splits(long N);   // the collect pass's slicing, which the large-k count pass shares
// Slices of a pass that walks `tiles` gallery tiles against one fixed query tile (recommend, discover, MaxSim): one workgroup
// per CU, every slice at least three tiles (scan_plan.h: a slice costs its tiles plus about one tile time of fixed work)
int pass256_slices(long tiles);
// What the 256 x 256 main loop asks of its operands, checked by every launcher that runs it (`who`: the entry point's name
// in the messages; ldq = 0: both operands are gallery rows)
inline int g256_check_operands(const char* who, int D, long ldg, long ldq = 0) {
    REVO_REQUIRE(D % 64 == 0 && ldq % 8 == 0 && ldg % 8 == 0, std::string(who) + ": D must be a multiple of 64");
    REVO_REQUIRE(256l * ldg * 2 < (1l << 31) && 256l * ldq * 2 < (1l << 31), std::string(who) + ": row too long for the DMA window");
    return 0;
}
// Fallback passes over the entries ws.ctr[CTR_UNCERTIFIED] (device count; launches are sized for max_entries).
// exact_finish: fp32 re-score of every collected row, exact top-k; entries whose list overflowed go to ws.over_j.
// bruteforce: for those, the fp32 score of EVERY gallery row (same fma chain as the re-score), exact top-k.
// out_compact = 0: results go to row unc_q[j] of the outputs; 1: to row j (unc_q then only names the query row in Qf).
int launch_topk_exact_finish(const ExactWs& ws, int max_entries, const float* Qf, long ldqf, const float* Gf, long ldgf,
                             int D, int k, int has_thr, float thr, long idx_offset, int force_bruteforce, int out_compact,
                             float* out_scores, long long* out_idx, int* out_counts, hipStream_t st);
int launch_topk_exact_bruteforce(const ExactWs& ws, int max_entries, const float* Qf, long ldqf, const float* Gf, long ldgf,
                                 long N, int D, int k, int has_thr, float thr, long idx_offset, int out_compact,
                                 float* out_scores, long long* out_idx, int* out_counts, hipStream_t st,
                                 const uint32_t* allow = nullptr);
// (allow, optional: the allow-bitmap of a filtered search; the brute force skips rows whose bit is clear)
// entries from an explicit list (the row-sharded search's second round): entry j = query q_idx[j], collect bound
// need[j] - eps(query, this gallery); sets ws.ctr[CTR_UNCERTIFIED] = n
int launch_topk_exact_prepare(const ExactWs& ws, const int* q_idx, const float* need, int n, const CertArgs& cert, int D,
                              const uint64_t* cand, long cand_stride, int ksel, hipStream_t st);
// (cand: the handle's candidate lists of the last scan, [Q][cand_stride], best first: with segments to draw from
//  (cert.nsegs > 0) an entry whose bound they cover is filled from them and numbered from the back, ExactWs::cap;
//  every ws.ctr slot must be zero when this runs)
// bounds[q][0..top_m) = order-preserving u32 scores of the query's best top_m candidates (0 = none)
int launch_topk_publish(const uint64_t* part, long part_stride, int Q, int top_m, uint32_t* bounds, hipStream_t st);
// 256 x 256 tile scan (topk256.hip): survivors are appended to per-(query, slice) segments of 2 * ksel keys and
// counted in per-query score histograms; launch_topk_reduce_segs then picks each query's best ksel keys
int topk_scan256_splits(int Q, long rows);
// queries the main launch of a search takes; the rest (a ragged tail of <= 128 queries) runs as a second launch in the
// small-query mode of the kernel when that is cheaper (Q = one launch)
int topk_scan256_main_queries(int Q, long rows);
long topk_scan256_plan_dump(int Q, long rows, long* out, int cap);   // the launch's phases (reporting / CPU tests)
int topk_scan256_hist_buckets();      // u32 counters per query in `hist`
int topk_scan256_hist_shift();        // bucket width = 2^shift ulps of the fp32 score above the pre-pass bound
#ifdef REVO_EXPERIMENTS
void topk_scan256_set_debug(int d);   // timing experiments (bit 0 / 2: results are wrong): librevo_exp.so only
unsigned long long* topk_scan256_stats();
#endif
// seg [Q][splits][2 ksel] keys, seg_cnt [Q][splits]; tau_g [Q] live admission bounds (in: = tau_base), tau_base [Q]
// the pre-pass bound (constant), hist [Q][buckets] zeroed and then seeded by launch_topk_select_rows
int launch_topk_scan256(const bf16_t* Qb, long ldq, const bf16_t* Gb, long ldg, int Q, long N, int D, long n_begin,
                        int splits, uint64_t* seg, int* seg_cnt, uint32_t* tau_g, const uint32_t* tau_base, uint32_t* hist,
                        int ksel, hipStream_t st, const float* marg = nullptr, int* dropflag = nullptr,
                        const uint32_t* allow = nullptr);
// allow (optional): the search's allow-bitmap, zero-padded to whole 256-row tiles; n_begin must then be a multiple of 256
// marg / dropflag (optional, [Q]): admit every score >= max(pre-pass bound, bound - marg[q]) instead of >= bound, and flag
// the queries whose segments a drain or a recomputed tile touched (CertArgs: the finish step's segment collect)
// out[q][ksel] = best ksel distinct keys (sorted, best first) of prelist[q][ksel] and the query's segments;
// bounds (optional) [Q][top_m]: the order-preserving u32 scan scores of each query's best top_m candidates (what
// launch_topk_publish writes: the row-sharded search's published admission scores, without a launch of their own)
int launch_topk_reduce_segs(const uint64_t* seg, const int* seg_cnt, int splits, const uint64_t* prelist, uint64_t* out,
                            int Q, int ksel, hipStream_t st, uint32_t* bounds = nullptr, int top_m = 0);
// pre-pass of the 256 x 256 scan: KSEL best columns of every row of a [Q][n] fp32 score matrix -> part[q][slot];
// tau0[q] = the KSEL-th score; hist (optional): the kept scores are counted into the query's histogram
int launch_topk_select_rows(const float* scores, long ld, int n, int Q, uint64_t* part, long part_row_stride, int slot,
                            uint32_t* tau0, int ksel, uint32_t* hist, int hist_buckets, int hist_shift, hipStream_t st,
                            uint32_t* tau_copy = nullptr, float est_z = 0.f, const uint32_t* allow = nullptr);
// (est_z != 0: tau0[q] = max(KSEL-th best score, mean + est_z * sigma of the row's scores): an estimated admission level)
// ---- large-k search (revo_search_topk_large; topk_large.hip): sample bound, count pass, level, collect
// of the band, fp32 finish; queries whose band may exceed LARGE_CAP rows take the exhaustive fallback
constexpr int LARGE_K_MAX = 1024;
constexpr int LARGE_NB = 4096;         // count-pass buckets per query (about eps / 4 each)
constexpr int LARGE_CAP = 8192;        // band rows per query: what the finish sorts in LDS (64 KiB of keys)
constexpr int LARGE_LVL = 8;           // floats per query in LargeWs::lvl: lo, bucket base, 1 / step, step, eps
constexpr int LARGE_FB_SLICES = 256;   // gallery slices of the fallback's scoring pass
struct LargeWs {
    float* lvl;            // [Q][LARGE_LVL]
    uint32_t* hist;        // [Q][LARGE_NB] (zeroed by the search's first kernel)
    int* ctr;              // [0] band entries, [1] fallback entries (zeroed with hist)
    int* band_q; float* band_lb; int* band_cnt;   // [Q]: band entry j's query, collect bound, rows collected
    bf16_t* band_qb;       // [Q][D] band entry j's bf16 query row (the collect pass reads compacted query tiles)
    uint64_t* band_col;    // [Q][LARGE_CAP] band entry j's keys: bf16 keys from the collect pass, fp32 keys after the re-score
    int* fb_q;             // [Q] fallback entry i's query
    float* fb_scores;      // [F][N] the fp32 scores of one round of fallback entries (NaN: row not allowed)
    int F;
    int* stats;            // ExactWs::ctr of the handle (CTR_COLLECTED, CTR_LARGE_FALLBACK)
};
struct LargeCountArgs {
    const bf16_t* Qb; long ldq; const bf16_t* Gb; long ldg;
    long N; int D, nq, splits;
    const float* lvl; uint32_t* hist;
    const uint32_t* allow;       // optional allow-bitmap, padded to whole 256-row tiles
};
// pre: [Q][ld] bf16-GEMM scores of the first n_s rows (n_s = 0: no sample, lo = -inf)
int launch_topk_large_sample(const float* pre, long ld, int n_s, const uint32_t* allow, const float* qstat, const uint32_t* gstat,
                             int D, int Q, int k, int has_thr, float thr, const LargeWs& ws, hipStream_t st);
int launch_topk_large_count(const bf16_t* Qb, long ldq, const bf16_t* Gb, long ldg, long N, int D, int Q, const LargeWs& ws,
                            const uint32_t* allow, hipStream_t st);
int launch_topk_large_level(const LargeWs& ws, const bf16_t* Qb, long ldq, int D, int Q, int k, int force_fallback, hipStream_t st);
// band entries: fp32 re-score, sort, results to row band_q[j] of the outputs (launches sized for max_entries)
int launch_topk_large_finish(const LargeWs& ws, int max_entries, const float* Qf, long ldqf, const float* Gf, long ldgf, int D,
                             int k, int has_thr, float thr, long idx_offset, float* out_scores, long long* out_idx,
                             int* out_counts, hipStream_t st);
int launch_topk_large_fallback(const LargeWs& ws, int max_entries, const float* Qf, long ldqf, const float* Gf, long ldgf, long N,
                               int D, int k, int has_thr, float thr, long idx_offset, float* out_scores, long long* out_idx,
                               int* out_counts, const uint32_t* allow, hipStream_t st, int skip_self = 0);
// (skip_self: Qf IS Gf and an entry's query is a gallery row -- revo_gallery_knn: that row itself is left out, by index)
// ------------------------------------------------- candidate pipeline ----
// Pairs, range and recommend searches: join on the 256 x 256 main loop -> counted candidate buffer,
// fp32 re-score -> 64-bit sort keys, sort, emit.  Shared device code: candidates.h; host side: candidate_search.hip's CandidateWs.
// ---- the sort and the prefix sum (radix_sort.hip)
constexpr int SORT_MAX_BLOCKS = 2048;        // at most this many blocks per radix pass (the offsets scan is one workgroup)
// ascending sort of n (key, value) entries over the low key_bits bits; cnt: 256 * SORT_MAX_BLOCKS words; the result is in
// (*out_keys, *out_vals), one of the two buffer pairs
int launch_sort_keys_u64(uint64_t* keys, float* vals, uint64_t* keys_alt, float* vals_alt, long n, int key_bits, uint32_t* cnt,
                         uint64_t** out_keys, float** out_vals, hipStream_t st);
// inclusive prefix sums of c[0 .. n) in place (one workgroup)
int launch_inclusive_sums_u64(unsigned long long* c, long n, hipStream_t st);
// ---- near-duplicate pairs of one gallery (revo_gallery_pairs; pairs.hip): the join walks the upper triangle of row-tile pairs
constexpr long PAIRS_WS_KEYS = 1l << 20;     // candidate keys the workspace holds before its first regrow
constexpr long PAIRS_MAX_CAND = 1l << 28;    // candidate pairs a call may have (2 GiB of keys); more: status -2
struct PairsJoinArgs {
    const bf16_t* Gb; long ldg;   // the gallery's bf16 rows
    long N; int D;
    long T, pairs;                // set by the launcher: row tiles, tile pairs of the upper triangle
    const uint32_t* gstat;        // [2] the gallery's running maxima (max ||g||, max ||gb - g||), fp32 bit patterns
    float thr;
    const uint32_t* allow;        // optional allow-bitmap, padded to whole 256-row tiles
    unsigned long long* cnt;      // candidates found (counts past cap)
    uint64_t* keys; long cap;     // [cap] candidate keys (i << 32) | j
};
int launch_pairs_join(const PairsJoinArgs& a, hipStream_t st);
// sets a.T, a.pairs and the join's grid (0: no rows); `who` names the caller in the messages (pairs.hip; clusters.hip joins by it too)
int pairs_join_plan(PairsJoinArgs& a, const char* who, long* wgs);
// fp32 score of candidates [0, n); those >= thr appended to out_keys ((i << b) | j) / out_scores, count in *kept
int launch_pairs_rescore(const uint64_t* cand, long n, const float* Gf, long ldg, int D, float thr, int b,
                         unsigned long long* kept, uint64_t* out_keys, float* out_scores, hipStream_t st);
int launch_pairs_emit(const uint64_t* keys, const float* vals, long n, int b, long long* pairs, float* scores, hipStream_t st);
// ---- duplicate clusters (revo_gallery_clusters; clusters.hip): the pairs join with a union-find
// (unionfind.h) in its epilogue -- certain edges are merged in place, only the pairs inside the rounding bound are stored
struct ClustersJoinArgs {
    PairsJoinArgs j;              // the pairs join's arguments (cnt / keys / cap: the AMBIGUOUS pairs)
    uint32_t* parent;             // [N + 1] the union-find, parent[r] <= r; parent[N]: the device error word (a union-find
                                  // loop hit its trip limit) -- one pointer: the join has no scalar register to spare
};
int launch_clusters_init(uint32_t* parent, uint32_t* sizes, long N, unsigned long long* ctr4, hipStream_t st);
int launch_clusters_join(const ClustersJoinArgs& a, hipStream_t st);
// fp32 score of the ambiguous pairs [0, n); those >= thr are united
int launch_clusters_rescore(const uint64_t* cand, long n, const float* Gf, long ldg, int D, float thr, uint32_t* parent,
                            long N, hipStream_t st);
// labels[r] = root of r (-1: not allowed), sizes[root] = rows of its component; then the rows of components of >= 2 rows as
// keys (label << b) | row (count: ctr4[0]; clusters: ctr4[1]; ctr4[2] = the error word)
int launch_clusters_labels(uint32_t* parent, const uint32_t* allow, long N, int b, long long* labels, uint32_t* sizes,
                           uint64_t* keys, unsigned long long* ctr4, hipStream_t st);
// sorted keys -> members; rank [n] workspace; offsets [n_clusters + 1]
int launch_clusters_emit(const uint64_t* keys, long n, long n_clusters, int b, unsigned long long* rank, long long* members,
                         long long* offsets, hipStream_t st);
// ---- deduplicating append (revo_gallery_append_unique; dedup.hip): the pairs join restricted to the tile
// pairs whose column tile holds a batch row (dedup_plan.h), certain edges applied in place, a one-workgroup greedy selection
constexpr long DEDUP_MAX_BATCH = 16384;      // batch rows of one call (the n x n bit matrix: 32 MB; the kept bitmap: 2 KB of LDS)
constexpr uint32_t DEDUP_NONE = 0xffffffffu; // first_old / rep: no row
// the edges of one call, one array of words: first_old [dedup_pad(n)] | mat [n][dedup_words(n)].  first_old[j]: the lowest
// gallery row that is a neighbour of batch row j (DEDUP_NONE: none); bit i of mat row j: batch rows i < j are neighbours.
// (One pointer, the sizes derived from n: the join has no scalar register to spare.)
__host__ __device__ inline uint32_t dedup_words(long n) { return (uint32_t)((n + 63) / 64 * 2); }   // even: read as 64-bit words
__host__ __device__ inline uint32_t dedup_pad(long n) { return (uint32_t)((n + 63) / 64 * 64); }
inline size_t dedup_edge_words(long n) { return (size_t)dedup_pad(n) + (size_t)n * dedup_words(n); }
struct DedupJoinArgs {
    PairsJoinArgs j;              // the pairs join's arguments over all N0 + n rows (allow unused; cnt / keys / cap: the AMBIGUOUS pairs)
    uint32_t N0;                  // gallery rows in front of the batch
    uint32_t* edges;
};
int launch_dedup_join(const DedupJoinArgs& a, hipStream_t st);
// fp32 score of the ambiguous pairs [0, n); those >= thr become edges (nb: batch rows)
int launch_dedup_rescore(const uint64_t* cand, long n, const float* Gf, long ldg, int D, float thr, uint32_t* edges, long N0,
                         long nb, hipStream_t st);
struct DedupSelectArgs {
    const uint32_t* edges;
    long n, N0;
    uint32_t* rep;                // [n] the representative's row BEFORE the compaction (batch row i: N0 + i); DEDUP_NONE: kept
    long long* rows;              // [n] the row's own final row, or its representative's
    uint32_t* n_kept;             // [1]
};
int launch_dedup_select(const DedupSelectArgs& a, hipStream_t st);
// scores [n] (-inf: kept) and the remove-bitmap (nwords words) of the dropped rows over the rows from N0 & ~31 on
int launch_dedup_finish(const uint32_t* rep, long n, long N0, const float* Gf, long ldg, int D, float* scores, uint32_t* bits,
                        long nwords, hipStream_t st);
// ---- exact kNN graph (revo_gallery_knn; knn.hip): the pairs join with a level PER ROW.  An estimated
// level t_r for every row (sample pass), the join keeps pair (i, j) when its bf16 score reaches min(lb_i, lb_j), the re-score
// turns a candidate into a directed entry for every end whose level it reaches, sort by (row, score), select with a
// certificate per row; rows without one take the exhaustive fp32 fallback of the large-k search (LargeWs)
constexpr int KNN_K_MAX = 64;
constexpr long KNN_SAMPLE = 8192;            // sample rows of the level pass (at most); no more allowed rows: no estimate
constexpr long KNN_MIN_KEYS = 1l << 16;      // candidate keys of the smallest workspace
constexpr long KNN_MAX_KEYS = 1l << 28;      // and of the largest (the workspace takes 48 bytes per key)
constexpr size_t KNN_FB_BYTES = 256ul << 20; // the fallback's score buffer: rows of a round = this / (4 N), 1 .. 1024
// sample row s is gallery row s * stride; S sample rows.  Sb [ST * 256][D] their bf16 rows (rows past S: zeros), sallow
// [ST * 8] the bitmap of the ALLOWED sample rows; ctr[2] counts the allowed rows of the gallery, ctr[3] those of the sample
int launch_knn_sample(const bf16_t* Gb, long ldg, long N, int D, long S, long stride, const uint32_t* allow, bf16_t* Sb,
                      uint32_t* sallow, unsigned long long* ctr, hipStream_t st);
struct KnnLevelArgs {
    const bf16_t* Gb; long ldg;   // the gallery's bf16 rows
    long N; int D;
    const bf16_t* Sb; long S, stride;   // the sample (launch_knn_sample)
    const uint32_t* sallow;
    float *sum, *sq;              // [4][rows] per wave column: sum and sum of squares of row r's bf16 scores against the allowed
    long rows;                    // sample rows other than r itself; rows = the gallery's rows padded to whole 256-row tiles
    const float* lb;              // null, or the counting pass: sum = the count of those scores that reach lb[r]
};
int launch_knn_level_pass(const KnnLevelArgs& a, hipStream_t st);
// behind the counting pass: rows whose bound far too many sample rows reach get level = lb = +inf (the fallback's) and leave
// the sample (sallow; pruned[0], zeroed by the caller, counts them)
int launch_knn_dense_rows(const KnnLevelArgs& a, const unsigned long long* ctr, int k, uint32_t* sallow, int* pruned, float* level,
                          float* lb, hipStream_t st);
// level[r] / lb[r] for r < rows (rows: padded to whole tiles; a row past N or not allowed: +inf / +inf).  level_mode: the
// debug knob (include/revo.h revo_debug_set_knn); have_pass = 0: no sample pass ran, every level is the floor; keep_dense: the
// second round -- rows launch_knn_dense_rows set to +inf stay there; pruned[0]: the sample rows it took out
int launch_knn_levels(const KnnLevelArgs& a, const uint32_t* allow, const uint32_t* gstat, const unsigned long long* ctr, int k,
                      int has_thr, float thr, int level_mode, int have_pass, int keep_dense, const int* pruned, float* level,
                      float* lb, hipStream_t st);
struct KnnJoinArgs {
    PairsJoinArgs j;              // the pairs join's arguments (thr unused)
    const float* lb;              // [T * 256] the rows' bf16-score bounds
    uint32_t* lost;               // [T * 8] bit r: a candidate key of row r found no room in the workspace
};
int launch_knn_join(const KnnJoinArgs& a, hipStream_t st);
// fp32 score v of candidates [0, n): a directed entry (row << 32 | ~orderable score, partner) for row i when v >= level[i] and
// one for row j when v >= level[j]; count in *kept; out arrays hold 2 n entries
int launch_knn_rescore(const uint64_t* cand, long n, const float* Gf, long ldg, int D, const float* level,
                       unsigned long long* kept, uint64_t* out_keys, float* out_partner, hipStream_t st);
// sorted entries -> each row's best k by (score desc, index asc), padding and counts; a row without a certificate is appended
// to fb_q (count: fb_ctr[1]).  floor_level: the threshold or -inf
int launch_knn_select(const uint64_t* keys, const float* partner, long n, long N, int k, float floor_level, const float* level,
                      const uint32_t* lost, const uint32_t* allow, int* fb_q, int* fb_ctr, float* scores, long long* idx,
                      int* counts, hipStream_t st);
// ---- exact spherical k-means (revo_gallery_kmeans; kmeans.hip): an assignment is two walks of every row
// tile over the centroid tiles (best bf16 score per row; candidates inside the rounding band of it), an fp32 re-score folded
// per row, a finish; an update is a sort by (label, row), chunked fp32 sums in a fixed order and the append's normalisation
constexpr long KMEANS_MAX_CENTROIDS = 65536;
constexpr int KMEANS_MAX_ITER = 1000;
constexpr long KMEANS_MIN_KEYS = 1l << 16;   // candidate keys of the smallest workspace
constexpr long KMEANS_MAX_CAND = 1l << 28;   // candidates an assignment may have (2 GiB of keys); more: status -2
// per row, once per call: inv [N] = the factor the query normalisation gives the row's fp32 master row; rstat [N][2] =
// (||inv gb - fl(g inv)||, inv ||gb||), the row's rounding norms against its own bf16 scan row
int launch_kmeans_rows(const float* Gf, const bf16_t* Gb, long ldg, long N, int D, float* inv, float* rstat, hipStream_t st);
struct KmeansAssignArgs {
    const bf16_t* Gb; long ldg;   // the gallery's bf16 rows
    long N; int D;
    const bf16_t* Cb; long C;     // the centroids' bf16 rows, [ceil(C / 256) * 256][D], zero rows past C
    long rows;                    // the gallery's rows padded to whole 256-row tiles
    float* best;                  // [4][rows] per wave column: the row's largest bf16 score over the centroids
    float* thr;                   // [rows] the candidate bound of each row (+inf: past N or not allowed)
    const uint32_t* allow;        // optional allow-bitmap, padded to whole 256-row tiles
    unsigned long long* cnt;      // candidates found (counts past cap)
    uint64_t* keys; long cap;     // [cap] candidate keys (row << 32) | centroid
};
int launch_kmeans_best(const KmeansAssignArgs& a, hipStream_t st);
// cstat [2]: the running maxima max ||c||, max ||cb - c|| of the centroids (launch_l2norm_rows max_stats)
int launch_kmeans_bound(const KmeansAssignArgs& a, const float* inv, const float* rstat, const uint32_t* cstat, hipStream_t st);
int launch_kmeans_decide(const KmeansAssignArgs& a, hipStream_t st);
// fp32 score of candidates [0, n) folded into rowkey[row] (zeroed by the caller) = max of make_key(score, centroid);
// ncand[row] (zeroed by the caller) counts the row's candidates
int launch_kmeans_rescore(const uint64_t* cand, long n, const float* Gf, long ldg, const float* inv, const float* Cf, int D,
                          unsigned long long* rowkey, uint32_t* ncand, hipStream_t st);
// labels / scores of rows [0, N) from their keys (no key: -1 / -inf); ctr[0] += labels that differ from the old ones, ctr[1] +=
// rows with more than one candidate, ctr[2] += rows with a label; sizes [C] = members per centroid
int launch_kmeans_finish(const unsigned long long* rowkey, const uint32_t* ncand, long N, long C, int* labels, float* scores,
                         unsigned long long* sizes, unsigned long long* ctr, hipStream_t st);
struct KmeansUpdateArgs {
    const int* labels; long N; long C; int D;
    int b;                        // bits of a row index (the row field of the sort key)
    const float* Gf; long ldg;    // the gallery's fp32 master rows
    const unsigned long long* sizes;        // [C] launch_kmeans_finish's
    uint64_t *keys, *keys_alt; float *vals, *vals_alt; uint32_t* hist;   // [N] each, and the sort's digit counts
    unsigned long long *moff, *coff;        // [C] inclusive member / chunk offsets
    float* part; long part_chunks;          // [part_chunks][D] chunk partials, part_chunks >= N / 256 + C
    float* sums;                  // [C][D]
    const float* Cf_old; const bf16_t* Cb_old;   // the centroids of this step
    float* Cf_new; bf16_t* Cb_new;          // the centroids of the next one
    uint32_t* cstat;              // [2] running maxima of the centroids' norms (not reset: upper bounds for the kept rows too)
};
int launch_kmeans_update(const KmeansUpdateArgs& a, hipStream_t st);
// ---- range search (revo_search_range; range.hip): the join runs the 256 x 256 scan's work plan, with a
// bound per query
constexpr int RANGE_CHUNK = 1024;            // queries per candidate pass (fewer when the sort key would pass 64 bits)
constexpr long RANGE_WS_PER_QUERY = 1024;    // candidate keys per query of a chunk the workspace holds before a regrow
constexpr long RANGE_MAX_CAND = 1l << 28;    // candidates a call may have, over all its chunks (2 GiB of keys); more: status -2
constexpr int RANGE_PHASES = 8;              // = S256_PHASES (scan_plan.h)
struct RangeJoinArgs {
    const bf16_t* Qb; long ldq;   // the chunk's bf16 query rows
    const bf16_t* Gb; long ldg;   // the gallery's bf16 rows
    int Q; long N; int D;
    const float* qstat;           // [Q][2] the queries' rounding norms (launch_l2norm_rows row_stats)
    const uint32_t* gstat;        // [2] the gallery's running maxima (max ||g||, max ||gb - g||), fp32 bit patterns
    float thr;
    const uint32_t* allow;        // optional allow-bitmap, padded to whole 256-row tiles
    unsigned long long* cnt;      // candidates found (counts past cap)
    uint64_t* keys; long cap;     // [cap] candidate keys (query << 32) | row
    // set by the launcher: the scan's phases (launch_topk_scan256)
    int nph;
    int ph_first[RANGE_PHASES + 1], ph_q0[RANGE_PHASES], ph_qn[RANGE_PHASES], ph_ns[RANGE_PHASES];
};
int launch_range_join(const RangeJoinArgs& a, hipStream_t st);
// fp32 score of candidates [0, n) (query rows Qf, gallery rows Gf); those >= thr appended to out_keys ((query << (32 + b)) |
// (~order-preserving score bits << b) | row) / out_scores, count in *kept, per query in counts[query]
int launch_range_rescore(const uint64_t* cand, long n, const float* Qf, long ldq, const float* Gf, long ldg, int D, float thr,
                         int b, unsigned long long* kept, unsigned long long* counts, uint64_t* out_keys, float* out_scores,
                         hipStream_t st);
// sorted keys -> row + idx_offset / scores
int launch_range_emit(const uint64_t* keys, const float* vals, long n, int b, long idx_offset, long long* idx, float* scores,
                      hipStream_t st);
// ---- search by examples (revo_search_recommend; recommend.hip): sample pass -> level tau; the join is a
// pass over gallery slices whose epilogue reduces over the example rows; candidates are rows
constexpr int RECOMMEND_MAX_EXAMPLES = 128;  // the example rows of a tile column live in one wave up to here
struct RecommendPassArgs {
    const bf16_t* Qb; long ldq;   // the bf16 example rows, positives first
    const bf16_t* Gb; long ldg;   // the gallery's bf16 rows
    int P, Nn;                    // positive / negative examples
    long N; int D;                // rows the pass covers (from row 0)
    const float* qstat;           // [P + Nn][2] the examples' rounding norms (launch_l2norm_rows row_stats)
    const uint32_t* gstat;        // [2] the gallery's running maxima (max ||g||, max ||gb - g||), fp32 bit patterns
    const uint32_t* allow;        // optional allow-bitmap, padded to whole 256-row tiles
    const float* tau;             // candidate pass: [1] the level (device)
    unsigned long long* cnt;      // candidate pass: [0] candidates found (counts past cap), [2] allowed rows met
    uint32_t* rows; long cap;     // candidate pass: [cap] candidate rows
    float* lb_out;                // sample pass: [N] lower bound of every row's score (-inf: not allowed)
};
int launch_recommend_pass(const RecommendPassArgs& a, int sample, hipStream_t st);
// tau[0] = the k-th largest of lb[0 .. n) (-inf when n < k), raised to thr when has_thr
int launch_recommend_level(const float* lb, int n, int k, int has_thr, float thr, float* tau, hipStream_t st);
// score(r) of candidate rows [0, n) against the P + Nn fp32 example rows Qf; those passing the threshold appended to out_keys
// ((~order-preserving score bits << b) | row) / out_scores, count in *kept
int launch_recommend_rescore(const uint32_t* cand, long n, const float* Qf, long ldq, int P, int Nn, const float* Gf, long ldg,
                             int D, int has_thr, float thr, int b, unsigned long long* kept, uint64_t* out_keys, float* out_scores,
                             hipStream_t st);
// the first min(n, k) sorted entries -> scores / row + idx_offset, padding behind them, counts[0]
int launch_recommend_emit(const uint64_t* keys, const float* vals, long n, int k, int b, long idx_offset, float* scores,
                          long long* idx, int* counts, hipStream_t st);
// ---- discovery and context search (revo_search_discover; discover.hip): the recommend search's plan
// (its level and emit kernels as they are) over context pairs; a pair's two example rows sit half a tile apart
constexpr int DISCOVER_MAX_PAIRS = 64;       // pairs, the target counting as one: what the 128-row form of the tile holds
struct DiscoverPassArgs {
    const bf16_t* Qb; long ldq;   // the bf16 example tile, discover_tile_rows rows: positive i in row i, negative i in row
                                  // rows / 2 + i, the target in row rows / 2 - 1, zero rows elsewhere
    const bf16_t* Gb; long ldg;   // the gallery's bf16 rows
    int n_pairs, has_target;
    long N; int D;                // rows the pass covers (from row 0)
    const float* qstat;           // [rows][2] the examples' rounding norms, by tile row (launch_l2norm_rows row_stats)
    const uint32_t* gstat;        // [2] the gallery's running maxima (max ||g||, max ||gb - g||), fp32 bit patterns
    const uint32_t* allow;        // optional allow-bitmap, padded to whole 256-row tiles
    const float* tau;             // candidate pass: [1] the level (device)
    unsigned long long* cnt;      // candidate pass: [0] candidates found (counts past cap), [2] allowed rows met
    uint32_t* rows; long cap;     // candidate pass: [cap] candidate rows
    float* lb_out;                // sample pass: [N] lower bound of every row's score (-inf: not allowed)
};
int discover_tile_rows(int n_pairs, int has_target);   // 64 or 128
int launch_discover_pass(const DiscoverPassArgs& a, int sample, hipStream_t st);
// score(r) of candidate rows [0, n) against the fp32 example tile Qf (the pass's layout, half = rows / 2); those passing the
// threshold appended to out_keys ((~order-preserving score bits << b) | row) / out_scores, count in *kept
int launch_discover_rescore(const uint32_t* cand, long n, const float* Qf, long ldq, int half, int n_pairs, int has_target,
                            const float* Gf, long ldg, int D, int has_thr, float thr, int b, unsigned long long* kept,
                            uint64_t* out_keys, float* out_scores, hipStream_t st);
// ---- boosted search (revo_search_boosted; boost.hip): the recommend search's plan (its level kernel as it
// is) for one query whose fp32 score s is rescored per row, final = fmaf(mult[r], s, bias[r]); the sample is strided
struct BoostPassArgs {
    const bf16_t* Qb; long ldq;   // the bf16 query row
    const bf16_t* Gb; long ldg;   // the gallery's bf16 rows
    long N; int D;                // the gallery's rows (both passes)
    const float* qstat;           // [2] the query's rounding norms (launch_l2norm_rows row_stats)
    const uint32_t* gstat;        // [2] the gallery's running maxima (max ||g||, max ||gb - g||), fp32 bit patterns
    const uint32_t* allow;        // optional allow-bitmap, padded to whole 256-row tiles
    const float* mult;            // [N] row multipliers, null: 1
    const float* bias;            // [N] row biases, null: 0
    int has_min; float min_sim;   // the cut on the similarity
    long n_sample;                // sample pass: its rows, a multiple of 256: tile i of it is gallery tile floor(i T / S)
    const float* tau;             // candidate pass: [1] the level (device)
    unsigned long long* cnt;      // candidate pass: [0] candidates found (counts past cap), [2] allowed rows met, [3] allowed rows
                                  // whose mult is negative or not finite or whose bias is not finite
    uint32_t* rows; long cap;     // candidate pass: [cap] candidate rows
    float* lb_out;                // sample pass: [n_sample] lower bound of the final score by sample position (-inf: not allowed,
                                  // past the gallery's end, or not certainly at or above min_sim)
};
int launch_boost_pass(const BoostPassArgs& a, int sample, hipStream_t st);
// s and final of candidate rows [0, n) against the fp32 query row Qf; those passing both cuts appended to out_keys
// ((~order-preserving final bits << b) | row) / out_scores (final), count in *kept; sim[row] = s of every kept row
struct BoostRescoreArgs {
    const uint32_t* cand; long n;
    const float* Qf; const float* Gf; long ldg; int D;
    const float* mult; const float* bias;
    int has_min; float min_sim; int has_thr; float thr;
    int b;
    unsigned long long* kept; uint64_t* out_keys; float* out_scores;
    float* sim;                   // [N]
};
int launch_boost_rescore(const BoostRescoreArgs& a, hipStream_t st);
// launch_recommend_emit, and sims[i] = sim[row of entry i] (-inf in the padding)
int launch_boost_emit(const uint64_t* keys, const float* vals, long n, int k, int b, long idx_offset, const float* sim,
                      float* scores, float* sims, long long* idx, int* counts, hipStream_t st);
// ---- multi-vector search (revo_search_maxsim; maxsim.hip): late-interaction MaxSim of up to 64 query
// vectors over the groups of the gallery's rows; the recommend search's pass form with a storing epilogue, bounds per group
constexpr int MAXSIM_MAX_VECTORS = 64;       // the query vectors of a tile column live in one wave (the 64-row form of the tile)
// the CSR of the handle's group ids: sorted keys (group << 32) | row -> gid [G] the distinct ids ascending, off [G + 1] their
// row ranges in rows [grouped rows] (rows ascending inside a group), pos_group [grouped rows] the dense group of a position;
// meta (device, 2 words) = { G, grouped rows }.  keys / keys_alt [N], vals / vals_alt [N], hist, flags [N]: scratch
int launch_maxsim_index(const int32_t* groups, long N, uint64_t* keys, uint64_t* keys_alt, float* vals, float* vals_alt,
                        uint32_t* hist, unsigned long long* flags, unsigned long long* meta, int32_t* gid, uint32_t* off,
                        uint32_t* rows, uint32_t* pos_group, hipStream_t st);
struct MaxsimPassArgs {
    const bf16_t* Qb; long ldq;   // the bf16 query vectors
    const bf16_t* Gb; long ldg;   // the gallery's bf16 rows
    int n, n_pad;                 // query vectors; n rounded up to 4
    long N; int D;
    const uint32_t* allow;        // optional allow-bitmap, padded to whole 256-row tiles
    float* S;                     // [N][n_pad] out: the bf16 scan score of every (allowed row, vector)
};
int launch_maxsim_pass(const MaxsimPassArgs& a, hipStream_t st);
// what the per-group kernels share
struct MaxsimGroupArgs {
    const float* S; int n, n_pad, lanes;   // lanes = maxsim_group_lanes(n_pad)
    const int32_t* gid; const uint32_t* off; const uint32_t* rows; long G;   // the CSR
    const uint32_t* allow;        // optional allow-bitmap
    const float* qstat;           // [n][2] the query vectors' rounding norms (launch_l2norm_rows row_stats)
    const uint32_t* gstat;        // [2] the gallery's running maxima (max ||g||, max ||gb - g||), fp32 bit patterns
    int D;
};
int maxsim_group_lanes(int n_pad);   // n_pad rounded up to a power of two: lanes of a wave that share one row
// lb / ub [G]: bounds of score(G) from the bf16 scan scores (-inf: no allowed row), acnt [G] allowed rows; cnt[2] += groups
// with an allowed row
int launch_maxsim_bounds(const MaxsimGroupArgs& a, float* lb, float* ub, uint32_t* acnt, unsigned long long* cnt, hipStream_t st);
// the groups with an allowed row and ub >= tau[0] -> cgroups (count cnt[3]), their allowed rows -> crows (count cnt[0])
int launch_maxsim_select(const MaxsimGroupArgs& a, long n_grouped, const uint32_t* pos_group, const float* ub, const uint32_t* acnt,
                         const float* tau, unsigned long long* cnt, uint32_t* crows, uint32_t* cgroups, hipStream_t st);
// S[row][0 .. n_pad) := the fp32 chain scores of every candidate row
int launch_maxsim_rescore(const uint32_t* crows, long n_rows, const float* Qf, long ldq, int n, int n_pad, const float* Gf, long ldg,
                          int D, float* S, hipStream_t st);
// score(G) of the candidate groups; those passing the threshold appended to out_keys ((~order-preserving score bits << 32) |
// dense group position) / out_scores, count in *kept
int launch_maxsim_reduce(const MaxsimGroupArgs& a, const uint32_t* cgroups, long n_groups, int has_thr, float thr,
                         unsigned long long* kept, uint64_t* out_keys, float* out_scores, hipStream_t st);
// the first min(n_kept, k) sorted entries -> scores / group ids / per-vector maxima and rows (optional), padding behind them
int launch_maxsim_emit(const MaxsimGroupArgs& a, const uint64_t* keys, const float* vals, long n_kept, int k, int n_vec,
                       long idx_offset, float* scores, int32_t* group_ids, int32_t* counts, float* part_scores, long long* part_rows,
                       hipStream_t st);
// ---- diverse search (revo_search_mmr; mmr.hip): the candidates' similarity matrices, greedy selection
struct MmrGramArgs {
    const float* Gf; long ldg;    // the gallery's fp32 master rows
    long N; int D;
    const long long* cand;        // [Q][C] candidate rows of each query, best first (index offset 0)
    const int* counts;            // [Q] candidates of each query (device)
    float* gram;                  // [Q][C][C] out: sim(i, j) for i, j < counts[q], i != j (the diagonal is written too)
    int Q, C;
    int tile;                     // candidate pairs per wave: 8 (8 x 8) or 4 (4 x 4)
    int W;                        // set by the launcher: workgroups per query
};
int launch_mmr_gram(const MmrGramArgs& a, hipStream_t st);
struct MmrSelectArgs {
    const float* rel;             // [Q][C] the candidates' scores
    const long long* cand;        // [Q][C]
    const int* counts;            // [Q]
    const float* gram;            // [Q][C][C]
    int C, k;
    float lam, diversity;         // lam = fl(1 - diversity)
    long idx_offset;
    float* scores; float* mmr;    // [Q][k] out, pick order: relevance, the value of the pick (mmr may be null)
    long long* idx;               // [Q][k] out: row + idx_offset
    int* out_counts;              // [Q] out: min(k, counts[q])
};
int launch_mmr_select(const MmrSelectArgs& a, int Q, hipStream_t st);
// ---- hybrid queries (revo_search_fusion, revo_topk_fuse; fusion.hip): rank / score fusion of m lists
constexpr int FUSION_MAX_LISTS = 64;
constexpr int FUSION_MAX_KEYS = 8192;   // m * C: what one workgroup sorts in LDS (two arrays of 64 KiB)
struct FusionArgs {
    const float* scores;          // [n][m][C] the lists' scores
    const long long* idx;         // [n][m][C] their rows (index offset 0), each in [0, 2^47)
    const int* counts;            // [n][m] entries of each list (device; more than C counts as C)
    int m, C, k;
    int method;                   // 0 = RRF, 1 = DBSF
    float rrf_k;
    float w[FUSION_MAX_LISTS];    // the lists' weights (by value: the call stays asynchronous)
    float t[FUSION_MAX_LISTS];    // the lists' thresholds (-inf: none)
    int has_thr; float thr;       // the cut on the fused score
    long idx_offset;
    float* out_scores;            // [n][k] out: F
    long long* out_idx;           // [n][k] out: row + idx_offset
    int* out_counts;              // [n] out
    int* out_ranks;               // [n][k][m] out (optional): 1-based position in list j, 0 = not a member
};
int launch_fusion_fuse(const FusionArgs& a, int n, hipStream_t st);
// list_scores[(i * k + e) * m + j] = the fp32 chain of every re-score over row out_idx[i][e] - idx_offset of Gf and the
// normalised query row Qf[i * m + j], for e < out_counts[i]; -inf behind
int launch_fusion_list_scores(const float* Qf, long ldq, const float* Gf, long ldg, int D, const long long* out_idx,
                              const int* out_counts, long idx_offset, int n, int m, int k, float* list_scores, hipStream_t st);
// all-padding result for an empty gallery
int launch_topk_fill_empty(float* s, long long* i, int* c, int Q, int k, hipStream_t st);
// merge P per-shard result lists [P][Q][k] -> [Q][k]
int launch_topk_merge(const float* scores, const long long* idx, int P, int Q, int k, int has_thr, float thr,
                      float* out_scores, long long* out_idx, int* out_counts, hipStream_t st);
// the merge's share of the exactness certificate of a row-sharded search (all optional: cert == null switches it off)
struct MergeCert {
    const float* cert; long cert_part_stride;   // [P][Q] per-shard bounds U_p + eps_p written by the shards' finish steps
    int* unc_count;                             // device counter (zeroed by the caller): uncertified queries
    int* unc_q; float* unc_need;                // [Q] their indices (in no particular order) and the score a row needs to enter
};
// the same with explicit distances (in elements) between the parts of the two arrays
int launch_topk_merge_strided(const float* scores, long score_part_stride, const long long* idx, long idx_part_stride, int P,
                              int Q, int k, int has_thr, float thr, float* out_scores, long long* out_idx, int* out_counts,
                              hipStream_t st, const MergeCert* mc = nullptr);

// ---- text-prompted regions (revo_vit_detect; detect.hip)
constexpr int DETECT_MAX_PROMPTS = 64;
constexpr int DETECT_MAX_CELLS = 1024;       // g * g of the region kernel: one workgroup holds an image's cells in LDS
// scores[(b * P + p) * cells + c] = the fp32 chain of every re-score over prompts[p] ([P][D], already normalised) and token row
// (b * S + cls + c) of tok ([.][ldt]); rows = images * cells
int launch_detect_scores(const float* tok, long ldt, int S, int cls, int cells, long rows, const float* prompts, int P, int D,
                         float* scores, hipStream_t st);
struct DetectRegionArgs {
    const float* scores;          // [batch][P][g * g]
    int batch, P, g, cls;
    const float* thr;             // [P] device
    int nbg, min_cells, max_regions;
    int* labels;                  // [batch][g * g] out (optional)
    int* counts;                  // [batch] out: regions emitted per image
    uint32_t* stage;              // detect_stage_words(): the images' slots -- prompt, cells, confidence, box, bitmap of slot
                                  // b * max_regions + k, one array after the other
    int* err;                     // device word, zeroed by the caller: != 0 afterwards = a loop hit its trip limit
};
size_t detect_stage_words(int batch, int max_regions, int words);
int launch_detect_regions(const DetectRegionArgs& a, hipStream_t st);
// the images' slots -> consecutive result rows (images ascending); every output pointer may be null
int launch_detect_compact(const int* counts, const uint32_t* stage, int batch, int max_regions, int words, int* r_img, int* r_prompt,
                          int* r_box, int* r_cells, float* r_conf, uint32_t* r_bits, hipStream_t st);

}  // namespace revo
