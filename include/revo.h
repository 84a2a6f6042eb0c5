/* librevo -- C ABI of the MI355X-native embed + search hot path of revers-o.
 *
 * This is the drop-in boundary: plain pointers and sizes, no
 * torch types.  Each entry point names the reference interface it replaces
 * (file:line relative to the reference tree).  The reference itself has no FFI:
 * its hot path is two Python calls into third-party packages, so the entry points
 * below are what a ctypes binding in core_system.py would call instead of
 *   self.pe_model.encode_image(...)          core_system.py:341, :442
 *   self.vector_db.search(...)               core_system.py:659-664
 *   client.recreate_collection / upsert      core_system.py:600-603, :621
 * (binding stub: INTEGRATION.md).
 *
 * Conventions: every function returns 0 on success and a negative status on
 * failure; the message is available from revo_last_error() (thread-local).
 * Nothing throws across the boundary.  `stream` is a hipStream_t (NULL = the
 * default stream); work is enqueued asynchronously on it and the caller owns
 * ordering (revo_sync).  A handle is bound to the device it was created on: every
 * entry point that takes a handle makes that device current for the call and
 * restores the caller's device on return, so handles on different GPUs can be
 * used from one process; a handle must not be used from two threads at once;
 * distinct handles are independent.  All device pointers (and the stream) passed
 * with a handle must belong to the handle's device; functions without a handle
 * (revo_topk_merge, revo_op_*, revo_preprocess_*) run on the current device.
 */
#ifndef REVO_H
#define REVO_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct revo_vit revo_vit;
typedef struct revo_gallery revo_gallery;

/* Dimensions of a Perception-Encoder vision tower (the values the reference gets
 * implicitly from pe.CLIP.from_config("PE-Core-L14-336"), core_system.py:177-181). */
typedef struct revo_vit_cfg {
    int32_t image_size, patch_size, width, layers, heads, mlp_dim, out_dim, pool_heads;
    int32_t use_cls;    /* class token + (0,0) rope position */
    int32_t use_ls;     /* LayerScale tensors (ls_1.gamma / ls_2.gamma) present */
    float ln_eps, rope_theta;
    int32_t pool_mlp_dim; /* hidden width of the attention-pool head's MLP (upstream: 4 * width, whatever mlp_dim is); 0 = 4 * width */
} revo_vit_cfg;

/* One checkpoint tensor: upstream name ("visual.conv1.weight", ...), fp32 values
 * in host or device memory. */
typedef struct revo_tensor {
    const char* name;
    const float* data;
    int64_t numel;
} revo_tensor;

const char* revo_last_error(void);
int32_t revo_version(void);
int32_t revo_sync(void* stream);

/* ---- embed: replaces load_pe_model + encode_image (core_system.py:169-203, :341, :442) */
int32_t revo_vit_create(const revo_vit_cfg* cfg, const revo_tensor* weights, int32_t n_weights, int32_t device,
                        int32_t max_batch, revo_vit** out);
int32_t revo_vit_destroy(revo_vit* vit);
/* images: NCHW at the model resolution on the device; image_dtype 0 = fp32 already
 * normalised to [-1,1] (what self.preprocess yields, core_system.py:439), 1 = uint8
 * (normalised (v/255-0.5)/0.5 inside the patchify kernel).  out: [B, out_dim] fp32 on
 * the device; normalize != 0 applies embedding / embedding.norm() (core_system.py:447). */
int32_t revo_vit_forward(revo_vit* vit, const void* images, int32_t image_dtype, int32_t batch, float* out,
                         int32_t normalize, void* stream);
/* The tokens per image of the ACTIVE grid (GRIDS below): gh * gw + use_cls; natively g * g + use_cls.  -1 for a null handle. */
int32_t revo_vit_seq_len(const revo_vit* vit);
/* GRIDS: native-aspect embedding -- the forward on a rectangular token grid.  g = image_size /
 * patch_size is the native side, P the patch side.  revo_vit_set_grid(vit, gh, gw, stream) makes every forward that follows on
 * the handle (revo_vit_forward, _forward_regions, _forward_tokens) take images [batch, 3, gh * P, gw * P] and run on S' = gh *
 * gw + use_cls tokens per image: patch (gy, gx) is token use_cls + gy * gw + gx, the class token, if any, token 0.  The token
 * budget is the native one, gh * gw <= g * g, so every workspace of the handle already fits and a forward costs at most what
 * the native one costs; any such (gh, gw) is accepted.  The shape holds until the next revo_vit_set_grid; (0, 0) or (g, g)
 * restores the native grid.  What changes with the grid, and nothing else does:
 *   positions  the class row of visual.positional_embedding is kept; its g x g patch rows are resampled to gh x gw by bilinear
 *              interpolation with half-pixel centres: source coordinate (o + 0.5) * g / g_out - 0.5 clamped below at 0, the
 *              upper neighbour clamped at g - 1 (F.interpolate(mode = "bilinear", align_corners = False), no antialiasing).
 *              Coordinates and the four weights in fp64, each weight rounded once to fp32, then one fp32 fma chain w00 p00 +
 *              w01 p01 + w10 p10 + w11 p11 in that order: within 6 * 2^-24 * max|corner| of the same formula in fp64.
 *   RoPE       the table revo_vit_create builds, with gx = c % gw, gy = c / gw of cell c and integer coordinates gx + use_cls,
 *              gy + use_cls: not rescaled to the native range.  Host fp64, each cos and sin rounded once.
 * Both are [UPSTREAM-RECALL], like the rest of the tower.  At (g, g) the native tables are used themselves.  A shape's tables
 * are built by the first revo_vit_set_grid that names it (a kernel and a copy on `stream`, which the call waits for) and kept:
 * the handle holds at most 64 shapes, the native one included, and refuses a 65th.  The result for an image depends on its
 * grid and on nothing else the caller did before.  Bitmaps of revo_vit_forward_regions have ceil(S' / 32) words per region
 * under a grid, revo_vit_forward_tokens writes batch * S' rows.  revo_vit_detect runs on the native grid only (its component
 * kernel walks a g x g map) and is refused under another with a message that names the grid; setting another grid ends the
 * life of a detect result.  Status -2 before the device is touched: a null handle, a non-positive side (other than (0, 0)),
 * gh * gw > g * g, a band of more than 65535 pixels (gh * P or gw * P), a 65th shape. */
int32_t revo_vit_set_grid(revo_vit* vit, int32_t grid_h, int32_t grid_w, void* stream);
/* REGIONS: a vector per region for one forward per image (masked attention pooling).
 * One body forward of the batch, ln_post and the pool's logits once; then for region r of image region_image[r] the head of
 * revo_vit_forward with its softmax restricted to the tokens the region's bitmap allows: region_bits [n_regions][ceil(S / 32)]
 * uint32, S = revo_vit_seq_len, token s allowed iff bit s & 31 of word s >> 5 is set (the layout of revo_search_set_filter);
 * bits at or past S are ignored.  Token 0 is the class token on towers that have one, patch (gy, gx) of the g x g grid is
 * token use_cls + gy * g + gx.  Disallowed tokens are skipped: their rows are not read, NaN or Inf in them changes nothing.
 *   out_global  [batch, out_dim] or NULL: exactly what revo_vit_forward writes, bit for bit.
 *   out_regions [n_regions, out_dim]: a region's row depends on its image and its bitmap alone -- not on the other regions
 *     of the call, their order or their number; a region that allows every token has its image's out_global row, bit for
 *     bit.  A region that allows no token gets zeros (not normalised).
 * region_image is a HOST array, each entry in [0, batch); region_bits is in host (bits_on_device = 0) or device memory.
 * Host arrays are copied into a pinned buffer of the handle before the call returns: the caller may free them on return.
 * A device bitmap is read by kernels on `stream`.  Any n_regions >= 0 (0: revo_vit_forward; out_global is required then);
 * the regions are taken in chunks that fit a fixed workspace the handle allocates on the first call with regions.
 * Enqueued on `stream` like a forward (a call with more than 4096 regions waits for its own earlier copies in between).
 * Status -2 before the device is touched: negative counts, null region arrays or out_regions with n_regions > 0, an image
 * index outside [0, batch), null handle or images, batch above max_batch. */
int32_t revo_vit_forward_regions(revo_vit* vit, const void* images, int32_t image_dtype, int32_t batch,
                                 const int32_t* region_image, const uint32_t* region_bits, int32_t bits_on_device,
                                 int32_t n_regions, float* out_global, float* out_regions, int32_t normalize, void* stream);
/* TOKENS: a vector per token from one forward (MaskCLIP-style dense features).  out_tokens [batch * S,
 * out_dim], S = revo_vit_seq_len: row b * S + s is, bit for bit, the row revo_vit_forward_regions writes for the region of
 * image b whose bitmap allows token s alone (a softmax over one token is exactly 1, so the head reads the token's ln_post row
 * itself; the head's fp32 GEMMs cut K the same way whatever the row count).  out_global [batch, out_dim] or NULL: the bits of
 * revo_vit_forward.  Enqueued on `stream` like a forward; the rows pass through the region workspace 512 at a time.  Status -2
 * before the device is touched: null handle, images or out_tokens, batch outside [1, max_batch], a bad image_dtype. */
int32_t revo_vit_forward_tokens(revo_vit* vit, const void* images, int32_t image_dtype, int32_t batch, float* out_global,
                                float* out_tokens, int32_t normalize, void* stream);
/* DETECT: text-prompted regions on the device -- token vectors scored against prompt vectors, every cell given to the prompt
 * that wins it, the label map cut into connected regions (the MaskCLIP construction; it stands where the reference hands
 * its text prompt to a third-party detector, core_system.py:249-262).  The contract is numerical: nothing is claimed about
 * detection quality on trained weights.  prompts: device [n_prompts, out_dim] fp32 (revo_text_forward's rows, or any vectors
 * of the space), the last n_background of them background prompts; thresholds: HOST [n_prompts].  g = image_size /
 * patch_size, c = gy * g + gx a cell, token use_cls + c of its image.
 *   t[b, c]     the normalised token vector of cell c: revo_vit_forward_tokens' row with normalize = 1.  The class token
 *               takes no part.
 *   s[b, p, c]  the score of prompt p, normalised like every search query by the same kernel, against t[b, c]: the one fp32
 *               fma chain of EXACTNESS -- the bits revo_search_range returns for prompt p against a gallery to which the
 *               token vectors were appended with normalize = 0.
 *   w[b, c]     the prompt with the largest s[b, ., c], compared in fp32 with -0 equal to +0; ties go to the lowest p; a NaN
 *               score never wins (every score NaN: no winner).
 *   label[b, c] = w if there is a winner, w < n_prompts - n_background and s[b, w, c] >= thresholds[w] (equality keeps the
 *               cell; -inf is allowed), else -1.  Background prompts compete for cells and produce no region.
 * A region is a maximal 4-connected set of cells of one image with equal label >= 0.  Its attributes: its prompt (the label);
 * cells, its cell count; its inclusive cell box gx0, gy0, gx1, gy1; confidence, the largest s[b, label, c] over its cells
 * (with +0 above -0, so that the bits are defined); first, its lowest cell index.  Regions with fewer than min_cells cells are
 * dropped; per image the rest are ordered by (confidence desc with -0 equal to +0, first asc) and cut at max_regions; images
 * ascend in the output.  bits [ceil(S / 32)] is the region's token bitmap in revo_vit_forward_regions' layout: only
 * patch-token bits are set.  With with_vectors, vectors[r] is bit for bit what revo_vit_forward_regions returns for
 * (region_image[r], bits[r]) with the same `normalize`; they come from the rows and logits of the call's one body forward.
 * out_global [batch, out_dim] or NULL: the bits of revo_vit_forward.  Two calls give identical bytes.
 * revo_vit_detect computes the result into the handle and writes the region count to the host *n_regions.  SYNCHRONOUS on
 * `stream`, like revo_gallery_pairs: the host needs the count to run the regions' head.  revo_vit_detect_read copies regions
 * [start, start + n) to host or device arrays (dst_on_device), each pointer NULL independently: region_image [n], region_prompt
 * [n], boxes [n][4], cells [n], confidence [n], bits [n][ceil(S / 32)], vectors [n][out_dim] (status -2 when the result was
 * computed without vectors).  revo_vit_detect_maps copies s ([batch][n_prompts][g * g]) and label ([batch][g * g]), each NULL
 * independently.  The result lives in the handle until the next forward of any kind on it (revo_vit_forward, _regions, _tokens,
 * _detect): after one, or with no result, both reads give status -2, as does a range past the end.
 * Limits (status -2 before the device is touched, the outputs untouched, the message naming the argument): 1 <= n_prompts <=
 * 64; 0 <= n_background < n_prompts; 1 <= min_cells; 1 <= max_regions <= g * g; g * g <= 1024; a NaN threshold, a null handle,
 * images, prompts, thresholds or n_regions, a batch outside [1, max_batch].  Zero regions is not an error.  Every loop of the
 * component labelling has a trip limit; one that is hit gives status -4 ("connected components did not converge").  The first
 * call allocates a workspace for max_batch images (the token vectors: max_batch * S * out_dim floats). */
int32_t revo_vit_detect(revo_vit* vit, const void* images, int32_t image_dtype, int32_t batch, const float* prompts,
                        int32_t n_prompts, const float* thresholds, int32_t n_background, int32_t min_cells, int32_t max_regions,
                        float* out_global, int32_t with_vectors, int32_t normalize, int64_t* n_regions, void* stream);
int32_t revo_vit_detect_read(revo_vit* vit, int64_t start, int64_t n, int32_t* region_image, int32_t* region_prompt,
                             int32_t* boxes, int32_t* cells, float* confidence, uint32_t* bits, float* vectors,
                             int32_t dst_on_device);
int32_t revo_vit_detect_maps(revo_vit* vit, float* scores, int32_t* labels, int32_t dst_on_device);
/* Run-time telemetry of the LayerNorm folded into the GEMMs around it (batch-sized forwards: ln_1 / ln_2 are not kernels;
 * qkv / fc1 read A = bf16(x) UN-CENTRED and apply rstd * (acc - mean * csum) + b' in their epilogues).  The form is the same
 * function as LayerNorm-then-GEMM, but its rounding error grows with |mean| / std of a row (bf16(x) spends its 8 bits on
 * the common offset): measured rms error against the fp64 LayerNorm + linear, relative to LayerNorm kernel -> bf16 -> GEMM:
 * 1.00 x at offset 0, 1.5 x at 2 sigma, 4.9 x at 8.5 sigma, 18.7 x at 33 sigma -- about 0.57 x the offset in sigmas
 * (tests/test_gpu_ln_fold.py::test_fold_error_against_the_row_offset records the curve and holds it to a bound).  The
 * reference normalises in the activations' precision before the matmul (oracle/pe_vit.py:146-155 <- core_system.py:341), so on
 * a trained checkpoint this is the number to look at first if embeddings drift: out4 = { rows the consuming GEMMs merged
 * statistics for since the last reset (each row of each folded LayerNorm of each forward, counted once; rows that a
 * separate leftover-row kernel takes -- none at the headline shapes -- are not sampled), of those: rows with |mean| * rstd > out4[3], rows with |mean| * rstd > 4 *
 * out4[3], the ratio that counts as large (8) }.  The counters are read, and with reset != 0 cleared, ON `stream` -- behind the
 * forwards already enqueued there, ahead of the next -- and the call returns when `stream` has drained. */
int32_t revo_vit_stats(revo_vit* vit, double* out4, int32_t reset, void* stream);

/* ---- TEXT: the text tower of the same CLIP checkpoint (the reference loads it at core_system.py:181 and never calls it):
 * prompts -> vectors in the space of revo_vit_forward's, so a sentence can be a search query.
 *   x = token_embedding[tokens] + positional_embedding[:seq_len];  pre-LN blocks with CAUSAL attention (no RoPE, no class
 *   token);  p = ln_final(x[b, first position of the prompt's largest token id]);  out = p . text_projection, optionally
 *   normalised.  [UPSTREAM-RECALL] for the structure; every dimension comes from the checkpoint.
 * Tensor names are the upstream ones without a prefix: token_embedding.weight [vocab, width], positional_embedding
 * [context, width], transformer.resblocks.{i}.{ln_1, ln_2, attn.in_proj_*, attn.out_proj.*, mlp.c_fc.*, mlp.c_proj.*,
 * ls_1.gamma, ls_2.gamma (use_ls)}, ln_final.{weight, bias}, text_projection [width, out_dim]; anything else is refused. */
typedef struct revo_text revo_text;
typedef struct revo_text_cfg {
    int32_t context_length, vocab_size, width, layers, heads, mlp_dim, out_dim, use_ls;
    float ln_eps;
} revo_text_cfg;
/* Refused with a message (-2, before the device is touched): head_dim other than 64, context_length over 128, width or
 * mlp_dim not a multiple of 64, out_dim not a multiple of 4, a missing / mis-sized / unexpected tensor. */
int32_t revo_text_create(const revo_text_cfg* cfg, const revo_tensor* weights, int32_t n_weights, int32_t device,
                         int32_t max_batch, revo_text** out);
int32_t revo_text_destroy(revo_text* text);
/* tokens: HOST int32 [batch][seq_len], 1 <= seq_len <= context_length (a shorter seq_len computes the same rows: a causal
 * row never sees what follows it); out: device fp32 [batch, out_dim].  Every id must lie in [0, vocab_size): otherwise status
 * -2 with a message naming the prompt and the position, before the device is touched.  The tokens are copied through a
 * pinned buffer of the handle: the caller may free them on return.  Enqueued on `stream` like revo_vit_forward. */
int32_t revo_text_forward(revo_text* text, const int32_t* tokens, int32_t batch, int32_t seq_len, float* out,
                          int32_t normalize, void* stream);

/* ---- gallery: replaces recreate_collection(size=D, COSINE) + upsert (core_system.py:600-622) */
int32_t revo_gallery_create(int32_t dim, int64_t capacity, int32_t device, int32_t keep_f32, revo_gallery** out);
int32_t revo_gallery_destroy(revo_gallery* g);
/* vecs: [n, dim] fp32, host (src_on_device = 0) or device memory.  normalize != 0
 * L2-normalises each row at insert, as qdrant does for Distance.COSINE.  A device source is read by a kernel enqueued on
 * `stream` (no host round trip); a host source is staged in chunks and the call waits for `stream` before it returns (the
 * caller may free it on return). */
int32_t revo_gallery_append(revo_gallery* g, const float* vecs, int64_t n, int32_t normalize, int32_t src_on_device,
                            void* stream);
int64_t revo_gallery_size(const revo_gallery* g);
/* Empties the gallery.  Takes no stream and touches no device memory: the certificate's row maxima are reset on the stream of
 * the next append, ahead of its kernel, so the caller orders a clear exactly as it orders that append (appends still pending
 * on another stream need an event first, as for any two calls on one handle). */
int32_t revo_gallery_clear(revo_gallery* g);
/* copy rows [start, start+n) of the fp32 master copy to dst (host or device); needs keep_f32.  Takes no stream: the caller must
 * first have waited for the streams of the appends, updates and removes that wrote those rows; the copy runs on the default
 * stream and has completed when the call returns. */
int32_t revo_gallery_read(revo_gallery* g, int64_t start, int64_t n, float* dst, int32_t dst_on_device);

/* ---- EDIT: rows leave and change in place (the points-delete and the replacing upsert of the database behind the
 * reference)
 * revo_gallery_remove takes out every row whose bit is set in remove_bits -- the layout of revo_search_set_filter: bit
 * (r & 31) of word r >> 5, ceil(rows / 32) words, host (src_on_device = 0) or device memory, bits at or past `rows`
 * ignored.  `rows` must equal revo_gallery_size(g) (status -2 otherwise).  The survivors keep their relative order: survivor
 * number j becomes row j, in the bf16 scan copy and in the fp32 master (where the gallery has one).  revo_gallery_size drops
 * by *n_removed (host); the capacity is unchanged, so a later append uses the freed rows.  SYNCHRONOUS on `stream`, like
 * revo_gallery_pairs: the host needs the new size.
 * Contract: after the call every entry point of this library returns, byte for byte -- scores, indices, counts, offsets and
 * padding -- what it returns on a fresh gallery to which the surviving fp32 master rows were appended in order with
 * normalize = 0; for a keep_f32 = 0 gallery, what a keep_f32 = 0 gallery built from the same original vectors minus the
 * removed ones returns.  The certificate's running row maxima are NOT recomputed: the maxima over the old rows are upper
 * bounds of the maxima over the survivors, so every certificate stays valid and every result exact (a removed row of huge
 * norm merely leaves the bound looser than a fresh gallery's); they start over, as in revo_gallery_clear, when the gallery
 * becomes empty.
 * The rows move in place in chunks on `stream`: no second copy of the gallery (device memory beyond it: one staging chunk of
 * at most 64 MB, 8 bytes per chunk, and the bitmap's copy when it comes from the host), no traffic for the rows in front of
 * the first removed row.
 * revo_gallery_update overwrites row row_idx[i] (HOST array of n entries) with vecs[i] ([n, dim] fp32, host or device)
 * exactly as an append would have written it: the same normalisation arithmetic, fp32 master, bf16 row, and the row's share
 * merged into the certificate's maxima (which therefore also stay upper bounds).  An index outside [0, size) or a repeated
 * index gives status -2 before the device is touched; n = 0 does nothing.  Enqueued on `stream` like an append, behind one
 * wait for `stream`: the host index array has been read when the call returns.
 * Both invalidate a held pairs, clusters and range result (their _read gives -2, as after an append) and the two-phase candidate
 * state.  A remove that removes at least one row also drops the multi-vector search's index, and a filter or group ids set
 * for the old size fail the next search with the message an append gives (set them again); an update leaves filter, group
 * ids and index valid (none depends on a row's values).  A null handle or pointer or a negative count: status -2, nothing
 * written.  A sharded search (ShardedSearch) over the handle is to be refreshed after a remove. */
int32_t revo_gallery_remove(revo_gallery* g, const uint32_t* remove_bits, int64_t rows, int32_t src_on_device,
                            int64_t* n_removed, void* stream);
int32_t revo_gallery_update(revo_gallery* g, const int64_t* row_idx, const float* vecs, int64_t n, int32_t normalize,
                            int32_t src_on_device, void* stream);

/* ---- DEDUP: the deduplicating append (insert-time dedup of a points database)
 * The gallery holds rows 0 .. N - 1; the call brings n vectors x_0 .. x_{n-1} (vecs: [n, dim] fp32, host or device, as
 * revo_gallery_append takes them) and a threshold t.  m_j is the fp32 master row an ordinary append would write for x_j: the
 * same normalisation arithmetic, the same bits.  s(a, b) is the PAIRS score of two fp32 master rows: the one fma chain, the
 * bits revo_gallery_pairs reports, symmetric bit for bit.  The rows are decided in order j = 0, 1, ...:
 *   D_j = { gallery rows i < N with s(i, m_j) >= t }  united with  { batch rows j' < j that were KEPT and have s(m_j', m_j) >= t }
 *   D_j empty: x_j is KEPT and becomes row N + (number of rows kept before it);
 *   otherwise x_j is DROPPED, and its representative is the member of D_j with the lowest final row index: first seen wins,
 *   gallery rows come before batch rows.
 * A dropped row never suppresses a later one: a greedy leader selection in index order, not connected components.
 * Outputs, n entries each, host or device memory (dst_on_device): rows[j] (int64) = the row's own new row index, or its
 * representative's; scores[j] (fp32) = -inf for a kept row, else the PAIRS bits of s(representative, m_j); *n_kept (host).
 * Consequences:
 *   - after the call every entry point of this library returns, byte for byte, what it returns on a gallery to which only
 *     the kept vectors were appended in order (the wording of revo_gallery_remove's contract; as there, the certificate's
 *     running row maxima may stay looser upper bounds: they include the dropped rows');
 *   - revo_gallery_pairs(t) afterwards holds no pair with an end >= N;
 *   - splitting the batch into consecutive calls, down to one row per call, gives the same rows, scores and gallery;
 *   - two calls on equal galleries give identical bytes;
 *   - the number of duplicate pairs imposes no limit: nothing proportional to the certain edges is stored (16 384 identical
 *     rows are one call).  Only pairs whose bf16 score lies INSIDE the rounding bound of t are stored for the fp32 re-score;
 *     more than 2^28 of those give status -2 (move the threshold).
 * SYNCHRONOUS on `stream`, like revo_gallery_remove: the host needs the new size.  Needs the fp32 master rows (keep_f32 = 0:
 * status -2) and row indices below 2^31, as PAIRS.  0 <= n <= 16 384 per call (larger inputs: consecutive calls, which the
 * semantics make equivalent).  CAPACITY: room for N + n rows is required even if few are kept -- every row of the batch is
 * first written behind the gallery's end.  Status -2 with a message, before the device is touched and with nothing written:
 * a null handle or pointer (vecs may be null at n = 0), a negative or too-large n, a NaN threshold, keep_f32 = 0,
 * insufficient capacity.  On any failure the gallery is as before, with size N.  The handle's filter is NOT consulted (an
 * append invalidates it anyway).  The call invalidates whatever an append invalidates: held pairs, clusters, knn and range
 * results, the two-phase candidate state, the multi-vector index, and filter or group ids sized for N (when a row was kept).
 * revo_search_stats afterwards: slot 3 = ambiguous pairs re-scored in fp32, slot 7 = join passes, every other slot 0. */
int32_t revo_gallery_append_unique(revo_gallery* g, const float* vecs, int64_t n, int32_t normalize, int32_t src_on_device,
                                   float threshold, int64_t* rows, float* scores, int32_t dst_on_device,
                                   int64_t* n_kept, void* stream);

/* ---- search: replaces vector_db.search(query_vector, limit, score_threshold) (core_system.py:659-664)
 * queries: [n_queries, dim] fp32 on the device (normalised internally, cosine semantics).
 * Results, best first under (score desc, index asc): scores [n_queries, k] fp32, indices
 * [n_queries, k] int64 (row index + index_offset), counts [n_queries] int32; entries past
 * counts[q] are -inf / -1.  has_threshold != 0 keeps only score >= threshold.
 *
 * EXACTNESS.  The reference's search is an exhaustive one (qdrant local mode: scores = G @ q over every row, then the
 * ranking).  This search returns exactly what an exhaustive scoring of the gallery's fp32 rows would -- the same rows
 * in the same order, every score an fp32 dot product in one fixed summation order -- although its scan selects on bf16
 * scores: each query carries a certificate (the k-th re-scored score must exceed the best bf16 score of any row that
 * was not re-scored by more than a rigorous bound of |bf16 score - fp32 score|, computed from the rounding norms of
 * the query and of the gallery's rows), and a query that fails it is re-done by a collecting pass over the gallery
 * (every row within that bound of what is needed, re-scored in fp32) and, if that list overflows, by a brute-force
 * fp32 pass.  Searches with k > 25 (64 candidates leave the certificate too little room on ordinary data) scan with an
 * admission margin of twice that bound: what an uncertified query needs is then among the rows its scan kept, and it is
 * re-done exactly WITHOUT another pass over the gallery.  All of it is enqueued on `stream`; revo_search_stats reports how often it happened.  (A gallery created
 * with keep_f32 = 0 has no fp32 rows: it returns the scan's own scores and certifies nothing.)
 * What "exactly" is relative to: the ranking is the exhaustive one UNDER THIS LIBRARY'S fp32 SUMMATION ORDER (one fused
 * multiply-add chain over the D products, k = 0 .. D - 1, of the fp32 query and the fp32 gallery row, both normalised in
 * fp32).  The reference accumulates the same products in float64 and rounds once (numpy G @ q on Python floats): two rows
 * whose true scores differ by less than the fp32 chain's rounding error (about D * 2^-24 * |score| <= 3e-7 at D = 1024) can
 * come out in either order there and here.  tests/test_gpu_search.py therefore compares with the float64 oracle up to
 * swaps of ADJACENT results inside that band (`near_tie`) -- a tolerance of the checker's arithmetic, not of this
 * search -- and asserts that the k-th place of no query of the headline 1 M x 1024 gallery falls inside it; exact
 * duplicates (scores equal to the bit) are always returned index-ascending.
 * FILTERED (revo_search_set_filter): a search of a handle with a filter returns exactly what the same exhaustive scoring
 * of the ALLOWED rows alone would -- the same scores, order, tie rule and threshold cut as an unfiltered search of a
 * gallery holding just those rows, with indices of this gallery.  A disallowed row is never admitted by any scan, never
 * counted towards an admission bound and never collected by the fallback; fewer than k allowed rows leave the tail of
 * a result empty (score -inf, index -1), none at all gives counts 0.
 * GROUPED (revo_search_groups): each row has a group id (int32 >= 0; -1 = in no group, never returned).  A group's key is
 * its best row under the order above (fp32 score desc, row index asc), counting only rows the filter allows and that
 * reach the threshold.  The result is the best `limit` groups in key order, each with its best `group_size` rows in the
 * same order -- exactly what grouping an exhaustive fp32 scoring of the allowed rows gives: the same bits (every score
 * from the one fma chain), ties and threshold cut as revo_search_topk.  A query's groups come from the certified top-50
 * of revo_search_topk when that list decides them (it holds every allowed row at or above the threshold, or >= limit
 * groups of which each of the first `limit` holds >= group_size of its rows: any row outside it ranks below all of
 * them); otherwise from two fp32 passes over the gallery (best groups, then the chosen groups' best rows).
 * LIMIT (galleries of more than 2^24 rows): the scan packs a row as a 24-bit index relative to its slice of the gallery, so
 * a slice holds at most 2^24 rows.  A query tile (256 queries) gets 32, 16, 8, 4, 2 or 1 slices as the call brings 8, 16,
 * 32, 64, 128 or 256 query tiles and more; a call is therefore refused (status -2, "a gallery slice holds at most 2^24 rows",
 * nothing written) from 65 281 queries on when the scan covers more than 2^24 rows (the gallery less a pre-pass of at most
 * 32 768 rows), from 32 513 when more than 2^25 and from 16 129 when more than 2^26 (tests/test_scan_plan.py walks the plan
 * at 2^24 - 1 .. 2^27 rows); larger galleries are refused at fewer queries still.  Whatever the message says about splits,
 * the caller's remedy is to search fewer queries per call: up to 16 128 at a time are served on every gallery of up to 2^27
 * rows. */
int32_t revo_search_topk(revo_gallery* g, const float* queries, int32_t n_queries, int32_t k, int32_t has_threshold,
                         float threshold, int64_t index_offset, float* scores, int64_t* indices, int32_t* counts,
                         void* stream);
/* LARGE K: the same search for 1 <= k <= 1024, same arguments, same result contract word for word (EXACTNESS, FILTERED,
 * threshold, index_offset, padding, the filter's lifecycle).  Needs the fp32 master rows (keep_f32 = 0: status -2).  It
 * takes its own path for every k (the k <= 50 path of revo_search_topk cannot be widened: 32 or 64 candidates per query):
 * the k-th best bf16 score of a sample of the first rows bounds where the answer can start; one MFMA pass histograms every
 * allowed row above that; the histogram gives a band {bf16 score >= b} that provably holds every row of the exact top-k,
 * ties included (b = h - 2 eps, h = a score that k rows reach in bf16); a collecting pass gathers the band, which is
 * re-scored in fp32 (the same chain as every other re-score: the same bits) and sorted.  A query whose band may exceed
 * 8192 rows (thousands of rows within the error bound of its k-th score: near-duplicates) is answered by an exhaustive
 * fp32 scoring of its allowed rows and an exact selection instead.  On `stream`, no host round trip.  revo_search_stats
 * after it: slot 3 = band rows re-scored in fp32, slot 6 = queries that took the exhaustive fallback.  Not for the
 * two-phase sharded protocol below (k <= 50 there). */
int32_t revo_search_topk_large(revo_gallery* g, const float* queries, int32_t n_queries, int32_t k, int32_t has_threshold,
                               float threshold, int64_t index_offset, float* scores, int64_t* indices, int32_t* counts,
                               void* stream);
/* ---- near-duplicate pairs of one gallery (no reference counterpart; same exactness contract as the searches)
 * PAIRS.  The result is exactly the set of pairs (i, j), i < j, of rows that the handle's filter allows (both of them;
 * revo_search_set_filter, with its lifecycle: a filter set for another gallery size gives status -2) whose fp32 score
 * reaches `threshold`.  A score is the fma chain of every re-score in this library (EXACTNESS) over the two fp32 master
 * rows: the same bits a search returns for the same two fp32 rows, and, the product inside fmaf being commutative,
 * score(i, j) == score(j, i) bit for bit.  Pairs are ordered by (i asc, j asc); two calls give identical bytes.  (i, i) is
 * never returned; identical rows at distinct indices are.  How: one MFMA pass over the upper triangle of 256 x 256 tiles of
 * the gallery's bf16 rows keeps every pair whose bf16 score is within the certificate's rounding bound of the threshold
 * (for a row against a row), and those candidates are re-scored in fp32 and sorted on the device.
 * revo_gallery_pairs computes the result into the handle's workspace and writes the pair count to the host *n_pairs.  Unlike
 * the searches it is SYNCHRONOUS on `stream`: it reads the candidate count between its passes.  Needs the fp32 master rows
 * (keep_f32 = 0: status -2) and row indices below 2^31.  A threshold so low that more than 2^28 candidate pairs qualify
 * gives status -2, the count in revo_last_error().  revo_search_stats after it: slot 3 = candidate pairs re-scored in fp32,
 * slot 7 = join passes run (1, or 2 when the candidate workspace had to grow), every other slot 0.
 * revo_gallery_pairs_read copies result entries [start, start + n) to pairs ([n][2] int64) and scores ([n] fp32), host or
 * device memory (dst_on_device).  Like every _read entry point (_pairs, _clusters, _knn, _kmeans and its _centroids, _range,
 * revo_vit_detect_read and _maps) it takes no stream: the result it copies is complete, because the call that computed it is
 * SYNCHRONOUS; the copy runs on the default stream and has completed when the call returns, so a device destination may then
 * be used on any stream.  A result stays valid until the next revo_gallery_pairs call or a change of the gallery's
 * rows: after an append or a clear, or with no result, it gives status -2, as does a range past the result. */
int32_t revo_gallery_pairs(revo_gallery* g, float threshold, int64_t* n_pairs, void* stream);
int32_t revo_gallery_pairs_read(revo_gallery* g, int64_t start, int64_t n, int64_t* pairs, float* scores,
                                int32_t dst_on_device);
/* ---- duplicate clusters: the groups of near-duplicates, not the pairs (no reference counterpart)
 * CLUSTERS.  The graph: its vertices are the rows that the handle's filter allows (revo_search_set_filter, with its
 * lifecycle: a filter set for another gallery size gives status -2); {i, j}, i != j, is an edge exactly when the PAIRS score
 * of the two fp32 master rows -- the one fma chain, symmetric bit for bit -- is >= `threshold`.  Wherever revo_gallery_pairs
 * is defined the edge set is its result set.  labels ([size] int64): labels[r] = the lowest row index of r's connected
 * component; an allowed row with no edge is its own label; a row the filter excludes has -1.  A cluster is a component of
 * at least two rows; clusters are ordered by their lowest row, ascending, and members ascend within a cluster: offsets
 * ([n_clusters + 1] int64, CSR, offsets[0] = 0, offsets[n_clusters] = n_members), members ([n_members] int64).  Two calls
 * give identical bytes: neither the number of join passes nor the order in which the device merges affects the result.
 * How: the PAIRS join with a lock-free union-find in its epilogue.  A pair whose bf16 score is above the threshold by more
 * than the certificate's rounding bound is certainly an edge and is merged in place, never stored; only the pairs inside
 * the bound of the threshold are stored and re-scored in fp32.  So a cluster's size sets no limit (24 000 identical rows
 * are one cluster, where revo_gallery_pairs refuses their 2.9e8 pairs); more than 2^28 pairs INSIDE the bound give status
 * -2, the count in revo_last_error().  Labels, sizes, the sort of the members and the offsets are computed on the device.
 * revo_gallery_clusters computes the result into the handle and writes the two counts to the host *n_clusters and
 * *n_members.  SYNCHRONOUS on `stream`, like revo_gallery_pairs.  Needs the fp32 master rows (keep_f32 = 0: status -2) and
 * row indices below 2^31; a NaN threshold, a null handle or a null count pointer give status -2 before the device is
 * touched.  An empty gallery, or a filter that allows no row: zero clusters, labels none or all -1.  Every loop of the
 * union-find has a trip limit; one that is hit gives status -4 ("clusters: union-find did not converge").
 * revo_search_stats after it: slot 3 = pairs re-scored in fp32 (the ambiguous ones only), slot 7 = join passes run (1, or 2
 * when the candidate workspace had to grow), every other slot 0.
 * revo_gallery_clusters_read copies labels, offsets and members, host or device memory (dst_on_device); each of the three
 * pointers may be NULL independently.  The result stays valid until the next revo_gallery_clusters call or a change of the
 * gallery's rows (append, clear, remove, update): after one, or with no result, it gives status -2.  A pairs result and a
 * range result stay valid across revo_gallery_clusters, and its result across revo_gallery_pairs and revo_search_range. */
int32_t revo_gallery_clusters(revo_gallery* g, float threshold, int64_t* n_clusters, int64_t* n_members, void* stream);
int32_t revo_gallery_clusters_read(revo_gallery* g, int64_t* labels, int64_t* offsets, int64_t* members,
                                   int32_t dst_on_device);
/* ---- exact kNN graph: every row's k nearest other rows (the database's "distance matrix" query; no counterpart in the
 * reference's own code)
 * KNN.  The vertices are the rows that the handle's filter allows (revo_search_set_filter, with its lifecycle: a filter set
 * for another gallery size gives status -2).  score(i, j) is the PAIRS score: the one fma chain over the two fp32 master rows,
 * symmetric bit for bit; wherever revo_gallery_pairs returns (i, j), the two calls give the same bits.  For every allowed row i
 * the result is the best k allowed rows j != i, ordered by (score desc, index asc) and, with has_threshold, cut at score >=
 * threshold: exactly what an exhaustive fp32 scoring of the allowed rows gives.  Row i itself is never returned; rows identical
 * to it at other indices are, index-ascending.  Fewer than k qualifying rows leave the tail at -inf / -1, the number found in
 * counts[i]; a row the filter excludes has counts 0 and an empty list, and it is nobody's neighbour.  Two calls give
 * identical bytes: neither the level estimate, nor the workspace size, nor the number of join passes, nor the order of the
 * device's appends changes a byte.
 * How: the PAIRS join with a level per row.  A pass of all rows against a sample of at most 8 192 rows estimates, per row, a
 * level that a few times k rows reach; the join keeps pair (i, j) when its bf16 score is within the certificate's rounding
 * bound of the lower of the two levels; the candidates are re-scored in fp32, sorted by row on the device, and every row takes
 * the best k of its entries.  A row is certified when none of its candidates was dropped for want of workspace and it has k
 * entries at or above its level (or its level is the threshold / -inf); every other row is answered by an exhaustive fp32
 * scoring of the allowed rows, on the device, in batches.  The estimate is never trusted: it decides speed only.  A gallery of
 * mostly identical rows (each of n duplicates has n - 1 equal partners) is therefore slow -- one pass over the fp32 rows
 * per row -- but correct.
 * Limits: 1 <= k <= 64; needs the fp32 master rows (keep_f32 = 0: status -2) and row indices below 2^31.  A NaN threshold, k
 * out of range, a null handle or a null n_rows give status -2 before the device is touched.  *n_rows receives the gallery
 * size; an empty gallery or a filter that allows no row is not an error.  SYNCHRONOUS on `stream`, like revo_gallery_pairs.
 * revo_search_stats after it: slot 3 = candidates re-scored in fp32, slot 6 = rows answered by the exhaustive fallback,
 * slot 7 = join passes run (1; 0 for an empty gallery), every other slot 0.
 * revo_gallery_knn_read copies rows [start, start + n) of the result to indices ([n][k] int64), scores ([n][k] fp32) and
 * counts ([n] int32), host or device memory (dst_on_device); each of the three pointers may be NULL independently.  The
 * result lives in the handle: it stays valid across revo_gallery_pairs, revo_gallery_clusters and revo_search_range, and
 * their results across it; append, clear, remove and update invalidate it: after one, with no result, or for a range past
 * the end, _read gives status -2. */
int32_t revo_gallery_knn(revo_gallery* g, int32_t k, int32_t has_threshold, float threshold, int64_t* n_rows, void* stream);
int32_t revo_gallery_knn_read(revo_gallery* g, int64_t start, int64_t n, int64_t* indices, float* scores, int32_t* counts,
                              int32_t dst_on_device);
/* ---- exact spherical k-means: a partition of the gallery into themes, each with a centre and a size (no counterpart in the
 * reference's own code)
 * KMEANS.  Input: C = n_centroids initial centroids, fp32 [C][dim], host (src_on_device = 0) or device memory.  normalize = 1:
 * they are normalised exactly as revo_gallery_append(normalize = 1) normalises a row (the same kernel, the same bits);
 * normalize = 0: they are used as given, bit for bit.
 * Participants: the rows that the handle's filter allows (revo_search_set_filter, with its lifecycle: a filter set for another
 * gallery size gives status -2).  Every other row has label -1 and score -inf and contributes to no centroid.
 * Assignment: label[i] = the centroid with the largest score(i, c); ties go to the lowest c.  score(i, c) is the fp32 fma chain
 * of every other re-score in this library (EXACTNESS) over q_i and the centroid's fp32 row, where q_i is the row's fp32 master
 * row as a QUERY: passed through the normalisation every search applies to its queries (for a master row of unit length that
 * moves an element by an ulp at most; a row stored with normalize = 0 is scaled to unit length).  scores[i] = score(i,
 * label[i]) with exactly those bits.  So labels and scores are byte for byte what revo_search_topk(k = 1) returns for the fp32
 * master rows as queries against a gallery that holds the centroids (appended with normalize = 0).
 * Update: for centroid c, its members in ascending row order are split into consecutive chunks of 256; a chunk's partial sum is
 * a plain sequential fp32 add chain over its members' fp32 master rows (as stored) starting from +0.0f; the centroid's sum is
 * the sequential fp32 add chain of the partials in chunk order starting from +0.0f -- no fma, no trees: a numpy float32 loop
 * reproduces it.  The new centroid is that sum normalised by the append's normalisation.  A centroid keeps its previous bits
 * when it has no members, or when its sum has a squared norm (the normalisation's own) that is zero or not finite.
 * Iteration: step t assigns against the centroids C_t.  If t >= 1 and no label changed: stop, *converged = 1.  Else if t =
 * max_iter: stop, *converged = 0.  Else C_{t+1} = update(labels_t).  *n_iter = updates done.  So the returned labels are always
 * the exact assignment against the returned centroids, max_iter = 0 is a pure assignment, and -- the update being a function of
 * the labels alone -- a converged result is a fixed point bit for bit.
 * Two calls give identical bytes: neither the order of the device's atomics, nor the workspace size, nor the number of passes
 * reaches a byte.
 * How: the centroids get a bf16 copy beside their fp32 rows; per step two MFMA passes of every row tile over the centroid tiles
 * -- each row's best bf16 score, then every (row, centroid) whose bf16 score is within twice the certificate's rounding bound
 * (for that row against the centroids) of it -- and an fp32 re-score of those candidates, folded per row by a maximum over
 * (score, lowest centroid).  Every maximiser of the fp32 score is provably among a row's candidates.  The update sorts (label,
 * row) keys on the device and sums chunks in the fixed order.
 * The result lives in the handle, like the kNN graph's: labels [size] int32, scores [size] fp32, sizes [C] int64 (members per
 * centroid under the returned labels) and centroids [C][dim] fp32.  revo_gallery_kmeans_read copies rows [start, start + n) of
 * labels and scores, revo_gallery_kmeans_centroids the centroids and sizes, to host or device memory (dst_on_device); each
 * output pointer may be NULL independently.  The result stays valid across revo_gallery_pairs, revo_gallery_clusters,
 * revo_gallery_knn and revo_search_range, and their results across it; append, clear, remove and update invalidate it: after
 * one, with no result, or for a range past the end, the two read calls give status -2.
 * Limits: 1 <= n_centroids <= 65 536; 0 <= max_iter <= 1 000; dim a multiple of 64; needs the fp32 master rows (keep_f32 = 0:
 * status -2) and row indices below 2^31.  A null pointer, n_centroids or max_iter out of range give status -2 before the device
 * is touched.  A centroid row that is not finite, or has zero norm under normalize = 1, gives status -2 (found from the
 * normalisation pass's statistics).  More than 2^28 candidates in one assignment give status -2.  An empty gallery or a filter
 * that allows no row is not an error: all sizes 0, the centroids returned as normalised.  *n_rows receives the gallery size.
 * SYNCHRONOUS on `stream`, like revo_gallery_pairs: the host reads the changed-label and candidate counts between passes.
 * revo_search_stats after it, summed over the steps: slot 3 = (row, centroid) candidates re-scored in fp32 beyond the one score
 * per row, slot 6 = rows whose label needed a re-score to decide (more than one candidate), slot 7 = assignment passes run
 * (one per step, one more for each step whose candidate workspace had to grow), every other slot 0. */
int32_t revo_gallery_kmeans(revo_gallery* g, const float* centroids, int32_t n_centroids, int32_t normalize,
                            int32_t src_on_device, int32_t max_iter, int32_t* n_iter, int32_t* converged, int64_t* n_rows,
                            void* stream);
int32_t revo_gallery_kmeans_read(revo_gallery* g, int64_t start, int64_t n, int32_t* labels, float* scores,
                                 int32_t dst_on_device);
int32_t revo_gallery_kmeans_centroids(revo_gallery* g, float* centroids, int64_t* sizes, int32_t dst_on_device);
/* ---- range search: every row above a threshold, per query (the reference's score_threshold without its limit,
 * core_system.py:659-664)
 * RANGE.  For each query q the result is exactly the rows the handle's filter allows (revo_search_set_filter, with its
 * lifecycle: a filter set for another gallery size gives status -2) whose fp32 score is >= threshold.  Scores and tie rule
 * are the EXACTNESS contract of revo_search_topk: every score comes from the one fma chain, so it has the bits the other
 * searches return.  Within a query, results are ordered by (score desc, row index asc).  Indices are row + index_offset.
 * offsets[q] .. offsets[q + 1] is query q's slice (CSR), with offsets[0] = 0 and offsets[n_queries] = *n_results.  Two calls
 * give identical bytes.  How: one MFMA pass over the gallery's bf16 rows per chunk of queries keeps every row whose bf16
 * score is within the certificate's rounding bound of the threshold for that query, and those candidates are re-scored in
 * fp32 and sorted on the device.
 * revo_search_range computes the result into the handle and writes its entry count to the host *n_results.  Like
 * revo_gallery_pairs it is SYNCHRONOUS on `stream`.  Needs the fp32 master rows (keep_f32 = 0: status -2); a NaN threshold, a
 * negative n_queries or a null pointer (queries may be null when n_queries = 0) give status -2.  More than 2^28 candidates
 * in one call give status -2, the count in revo_last_error().  n_queries = 0: *n_results = 0 and offsets = {0}; an empty
 * gallery, or a filter that allows no row: all offsets 0.  revo_search_stats after it: slot 3 = candidates re-scored in
 * fp32, slot 7 = candidate passes run (1, or 2 when the candidate workspace had to grow; 0 when no pass ran), every other
 * slot 0.
 * revo_search_range_read copies the offsets ([n_queries + 1] int64; offsets may be NULL) and result entries
 * [start, start + n) to indices ([n] int64) and scores ([n] fp32), host or device memory (dst_on_device).  A result stays
 * valid until the next revo_search_range call or a change of the gallery's rows: after an append or a clear, or with no
 * result, it gives status -2, as does a range past the result.  revo_gallery_pairs and the top-k searches leave it valid
 * (and a range search leaves a pairs result valid). */
int32_t revo_search_range(revo_gallery* g, const float* queries, int32_t n_queries, float threshold, int64_t index_offset,
                          int64_t* n_results, void* stream);
int32_t revo_search_range_read(revo_gallery* g, int64_t* offsets, int64_t start, int64_t n, int64_t* indices, float* scores,
                               int32_t dst_on_device);
/* ---- search by examples: "more like these, and not like those" (relevance feedback; the best_score strategy of the
 * vector database the reference sits on)
 * RECOMMEND.  examples: [n_positive + n_negative, dim] fp32 on the device, the positives first; n_positive >= 1,
 * n_negative >= 0, n_positive + n_negative <= 128.  They are normalised like every query.  For a gallery row r, with
 * s(e, r) the fp32 score of example e against row r (the one fma chain of EXACTNESS: the bits every search returns),
 *   sp = max of s over the positives,  sn = max of s over the negatives  (no negatives: score = sp)
 *   score(r) = sp           if sp > sn
 *            = -(sn * sn)   otherwise   (one fp32 multiply, rounded to nearest, fused with nothing)
 * The result is the best k (1 <= k <= 1024) rows the handle's filter allows (revo_search_set_filter, with its lifecycle),
 * ordered by (score desc, row index asc); has_threshold keeps score >= threshold.  Outputs as revo_search_topk_large for ONE
 * query: scores [k], indices [k] (row + index_offset), counts [1], device memory, padding -inf / -1.  EXACT: the rows, order
 * and score bits that computing score(r) as written for every allowed row and sorting gives.  So one positive and no
 * negative returns what revo_search_topk_large returns for that vector, no negatives return the merge (max per row) of the
 * positives' single searches, and two calls give identical bytes.  How: with e the largest rounding bound of the
 * certificate over the examples, a row's bf16 scan scores bound score(r) from both sides (per branch of the formula, which
 * jumps at sp = sn); the k-th largest lower bound over a sample of the first rows is a level tau that k rows reach; one
 * MFMA pass over the gallery's bf16 rows, which reduces each tile's scores over the example rows in registers, keeps every
 * allowed row whose upper bound reaches tau; those rows are re-scored in fp32 against every example and sorted on the
 * device.  No certificate can fail: tau is a proven lower bound of the k-th score whatever the data; bad data costs
 * candidates, never exactness.
 * Like revo_search_range it is SYNCHRONOUS on `stream`.  Needs the fp32 master rows (keep_f32 = 0: status -2).  A null
 * handle or pointer, n_positive < 1, n_negative < 0, more than 128 examples, k outside 1..1024 or a NaN threshold give
 * status -2 before the device is touched.  An empty gallery, or a filter that allows no row: counts = 0, all padding.
 * revo_search_stats after it: slot 3 = candidate rows re-scored in fp32, slot 7 = 1 when the candidate pass met an allowed
 * row (0: empty gallery, or no row allowed), every other slot 0.  A pairs or a range result held by the handle stays valid. */
int32_t revo_search_recommend(revo_gallery* g, const float* examples, int32_t n_positive, int32_t n_negative, int32_t k,
                              int32_t has_threshold, float threshold, int64_t index_offset, float* scores, int64_t* indices,
                              int32_t* counts, void* stream);
/* ---- discovery and context search over (positive, negative) pairs: "the kind of thing I mean is on THIS side of each of
 * these judgements" -- each pair stays a constraint of its own instead of being folded into one score as RECOMMEND does
 * DISCOVER.  target: [dim] fp32 on the device, or NULL; positives / negatives: [n_pairs, dim] fp32 on the device each, pair
 * i = (positives[i], negatives[i]).  All are normalised like every query.  For a gallery row r, with s(v, r) the fp32 score
 * of vector v against row r (the one fma chain of EXACTNESS: the bits every search returns), sp_i = s(positives[i], r),
 * sn_i = s(negatives[i], r), fs(x) = x / (1 + |x|):
 *   discovery (target != NULL, 0 <= n_pairs <= 63):
 *     rank_i = +1 if sp_i > sn_i else -1;  R = sum of rank_i (an integer, exact);
 *     sig = 0.5 * (fs(s(target, r)) + 1);  score(r) = (float)R + sig
 *   context (target == NULL, 1 <= n_pairs <= 64):
 *     loss_i = fs(min((sp_i - sn_i) - FLT_EPSILON, 0));  score(r) = loss_0 + loss_1 + ... added in pair order, starting
 *     from loss_0.  The score is <= 0; it is +0 for a row on the positive side of every pair.
 * Every operation above is ONE fp32 operation rounded to nearest, in the order written, nothing fused: numpy in float32
 * reproduces the bits.  These formulas are the contract.  So a row is ranked first by how many pairs it sits on the right
 * side of and only then by its similarity to the target (0 < sig < 1); zero pairs with a target rank by sig alone.
 * The result is the best k (1 <= k <= 1024) rows the handle's filter allows (revo_search_set_filter, with its lifecycle),
 * ordered by (score desc, row index asc); has_threshold keeps score >= threshold.  Outputs as revo_search_recommend: scores
 * [k], indices [k] (row + index_offset), counts [1], device memory, padding -inf / -1.  EXACT: the rows, order and score
 * bits that computing score(r) as written for every allowed row and sorting gives; two calls give identical bytes.  How:
 * RECOMMEND's plan.  With e the largest rounding bound of the certificate over the examples, the bf16 scan scores decide a
 * pair's side unless their difference is within 2 e of zero (such a pair counts +1 in the upper bound of R and -1 in the
 * lower), and bound sig and every loss_i from both sides; the k-th largest lower bound over a sample of the first rows is a
 * level k rows reach; one MFMA pass keeps the allowed rows whose upper bound reaches it (a pair's two example rows are
 * laid out so that their scores meet in one lane's registers); those rows are re-scored in fp32 and sorted on the device.
 * No certificate can fail.
 * SYNCHRONOUS on `stream`.  Needs the fp32 master rows (keep_f32 = 0: status -2).  A null handle or output pointer, null
 * positives or negatives with n_pairs > 0, n_pairs outside the mode's range, k outside 1..1024 or a NaN threshold give
 * status -2 before the device is touched, the outputs untouched.  An empty gallery, or a filter that allows no row: counts =
 * 0, all padding.  revo_search_stats after it: slot 3 = candidate rows re-scored in fp32, slot 7 = 1 when the candidate pass
 * met an allowed row, every other slot 0.  A pairs or a range result held by the handle stays valid. */
int32_t revo_search_discover(revo_gallery* g, const float* target, const float* positives, const float* negatives,
                             int32_t n_pairs, int32_t k, int32_t has_threshold, float threshold, int64_t index_offset,
                             float* scores, int64_t* indices, int32_t* counts, void* stream);
/* ---- boosted search: "images like this one, but prefer those taken near this date / near this place / from trusted sources"
 * (the score-boosting query of the vector database the reference sits on, over EVERY allowed row instead of a prefetched
 * candidate list)
 * BOOSTED.  query: [dim] fp32 on the device, ONE query, normalised like every query.  mult / bias: [rows] fp32 on the device,
 * one entry per gallery row in row order; either may be NULL.  For a gallery row r, with s(r) the fp32 score of the query
 * against row r (the one fma chain of EXACTNESS: the bits every search returns), m = mult[r] (NULL: 1), b = bias[r] (NULL: 0),
 *   final(r) = fmaf(m, s(r), b)     ONE correctly rounded fused multiply-add
 * With both arrays NULL final = s with no operation at all: the call is revo_search_topk_large for one query, bit for bit.
 * The result is the best k (1 <= k <= 1024) rows the handle's filter allows (revo_search_set_filter, with its lifecycle)
 * that have s(r) >= min_similarity when has_min_similarity (a cut on the SIMILARITY, not on the boosted score) and
 * final(r) >= threshold when has_threshold, ordered by (final desc, row index asc).  Outputs, padding and index_offset as
 * revo_search_recommend: scores [k] (final), indices [k], counts [1]; similarities [k] carries s(r) of every hit (padding
 * -inf).  EXACT: the rows, their order and both score arrays are those of computing final for every allowed row and sorting;
 * two calls give identical bytes.  How: RECOMMEND's plan.  With a a row's bf16 scan score and e the query's rounding bound,
 * s lies in [lo, hi] = [a - e, a + e] moved outward by their own rounding; a correctly rounded fma is monotone in each
 * argument and m >= 0, so final lies in [fmaf(m, lo, b), fmaf(m, hi, b)] with no further widening.  A row can pass the
 * minimum similarity only if hi reaches it and certainly passes if lo does.  tau = the k-th largest lower bound over the
 * sample rows that certainly pass (raised to the threshold) is a level k rows reach, for ANY sample: here 256-row tiles
 * strided evenly over the gallery (boosts that grow with the row index, as timestamps do, leave no good row in a prefix).
 * One MFMA pass keeps every allowed row that can pass and whose upper bound reaches tau; those rows are re-scored in fp32
 * and sorted on the device.  No certificate can fail and there is no fallback.
 * DOMAIN.  On every allowed row mult must be finite and >= 0 and bias finite.  The pass reads both for every allowed row
 * and counts the rows outside the domain: the call then returns status -2 with that count in revo_last_error() and the
 * outputs are not to be used -- never a wrong answer.  Rows the filter does not allow are not inspected.
 * SYNCHRONOUS on `stream`, like revo_search_recommend.  Needs the fp32 master rows (keep_f32 = 0: status -2).  A null handle,
 * query or output pointer, k outside 1..1024, a NaN threshold or a NaN min_similarity give status -2 before the device is
 * touched.  An empty gallery, or a filter that allows no row: counts = 0, all padding.  revo_search_stats after it: slot 3 =
 * candidate rows re-scored in fp32, slot 7 as for RECOMMEND, every other slot 0.  A pairs or a range result held by the
 * handle stays valid. */
int32_t revo_search_boosted(revo_gallery* g, const float* query, const float* mult, const float* bias, int32_t k,
                            int32_t has_threshold, float threshold, int32_t has_min_similarity, float min_similarity,
                            int64_t index_offset, float* scores, float* similarities, int64_t* indices, int32_t* counts,
                            void* stream);
/* ---- multi-vector search: "which images contain ALL of what this image shows?" -- a point is a set of vectors (the rows of
 * one group), a query is a set of vectors, the score is late-interaction MaxSim (the multi-vector comparator of the vector
 * database the reference sits on)
 * MAXSIM.  queries: [n_vectors, dim] fp32 on the device, 1 <= n_vectors <= 64, normalised like every query.  Groups are the
 * handle's revo_search_set_groups ids: arbitrary int32 >= 0, sparse or non-contiguous, -1 = no group; the filter is the
 * handle's revo_search_set_filter.  Both keep their lifecycle (set for another gallery size: status -2).  With s(i, r) the
 * fp32 score of query vector i against row r (the one fma chain of EXACTNESS: the bits every search returns) and, for a
 * group G, A(G) the set of its rows the filter allows (a group with empty A(G) is not a result):
 *   M_i(G)   = max of s(i, r) over r in A(G)   (compared in fp32, -0 equal to +0)
 *   score(G) = (((M_0 + M_1) + M_2) + ...) + M_{n-1}
 * each addition ONE fp32 addition rounded to nearest, in query order, starting from M_0: numpy in float32 reproduces the
 * bits.  These formulas are the contract.  The result is the best k (1 <= k <= 1024) groups ordered by (score desc, group
 * id asc), -0 ordered as +0; has_threshold keeps score >= threshold (the raw sum, in [-n, n]).
 * Outputs (device memory): scores [k], group_ids [k], counts [1]; optional, NULL independently: part_scores [k][n_vectors]
 * = M_i and part_rows [k][n_vectors] = index_offset + the LOWEST allowed row of the group that attains M_i (part_scores
 * holds that row's own score bits).  Padding -inf, -1, -inf, -1.  An empty gallery, no allowed row with a group, or every
 * group cut by the threshold: counts = 0, all padding.
 * EXACT: the groups, order and bits that evaluating the formulas for every group and sorting gives; two calls give
 * identical bytes.  So n_vectors = 1 with every row its own group returns the rows, order and score bits of
 * revo_search_topk_large; n_vectors = 1 with arbitrary groups returns the group keys of revo_search_groups(limit = k,
 * group_size = 1) wherever that call is defined; the same vector given twice returns the one-vector order with scores
 * fl(M + M).  How: a CSR of group -> rows is built on the device at the first call after revo_search_set_groups (sorted
 * (group, row) keys) and cached in the handle until the ids or the rows change; one MFMA pass over the gallery's bf16 rows
 * with the query vectors as the other operand stores every (allowed row, vector) scan score into a workspace of rows x
 * n_pad x 4 bytes (n_pad = n_vectors rounded up to 4); per group the maxima m_i of those give a = sum m_i, and with e_i the
 * certificate's rounding bound of vector i, score(G) lies within sum e_i plus the rounding of the two fp32 sums of a; tau =
 * the k-th largest lower bound over ALL groups (raised to the threshold) is a level k groups reach; the allowed rows of the
 * groups whose upper bound reaches tau are re-scored in fp32, work split by (row, four vectors), never one wave per group;
 * an exact group reduction, the device radix sort and the emit follow.  No certificate can fail: bad data costs
 * candidates, never exactness.
 * SYNCHRONOUS on `stream`, like revo_search_recommend.  Needs the fp32 master rows (keep_f32 = 0: status -2).  A null
 * handle, null queries, scores, group_ids or counts, n_vectors outside 1..64, k outside 1..1024 or a NaN threshold give
 * status -2 before the device is touched, the outputs untouched, the message naming the argument.  No group ids set, or
 * group ids or a filter set for another size: status -2.  The score workspace cannot be allocated: status -3, its size in
 * the message.  revo_search_stats after it: slot 3 = rows re-scored in fp32 (the allowed rows of the candidate groups),
 * slot 7 = 1 when the pass met an allowed row with a group, every other slot 0.  A pairs or a range result held by the
 * handle stays valid. */
int32_t revo_search_maxsim(revo_gallery* g, const float* queries, int32_t n_vectors, int32_t k, int32_t has_threshold,
                           float threshold, int64_t index_offset, float* scores, int32_t* group_ids, int32_t* counts,
                           float* part_scores, int64_t* part_rows, void* stream);
/* ---- diverse search: top-k by maximal marginal relevance (the Mmr(diversity, candidates_limit) re-ranking of a nearest-
 * neighbour query in the vector database the reference sits on: a gallery of video frames and region crops is full of
 * near-identical rows, and the plain top-10 of one is ten copies of the same frame)
 * MMR.  1 <= k <= candidates <= 1024, 0 <= diversity <= 1.  queries as every search: [n_queries, dim] fp32 on the device,
 * normalised internally.
 * Candidates of a query: exactly the result of revo_search_topk_large(g, q, k = candidates, has_threshold, threshold) --
 * the same rows, order (score desc, row asc), score bits, filter semantics (revo_search_set_filter, with its lifecycle) and
 * threshold cut.  Call them c_0 .. c_{n-1} (n <= candidates) and rel(i) their scores.
 * Similarity sim(i, j): the fp32 score of the two candidates' fp32 master rows under the one fma chain of EXACTNESS -- the
 * bits revo_gallery_pairs reports for that pair (PAIRS).  Symmetric bit for bit; sim(i, i) is never used.
 * Selection: lam = 1.0f - diversity (one fp32 subtraction).  S = the candidates picked so far, empty at the start.  Each of
 * the min(k, n) steps picks, among the candidates not in S, the one with the largest
 *   v(i) = fl( fl(lam * rel(i)) - fl(diversity * m(i)) ),   m(i) = max over j in S of sim(i, j)
 * (S empty: v(i) = fl(lam * rel(i))): three separately rounded fp32 operations, nothing fused.  Values compare as fp32
 * numbers with -0 = +0; among equal values the lower candidate position i wins.
 * Outputs (device memory; [n_queries, k] each, counts [n_queries]) in PICK order: indices = row + index_offset, scores =
 * rel (the bits the plain search returns), mmr_values = the v the row was picked with (mmr_values may be NULL).  Padding
 * -inf / -inf / -1.  Two calls give identical bytes.  So diversity = 0 returns exactly revo_search_topk_large(k)'s rows,
 * order and score bits; k = candidates returns a permutation of the candidates; the first pick is c_0 whenever lam > 0.
 * How: the inner large-k search writes the candidate lists into the handle's workspace; one kernel computes each query's
 * n x n similarity matrix from the gathered fp32 master rows (vector fma chains in the fixed order, no MFMA); one workgroup
 * per query runs the greedy selection with the matrix row of each pick.
 * Asynchronous on `stream` like revo_search_topk_large (no host round trip).  Needs the fp32 master rows (keep_f32 = 0:
 * status -2).  A null handle or pointer (queries may be null when n_queries = 0), a negative n_queries, candidates outside
 * 1..1024, k outside 1..candidates, a diversity that is NaN or outside [0, 1], or a NaN threshold give status -2 before
 * the device is touched, the outputs untouched.  An empty gallery, or a filter that allows no row: counts = 0, all padding.
 * revo_search_stats after it: what the inner large-k search leaves (slot 3 = band rows re-scored in fp32, slot 6 = queries
 * that took the exhaustive fallback, every other slot 0).  A pairs or a range result held by the handle stays valid; the
 * two-phase state below is dropped as revo_search_topk_large drops it. */
int32_t revo_search_mmr(revo_gallery* g, const float* queries, int32_t n_queries, int32_t k, int32_t candidates,
                        float diversity, int32_t has_threshold, float threshold, int64_t index_offset, float* scores,
                        float* mmr_values, int64_t* indices, int32_t* counts, void* stream);
/* ---- hybrid queries: several searches fused into one result by rank or by normalised score (the prefetch + fusion query of
 * the vector database the reference sits on: "frames that look like this picture AND match these words").  Text-image cosines
 * of a CLIP model lie far below image-image cosines, so adding raw scores -- or searching with an averaged vector -- ranks by
 * the image term alone; fusing ranks (reciprocal rank fusion, RRF) or per-list standardised scores (distribution-based score
 * fusion, DBSF) does not.
 * FUSION.  A fused search has m lists, 1 <= m <= 64 (n_lists); a call carries n >= 0 fused searches (n_searches), n * m < 2^31.
 * queries: [n, m, dim] fp32 on the device, list j of search i is row i * m + j, normalised internally.  limit = C is every
 * list's length, 1 <= C <= 1024 and m * C <= 8192; 1 <= k <= 1024 rows are returned.  method: 0 = RRF, 1 = DBSF.  rrf_k: fp32,
 * finite and >= 0, used by RRF only.  weights: host float[m] or NULL (all 1), each finite and >= 0.  list_thresholds: host
 * float[m] or NULL (none); -inf = no cut for that list, NaN is refused.  has_threshold / threshold cut on the fused score.
 * List L_ij: exactly the result of revo_search_topk_large(g, q_ij, k = C, no threshold) -- the same rows, order (score desc,
 * row asc), score bits, filter semantics (revo_search_set_filter, with its lifecycle).  An entry whose score is < t_j is
 * dropped; a kept entry keeps its 1-based position r in the UNCUT list; the kept entries, in position order, are the list's
 * members.
 * Contribution of a member:
 *   RRF   c = fl32(w_j / fl32(rrf_k + fl32(r))): two fp32 operations, the division correctly rounded.
 *   DBSF  fp64 throughout, every operation rounded on its own, nothing contracted to an fma.  Over the members' scores in
 *         position order (n_m of them): S = ((s_1 + s_2) + ...), mu = S / n_m, V = sum of (s - mu) * (s - mu) in the same
 *         order, sd = sqrt(V / n_m).  If !(sd > 0): v = 0.5f; otherwise v = fl32((s - (mu - 3 * sd)) / (6 * sd)), not clamped.
 *         c = fl32(w_j * v).
 * Fused score F(row): the sequential fp32 sum of the row's contributions over j ascending, starting from the first one
 * present.  A row in no list is not a candidate; a row whose only lists have weight 0 is a candidate with F = 0.
 * Result: the candidates ordered by (F desc as fp32 numbers with -0 = +0, row asc), those with F < threshold cut, the first k.
 * Outputs (device): scores [n, k] = F (its own bits, a -0 included), indices [n, k] = row + index_offset, counts [n]; optional
 * (NULL allowed) ranks [n, k, m] int32 = r, or 0 where the row is no member of list j, and list_scores [n, k, m] fp32 = the
 * row's score against q_ij under the one fma chain of EXACTNESS for every j, member or not (wherever revo_search_topk_large
 * returns that row for that query it returns these bits).  Padding -inf / -1 / 0 / -inf.  Two calls give identical bytes.
 * How: one inner large-k search over all n * m queries into the handle's workspace; one workgroup per fused search gathers
 * the members as 64-bit words, sorts them in LDS (equal rows become one run), sums each run sequentially, sorts the runs by F
 * and writes the first k; a second kernel scores the (result row, list) pairs.  Asynchronous on `stream`, no host round trip.
 * Needs the fp32 master rows (keep_f32 = 0: status -2).  A null handle, queries (unless n = 0) or scores / indices / counts,
 * n < 0, or m, C, m * C, k, method, rrf_k, a weight, a list threshold (NaN) or the fused threshold (NaN) outside the domains
 * above give status -2 before the device is touched, the outputs untouched.  An empty gallery, or a filter that allows no
 * row: counts = 0, all padding.  revo_search_stats after it: what the inner large-k search leaves.  A pairs or a range result
 * held by the handle stays valid; the two-phase state is dropped as revo_search_topk_large drops it.
 * revo_topk_fuse is the same fusion over lists the caller already holds -- the merged lists of a row-sharded search, lists
 * from two galleries of the same items: scores and indices [n, m, C], counts [n, m], all on the device.  No gallery, no
 * list_scores.  Entries past a list's count are ignored (a count above C counts as C).  Indices must lie in [0, 2^47);
 * neither that nor duplicates are checked on the device.  Lists need not be sorted: the threshold cut is per entry, the
 * statistics run over the kept entries in position order.  A row that occurs twice in one list contributes once per
 * occurrence in position order, and ranks reports the first.  revo_search_fusion is this op applied to its inner lists, bit
 * for bit.  Launches on the current device. */
int32_t revo_search_fusion(revo_gallery* g, const float* queries, int32_t n_searches, int32_t n_lists, int32_t limit,
                           int32_t method, float rrf_k, const float* weights, const float* list_thresholds, int32_t k,
                           int32_t has_threshold, float threshold, int64_t index_offset, float* scores, int64_t* indices,
                           int32_t* counts, int32_t* ranks, float* list_scores, void* stream);
int32_t revo_topk_fuse(const float* scores, const int64_t* indices, const int32_t* counts, int32_t n_searches,
                       int32_t n_lists, int32_t limit, int32_t method, float rrf_k, const float* weights,
                       const float* list_thresholds, int32_t k, int32_t has_threshold, float threshold,
                       float* out_scores, int64_t* out_indices, int32_t* out_counts, int32_t* out_ranks, void* stream);
/* ---- the same search in two phases, for a gallery that is row-sharded over several GPUs / ranks (one shard per
 * handle).  The reference has a single process and a single collection (core_system.py:659-664); this is the
 * scale-out of that call.  Per rank:
 *   1. revo_search_candidates: scan the shard (same kernels as revo_search_topk); the query's candidates stay in the
 *      handle, and bounds [n_queries, top_m] receives the scan scores of the best top_m of them as order-preserving
 *      uint32 (0 = none).  top_m <= revo_search_ksel(k); parts * top_m >= min(64, 2 * revo_search_ksel(k)) makes the bound below tight.
 *   2. all-gather `bounds` over the ranks -> all_bounds [parts, n_queries, top_m]   (RCCL; 4 * top_m bytes per query and rank)
 *   3. revo_search_finish: only candidates that can still be among the best j = min(64, 2 * revo_search_ksel(k)) of the
 *      WHOLE gallery (scan score at or above the j-th largest published score) are re-scored in fp32; results as
 *      revo_search_topk.  (Twice the unsharded search's candidates: with that margin the exactness certificate of the
 *      merge all but never fails on ordinary data, which saves the protocol's second round.)
 *      all_bounds may be NULL (re-score every candidate).  Same queries, k and stream as step 1.
 *   4. all-gather the per-rank results and revo_topk_merge_packed them (with revo_search_finish's cert block and the
 *      merge's unc_* outputs: the cross-shard exactness certificate; step 5 re-does what it cannot certify).
 *      revo_topk_merge on plain [parts, n_queries, k] arrays is valid only for shards that do NOT estimate (no
 *      revo_search_set_total_rows, or revo_search_estimates(k) == 0) and then certifies nothing across shards.
 * With steps 4 and 5 the merged result equals the unsharded revo_search_topk of the concatenated gallery.
 * The ordinary case is ONE exchange per search: shards that know the total row count (revo_search_set_total_rows) and
 * search for k <= 25 skip steps 2-3's exchange (revo_search_estimates(k) == 1: all_bounds = NULL on every rank). */
int32_t revo_search_ksel(int32_t k);     /* candidates the scan keeps per query for a top-k search (32 or 64) */
/* Tell a shard's handle how many rows the WHOLE row-sharded gallery has (0 = forget).  revo_search_candidates then starts
 * its scan from an estimate of the score a candidate of the whole gallery has to reach (extrapolated from the shard's own
 * first rows) instead of what the shard's own rows would admit: fewer survivors per tile, a faster scan.  The estimate is
 * not trusted: step 4's certificate counts it as the score an unseen row may have, and step 5 re-does what it cannot
 * certify -- results are the exhaustive search's whatever the estimate was, PROVIDED the certificate is used: once a total
 * is set, revo_search_finish refuses cert = NULL after an estimating scan (status -2), and revo_topk_merge_packed with its
 * unc_* outputs plus revo_search_exact are mandatory parts of the search.  revo_search_topk ignores the setting. */
int32_t revo_search_set_total_rows(revo_gallery* g, int64_t total_rows);
/* Restrict the following searches of this handle (revo_search_topk, _candidates, _finish, _exact) to the rows whose
 * bit is set: bit (r & 31) of word r >> 5.  `rows` must equal revo_gallery_size(g).  The bitmap (ceil(rows / 32)
 * words, host or device memory) is copied into the handle on `stream`.  NULL clears the filter.
 * The handle owns its copy (a host bitmap has been read when this returns; a device one is read on `stream`).  A search
 * while the gallery's size differs from `rows` (rows appended after the filter was set) fails (status -2).  A filtered
 * shard of a row-sharded search never scans against the estimate of revo_search_set_total_rows: pass the exchanged
 * bounds (all_bounds) to revo_search_finish. */
int32_t revo_search_set_filter(revo_gallery* g, const uint32_t* allow_bits, int64_t rows, int32_t src_on_device,
                               void* stream);
/* The group id of every row for the following grouped searches of this handle (GROUPED above): group_of_row[r] >= 0, or
 * -1 for none; `rows` must equal revo_gallery_size(g).  Host or device memory, copied into the handle on `stream` (a host
 * array has been read when this returns).  NULL clears them.  Lifecycle as revo_search_set_filter: a grouped search while
 * the gallery's size differs from `rows` fails (status -2). */
int32_t revo_search_set_groups(revo_gallery* g, const int32_t* group_of_row, int64_t rows, int32_t src_on_device,
                               void* stream);
/* The best `limit` groups of each query (1 <= limit <= 50, 1 <= group_size <= 50, limit * group_size <= 50), with the
 * handle's filter and group ids; needs the fp32 master rows (keep_f32 = 1).  Device outputs: scores / indices
 * [n_queries, limit, group_size] (row index + index_offset), hit_counts [n_queries, limit] (rows in each group's list),
 * group_ids [n_queries, limit], group_counts [n_queries] (groups returned).  Padding: score -inf, index -1, hit count 0,
 * group id -1.  No host round trip; revo_search_stats slot 5 counts the queries that took the fp32 passes. */
int32_t revo_search_groups(revo_gallery* g, const float* queries, int32_t n_queries, int32_t limit, int32_t group_size,
                           int32_t has_threshold, float threshold, int64_t index_offset, float* scores, int64_t* indices,
                           int32_t* hit_counts, int32_t* group_ids, int32_t* group_counts, void* stream);
/* 1 if a two-phase search for the best k on shards that know the total row count scans against that estimate (then every
 * shard's list is already cut at the whole gallery's level and step 2's exchange may be skipped: pass all_bounds = NULL to
 * revo_search_finish on EVERY rank), 0 if not (k > 25: those scans run with the admission margin of revo_search_topk instead) */
int32_t revo_search_estimates(int32_t k);
/* how a search of n_queries against the gallery's current rows would run (reporting only): out4 = { 1 if the 256 x 256
 * scan takes it (0: the small-gallery scan), rows covered by the pre-pass GEMM, gallery slices per query tile, ksel } */
int32_t revo_search_plan(const revo_gallery* g, int32_t n_queries, int32_t k, int64_t* out4);
int32_t revo_search_candidates(revo_gallery* g, const float* queries, int32_t n_queries, int32_t k, int32_t top_m,
                               uint32_t* bounds, void* stream);
int32_t revo_search_finish(revo_gallery* g, int32_t n_queries, int32_t k, int32_t has_threshold, float threshold,
                           int64_t index_offset, const uint32_t* all_bounds, int32_t parts, int32_t top_m, float* scores,
                           int64_t* indices, int32_t* counts, float* cert, void* stream);
/* cert ([n_queries] fp32; optional only while the shard does not estimate, see revo_search_set_total_rows): this shard's share of the exactness certificate -- the best fp32 score any of its
 * rows that was NOT re-scored can have (scan score of the best such row + the error bound; -inf if every row was
 * re-scored).  All-gathered with the results (it is the third block of the packed layout below) and checked by
 * revo_topk_merge_packed against the merged k-th score.
 *   5. revo_search_exact: second round for the queries that check failed for (none on ordinary data): entry j is query
 *      q_idx[j] of the last revo_search_candidates call, need[j] the fp32 score a row must reach to change its merged
 *      result (both device arrays, identical on every rank: the merge step's unc_q / unc_need, sorted by query).  The
 *      shard collects every row whose scan score is within the error bound of need[j], re-scores it in fp32 and returns
 *      its exact local top-k in row j of scores / indices / counts ([n, k], [n, k], [n]); all-gathered and merged like
 *      step 4, these replace the queries' first-round results. */
int32_t revo_search_exact(revo_gallery* g, int32_t n, const int32_t* q_idx, const float* need, int32_t k,
                          int32_t has_threshold, float threshold, int64_t index_offset, float* scores, int64_t* indices,
                          int32_t* counts, void* stream);
/* counters of the handle's last search, read after `stream` has drained (host array of 8): out8 = { queries the
 * certificate failed for (-1: the gallery has no fp32 rows), of those: brute-forced, queries the certificate was
 * evaluated for, rows the exact passes re-scored, of the failed queries: resolved from what the scan had kept (no second
 * pass over the gallery: searches with k > 25 scan with an admission margin for that), grouped search
 * (revo_search_groups): queries its top-50 did not decide (answered by the fp32 passes), revo_search_topk_large: queries
 * that took the exhaustive fallback (0 after every other search), revo_gallery_pairs: join passes, revo_search_range:
 * candidate passes (0 after every other search) }.  After revo_search_topk_large slot 3 counts the rows of the bands it
 * re-scored and slots 0, 1, 2, 4, 5 are 0; after revo_gallery_pairs see PAIRS, after revo_gallery_clusters see CLUSTERS, after revo_search_range see RANGE,
 * after revo_search_recommend see RECOMMEND, after revo_search_boosted see BOOSTED, after revo_search_mmr see MMR, after revo_search_maxsim see MAXSIM, after
 * revo_gallery_knn see KNN, after revo_gallery_kmeans see KMEANS. */
int32_t revo_search_stats(revo_gallery* g, int32_t* out8, void* stream);
/* merge `parts` result sets laid out [parts, n_queries, k] (the all-gathered per-shard
 * results of a row-sharded gallery) into one [n_queries, k] set, same ordering rule. */
int32_t revo_topk_merge(const float* scores, const int64_t* indices, int32_t parts, int32_t n_queries, int32_t k,
                        int32_t has_threshold, float threshold, float* out_scores, int64_t* out_indices,
                        int32_t* out_counts, void* stream);

/* One result set packed for a single all-gather: [n_queries, k] int64 indices, [n_queries, k] fp32 scores, then
 * [n_queries] fp32 certificate bounds (revo_search_finish's cert), padded to revo_topk_packed_bytes(n_queries, k) bytes;
 * `packed` holds `parts` such blocks back to back.  unc_count / unc_q / unc_need (optional, device: [1], [n_queries],
 * [n_queries]): the merge checks every query's certificate over all shards and lists the queries that fail it (in no
 * particular order) with the score a row needs to enter their result -- the input of revo_search_exact. */
int64_t revo_topk_packed_bytes(int32_t n_queries, int32_t k);
int32_t revo_topk_merge_packed(const void* packed, int32_t parts, int32_t n_queries, int32_t k, int32_t has_threshold,
                               float threshold, float* out_scores, int64_t* out_indices, int32_t* out_counts,
                               int32_t* unc_count, int32_t* unc_q, float* unc_need, void* stream);

/* ---- single kernels, exposed for parity tests and micro-benchmarks (device pointers) */
int32_t revo_op_gemm(int32_t epilogue, const void* a_bf16, int64_t lda, const void* b_bf16, int64_t ldb, int32_t m,
                     int32_t n, int32_t k, void* c, int64_t ldc, const float* bias, const float* gamma, void* stream);
/* C bf16 = rope(A . B^T + bias): the QKV projection with the axial rotary embedding of the first
 * rope_cols columns fused into the epilogue (cos_sin: [seq][head_dim/2] (cos, sin) pairs; row r is token r % seq) */
int32_t revo_op_gemm_rope(const void* a_bf16, int64_t lda, const void* b_bf16, int64_t ldb, int32_t m, int32_t n, int32_t k,
                          void* c_bf16, int64_t ldc, const float* bias, const float* cos_sin, int32_t seq,
                          int32_t head_dim, int32_t rope_cols, void* stream);
/* The two halves of a LayerNorm folded into the GEMMs around it (how the forward runs ln_1 / ln_2 of batch-sized calls; the
 * gain and shift live in the consuming GEMM's weights: W' = bf16(gamma . W), bias' = bias + W beta, csum_j = sum_k W'_jk):
 *  - revo_op_gemm_resid_ln: the residual GEMM  C f32 [m][n] += gamma * (A . B^T + bias)  which, where its launch form covers all
 *    rows with the persistent 256 x 256 kernel (then *done = 1; else only C is written and *done = 0), also writes
 *    xb bf16 [m][ldxb] = bf16(new C) and stats [m][n / 256] pairs of float (mean, sum of squared deviations) of every
 *    256-column slice of the new row;
 *  - revo_op_gemm_ln_in: C bf16 = epilogue(rstd * (A . B^T - mean * csum) + bias), epilogue 0 = plain, 1 = exact-erf GELU, the
 *    row's mean and rstd = 1 / sqrt(var + eps) merged from `parts` slices of `stats` as written above. */
/*    With xlo (bf16 [m][ldxb]) the residual stream itself may be in two bf16 planes (xb_bf16, xlo) = (bf16(x), bf16(x - bf16(x))),
 *    as the forward keeps it between folded GEMMs: x_in_planes != 0 takes the old values from there instead of c, planes_out
 *    != 0 writes the new ones there instead of to c (needs a folding form, else status -2); stats may be NULL for planes in,
 *    fp32 out (the last residual GEMM of a forward). */
int32_t revo_op_gemm_resid_ln(const void* a_bf16, int64_t lda, const void* b_bf16, int64_t ldb, int32_t m, int32_t n, int32_t k,
                              float* c, int64_t ldc, const float* bias, const float* gamma, void* xb_bf16, int64_t ldxb,
                              void* stats, int32_t* done, void* xlo_bf16, int32_t x_in_planes, int32_t planes_out, void* stream);
int32_t revo_op_gemm_ln_in(int32_t epilogue, const void* a_bf16, int64_t lda, const void* b_bf16, int64_t ldb, int32_t m, int32_t n,
                           int32_t k, void* c_bf16, int64_t ldc, const float* bias, const float* csum, const void* stats,
                           int32_t parts, float eps, void* tele, void* stream);
/*    tele (optional; device, 3 x uint64, zeroed by the caller): the counters behind revo_vit_stats -- rows merged, rows with
 *    |mean| * rstd > 8, rows with |mean| * rstd > 32. */
/* The two launches of the forward that the entries above cannot make:
 *  - revo_op_gemm_ln_in_rope: the qkv projection of a batch-sized forward, revo_op_gemm_ln_in's folded consumer with
 *    revo_op_gemm_rope's rotary epilogue (rope of rstd * (A . B^T - mean * csum) + bias);
 *  - revo_op_gemm_resid_norm: revo_op_gemm's residual epilogue (C f32 += gamma * (A . B^T + bias), split-K scratch of its
 *    own) with the LayerNorm that follows offered to the launcher as a one-image forward offers it: where the form is split-K
 *    with the LayerNorm in the reduce, ln_out (bf16 [m][ln_ldo]) receives the normalised new rows (no affine) and
 *    *fused = 1; else only C is written and *fused = 0. */
int32_t revo_op_gemm_ln_in_rope(const void* a_bf16, int64_t lda, const void* b_bf16, int64_t ldb, int32_t m, int32_t n, int32_t k,
                                void* c_bf16, int64_t ldc, const float* bias, const float* csum, const void* stats, int32_t parts,
                                float eps, const float* cos_sin, int32_t seq, int32_t head_dim, int32_t rope_cols, void* stream);
int32_t revo_op_gemm_resid_norm(const void* a_bf16, int64_t lda, const void* b_bf16, int64_t ldb, int32_t m, int32_t n, int32_t k,
                                float* c, int64_t ldc, const float* bias, const float* gamma, void* ln_out_bf16, int64_t ln_ldo,
                                float eps, int32_t* fused, void* stream);
/* ---- calibration probes (bench.py's `calibration` object; not on the reference's path: nothing there to cite).  Two fixed
 * kernels that say how fast the BOX is, so that bench lines taken on different MI355X devices can be compared:
 *  - revo_probe_mfma: `blocks` workgroups of four waves, each wave `iters` trips of 32 register-resident
 *    v_mfma_f32_16x16x32_bf16 on operands read once from src (bf16, n_elems of them, random data); sink receives one
 *    float per thread (blocks * 256).  revo_probe_mfma_flops(blocks, iters) = the launch's FLOPs.
 *  - revo_probe_copy: dst[0, bytes) = src[0, bytes), 16 bytes per lane (the HBM copy rate: 2 * bytes of traffic). */
int32_t revo_probe_mfma(const void* src_bf16, int64_t n_elems, float* sink, int32_t blocks, int32_t iters, void* stream);
int64_t revo_probe_mfma_flops(int32_t blocks, int32_t iters);
int32_t revo_probe_copy(void* dst, const void* src, int64_t bytes, void* stream);
#ifdef REVO_EXPERIMENTS
/* Kernel-variant selection and timing experiments: compiled only into librevo_exp.so (`make exp`: the same sources
 * with -DREVO_EXPERIMENTS; used by scripts/ and by the forced-tile runs of tests/test_gpu_kernels.py), never into
 * librevo.so, whose kernels are chosen by its size heuristics alone.  Process-global, not thread-safe.
 * Every variant computes the same result (split-K changes the fp32 summation order only). */
/* Parity-test hooks (tests/ load librevo_exp.so for them; the product library has no way to stop a forward early, to
 * read intermediate buffers, or to switch the exactness machinery of a search off):
 * run only the first n transformer blocks (n = -1: the whole forward; n = -2: stop after the patch embedding, before
 * ln_pre) and copy the fp32 residual stream [batch*seq, width] of the last forward to dst (device). */
int32_t revo_vit_set_debug_layers(revo_vit* vit, int32_t n_layers);
int32_t revo_vit_read_residual(revo_vit* vit, int32_t batch, float* dst, void* stream);
/* other intermediate buffers of the last forward (device to device): which = 0 the residual stream (fp32 [batch*seq, width]),
 * 1 the ln_post output after a whole forward (fp32 [batch*seq, width]: the head works in fp32), 2 the attention-pool
 * output after its MLP residual, before proj (fp32 [batch, width]) */
int32_t revo_vit_read_tap(revo_vit* vit, int32_t which, int32_t batch, void* dst, void* stream);
/* the text tower's: n = -2 stops after the token embedding, n >= 0 after the first n blocks, -1 runs the whole forward;
 * read_residual copies the fp32 residual stream [batch * seq_len of the last forward, width] to dst (device) */
int32_t revo_text_set_debug_layers(revo_text* text, int32_t n_layers);
int32_t revo_text_read_residual(revo_text* text, int32_t batch, float* dst, void* stream);
/* how the certificate treats the handle's searches: 0 = certificate + fallback (the product library's only behaviour),
 * 1 = every query takes the collecting pass, 2 = every query takes the brute-force pass -- and every query of a grouped
 * search the grouped fp32 passes, and every query of revo_search_topk_large its exhaustive fallback (1 and 2: parity tests of the fallback against the fast path), 3 = certificate evaluated and counted but no fallback (timing only: NOT exact) */
int32_t revo_search_set_mode(revo_gallery* g, int32_t mode);
/* rows per chunk of revo_gallery_remove (rounded up to a multiple of 32, at most 65536; 0 = the default, 64 MB of fp32 rows):
 * tests cross many chunk boundaries with a small gallery.  Same result for every value. */
int32_t revo_debug_set_remove_chunk(int64_t rows);
/* revo_gallery_knn's paths (tests hold every one of them to the same bytes; speed only): cap_keys = candidate keys its
 * workspace holds (0 = the default; small enough and keys are dropped, their rows take the fallback); level_mode 0 = the
 * estimate, 1 = every level -inf (or the threshold), 2 = every level +2.0: nothing is a candidate and every row falls back,
 * 3 = the sample-derived level raised by a fixed 0.05: some rows come up short and some do not. */
int32_t revo_debug_set_knn(int64_t cap_keys, int32_t level_mode);
/* revo_gallery_kmeans' candidate workspace (tests hold a workspace that has to grow to the bytes of the default run; speed
 * only): cap_keys = candidate keys it starts with (0 = the default). */
int32_t revo_debug_set_kmeans(int64_t cap_keys);
/* phase groups of the persistent 256 x 256 GEMM (an experiment, measured in round 5 and not adopted): 0 / 1 = off (all
 * workgroups in step), 2..4 = that many groups, a workgroup of group g doing the first (g + 1) / groups of its first tile at the start and the
 * rest of that tile last.  Result-preserving (bit-identical). */
int32_t revo_op_set_phase_groups(int32_t groups);
/* 0: the persistent body GEMMs' bf16 epilogues on the round-5 kernel (LDS-transposed stores, drained before the next main loop);
 * 1 (default): the queued-stores kernel.  Same bits either way (A/B timing, parity of the two kernels). */
int32_t revo_op_set_qstores(int32_t on);
/* diagnostic: device array [workgroups][items][4] of uint64 the phased kernel fills with 100 MHz time stamps (main loop
 * begin, main loop end, epilogue issued) and the piece's rows, for its first `items` pieces per workgroup; NULL = off */
int32_t revo_debug_gemm_stamps(void* buf, int32_t items);
/* diagnostic: device array [workgroups][2] of uint64 the body attention kernel fills with the shader-clock ticks and the 100 MHz
 * ticks of each workgroup's lifetime (their ratio x 100 MHz = the clock the chip holds under this kernel); NULL = off */
int32_t revo_debug_attention_clock(void* buf);
/* the GEMM launch forms issued since the last call with reset != 0, as a bitmask (gemm kernels and properties of the
 * launch: the GemmForm bits of revers-o_amd/csrc/kernels.h); reset != 0 also clears the record.  Host-side only. */
int32_t revo_debug_gemm_forms(int32_t reset);
/* 0 = size heuristic (default), 128 or 256 = force that GEMM tile */
int32_t revo_op_set_gemm_tile(int32_t tile);
/* bits 4-7 = force the XCD arrangement (N-stripes 1, 2, 4 or 8; 0 = heuristic), bits 8-11 = force the attention
 * waves per workgroup, bit 12 = disable the GEMM tail split, bit 16 = one workgroup per tile instead of the persistent
 * 256 x 256 GEMM, bit 17 = no split-K for the leftover rows of a residual GEMM, bit 18 = 256 x 256 tiles also for
 * problems with fewer than 100 of them, bit 19 = the two-buffer 128 x 64 kernel instead of its six-deep-ring form,
 * bit 20 = head_dim-64 attention on v_mfma_f32_16x16x32_bf16 instead of 32x32x16 (round 6's MFMA-shape experiment);
 * 0 = normal */
int32_t revo_op_set_variant(int32_t flags);
/* 0 = ln_1 / ln_2 as LayerNorm kernels in front of their GEMMs instead of the folded form (A/B timing, parity of one
 * against the other); 1 = default (folded, the residual stream in two bf16 planes between the folded GEMMs); 2 = folded
 * with the stream as fp32 rows plus a bf16 copy */
int32_t revo_op_set_ln_fold(int32_t on);
/* Timing experiments.  The variant bits above plus: bit 0 = skip the GEMM epilogue stores, bit 1 = skip the GEMM main loop,
 * bit 13 = skip the scan's selection, bit 15 = skip the scan's slow path (all four: WRONG RESULTS),
 * bit 14 = count scan events for revo_debug_scan_stats. */
int32_t revo_op_set_gemm_debug(int32_t flags);
/* The phases of the scan launch of a search of Q queries over `rows` scanned gallery rows (host logic only, no device):
 * out[0] = phases, out[1] = segment slots per query, then per phase: first block, first query tile, query tiles, slices.
 * Returns the number of workgroups of the launch (-1: bad arguments). */
int64_t revo_debug_scan_plan(int32_t Q, int64_t rows, int64_t* out, int32_t cap);
/* The launch plan of a GEMM (revers-o_amd/csrc/gemm_plan.h) under the library's current switches (revo_op_set_variant,
 * revo_op_set_qstores, revo_op_set_gemm_tile ...): host logic only, no device.  epi: 0 bf16, 1 bf16 + GELU, 2 residual, 3 fp32,
 * 4 patch embedding, 5 bf16 + RoPE (with the table's rows, the head dimension and the rotated columns).  ws_elems: the
 * split-K workspace in fp32 elements (0: none).  offers: bit 0 a LayerNorm to fuse behind a residual GEMM, 1 the folded
 * LayerNorm's producer outputs, 2 residual stream read from planes, 3 written to planes, 4 the folded LayerNorm's row
 * statistics (consumer), 5 the caller prefers 256 x 256 tiles.  out (cap >= 30): [0] the GemmForm bits of the call (-1: the
 * launcher refuses the call), [1] steps (1 or 2), then 14 values per step: kernel form bit, first row, rows, XCD
 * arrangement gy, persistent workgroups per XCD, grid x, grid y, 192-row tile rows, how many of them tall, leftover rows
 * fused into the launch, split-K parts, the reduce does the LayerNorm, plane format pair, folds.  Returns out[0]; -2: bad
 * arguments. */
int64_t revo_debug_gemm_plan(int32_t epi, int32_t m, int32_t n, int32_t k, int64_t lda, int64_t ldb, int64_t ldc, int64_t ws_elems,
                             int32_t offers, int32_t rope_seq, int32_t rope_head_dim, int32_t rope_cols, int64_t* out, int32_t cap);
/* 1 if a forward of `batch` images keeps the residual stream in two bf16 planes between its folded GEMMs (reporting) */
int32_t revo_debug_stream_in_planes(const revo_vit* vit, int32_t batch);
/* The tables of the ACTIVE grid shape (GRIDS), device to device on `stream`: pos_dst [S'][width] fp32, rope_dst [S'][head_dim /
 * 2][2] fp32 (cos, sin) -- for the tests that hold them to the fp64 formulas. */
int32_t revo_vit_read_grid_tables(revo_vit* vit, float* pos_dst, float* rope_dst, void* stream);
/* copies bytes of the handle's search workspace to host_dst (host_dst NULL: returns the workspace size) */
int64_t revo_debug_read_workspace(revo_gallery* g, int64_t offset, int64_t bytes, void* host_dst);
/* experiment: bounds = device array [Q] of order-preserving u32 scan scores (the format revo_search_candidates publishes)
 * that the next searches on this handle take as lower limits of their admission bounds (NULL: off).  Stands in for a
 * bound exchanged between the shards before the scan; the caller guarantees each is <= the query's true ksel-th score. */
int32_t revo_debug_seed_bounds(revo_gallery* g, const uint32_t* bounds);
/* experiment (scripts/gridbar_probe.py): `iters` stages of "every workgroup writes n16 x 16 bytes, a device-wide
 * synchronisation, every workgroup reads another XCD's slice", as ONE launch with grid barriers (mode 0: a counter, mode 2: a flag word per workgroup, mode 3: XCD-hierarchical counters; the grid must be
 * co-resident; the spin is bounded: ctr_err[1] != 0 afterwards = timed out (1) or read stale data (2)) or as 2 x iters launches
 * (mode 1).  ctr_err: 1696 device words; stamps: 2 x iters uint64 (100-MHz clock of workgroup 0 around each barrier) or NULL. */
int32_t revo_probe_gridbar(int32_t mode, void* ctr_err, void* buf, int32_t n16, int32_t blocks, int32_t threads,
                           int32_t iters, float* sink, void* stamps, void* stream);
/* counters of the fused scan when debug bit 14 is set */
int32_t revo_debug_scan_stats(int64_t* out8);
#endif
/* (w / b NULL: normalise only -- how the forward runs the LayerNorms it cannot fold: their gain and shift live in the weights
 * of the linear layer behind them) */
int32_t revo_op_layernorm(const float* x, int64_t ldx, const float* w, const float* b, float eps, int32_t rows,
                          int32_t width, void* out, int64_t ldo, int32_t out_is_bf16, void* stream);
/* ln_post with the attention pool's logits out of the same pass (K9 + K10's scores): out = LayerNorm(x) in fp32 and
 * logits[(r / seq * heads + h) * seq + r % seq] = out[r] . qk[h] + ck[h] (qk [heads, width], ck [heads]; rows % seq == 0).
 * A row's results do not depend on how many rows the call has (a batch takes four rows per wave): same bits. */
int32_t revo_op_layernorm_logits(const float* x, int64_t ldx, const float* w, const float* b, float eps, int32_t rows,
                                 int32_t width, float* out, int64_t ldo, const float* qk, const float* ck, int32_t heads,
                                 int32_t seq, float* logits, void* stream);
/* the head's fp32 linear layers (head.hip gemm_f32_skinny_kernel; M = batch rows, weights [N, K] streamed once):
 * C = epi(A . Wt^T + bias), epi 0 = none, 1 = exact GELU, 2 = added to what C holds.  K % 16 == 0, rows 16-byte aligned.
 * K is cut into the same sixteen ranges, summed in the same order, whatever M is: a row's result does not depend on the
 * other rows of the call, bit for bit. */
int32_t revo_op_linear_f32(int32_t epi, const float* A, int64_t lda, const float* Wt, int64_t ldw, const float* bias, int32_t M,
                           int32_t N, int32_t K, float* C, int64_t ldc, void* stream);
/* the same kernel with grouped A rows, as the pool's value projection runs it: output columns [g * group_cols,
 * (g + 1) * group_cols) read row m of A at A + g * a_group_stride + m * lda (one pooled row per head).  group_cols == 0: no
 * groups (revo_op_linear_f32); otherwise group_cols % 16 == 0 and a_group_stride % 4 == 0.  Same K split and order: the bits
 * of revo_op_linear_f32 on group g's rows and columns. */
int32_t revo_op_linear_f32_grouped(int32_t epi, const float* A, int64_t lda, int64_t a_group_stride, int32_t group_cols,
                                   const float* Wt, int64_t ldw, const float* bias, int32_t M, int32_t N, int32_t K, float* C,
                                   int64_t ldc, void* stream);
/* the pool's probe folded into its key projection at load time (head.hip probe_qk_kernel): qk[h * width + i] = sum over the
 * rows o of head h (o in [h * width / heads, (h + 1) * width / heads)) of q[o] * Wk[o * width + i], ck[h] = sum of q[o] * bk[o];
 * q [width] (already scaled), Wk [width, width], bk [width], all fp32 on the device.  width % heads == 0. */
int32_t revo_op_probe_qk(const float* q, const float* Wk, const float* bk, int32_t width, int32_t heads, float* qk, float* ck,
                         void* stream);
/* the row normaliser (elementwise.hip l2norm_rows_kernel) whole: the kernel that writes every gallery row and every query,
 * example and prompt, and measures the rounding norms the exactness certificate is built from.  All pointers device memory.
 *   src [rows][ld_src] fp32; row r goes to row r of the outputs or, with dst_rows (int64 [rows]), to row dst_rows[r]: the
 *   same bits either way.  dst_f32 [..][ld_f32] fp32 and dst_bf16 [..][ld_bf16] bf16 (round to nearest even of the fp32
 *   row) are each optional (null).  normalize = 0: y = x, a bit copy.  normalize = 1: y = x * (1 / sqrt(sum x^2)), the sum
 *   in fp32: lane l of a wave adds columns l, l + 64, ... by fma, then the xor butterfly 32 .. 1 -- one order for a row
 *   whatever the batch, its position in it, or the form (registers up to dim 2048, a loop above).
 *   The normalised row is within a few ulp of x / ||x|| (tests/_norm_bounds.py gives the terms) for
 *   sqrt(dim) * 2^-62 <= ||x|| < 2^64.  From 2^64 up that fp32 sum is +inf and the row comes out as zeros.  Below the range
 *   the sum is partly, then wholly (||x|| < 2^-63) subnormal and loses bits -- the row still comes out near unit length,
 *   with an error that grows to a few per cent near sqrt(dim) * 2^-72 -- and once every x^2 rounds to 0 (every
 *   |x| <= 2^-75) the row is left as it is, like an all-zero row.  e / e.norm() in fp32 does the same at both ends.
 *   row_stats (optional) [rows][2], by SOURCE row: ||bf16(y) - y||, ||bf16(y)||.  max_stats (optional) [2]: max'ed, never
 *   overwritten, with ||y|| and ||bf16(y) - y|| of every finite row (a NaN / Inf row is left out).  The sums of squares are
 *   taken on the row scaled by a power of two from its largest element, so a finite row of ANY length has its norms
 *   measured: rows stored with normalize = 0 are certified whatever their length.  (A norm past fp32's range, 2^128, is
 *   +inf in max_stats: no search is certified against such a row.)
 *   zero_a / zero_b (optional): zero_a_words / zero_b_words 32-bit words set to 0 by the same launch (rows >= 1).
 * Status -2 before the device is touched: null src, rows < 0, dim < 1, a stride below dim, a null array to clear with a
 * positive count.  rows = 0 does nothing. */
int32_t revo_op_l2norm_rows(const float* src, int64_t ld_src, float* dst_f32, int64_t ld_f32, uint16_t* dst_bf16, int64_t ld_bf16,
                            int64_t rows, int32_t dim, int32_t normalize, float* row_stats, float* max_stats, uint32_t* zero_a,
                            int64_t zero_a_words, uint32_t* zero_b, int64_t zero_b_words, const int64_t* dst_rows, void* stream);
/* the certificate's maxima of a gallery as its searches read them, to HOST out[2]: out[0] >= ||g||, out[1] >= ||bf16(g) - g||
 * for every row g now present (running maxima over every row written since the gallery was last empty: upper bounds after a
 * remove or an update; both 0 for an empty gallery).  Waits for `stream`.  Null argument: status -2. */
int32_t revo_op_gallery_cert_stats(revo_gallery* g, float* out, void* stream);
/* the attention pool's weighted row sums (K10; head.hip): u[(b * heads + h) * width + c] = sum_s softmax_s(logits[b, h, :])[s] *
 * x[b * seq + s][c], all fp32; logits [batch, heads, seq].  A column's sum is taken in one fixed order whatever the batch
 * (the batch only decides how many columns a lane carries): bit-identical between a batch and its images one at a time. */
int32_t revo_op_pool_rows(const float* x, int64_t ldx, const float* logits, int32_t batch, int32_t seq, int32_t width,
                          int32_t heads, float* u, void* stream);
/* the same sums over a region's tokens (region_pool.hip): u[(r * heads + h) * width + c] for region r of image region_image[r]
 * (DEVICE int32, [n_regions]), softmax and sum restricted to the tokens region_bits [n_regions][ceil(seq / 32)] (device) allows,
 * in the order of revo_op_pool_rows restricted to them: every token allowed = that function's bits; none (or an image index
 * outside [0, batch)) = zeros.  Disallowed rows and logits are never read. */
int32_t revo_op_pool_rows_masked(const float* x, int64_t ldx, const float* logits, const int32_t* region_image,
                                 const uint32_t* region_bits, int32_t n_regions, int32_t batch, int32_t seq, int32_t width,
                                 int32_t heads, float* u, void* stream);
/* the kernels of revo_vit_detect without a tower (detect.hip; DETECT above is their contract):
 *  - revo_op_detect_scores: tokens [rows][dim] and prompts [n_prompts][dim] fp32; prompts_norm [n_prompts][dim] receives the
 *    prompts normalised as every search normalises its queries; scores[p * rows + r] = the fma chain over prompts_norm[p] and
 *    tokens[r] (the token rows are used as given).  dim % 4 == 0, 1 <= n_prompts <= 64.  Enqueued on `stream`.
 *  - revo_op_detect_regions: scores [batch][n_prompts][g * g] and thresholds [n_prompts] (DEVICE here) -> labels [batch][g * g],
 *    counts [batch] (regions per image) and the regions of all images, image after image, in revo_vit_detect_read's arrays
 *    (each sized for batch * max_regions regions; bits [.][ceil((g * g + use_cls) / 32)], cell c at bit use_cls + c); every
 *    output but counts may be NULL.  A staging buffer lives for the length of the call, which is SYNCHRONOUS on `stream`;
 *    status -4 as revo_vit_detect. */
int32_t revo_op_detect_scores(const float* tokens, int64_t rows, const float* prompts, int32_t n_prompts, int32_t dim,
                              float* prompts_norm, float* scores, void* stream);
int32_t revo_op_detect_regions(const float* scores, int32_t batch, int32_t n_prompts, int32_t g, int32_t use_cls,
                               const float* thresholds, int32_t n_background, int32_t min_cells, int32_t max_regions,
                               int32_t* region_image, int32_t* region_prompt, int32_t* boxes, int32_t* cells, float* confidence,
                               uint32_t* bits, int32_t* labels, int32_t* counts, void* stream);
int32_t revo_op_rope(void* qkv_bf16, int64_t ld, const float* cos_sin, int32_t rows, int32_t seq, int32_t width,
                     int32_t heads, void* stream);
int32_t revo_op_attention(const void* qkv_bf16, int64_t ld, void* out_bf16, int64_t ldo, int32_t batch, int32_t seq,
                          int32_t heads, int32_t head_dim, void* stream);
/* causal attention of the text tower (text.hip) on the same qkv layout: 1 <= seq <= 128, head_dim 64, fp32 scores and a
 * two-pass softmax with the row's real maximum.  Output row i is a function of rows 0..i of its sequence alone, bit for
 * bit, whatever finite values the rows past i hold.  ld % 8 == 0, ldo % 4 == 0. */
int32_t revo_op_attention_causal(const void* qkv_bf16, int64_t ld, void* out_bf16, int64_t ldo, int32_t batch, int32_t seq,
                                 int32_t heads, int32_t head_dim, void* stream);
/* x[(b * seq + s) * ldx + c] = table[tokens_dev[b * seq + s]][c] + pos[s][c] (one fp32 add: bit-exact); tokens_dev: DEVICE
 * int32 [batch * seq]; an id outside [0, vocab) gives a row of NaN instead of a wild read.  width % 4 == 0, ldx % 4 == 0. */
int32_t revo_op_embed_tokens(const int32_t* tokens_dev, const float* table, const float* pos, int32_t batch, int32_t seq,
                             int32_t vocab, int32_t width, float* x, int64_t ldx, void* stream);
/* end-of-text pooling of the text tower: out[b * width + c] = x[(b * seq + s_b) * ldx + c], s_b the FIRST position of prompt
 * b's largest id (a copy: bit-exact); tokens_dev: DEVICE int32 [batch * seq], any int32 values.  width % 4 == 0, ldx % 4 == 0,
 * ldx >= width; out is dense [batch][width]. */
int32_t revo_op_pool_eot(const int32_t* tokens_dev, const float* x, int64_t ldx, int32_t batch, int32_t seq, int32_t width,
                         float* out, void* stream);
int32_t revo_op_f32_to_bf16(const float* src, int64_t ld_src, void* dst_bf16, int64_t ld_dst, int64_t rows,
                            int32_t cols, void* stream);

/* ---- per-kernel-class device timing (HIP events on the launch stream) for bench.py.
 * on: 0 = off, 1 = every kernel class, 2 = only the four body GEMM classes (the roofline kernel),
 * 3 = every fourth launch of each of those classes (all layers have the same shapes);
 * an event pair costs a few microseconds of stream time per kernel, so the timed region uses 3. */
int32_t revo_prof_enable(int32_t on);
int32_t revo_prof_reset(void);
/* writes a JSON object {"class": {"launches": n, "ms": t}, ...} into buf */
int32_t revo_prof_report(char* buf, int32_t capacity);

/* ---- preprocessing: crop + squash-resize on the device ----------
 * Replaces the host-side  self.preprocess(image_pil.convert("RGB"))  resize of
 * core_system.py:335 / :439 (transform built at :200) for frames that are already decoded to
 * uint8 RGB in device memory, and implements the per-region crop the reference leaves as a
 * placeholder (core_system.py:406 "Use global for now"; crop idea at :687-690).
 * Bit-identical to PIL's  Image.crop(box).resize((S, S), Image.BILINEAR).
 * `jobs` is a HOST array; src pointers are device memory, interleaved RGB (H x W x 3).
 * out: device uint8 [n][3][out_size][out_size], ready for revo_vit_forward(image_dtype = 1).
 * Asynchronous on `stream` like everything else (`jobs` is read before the call returns; the source frames and `out`
 * must stay valid until the stream has run the work).  Calls on one device share a workspace: calls on one stream
 * are ordered by it, a call on another stream first waits for the previous call's stream. */
typedef struct revo_crop_job {
    const uint8_t* src;      /* device pointer to the top-left pixel of the source image */
    int32_t height, width;   /* source image size in pixels */
    int64_t row_stride;      /* bytes between source rows (>= width * 3) */
    int32_t x0, y0, x1, y1;  /* crop box, half-open [x0, x1) x [y0, y1); the whole image = 0, 0, width, height */
} revo_crop_job;
int32_t revo_preprocess_crop_resize(const revo_crop_job* jobs, int32_t n, int32_t out_size, uint8_t* out, void* stream);
/* The same to out_h x out_w: out [n, 3, out_h, out_w], bit-identical to Image.crop(box).resize((out_w, out_h), Image.BILINEAR)
 * -- the input of a forward under revo_vit_set_grid(gh, gw) with out_h = gh * P, out_w = gw * P.  The entry above is this one
 * with out_h = out_w = out_size.  Each of out_h, out_w in 1..4096 (status -2 before the device is touched). */
int32_t revo_preprocess_crop_resize_hw(const revo_crop_job* jobs, int32_t n, int32_t out_h, int32_t out_w, uint8_t* out,
                                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* REVO_H */
