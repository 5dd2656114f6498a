/*
 * surya_amd.h -- C ABI of libsurya_amd.so, the MI355X (gfx950) implementation of surya's batched model-inference
 * hot path. Plain pointers and sizes only; no torch types. All device pointers are HIP device memory owned by the
 * caller (PyTorch-ROCm caching allocator on the Python side); the library owns only what it allocates in
 * *_create(): KV-cache slots, activation workspaces and small pinned staging buffers, freed by *_destroy().
 *
 * Nothing like this exists in the reference (it has no native code at all): each entry point
 * cites the reference Python interface it replaces. The reference-side binding a maintainer would add is shown in
 * INTEGRATION.md.
 *
 * Conventions
 *   - every function returns int: 0 = ok, <0 = SA_ERR_* (caller error), >0 = hipError_t passthrough.
 *     Nothing throws across the ABI.
 *   - all work is enqueued on the hipStream_t passed in (as void*); functions do not synchronise unless
 *     documented ("sync"). A handle is re-entrant but not thread-safe: one host thread per handle, like the
 *     reference's single-threaded device path (surya/settings.py:179-183).
 *   - dtype: 0 = fp32 ("reference mode": exact-f32 MFMA, used for bit-exact token tests), 1 = bf16, 2 = fp16 (every engine and the op-level
 *     entries). surya_rec_config takes all three: SA_DTYPE_F16 runs the recogniser -- vision encoder, prompt prefill, KV append, the decode steps
 *     with the device-resident greedy loop, the heads, surya_rec_copy_last_logits, surya_rec_encode_only -- in fp16 with torch's .half()
 *     rounding (nearest even, overflow to +-inf; no loss scaling, no clamping) and fp32 accumulation; surya_rec_set_mx_weights and
 *     surya_rec_set_kv_fp8 return SA_ERR_UNSUPPORTED on an fp16 handle as on an fp32 one.
 */
#ifndef SURYA_AMD_H
#define SURYA_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SA_OK 0
#define SA_ERR_ARG (-1)
#define SA_ERR_SHAPE (-2)
#define SA_ERR_UNSUPPORTED (-3)
#define SA_ERR_STATE (-4)
#define SA_ERR_NOMEM (-5)

#define SA_DTYPE_F32 0
#define SA_DTYPE_BF16 1
#define SA_DTYPE_F16 2

/* Library / build info: returns a static string "surya_amd <version> gfx950". */
const char* surya_amd_version(void);

/* ------------------------------------------------------------------------------------------------------------
 * Recognition model: vision encoder + decoder + heads.
 * Replaces SuryaModel.forward (surya/common/surya/__init__.py:274-338), process_outputs / decode / prefill
 * (surya/recognition/__init__.py:294-471) and ContinuousBatchingCache (surya/recognition/cache.py:7-109).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct surya_rec_config {
    /* vision encoder (surya/common/surya/encoder/config.py:18-53) */
    int32_t enc_depth, enc_hidden, enc_inter, enc_inter_pad, enc_heads;
    int32_t patch_dim, patch_dim_pad;    /* 588 and its K padding (multiple of 64) */
    int32_t merge;                       /* spatial_merge_size */
    int32_t window_tokens;               /* window_size / merge / patch_size (merged tokens per window side) */
    int32_t enc_out_hidden;
    uint32_t fullatt_mask;               /* bit i set: block i attends over the whole image */
    float enc_eps;
    /* decoder (surya/common/surya/decoder/config.py:28-85) */
    int32_t vocab, dec_hidden, dec_inter, dec_layers, dec_heads, dec_kv_heads, dec_head_dim;
    float dec_eps;
    /* model (surya/common/surya/config.py:12-71) */
    int32_t bbox_size, embed_multiplier;
    int32_t image_token_id, pad_token_id, eos_token_id;
    /* capacities */
    int32_t max_slots;            /* continuous-batching slots (RecognitionPredictor batch size) */
    int32_t max_kv_len;           /* prompt + generated tokens per slot */
    int32_t max_patches;          /* encoder chunk capacity in patches (reference: encoder_chunk_size) */
    int32_t max_prefill_tokens;   /* packed prompt tokens per prefill call */
    int32_t dtype;
} surya_rec_config;

/* Weight table: device pointers in the compute dtype (inv_freq tables are fp32), kernel layout:
 *   Linear weights [out, in_padded] row-major; gate|up fused and row-interleaved (g0,u0,g1,u1,...), q|k|v fused.
 * Index = SA_RW_* for globals, SA_RW_ENC(l, k), SA_RW_DEC(l, k) for layers. The Python loader
 * (surya_amd/recognition/weights.py) builds it from the reference's state-dict names. */
enum {
    SA_RW_PATCH = 0, SA_RW_MERGER_LN, SA_RW_FC1_W, SA_RW_FC1_B, SA_RW_FC2_W, SA_RW_FC2_B, SA_RW_IMG_H, SA_RW_IMG_W,
    SA_RW_DEC_NORM, SA_RW_TOK_EMBED, SA_RW_LM_W, SA_RW_LM_B, SA_RW_BBOX_W, SA_RW_BBOX_B, SA_RW_ENC_INVFREQ,
    SA_RW_DEC_INVFREQ, SA_RW_GLOBALS
};
enum { SA_RE_NORM1 = 0, SA_RE_QKV_W, SA_RE_QKV_B, SA_RE_PROJ_W, SA_RE_PROJ_B, SA_RE_NORM2, SA_RE_GU_W, SA_RE_GU_B,
       SA_RE_DOWN_W, SA_RE_DOWN_B, SA_RE_COUNT };
enum { SA_RD_LN1 = 0, SA_RD_QKV_W, SA_RD_QKV_B, SA_RD_O_W, SA_RD_LN2, SA_RD_GU_W, SA_RD_DOWN_W, SA_RD_COUNT };
#define SA_RW_ENC(l, k) (SA_RW_GLOBALS + (l) * SA_RE_COUNT + (k))
#define SA_RW_DEC(cfg_enc_depth, l, k) (SA_RW_GLOBALS + (cfg_enc_depth) * SA_RE_COUNT + (l) * SA_RD_COUNT + (k))
#define SA_RW_TOTAL(enc_depth, dec_layers) (SA_RW_GLOBALS + (enc_depth) * SA_RE_COUNT + (dec_layers) * SA_RD_COUNT)

typedef struct surya_rec surya_rec;

/* Bytes of device memory *_create will allocate for this config (KV cache + workspaces). */
size_t surya_rec_workspace_bytes(const surya_rec_config* cfg);

/* Create a model instance. `weights` has SA_RW_TOTAL entries; the caller keeps the tensors alive. */
int surya_rec_create(const surya_rec_config* cfg, const void* const* weights, int n_weights, surya_rec** out);
int surya_rec_destroy(surya_rec* h);

/* Host-only planning of the vision encoder's index math for one packed batch of images: window order
 * (get_window_index, encoder/__init__.py:552-597), rotary position ids (rot_pos_emb, :523-550), window / image
 * segment boundaries (:615-646). Runs without a GPU; exposed for tests.
 *   grid_hw      [n_images*2]  patch-grid (h, w) per image (both even)
 *   src_row      [P]           window-ordered row r reads original tile row src_row[r]
 *   pos_hw       [P*2]         (h, w) patch coordinates in window order
 *   cu_window    [*n_windows+1] patch offsets of the (non-empty) windows, capacity P/4 + n_images + 1
 *   merged_src   [P/merge^2]   window-ordered merged token g came from original merged token merged_src[g]
 */
int surya_rec_plan_encoder(const surya_rec_config* cfg, const int32_t* grid_hw, int n_images, int32_t* src_row,
                           int32_t* pos_hw, int32_t* cu_window, int32_t* n_windows, int32_t* merged_src);

/* Prefill n sequences into KV slots (replaces RecognitionPredictor.prefill's model call + cache merge,
 * recognition/__init__.py:354-471 and cache.py:57-105).
 *   tiles        device fp32 [P, patch_dim], merge-block-major rows as produced by the processor
 *                (processor/__init__.py:214-228), images concatenated in sequence order
 *   grid_hw      host [n_images*2]
 *   input_ids    host, packed prompt tokens of all sequences (no padding)
 *   seq_offsets  host [n_seqs+1]
 *   slot_ids     host [n_seqs] destination slots (distinct, < max_slots)
 * Image features are scattered to the positions where input_ids == image_token_id, in order
 * (common/surya/__init__.py:214-225). Afterwards each slot holds its first generated token as next input and
 * outputs(step 0) hold token / score / bbox for the slots given. Enqueue only. */
int surya_rec_prefill(surya_rec* h, const float* tiles, const int32_t* grid_hw, int n_images, const int32_t* input_ids,
                      const int32_t* seq_offsets, const int32_t* slot_ids, int n_seqs, void* stream);

/* surya_rec_prefill with one prompt shared by several slots: sequence i is encoded and prefilled ONCE, into its lead slot
 * fan_slots[fan_offsets[i]], and afterwards occupies every slot of fan_slots[fan_offsets[i] .. fan_offsets[i + 1]) -- any slots, in any
 * order, at least one per sequence. Every fan slot gets the sequence's length, a head row of its own (so with forced decoding on, its own
 * forced column, cursor and step outputs; with forcing off the fan slots run identical greedy streams) and, behind the decoder layers,
 * a copy of the lead's prompt rows of every layer, kv head, K and V (csrc/kv_fanout.h). Outputs(step 0) hold token / score / bbox for
 * every fan slot. The other arguments, tiles == NULL included, are surya_rec_prefill's, and the lead slots take that call's code path.
 *   fan_offsets  host [n_seqs+1], fan_offsets[0] == 0, strictly increasing
 *   fan_slots    host [fan_offsets[n_seqs]], distinct, < max_slots, at most max_slots in all
 * Checked before anything is enqueued or changed: SA_ERR_ARG for offsets that do not start at 0 or do not increase (an empty fan), a slot
 * out of range or named twice, more than max_slots fan slots; SA_ERR_STATE while beam search (which owns whole groups and forks on its
 * own) or the FP8 KV cache is on. Enqueue only. */
int surya_rec_prefill_shared(surya_rec* h, const float* tiles, const int32_t* grid_hw, int n_images, const int32_t* input_ids,
                             const int32_t* seq_offsets, const int32_t* fan_offsets, const int32_t* fan_slots, int n_seqs, void* stream);
/* Test hook, like surya_rec_copy_last_logits: rows [0, rows) of every layer's and kv head's run of `slot` in the KV cache, to the device
 * buffers k_out / v_out [dec_layers][dec_kv_heads][rows][dec_head_dim] of the handle's dtype. SA_ERR_ARG for a slot out of range or rows
 * outside 1..max_kv_len. Enqueue only. */
int surya_rec_copy_kv_rows(surya_rec* h, int slot, int rows, void* k_out, void* v_out, void* stream);

/* The prompt store: prompts that outlive their slots (csrc/kv_store.h). A kept prompt ("entry") is a range [first, first + len) of store
 * rows that holds the prompt's K and V rows of every layer and kv head -- [K | V][layer][kv_head][rows][head_dim] of the handle's dtype --
 * and, in a side array indexed by `first`, the pre-norm hidden row the prefill's head pass reads for the first token. The caller hands out
 * row ranges, as it hands out slots; the handle keeps a table of live entries (first -> len) and checks every call against it. A handle
 * that never reserves rows allocates nothing. Only the prompt is kept: rows appended by decode steps are not.
 *
 * surya_rec_reserve_prompts: the store holds at least `rows` rows afterwards (never shrinks; rows <= the current capacity changes
 * nothing). Growing allocates a new block, copies the old rows over in stream order and frees the old block once they are there (it waits
 * for the device). No captured decode step holds an address of the store, so none is dropped. SA_ERR_ARG for rows < 0; an allocation
 * failure leaves the store as it was. */
int surya_rec_reserve_prompts(surya_rec* h, int rows, void* stream);
/* surya_rec_prefill that also keeps prompts: behind the decoder layers, sequence i with keep_first[i] >= 0 has its rows [0, len_i) and its
 * last hidden row copied to the store at row keep_first[i] (in this call, because the hidden rows do not survive the next launch that
 * uses the workspace), and [keep_first[i], keep_first[i] + len_i) becomes a live entry. The slots take surya_rec_prefill's code path and
 * emit their first token as ever; the other arguments are that call's.
 *   keep_first   host [n_seqs], first store row of sequence i, or -1 to keep nothing of it
 * Checked before anything is enqueued or changed: SA_ERR_ARG for a value below -1, a range that reaches past the reserved rows or
 * overlaps a live entry or another range of this call; SA_ERR_STATE while the FP8 KV cache is on. Enqueue only. */
int surya_rec_prefill_keep(surya_rec* h, const float* tiles, const int32_t* grid_hw, int n_images, const int32_t* input_ids,
                           const int32_t* seq_offsets, const int32_t* slot_ids, int n_seqs, const int32_t* keep_first, void* stream);
/* Land kept prompts in slots: entry first[i] is read once and written to every slot of fan_slots[fan_offsets[i] .. fan_offsets[i + 1]).
 * Every fan slot gets the entry's length as kv_len and a head row of its own, computed from the stored hidden row by the kernels that end
 * a prefill: outputs(step 0) and the slots' next tokens are what surya_rec_prefill of the same prompt would have left, under whatever the
 * surya_rec_set_slot_* calls before it set on the slots (masks, pattern / lexicon / boost states, forced columns). With beam search on
 * every fan is one lead slot of a whole group and the first selection follows, as in surya_rec_prefill.
 *   first        host [n], live entries (an entry may be named more than once)
 *   fan_offsets  host [n+1], fan_offsets[0] == 0, strictly increasing
 *   fan_slots    host [fan_offsets[n]], distinct, < max_slots, at most max_slots in all
 * Checked before anything is enqueued or changed: SA_ERR_ARG for an unknown entry and for what surya_rec_prefill_shared refuses in its
 * fans (with beam search on also a fan of more than one slot, or a slot that does not lead a whole group); SA_ERR_STATE while the FP8 KV
 * cache is on (the store holds bf16 / fp16 / fp32 rows only). MXFP8 decode weights are fine: no prefill kernel reads them. Enqueue only. */
int surya_rec_restore(surya_rec* h, const int32_t* first, const int32_t* fan_offsets, const int32_t* fan_slots, int n, void* stream);
/* Forget entries: host bookkeeping only, their rows may be handed out again. SA_ERR_ARG (and nothing forgotten) if one of them is not a
 * live entry or is named twice. */
int surya_rec_drop_prompts(surya_rec* h, const int32_t* first, int n);
/* Test hooks: the store's capacity in rows and the number of live entries. */
int surya_rec_prompt_store_info(surya_rec* h, int32_t* cap_rows, int32_t* live_entries);

/* Look-ahead encoding (no counterpart in the reference, which encodes inside the prefill call, common/surya/__init__.py:
 * 130-195): run the vision encoder for the images of the NEXT prompts on the library's own low-priority stream (after
 * the work already queued on `stream`, which produced `tiles`), concurrently with decode steps on `stream`. The merged
 * image embeddings stay inside the handle; a later surya_rec_prefill with tiles == NULL consumes them front to back
 * (its images must be the next ones in the order given here; grid_hw is still required). At most one look-ahead batch is
 * outstanding: SA_ERR_STATE while the previous one has unconsumed images, SA_ERR_SHAPE above max_prefill_tokens image
 * tokens. n_images == 0 (tiles / grid_hw may be NULL) discards whatever is unconsumed: what a caller does before it starts a
 * new batch of lines if its previous loop may have ended early. Enqueue only. */
int surya_rec_encode_ahead(surya_rec* h, const float* tiles, const int32_t* grid_hw, int n_images, void* stream);

/* Set the list of slots that take part in decode steps (host bookkeeping of batch_prompt_mapping,
 * recognition/__init__.py:125-136). */
int surya_rec_set_active(surya_rec* h, const int32_t* slots, int n_active, void* stream);

/* Run `n_steps` greedy decode steps for the active slots without host round trips (replaces
 * RecognitionPredictor.decode + process_outputs, recognition/__init__.py:294-352). Step s writes
 * outputs(step s). n_steps <= SA_MAX_STEPS. Enqueue only. */
#define SA_MAX_STEPS 16
int surya_rec_decode(surya_rec* h, int n_steps, void* stream);

/* Sync the stream and copy the outputs of steps [0, n_steps) to host arrays indexed [step][slot]:
 *   tokens int32 [n_steps*max_slots], scores fp32 [n_steps*max_slots], bboxes int32 [n_steps*max_slots*6]. */
int surya_rec_read_outputs(surya_rec* h, int n_steps, int32_t* tokens, float* scores, int32_t* bboxes, void* stream);

/* Pipelined pair (the reference blocks on .cpu() after every step, recognition/__init__.py:545-576; here the host may run
 * one call behind the device): decode_async = surya_rec_decode with its outputs in ring half `ring` (0 or 1,
 * n_steps <= SA_MAX_STEPS / 2) plus an async copy of that half to pinned host memory and an event; wait_outputs blocks on
 * that event only (NOT on the stream, so a later decode_async may already be queued) and returns the arrays laid out
 * like read_outputs. A slot whose line finished inside call n still steps through call n + 1; its KV length is clamped
 * to max_kv_len - 1 on the device and the caller ignores its outputs. (How every read_* / wait_* pair below shares one mirror
 * layout: DESIGN.md 4m.) */
int surya_rec_decode_async(surya_rec* h, int n_steps, int ring, void* stream);
int surya_rec_wait_outputs(surya_rec* h, int n_steps, int ring, int32_t* tokens, float* scores, int32_t* bboxes);

/* Line-crop pre-processing on the device: page pixels -> image_tiles for n_lines lines in one call.
 * Replaces, per line, slice_bboxes_from_image / slice_and_pad_poly (surya/input/processing.py:35-101), scale_to_fit
 * (surya/common/surya/processor/__init__.py:141-178, LANCZOS4) and _process_and_tile (:185-230: CUBIC round-up to multiples of
 * patch * merge, x / 255 in fp64, (x - mean) / std in fp32, merge-block-major patch rows).
 * pages: device uint8, every page HWC at its descriptor's byte offset, `pixel_stride` bytes per pixel: 3 (RGB) or 4 (RGBX, the
 * layout PIL keeps in memory -- the host then uploads page memory as is instead of repacking it, ~2 ms per 1024^2 page). lines: device array of n_lines descriptors
 *   { int64 page_off; int32 page_w, page_h; int32 x0, y0, cw, ch (crop rectangle, inside the page, >= 1 px);
 *     int32 has_poly; float poly[8] (4 vertices relative to the crop origin; pixels outside read as pad_value);
 *     int32 mid_w, mid_h (size after scale_to_fit); int32 out_w, out_h (multiples of patch * merge);
 *     int64 mask_off (bytes into mask_arena, cw * ch per polygon line); int64 mid_off (floats into mid_arena, 3 mid_w mid_h per
 *     line whose mid size differs from its crop size); int64 tile_row (first row of the line in tiles) }   -- 112 bytes, C layout.
 * tiles: device fp32 [sum (out_h / patch) (out_w / patch)][3 patch^2]. The host computes only these integers
 * (surya_amd/recognition/preprocess_gpu.py). any_poly: some line has a polygon; max_stage1_width: largest mid_w among the lines whose
 * mid size differs from their crop size (0 = no line needs the Lanczos stage). Enqueue only; every buffer is caller-owned. */
int surya_rec_preprocess(const uint8_t* pages, const void* lines, int n_lines, uint8_t* mask_arena, float* mid_arena, float* tiles,
                         int patch_size, int merge_size, float pad_value, const float* mean, const float* std, int any_poly,
                         int max_stage1_width, int pixel_stride, void* stream);

/* Rectification of rotated line quadrilaterals (RecognitionPredictor.rectify): n quads of the pages -> upright uint8 crops, each the
 * rule of warp_quad (surya_amd/common/imageops.py): output pixel (u, v) samples its page at the image of (u + 0.5, v + 0.5) under
 * the line's homography, minus 0.5 per axis, with 4 x 4 cubic taps (a = -0.75) around floor() of that point, replicate border,
 * float64 sums in tap order (horizontal pass first), rint, clamp to 0..255; uint8-equal to the host function. A crop is written
 * like a page (HWC, `pixel_stride` bytes per pixel, X = 0 with 4), so surya_rec_preprocess reads it through a descriptor whose
 * page is the crop: page_off = its offset, page_w / page_h = cw / ch = its size, x0 = y0 = 0, has_poly = 0.
 * pages, out: device; `out` may lie in the pages' allocation, in a disjoint range. descs: HOST array of n descriptors
 *   { int64 page_off; int32 page_w, page_h; int32 out_w, out_h; int64 out_off (bytes into out);
 *     double h[9] (row-major, h[8] = 1: crop corners (0,0), (out_w,0), (out_w,out_h), (0,out_h) -> the quad's p0..p3, grid-line
 *     coordinates: pixel i covers [i, i + 1)) }                                                          -- 104 bytes, C layout;
 * they are copied into the launches' kernel arguments, so the array may be reused as soon as the call returns. max_w, max_h: the
 * largest out_w / out_h of the call (grid sizing). SA_ERR_ARG, with nothing launched, when pixel_stride is not 3 or 4, a size is
 * non-positive or exceeds max_w / max_h, or (pixel_stride 4) a page_off or out_off is not a multiple of 4; n == 0 launches nothing.
 * What a descriptor addresses is not checked against the buffers: the caller keeps offsets and sizes inside them. Enqueue only. */
int surya_rec_rectify(const uint8_t* pages, const void* descs, int n, uint8_t* out, int pixel_stride, int max_w, int max_h, void* stream);

/* Unrolling of bent text lines along their centre lines (RecognitionPredictor.unroll): n bands of the pages -> upright uint8 crops,
 * each the rule of warp_columns (surya_amd/common/imageops.py): output column u has a centre C(u) = (Cx, Cy) on the centre line and a
 * unit normal N(u) = (Nx, Ny), made by curve_table on the host (arc-length parametrised, float64); output pixel (u, v) samples its page
 * at C(u) + (v + 0.5 - out_h / 2) N(u) - 0.5 per axis and from there on as surya_rec_rectify does: 4 x 4 cubic taps (a = -0.75) around
 * floor() of that point, replicate border, float64 sums in tap order (horizontal pass first), rint, clamp to 0..255; uint8-equal to
 * the host function. A crop is written like a page (HWC, `pixel_stride` bytes per pixel, X = 0 with 4), so surya_rec_preprocess reads it
 * as it reads a rectified crop. pages, out, tables: device; `out` may lie in the pages' allocation, in a disjoint range; tables: doubles,
 * 16-byte aligned. descs: HOST array of n descriptors
 *   { int64 page_off; int32 page_w, page_h; int32 out_w, out_h; int64 out_off (bytes into out);
 *     int64 table_off (doubles into tables, even: the crop's [out_w][4] = Cx, Cy, Nx, Ny per column) }    -- 40 bytes, C layout;
 * they are copied into the launches' kernel arguments, so the array may be reused as soon as the call returns. max_w, max_h: the
 * largest out_w / out_h of the call (grid sizing). SA_ERR_ARG, with nothing launched, when pixel_stride is not 3 or 4, n is negative, a
 * pointer (pages, descs, tables, out) is null, tables is not 16-byte aligned, a size is non-positive or exceeds max_w / max_h, an offset
 * is negative, a table_off is odd, or (pixel_stride 4) a page_off or out_off is not a multiple of 4; n == 0 launches nothing. What a
 * descriptor addresses is not checked against the buffers: the caller keeps offsets and sizes inside them. Enqueue only. */
int surya_rec_unroll(const uint8_t* pages, const void* descs, int n, const double* tables, uint8_t* out, int pixel_stride, int max_w,
                     int max_h, void* stream);

/* Flattening of curled pages through a warp mesh (surya_amd.detection.dewarp): n pages -> uint8 outputs of the pages' own sizes, each the
 * rule of warp_mesh (surya_amd/common/imageops.py): the mesh of a w x h page with cell size `cell` is float64 [gh + 1][gw + 1][2],
 * gw = ceil(w / cell), gh = ceil(h / cell), entry (j, i) the displacement (dx, dy) at output point (i * cell, j * cell), grid-line
 * coordinates; output pixel (u, v) lies in cell (u / cell, v / cell), takes the bilinear form of the cell's four nodes at
 * ((u + 0.5 - i * cell) / cell, (v + 0.5 - j * cell) / cell) -- top and bottom edge along x first, then along y, float64, no contraction --
 * and samples its page at (u + 0.5 + dx) - 0.5, (v + 0.5 + dy) - 0.5 and from there on as surya_rec_rectify does: 4 x 4 cubic taps
 * (a = -0.75) around floor() of that point, replicate border, float64 sums in tap order (horizontal pass first), rint, clamp to 0..255;
 * uint8-equal to the host function. An output is written like a page (HWC, `pixel_stride` bytes per pixel, X = 0 with 4). pages, out,
 * meshes: device; `out` may lie in the pages' allocation, in a disjoint range; meshes: doubles, 16-byte aligned. descs: HOST array of n
 * descriptors
 *   { int64 page_off; int32 w, h; int32 cell, reserved (0); int64 out_off (bytes into out);
 *     int64 mesh_off (doubles into meshes, even: the page's [gh + 1][gw + 1][2]) }                        -- 40 bytes, C layout;
 * they are copied into the launches' kernel arguments, so the array may be reused as soon as the call returns. max_w, max_h: the
 * largest w / h of the call (grid sizing). SA_ERR_ARG, with nothing launched, when pixel_stride is not 3 or 4, n is negative, a pointer
 * (pages, descs, meshes, out) is null, meshes is not 16-byte aligned, a size is non-positive or exceeds max_w / max_h, cell is not a
 * multiple of 16 in 16 .. 1024, reserved is not 0, an offset is negative, a mesh_off is odd, (pixel_stride 4) pages, out, a page_off or
 * an out_off is not a multiple of 4, or max_h needs more than 65535 tiles; n == 0 launches nothing. The VALUES of a mesh are not checked
 * (check_mesh does that on the host): whatever they are, every read stays inside the page. What a descriptor addresses is not checked
 * against the buffers: the caller keeps offsets and sizes inside them. Enqueue only. */
int surya_warp_mesh(const uint8_t* pages, const void* descs, int n, const double* meshes, uint8_t* out, int pixel_stride, int max_w,
                    int max_h, void* stream);

/* Contrast adjustment of line crops (RecognitionPredictor.reread, LineRef.adjust): n crops of the pages -> their adjusted, padded
 * copies, each Pillow's ImageOps.autocontrast(crop, cutoff, preserve_tone=True, mask), byte for byte: 256 bins of the luma
 * (19595 R + 38470 G + 7471 B + 32768) >> 16 over the crop (has_poly: over the pixels of the 4-point polygon's mask, rasterised as
 * surya_rec_preprocess rasterises it), cutoff percent of the counts removed from the low end, then from the high end of what is
 * left, lo / hi the first / last bin left, lut[i] = clamp(int(i * (255.0 / (hi - lo)) + (-lo * scale))) in float64 (the identity when
 * hi <= lo), applied to the three channels of every pixel, the pixels outside the polygon being 255 before the LUT. A crop is
 * written like a page (HWC, `pixel_stride` bytes per pixel, X = 0 with 4), so surya_rec_preprocess reads it through a descriptor
 * whose page is the crop: page_off = its offset, page_w / page_h = cw / ch = its size, x0 = y0 = 0, has_poly = 0. The source may be
 * a crop surya_rec_rectify wrote earlier on the same stream.
 * pages, out, mask_arena, work, lo_hi: device; `out` may lie in the pages' allocation. descs: HOST array of n descriptors
 *   { int64 src_off (byte offset of the source page in `pages`); int32 src_w, src_h, x0, y0, w, h (the crop inside it), cutoff (0..49),
 *     has_poly; float poly[8] (relative to the crop origin); int64 out_off (byte offset of the copy in `out`), mask_off (byte offset
 *     of the line's w * h mask bytes in mask_arena, read with has_poly only) }                                 -- 88 bytes, C layout;
 * they are copied into the launches' kernel arguments, so the array may be reused as soon as the call returns. work: n * 1280 bytes,
 * 4-byte aligned (the histograms, then the LUTs); lo_hi: int32 [n][2], the bounds of every line. SA_ERR_ARG, with nothing launched
 * or written, when pixel_stride is not 3 or 4; a size is non-positive, a crop leaves its source or holds more than 2^28 pixels; a
 * cutoff is outside 0..49; has_poly is neither 0 nor 1, or 1 without a mask_arena; an offset is negative or (pixel_stride 4) not a
 * multiple of 4; two output ranges overlap, an output range overlaps the source page of any descriptor, or two mask ranges overlap;
 * work or lo_hi is null. n == 0 launches nothing. What a descriptor addresses is not checked against the buffers' ends: the caller
 * keeps offsets and sizes inside them. Enqueue only. */
int surya_rec_adjust_contrast(const uint8_t* pages, const void* descs, int n, uint8_t* out, uint8_t* mask_arena, void* work, int32_t* lo_hi,
                              int pixel_stride, void* stream);

/* Test hooks (tolerance tests of intermediate tensors):
 *   encode_only: run the vision encoder + 2-D position embedding, write [P/merge^2, dec_hidden] features in
 *                ORIGINAL token order (= get_image_embeddings, common/surya/__init__.py:130-195) to `out`
 *                (device, compute dtype).
 *   copy_last_logits: fp32 logits [rows, vocab] of the last prefill / decode step into `dst` (device, capacity
 *                max_rows rows); row r = r-th sequence of the prefill / r-th active slot. The product path keeps logits
 *                in LDS (greedy reduction in the lm_head epilogue), so this recomputes them on `stream` from the
 *                final-norm rows of that step. */
int surya_rec_encode_only(surya_rec* h, const float* tiles, const int32_t* grid_hw, int n_images, void* out, void* stream);
int surya_rec_copy_last_logits(surya_rec* h, float* dst, int max_rows, int* rows, void* stream);
/* Force the token fed to the next decode step (teacher forcing in parity tests). */
int surya_rec_set_next_tokens(surya_rec* h, const int32_t* slots, const int32_t* tokens, int n, void* stream);

/* MXFP8 weights for the decode steps (BASELINE.json configs[4]: the fp8 MFMA weight path of the texify configuration; the
 * reference has no fp8 mode -- its decode loop, surya/recognition/__init__.py:473-607, runs the checkpoint dtype). bf16
 * models only. Each projection is given as OCP e4m3 bytes in the SAME kernel layout as its bf16 weight (qkv fused, gate|up
 * row-interleaved, [out][in]) plus one E8M0 scale byte per 32 consecutive input features, stored K-TILE-MAJOR:
 * [in / 128][out][4] bytes (the 4 block scales of a row inside one 128-wide K-tile are one dword, and the dwords of
 * consecutive rows are contiguous -- what the GEMM's scale fetch reads in one piece). After this call
 * surya_rec_decode / _decode_async multiply MXFP8 activations (quantised inside the producing kernels) by these weights with
 * v_mfma_scale_f32_32x32x64_f8f6f4; prefill keeps the bf16 weights. table == NULL returns to the bf16 decode path.
 * The caller keeps the tensors alive. Needs dec_hidden, heads * head_dim and intermediate sizes that are multiples of 128.
 * Holds at every slot count: above 256 active rows only the GEMM tiles grow (csrc/gemm_mx.h; tuning mx_big_m_split / mx_big_m_gateup),
 * the split-K slice counts and the K order stay, so a line's tokens, scores and boxes do not depend on the number of active slots. */
enum { SA_MX_QKV_W = 0, SA_MX_QKV_S, SA_MX_O_W, SA_MX_O_S, SA_MX_GU_W, SA_MX_GU_S, SA_MX_DOWN_W, SA_MX_DOWN_S, SA_MX_COUNT };
enum { SA_MX_LM_W = 0, SA_MX_LM_S, SA_MX_GLOBALS };      /* after the per-layer entries */
#define SA_MX_TOTAL(dec_layers) ((dec_layers) * SA_MX_COUNT + SA_MX_GLOBALS)
int surya_rec_set_mx_weights(surya_rec* h, const void* const* table, int n);

/* FP8 (OCP e4m3) KV cache for the decode steps -- the second half of configs[4]'s fp8 path: at the texify horizon (KV 202 -> 970)
 * the decode-attention kernel is the largest of the step and moves its rows at HBM speed, so the lever is the bytes. Format "KV8":
 * per (slot, kv head, token) one power-of-two scale (the smallest with absmax / scale <= 448) + round-to-nearest-even e4m3
 * elements; K rows [slot][kv_head][max_kv_len][head_dim] bytes, V transposed per 128-token tile [slot][kv_head][T8 / 128][head_dim][128] bytes, scales fp32
 * [slot][kv_head][T8], T8 = max_kv_len rounded up to 256; the arrays live inside the handle. Prefill still attends over the bf16
 * cache and quantises the prompt's rows; decode steps read and append fp8 only (decode_attn_kv8.h). bf16 models, head_dim in
 * {32, 64, 128}. No reference counterpart (surya/recognition/__init__.py:379-395 offers HQQ 8-bit only): the format is pinned by
 * oracle/mx_oracle.py::kv8_quantize and tests/test_gpu_kv8.py. Call while no line is in flight. */
int surya_rec_set_kv_fp8(surya_rec* h, int on);

/* Constrained output: restrict the tokens of a line to an allowed set (a character whitelist / blacklist; surya_amd/recognition/
 * tokenizer.py::token_mask builds the sets). The reference has no such switch -- a caller patches process_outputs and masks
 * next_token_logits -- and here logits never exist outside a tile (the lm_head epilogues reduce each tile to one partial), so the
 * mask is applied inside those epilogues, before the max and the sum-exp pass: token = first argmax over the allowed ids, score =
 * softmax over the allowed ids, i.e. what process_outputs gives on next_token_logits.masked_fill(~allowed, -inf). The first token of a
 * line (the prefill's head pass) is constrained like every later one. The fused next-step embedding and the bbox head are untouched.
 *   set_token_masks: `masks` = host array [n_masks][ceil(vocab / 32)] of uint32, bit (c & 31) of word (c >> 5) set = id c allowed; it is
 *                copied into handle-owned device memory whose address never changes (captured decode steps stay valid while only the
 *                contents change), in stream order. Every mask needs an allowed id below vocab and n_masks <= SA_MAX_TOKEN_MASKS, else
 *                SA_ERR_ARG (nothing changes). n_masks == 0 switches back to the unmasked kernels: a handle that never saw a mask, or
 *                saw 0 last, launches exactly what it launched before this entry existed. Switching between the two drops captured
 *                decode steps, as surya_rec_set_kv_fp8 does. A new table sets every slot back to -1.
 *   set_slot_masks: mask id (row of the table, or -1 = unconstrained) of `n` slots; call it for the slots about to be prefilled. A slot
 *                keeps its id until it is set again or the table is replaced. SA_ERR_STATE without a table; a slot named twice, a slot
 *                or an id out of range: SA_ERR_ARG.
 * surya_rec_copy_last_logits keeps returning the UNMASKED logits (the mask lives in the greedy epilogues only): a test recomputes the
 * masked token and score from them. Call both while no line that they concern is in flight. */
#define SA_MAX_TOKEN_MASKS 64
int surya_rec_set_token_masks(surya_rec* h, const uint32_t* masks, int n_masks, void* stream);
int surya_rec_set_slot_masks(surya_rec* h, const int32_t* slots, const int32_t* mask_ids, int n, void* stream);

/* Alternatives: the SA_MAX_ALTERNATIVES most likely tokens of every step with their probabilities, i.e. what a caller of the reference gets
 * from a stable descending sort of softmax(next_token_logits) inside process_outputs (ties: lower id first). Logits never exist outside a
 * tile here, and a greedy partial keeps only its tile's winner, so the candidates are collected where the partials are: the lm_head's *_TOPK
 * epilogues write each tile's four best allowed columns beside its partial, and a small kernel behind the greedy head picks the row's four
 * best and divides by the head's own max and total (entry 0 is the emitted token, and its probability has the bits of the emitted score on
 * rows that go on; a row that chose eos / pad keeps score 0 and still reports its alternatives). With token masks set the alternatives
 * are the best ALLOWED tokens and the probabilities are over the allowed set. Tokens, scores, boxes and the next step's input do not change.
 *   set_alternatives: on = 0 / 1, anything else SA_ERR_ARG. The first switch-on allocates the candidate and output arrays (and their pinned
 *                mirror); a handle that never switches it on allocates nothing and launches exactly what it launched before this entry
 *                existed. Addresses never change afterwards. Switching drops captured decode steps, as surya_rec_set_token_masks does.
 *                Call while no line is in flight.
 *   read_alternatives / wait_alternatives: tokens [n_steps][max_slots][SA_MAX_ALTERNATIVES] int32 (-1 where fewer ids are allowed) and probs
 *                (0 there) of the steps surya_rec_read_outputs / surya_rec_wait_outputs return, same indexing, best first;
 *                surya_rec_decode_async mirrors the ring half behind the same event. SA_ERR_STATE while the feature is off, and from
 *                wait_alternatives for a ring half whose decode_async ran while it was off. */
#define SA_MAX_ALTERNATIVES 4
int surya_rec_set_alternatives(surya_rec* h, int on);
int surya_rec_read_alternatives(surya_rec* h, int n_steps, int32_t* tokens, float* probs, void* stream);
int surya_rec_wait_alternatives(surya_rec* h, int n_steps, int ring, int32_t* tokens, float* probs);

/* Forced decoding: align a known transcription. Given a line and its token ids, every step emits the forced id instead of the greedy one and
 * reports how likely the model found it -- what a caller of the reference gets from teacher-forcing input_ids and reading
 * log_softmax(next_token_logits)[forced]. Logits never exist outside a tile here and the next step's input is chosen on the device, so the
 * lm_head's *_FORCED epilogues pick the forced column's logit up where the partials are, and the greedy head feeds the forced id on.
 * A slot's ids are consumed one per head pass (the prefill's included: the first token of a line is forced too); a slot past the end of its
 * ids, or with none, free-runs with the bits of a handle that never switched the feature on. Under forcing token = the forced id,
 * score = p(id | image, preceding ids) (0 for eos / pad, as ever), and the box is the one predicted from the forced prefix.
 *   set_forced:  on = 0 / 1, anything else SA_ERR_ARG. The first switch-on allocates the id table [max_slots][SA_MAX_FORCED_TOKENS] (-1), the
 *                cursors and the outputs with their pinned mirror; a handle that never switches it on allocates nothing and launches exactly
 *                what it launched before this entry existed. Addresses never change afterwards. Switching drops captured decode steps;
 *                switch-off sets the table back to -1. SA_ERR_STATE while token masks or alternatives are on, and surya_rec_set_token_masks
 *                (n_masks > 0) / surya_rec_set_alternatives(1) return SA_ERR_STATE while forcing is on. Call while no line is in flight.
 *   set_forced_tokens: slot slots[i] gets tokens[offsets[i] .. offsets[i + 1]) (HOST arrays, offsets [n + 1]), -1 behind them, cursor 0; call
 *                it for the slots about to be prefilled, like surya_rec_set_slot_masks. Length 0: the slot free-runs. SA_ERR_STATE while
 *                off; SA_ERR_ARG, with nothing changed, for a slot named twice or out of range, an id outside [0, vocab) or a length above
 *                SA_MAX_FORCED_TOKENS.
 *   read_forced / wait_forced: [n_steps][max_slots] greedy_tokens (the model's own argmax), greedy_probs (its probability, 1 / total) and
 *                forced_logprobs (log p of the emitted token: the forced id, or the greedy one on a free-running slot) of the steps
 *                surya_rec_read_outputs / surya_rec_wait_outputs return, same indexing; surya_rec_decode_async mirrors the ring half
 *                behind the same event. SA_ERR_STATE while off, and from wait_forced for a ring half whose decode_async ran while off. */
#define SA_MAX_FORCED_TOKENS 1024
int surya_rec_set_forced(surya_rec* h, int on);
int surya_rec_set_forced_tokens(surya_rec* h, const int32_t* slots, const int32_t* tokens, const int32_t* offsets, int n, void* stream);
int surya_rec_read_forced(surya_rec* h, int n_steps, int32_t* greedy_tokens, float* greedy_probs, float* forced_logprobs, void* stream);
int surya_rec_wait_forced(surya_rec* h, int n_steps, int ring, int32_t* greedy_tokens, float* greedy_probs, float* forced_logprobs);

/* Beam search: the `width` best readings of a line instead of the greedy one -- what a caller of a seq2seq OCR engine gets from num_beams.
 * The reference cannot do it without replacing its cache; here a line owns `width` consecutive slots (a group, lead slot g * width), the
 * candidates of a beam are the SA_MAX_ALTERNATIVES tokens the *_TOPK epilogues already report (the best `width` of width x 4 candidates is
 * exact beam search for width <= 4), a small kernel behind topk_combine_kernel selects and places the survivors, and a copy kernel forks the
 * KV rows of a beam that continues twice. The rules are stated once, in csrc/beam_core.h: score = sum of log p(token | image, prefix), eos
 * included, no length normalisation, log p = float(log(double(p))), fp32 sums; a finished beam (eos, pad; at the first token also the
 * no-output id) stays in the set as one frozen candidate and keeps stepping on pad; order = score descending, parent slot ascending, rank
 * ascending; a parent's best child stays in the parent's slot, further children go to the slots of beams that did not survive, so a step
 * in which every beam continues once copies nothing; fewer candidates than slots leave empty beams (parent -1, score -inf). The line is
 * prefilled once, into the lead slot; the first selection takes the best `width` first tokens of that slot and forks the prompt's rows.
 * Per step the engine launches head -> combine -> select -> fork -> embed (the head does not fuse the next embedding: it depends on the
 * selection), three launches more than greedy; nothing in it needs the host, so surya_rec_decode(n) and surya_rec_decode_async keep working.
 *   set_beam:    width 0 = off, 2..SA_MAX_BEAMS = on, anything else SA_ERR_ARG; no_output_token_id: the tokenizer's id that ends a line at its
 *                first token (-1: none). The first switch-on allocates the beam arrays, their pinned mirror and the alternatives arena if
 *                it is absent; a handle that never switches it on allocates nothing and launches exactly what it launched before this entry
 *                existed. Switching drops captured decode steps. SA_ERR_STATE while forcing, the FP8 KV cache or MXFP8 weights are on, and
 *                surya_rec_set_forced(1) / surya_rec_set_kv_fp8(1) / surya_rec_set_mx_weights(non-NULL) return SA_ERR_STATE while beam
 *                search is on (the fork copies the bf16 / fp16 / fp32 caches only). Token masks are allowed: the candidates are then the
 *                allowed tokens; set a line's mask id on every slot of its group. surya_rec_set_alternatives stays independent, and
 *                surya_rec_read_alternatives / wait_alternatives also work while beam search is on (the alternatives of the beam that sat in
 *                the slot BEFORE the step's selection). Call while no line is in flight.
 *   while on:    surya_rec_prefill takes lead slots only (slot % width == 0 and slot + width <= max_slots, else SA_ERR_ARG), and
 *                surya_rec_set_active whole groups only, ascending (else SA_ERR_ARG). tokens / scores of surya_rec_read_outputs are each
 *                slot's own greedy choice and mean nothing; the box of a beam at a step is bboxes[step][its parent's slot].
 *   read_beam / wait_beam: [n_steps][max_slots] tokens (pad for a frozen or empty beam), parents (slot index inside the group the beam came
 *                from: its own index when it stayed in place, -1 = empty), ranks (which alternative of the parent), probs (the token's
 *                probability, 0 for a frozen or empty beam) and logps (cumulative score, -inf = empty) of the steps
 *                surya_rec_read_outputs / surya_rec_wait_outputs return, same indexing; surya_rec_decode_async mirrors the ring half behind
 *                the same event. SA_ERR_STATE while off, and from wait_beam for a ring half whose decode_async ran while off. */
#define SA_MAX_BEAMS 4
int surya_rec_set_beam(surya_rec* h, int width, int no_output_token_id);
int surya_rec_read_beam(surya_rec* h, int n_steps, int32_t* tokens, int32_t* parents, int32_t* ranks, float* probs, float* logps, void* stream);
int surya_rec_wait_beam(surya_rec* h, int n_steps, int ring, int32_t* tokens, int32_t* parents, int32_t* ranks, float* probs, float* logps);

/* Pattern-guided decoding: constrain a line to a regular expression (a date, an amount, an IBAN ...), i.e. an allowed set that depends on
 * what the line has emitted so far. A token mask is one set per line; here the slot's mask id MOVES: it follows a deterministic finite
 * automaton over the emitted tokens (surya_amd/recognition/pattern.py compiles the tables), and the greedy head, which picks each token,
 * takes the transition on the device -- behind the token, slot_state[slot] = next_state[state][tok_class[token]] and the slot's mask id =
 * state_mask[new state]. The next step's masked lm_head then reads the new state's row with no host round trip; a row that emitted eos /
 * pad keeps its state. The lm_head epilogues do not change, and captured decode steps stay valid (the addresses never change).
 *   set_patterns: HOST arrays tok_class [vocab] uint8 (class of each token id, < n_classes), next_state [n_states][n_classes] uint16
 *                (< n_states) and state_mask [n_states] uint8 (row of the CURRENT token-mask table), copied in stream order into
 *                handle-owned memory allocated on the first call at addresses that never change afterwards; every slot's state is set to
 *                -1 (no pattern). n_states == 0 switches the feature off: a handle that never saw a pattern, or saw 0 last, launches
 *                exactly what it launched before this entry existed. SA_ERR_ARG, with nothing changed, for n_states >
 *                SA_MAX_PATTERN_STATES, n_classes outside 1..SA_MAX_PATTERN_CLASSES or an entry out of range; SA_ERR_STATE without a
 *                token-mask table, and while forced decoding or beam search is on (surya_rec_set_forced(1) / surya_rec_set_beam(width)
 *                return SA_ERR_STATE while patterns are on). Switching on or off drops captured decode steps; new contents keep them.
 *                surya_rec_set_token_masks switches patterns off (the state -> row map names rows of the old table).
 *   set_slot_patterns: start state (or -1 = no pattern: the slot's mask id is left alone) of `n` slots; call it for the slots about to be
 *                prefilled, after surya_rec_set_slot_masks, which sets the states of the slots it names back to -1. A state >= 0 also
 *                sets the slot's mask id to state_mask[state]. SA_ERR_STATE while off; a slot named twice, a slot or a state out of range:
 *                SA_ERR_ARG.
 *   copy_slot_states: the states of all max_slots slots into `dst` (device, int32 [max_slots]), for tests. SA_ERR_STATE before the first
 *                set_patterns. */
#define SA_MAX_PATTERN_STATES 4096
#define SA_MAX_PATTERN_CLASSES 256
int surya_rec_set_patterns(surya_rec* h, const uint8_t* tok_class, const uint16_t* next_state, const uint8_t* state_mask, int n_states,
                           int n_classes, void* stream);
int surya_rec_set_slot_patterns(surya_rec* h, const int32_t* slots, const int32_t* start_states, int n, void* stream);
int surya_rec_copy_slot_states(surya_rec* h, int32_t* dst, void* stream);

/* Lexicon-guided decoding: read a line as exactly one entry of a word list (a city, a surname, a product code). A word list has about as
 * many distinct allowed sets as it has inner trie nodes, far beyond the SA_MAX_TOKEN_MASKS rows that patterns share with the allowlists,
 * so the automaton is sparse (CSR; surya_amd/recognition/lexicon.py compiles a minimised acyclic one for all lexicons of a call) and
 * every slot owns a mask-table row of its own, id SA_MAX_TOKEN_MASKS + slot, which a small kernel rewrites on the device behind each
 * token (csrc/lexicon.h): clear the old state's bits, set the new state's. The masked lm_head epilogues read that row like a static
 * one and do not change; logits are the same bits. A row that emitted eos / pad keeps its state and row.
 *   set_lexicon: HOST arrays edge_off [n_states + 1] (edges of state s: edge_off[s] .. edge_off[s + 1]), edge_tok [n_edges] (token ids,
 *                strictly ascending inside a state), edge_next [n_edges] (target states) and state_flags [n_states] (bit 0: terminal,
 *                eos and pad allowed; bit 1: no_output_token_id allowed), copied in stream order into handle-owned memory sized by need;
 *                every slot's lexicon state is set to -1. Everything is validated first -- offsets from 0 to n_edges and monotone,
 *                tokens inside [0, vocab) and ascending, targets < n_states, flags < 4, an allowed id in every state, no_output_token_id
 *                inside the vocabulary where a state names it, counts within SA_MAX_LEXICON_STATES / SA_MAX_LEXICON_EDGES: SA_ERR_ARG
 *                with nothing changed otherwise. SA_ERR_STATE without a token-mask table, and while forced decoding or beam search is
 *                on (their setters return SA_ERR_STATE while a lexicon is on). n_states == 0 switches the feature off: a handle that
 *                never saw a lexicon, or saw 0 last, launches exactly what it launched before this entry existed. Switching on or off,
 *                or growing the tables' memory, drops captured decode steps; new contents of the same capacity keep them. The first
 *                call also gives the mask table its max_slots dynamic rows (max_slots * cdiv(vocab, 32) * 4 bytes). It may be on
 *                together with patterns; a slot follows at most one of the two. surya_rec_set_token_masks switches it off.
 *                At the limits the tables take 21 MB on the device and as much pinned host memory (4 + 1 bytes per state, 8 per edge).
 *   set_slot_lexicon: start state (or -1 = no lexicon: the slot's mask id and row are left alone) of `n` slots; call it for the slots
 *                about to be prefilled, after surya_rec_set_slot_masks, which sets the lexicon state of the slots it names back to -1.
 *                A state >= 0 zeroes the slot's row, sets the state's bits and makes the row the slot's mask id. SA_ERR_STATE while
 *                off; a slot named twice, a slot or a state out of range: SA_ERR_ARG.
 *   copy_lexicon_states: the states of all max_slots slots into `dst` (device, int32 [max_slots]), for tests. SA_ERR_STATE before the
 *                first set_lexicon. */
#define SA_MAX_LEXICON_STATES (1 << 20)
#define SA_MAX_LEXICON_EDGES (1 << 21)
int surya_rec_set_lexicon(surya_rec* h, const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next, const uint8_t* state_flags,
                          int n_states, int n_edges, int no_output_token_id, void* stream);
int surya_rec_set_slot_lexicon(surya_rec* h, const int32_t* slots, const int32_t* start_states, int n, void* stream);
int surya_rec_copy_lexicon_states(surya_rec* h, int32_t* dst, void* stream);

/* Boosted decoding: prefer the words of a user list without forbidding anything else ("hot words"). A boosted slot follows a sparse
 * automaton of the lexicon's CSR form (surya_amd/recognition/boost.py compiles it) and owns the mask-table row a lexicon slot would, but
 * the row is the PREFERRED set S of the position: per step the lm_head runs its masked greedy epilogue (record A, over S) and its plain
 * one (record B, over every column, into a second partial buffer), and boost_head_kernel decodes from v' = v + beta * [in S] by the exact
 * rules of csrc/boost_core.h: token = first maximum of v', score = its softmax probability under v'. No GEMM kernel changes. The
 * automaton is total: a token without an edge goes to out_state (a state without edges) if it is a word unit -- bit set in row
 * word_row of the mask table -- and to the slot's root otherwise (csrc/boost.h). eos / pad keep state and row.
 *   set_boost:   HOST arrays as surya_rec_set_lexicon's (edge_off [n_states + 1], edge_tok [n_edges] strictly ascending inside a state,
 *                edge_next [n_edges]), all validated first -- offsets from 0 to n_edges and monotone, tokens inside [0, vocab), not eos
 *                or pad, ascending, targets < n_states, out_state a state without edges, word_row a row of the mask table, counts
 *                within SA_MAX_LEXICON_STATES / SA_MAX_LEXICON_EDGES: SA_ERR_ARG with nothing changed otherwise. SA_ERR_STATE without a
 *                token-mask table, while alternatives, beam search, forced decoding, patterns or a lexicon are on (their setters
 *                return SA_ERR_STATE while boosting is on), and where the greedy head on partials cannot run (tuning ghead != 2, hidden
 *                size > 2048). n_states == 0 switches the feature off: a handle that never saw a boost table, or saw 0 last, launches
 *                exactly what it launched before this entry existed. Switching on or off, or growing the tables' memory, drops captured
 *                decode steps; new contents of the same capacity keep them. Every slot is set to "not boosted". The first call
 *                allocates the dynamic mask rows (as set_lexicon's first call), the second partial buffer and the outputs below.
 *                surya_rec_set_token_masks switches it off. Static masks on other slots, MXFP8 weights and the fp8 KV cache are fine.
 *   set_slot_boost: root state (-1 = not boosted: beta +inf, state -1, mask id and row left alone) and beta (finite, >= 0, logit
 *                units) of `n` slots; call it for the slots about to be prefilled, after surya_rec_set_slot_masks, which sets the
 *                slots it names back to "not boosted". SA_ERR_STATE while off; a slot named twice, a slot, root or beta out of range:
 *                SA_ERR_ARG.
 *   copy_boost_states: the states of all max_slots slots into `dst` (device, int32 [max_slots]), for tests.
 *   read_boost / wait_boost: per step and slot, like surya_rec_read_outputs / surya_rec_wait_outputs: plain_tokens = the token the
 *                model would have emitted here without the boost (record B's index), plain_probs = the emitted token's probability
 *                without the boost. SA_ERR_STATE while off. */
int surya_rec_set_boost(surya_rec* h, const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next, int n_states, int n_edges,
                        int out_state, int word_row, void* stream);
int surya_rec_set_slot_boost(surya_rec* h, const int32_t* slots, const int32_t* roots, const float* betas, int n, void* stream);
int surya_rec_copy_boost_states(surya_rec* h, int32_t* dst, void* stream);
int surya_rec_read_boost(surya_rec* h, int n_steps, int32_t* plain_tokens, float* plain_probs, void* stream);
int surya_rec_wait_boost(surya_rec* h, int n_steps, int ring, int32_t* plain_tokens, float* plain_probs);

/* ------------------------------------------------------------------------------------------------------------
 * Op-level entry points (unit tests of the kernels through the same library; row-major, compute dtype).
 * ---------------------------------------------------------------------------------------------------------- */
/* Operands of every GEMM entry point below (surya_op_gemm, _rope, _splitk_*, surya_op_rec_gemm_f16) and of every GEMM an engine launches:
 * K > 0 and a multiple of one 128-byte K-tile (64 16-bit / 32 fp32 elements); X, W, C, R and the split-K slabs start on 16-byte boundaries and
 * ldx, ldw, ldc, ldr are multiples of 16 bytes of their element type (rows move in 16-byte chunks); bias starts on a boundary of 4 of its
 * elements. Anything else is refused with SA_ERR_SHAPE before any launch.
 * C[M,N] = X[M,K] W[N,K]^T + bias, epilogue: 0 none/bias, 1 +residual R, 2 gelu, 3 swiglu (W rows interleaved,
 * C is [M,N/2]), 4 hardswish, 5 relu, 8 geglu = gelu_tanh(gate) * up with gate, up and the gelu each rounded to the compute dtype
 * (the ADETR decoder's MLP, W rows interleaved like swiglu, C is [M,N/2]; fp32 and bf16 only, no bias, no R, out_f32 == 0; fp16: surya_op_gemm_geglu_f16 below).
 * Codes 6 and 7 are epilogues of the recogniser that take further operands and are not reachable here: SA_ERR_ARG.
 * out_f32 != 0: C (and R) are fp32 regardless of dtype. dtype SA_DTYPE_F16 takes the detector's epilogues (0, 1, 4, 5) and the
 * OCR-error classifier's gelu (2: the projection rounded to fp16, erf GELU, rounded; no R) with fp16 output only; anything else returns
 * SA_ERR_UNSUPPORTED. */
int surya_op_gemm(int dtype, int out_f32, int epi, const void* X, long ldx, const void* W, long ldw, void* C, long ldc,
                  const void* bias, const void* R, long ldr, int M, int N, int K, void* stream);
/* The vision qkv projection with the rotary embedding in its epilogue (launch_gemm<T, T, EPI_ROPE>, filled as the recognition encoder fills
 * it): C[M,N] = T(X W^T + bias), then columns n < rope_cols rotated in pairs (2j, 2j + 1) of each rope_D-wide head by
 * rope[m][(n % rope_D) / 2] = (cos, sin) (fp32 [M][rope_D / 2][2]; the weight rows are pair-interleaved), fp32 math, rounded to T once more.
 * Columns >= rope_cols are the plain projection. rope_D % 4 == 0, rope_cols a multiple of rope_D, rope 16-byte aligned. dtype fp32 / bf16 / fp16. */
int surya_op_gemm_rope(int dtype, const void* X, long ldx, const void* W, long ldw, void* C, long ldc, const void* bias, const float* rope,
                       int rope_cols, int rope_D, int M, int N, int K, void* stream);
int surya_op_rmsnorm(int dtype, const void* x, long ldx, const void* w, void* y, long ldy, int rows, int C, float eps,
                     void* stream);
/* Attention kernels by themselves (tests against fp32 PyTorch SDPA; synchronous -- the call returns after the kernel ran).
 * surya_op_attn: segment attention = the vision encoder's window / whole-image attention (non-causal varlen,
 * surya/common/surya/encoder/__init__.py:238-261) and the decoder prefill's causal GQA (decoder/__init__.py:101-128).
 * dtype bf16 and fp16 run attn_mfma_kernel<T, head_dim> (both forms, causal or not), fp32 runs attn_valu_kernel (reference mode). Segment s has seg_len[s] queries
 * and keys; its first query / key / value / output row starts at element offset q_off / k_off / v_off / o_off[s] (host
 * arrays) of q / k / v / out (device), rows `*_row` elements apart, heads `*_head` elements apart; query head h reads kv
 * head h / group. head_dim in {32, 64, 80, 128}.
 * surya_op_decode_attn: one decode step's attention, through the launcher the engines use (launch_decode_attn, csrc/decode_attn.h): row r = active slot
 * active_slots[r] with row_len[r] cached tokens; q|k|v of the new token = sum of n_slabs fp32 split-K slabs
 * qkv_part[slab][rows][(heads + 2 kv_heads) * head_dim] + qkv_bias, rounded to the storage dtype; RoPE from the (cos, sin) table
 * rope_cs[max_kv_len][head_dim / 2][2]; k, v appended to the caches [slot][kv_head][max_kv_len][head_dim] at row_len[r];
 * out[r][heads * head_dim] = attention over row_len[r] + 1 keys (decoder/__init__.py:193-234). bf16 runs
 * decode_attn_flash2_kernel (tuning dattn = 4, the default) or decode_attn_flash_kernel (dattn = 3), fp32 decode_attn_mfma_kernel, fp16
 * decode_attn_flash2_kernel<.., fp16_t> at head_dim 64 / 32 with heads / kv_heads <= 8 (the layout / table decoders' shapes) and at head_dim
 * 128 with heads / kv_heads <= 5 or <= 8 (the recogniser's; fp16 has no decode_attn_flash_kernel: dattn = 3 runs the flash2 kernel too). The hook
 * has no host bound on the contexts, so of decode_attn_flash2_kernel's two forms the two-buffer one runs at dattn_db = 1 only; the engine also
 * picks it at dattn_db = 0 once a context exceeds 128 keys. All pointers device. Enqueue only. */
int surya_op_attn(int dtype, int head_dim, const void* q, const void* k, const void* v, void* out, const int32_t* seg_len,
                  const int64_t* q_off, const int64_t* k_off, const int64_t* v_off, const int64_t* o_off, int n_seg, int heads, int group,
                  int causal, float scale, long q_row, long q_head, long k_row, long k_head, long o_row, long o_head, void* stream);
int surya_op_decode_attn(int dtype, int head_dim, const float* qkv_part, int n_slabs, const void* qkv_bias, void* out, void* kcache,
                         void* vcache, const int32_t* active_slots, const int32_t* row_len, const float* rope_cs, int rows, int heads,
                         int kv_heads, int max_kv_len, float scale, void* stream);
/* The KV8 kernels by themselves (tests): surya_op_kv8_quant_rows quantises rows (tok_slot[i], tok_pos[i]) of bf16 caches
 * [slot][kv_head][max_kv_len][head_dim] into the KV8 arrays (layout above); surya_op_decode_attn_kv8 = surya_op_decode_attn on those
 * arrays (bf16 model path only), appending the new token's quantised k / v. All pointers device; enqueue only. */
int surya_op_kv8_quant_rows(int head_dim, const void* kcache, const void* vcache, const int32_t* tok_slot, const int32_t* tok_pos, int n_tokens,
                            void* k8, void* v8t, float* kscale, float* vscale, int kv_heads, int max_kv_len, void* stream);
int surya_op_decode_attn_kv8(int head_dim, const float* qkv_part, int n_slabs, const void* qkv_bias, void* out, void* k8, void* v8t,
                             float* kscale, float* vscale, const int32_t* active_slots, const int32_t* row_len, const float* rope_cs, int rows,
                             int heads, int kv_heads, int max_kv_len, float scale, void* stream);
/* The same two launches with the MXFP8 copy of the output that the fp8 o-projection reads (tests): the hooks only fill out8 / sout / srows of
 * DecodeAttnArgs / DecodeAttnKv8Args. out8[rows][heads * head_dim] = e4m3 codes of the rows of `out` AS STORED (rounded to bf16 first), one E8M0
 * scale byte per 32 columns at sout[col / 128][srows][4] (K-tile-major, csrc/gemm_mx.h; oracle/mx_oracle.py::quantize is the definition);
 * srows >= rows, scale bytes of rows >= `rows` are not written; heads * head_dim a multiple of 128, else SA_ERR_ARG. Only the bf16 flash
 * kernels (decode_attn_flash2_kernel in both buffer forms, decode_attn_flash_kernel) and the KV8 kernel have the copy: dtype fp32
 * (decode_attn_mfma_kernel) and fp16 return SA_ERR_UNSUPPORTED and launch nothing.
 * What a launch may read. surya_op_decode_attn (all three kernels, every dtype): of the caches only rows < row_len[r] of the row's own slot
 * and kv heads can influence the result; row_len[r] = 0 is allowed (LayoutModel::decode_step at position 0 launches it) and then no cache row can
 * (decode_attn_flash_kernel and decode_attn_mfma_kernel still load row 0 through their clamp: its K copies are masked, its V copies zeroed). Cache rows
 * that were never appended, other slots and slabs >= n_slabs may hold anything, NaN included.
 * surya_op_decode_attn_kv8: K rows and k scales likewise; but the kernel fetches V^T (token-minor inside a 128-token tile) and the v scales by
 * whole 16-key blocks and multiplies what lies past the context by P = 0, so the V^T columns and v scales of tokens row_len[r] + 1 ..
 * (row_len[r] | 31) must be FINITE (RecModel zero-fills the arrays at creation and appends only finite rows). */
int surya_op_decode_attn_mx(int dtype, int head_dim, const float* qkv_part, int n_slabs, const void* qkv_bias, void* out, void* kcache,
                            void* vcache, const int32_t* active_slots, const int32_t* row_len, const float* rope_cs, int rows, int heads,
                            int kv_heads, int max_kv_len, float scale, void* stream, uint8_t* out8, uint8_t* sout, int srows);
int surya_op_decode_attn_kv8_mx(int head_dim, const float* qkv_part, int n_slabs, const void* qkv_bias, void* out, void* k8, void* v8t,
                                float* kscale, float* vscale, const int32_t* active_slots, const int32_t* row_len, const float* rope_cs, int rows,
                                int heads, int kv_heads, int max_kv_len, float scale, void* stream, uint8_t* out8, uint8_t* sout, int srows);

/* bf16 split-K projection of the decode step (launch_gemm_splitk): raw fp32 partial sums to part[*splitk][M][N] (capacity 8 slabs), no
 * epilogue; M <= 256 as the decoder runs it. */
int surya_op_gemm_splitk_bf16(const void* X, long ldx, const void* W, long ldw, float* part, int M, int N, int K, int* splitk, void* stream);
/* The same in fp16 (launch_gemm_splitk<fp16_t>, as RecModel<fp16_t> launches it; the 128 x 128 / 128 x 64 tiles above 256 rows included). */
int surya_op_gemm_splitk_f16(const void* X, long ldx, const void* W, long ldw, float* part, int M, int N, int K, int* splitk, void* stream);
/* The fp16 recogniser's GEMMs through launch_gemm, the launcher RecModel<fp16_t> uses (surya_op_gemm(SA_DTYPE_F16, ..) keeps refusing what it
 * refused). X [M][K], W [N][K], bias [N] or NULL: fp16. mode 0: 16-bit output, epi 0 bias, 1 residual (R fp16, required), 2 gelu, 3 swiglu
 * (W rows interleaved, C is [M][N/2]). mode 1: fp32 output C [M][N], epi 0 only (surya_rec_copy_last_logits). mode 2: the lm_head with greedy
 * partials, epi 6 only: C, R unused; amax receives one float4 {max, bits of the first argmax column, sum exp(v - max), 0} per (row, column tile)
 * at amax[(m * cdiv(N, *bn_used) + tile) * 4], *bn_used = the tile width chosen (>= 64: size amax for M * cdiv(N, 64) float4). Anything else
 * SA_ERR_UNSUPPORTED. Enqueue only. */
int surya_op_rec_gemm_f16(int mode, int epi, const void* X, long ldx, const void* W, long ldw, void* C, long ldc, const void* bias, const void* R,
                          long ldr, int M, int N, int K, float* amax, int* bn_used, void* stream);
/* MXFP8 ops (csrc/gemm_mx.h). quantize: fp32 rows [rows][K], K % 128 == 0 -> e4m3 [rows][K] + e8m0 scales K-tile-major
 * [K / 128][rows][4], with the rule every producer kernel uses (block scale = smallest power of two that keeps absmax <=
 * 448, round to nearest even). gemm_mx: C[M,N] fp32 = X W^T from MXFP8 operands (scales K-tile-major with M resp. N rows),
 * any M (above 256 rows the launchers pick larger tiles, same bits per element). mode 0: one pass; mode 1: split-K, `C` receives the slabs [*splitk][M][N] (capacity 8 slabs) and the caller sums
 * them; mode 2: SwiGLU epilogue -> MXFP8 [M][N/2] in q_out, scales [N / 256][M][4] in sq_out (N % 256 == 0). */
int surya_op_mx_quantize(const float* x, int rows, int K, uint8_t* q, uint8_t* scales, void* stream);
/* The lm_head launch by itself, through the launcher the recognition engine uses (launch_gemm / launch_gemm_mx with the greedy-partial
 * epilogue; above 256 rows the grouped 256 x 320 launch), so the epilogues can be tested at small K. dtype SA_DTYPE_F32 / BF16 / F16: X
 * [M][K], W [N][K], bias [N] or NULL in that dtype, SX = SW = NULL. dtype SA_OP_MXFP8: X, W e4m3 with e8m0 scales SX, SW laid out as
 * surya_op_gemm_mx takes them, bias bf16 [N] or NULL. masks = NULL: the unmasked epilogue. Otherwise the masked one: masks [n][ceil(N / 32)]
 * uint32, slot_mask [slots] int32 (row of masks or -1) and row_slot [M] int32 (NULL: row m is slot m), all DEVICE arrays as the engine
 * holds them; the caller keeps ids inside the table. amax receives one float4 {max, bits of the first argmax column, sum exp(v - max), 0}
 * per (row, column tile) at amax[(m * cdiv(N, *bn_used) + tile) * 4]; *bn_used = the tile width chosen (>= 64). Enqueue only. */
#define SA_OP_MXFP8 3
int surya_op_lm_head_partials(int dtype, const void* X, const void* SX, const void* W, const void* SW, const void* bias, int M, int N, int K,
                              const uint32_t* masks, const int32_t* slot_mask, const int32_t* row_slot, float* amax, int* bn_used, void* stream);
/* surya_op_lm_head_partials with the *_TOPK epilogue (same launchers, same arguments; masks = NULL: unconstrained, through the same kernel):
 * alt receives beside amax the tile's four best allowed columns inside N, alt[((m * tiles + tile) * 4 + j) * 2] = {float value, int32 column
 * bits}, value descending, column ascending among equal values, (-inf, 0x7fffffff) for missing entries; entry 0 is (max, argmax) of the
 * partial. With top_tokens / top_probs [M][4] (both or neither; DEVICE) it also runs the greedy head's reduction over the partials and the
 * combine kernel of the engine: head_token [M] int32 and head_score [M] float (DEVICE, required then) receive the head's token and
 * 1 / total (indexed by slot, like top_tokens / top_probs; row_slot = NULL: row m), scratch [16 * M + 16] float is working memory.
 * Enqueue only. */
int surya_op_lm_head_topk(int dtype, const void* X, const void* SX, const void* W, const void* SW, const void* bias, int M, int N, int K,
                          const uint32_t* masks, const int32_t* slot_mask, const int32_t* row_slot, float* amax, float* alt, int* bn_used,
                          int32_t* top_tokens, float* top_probs, int32_t* head_token, float* head_score, float* scratch, void* stream);
/* surya_op_lm_head_partials with the *_FORCED epilogue (same launchers; no masks): beside amax, which has the bits of the unmasked launch,
 * flogit[m] receives the accumulator-plus-bias value of column forced_col[m] (DEVICE int32 [M]) from the one tile that holds it; rows with
 * forced_col -1 (or outside [0, N)) are left untouched. Enqueue only. */
int surya_op_lm_head_forced(int dtype, const void* X, const void* SX, const void* W, const void* SW, const void* bias, int M, int N, int K,
                            const int32_t* forced_col, float* amax, float* flogit, int* bn_used, void* stream);
int surya_op_gemm_mx(int mode, const uint8_t* X, const uint8_t* SX, const uint8_t* W, const uint8_t* SW, int M, int N, int K,
                     float* C, int* splitk, uint8_t* q_out, uint8_t* sq_out, void* stream);

/* The recogniser's non-GEMM kernels by themselves (csrc/kernels.h), each through the launch code RecModel<T> uses (sa::launch_* of
 * csrc/kernels.h: the same grid and block arithmetic, the same choice of kernel instance, the same refusals). dtype SA_DTYPE_F32, SA_DTYPE_BF16
 * or SA_DTYPE_F16 (one entry per op; anything else SA_ERR_UNSUPPORTED): every `void*` operand is of that dtype. All pointers are caller-owned
 * device memory unless marked host; enqueue only; nothing is allocated. The MXFP8 copies (y8, sy) exist beside bf16 only, as in the engine
 * (SA_ERR_UNSUPPORTED otherwise); they want H % 128 == 0 and the scales K-tile-major, sy[(c / 128) * srows * 4 + row * 4 + (c / 32) % 4].
 * surya_op_rec_rmsnorm_rows: surya_op_rmsnorm with the engine's row gather: y[r] = Qwen2RMSNorm(x[src_row ? src_row[r] : r]), rows ldx / ldy
 *   elements apart. C and ldx multiples of 16 bytes, ldy of 4 elements.
 * surya_op_rec_rows: the prefill's row movers; dims is a HOST array:
 *   SA_REC_CONVERT_TILES dims {P, kin, kout}: src fp32 [.][kin] -> dst[r][0 .. kout) = T(src[index[r]]), zero from column kin on
 *   SA_REC_SCATTER_IMAGE dims {rows, H}: dst[index[r]] = T(src[r] + T(src2[index2[r]] + src3[index3[r]])) (merged tokens, row and column
 *                        position embeddings)
 *   SA_REC_SCATTER_ROWS  dims {rows, H}: dst[index[r]] = src[r]
 *   SA_REC_EMBED_TOKENS  dims {rows, H}: dst[r] = src[index[r]]; rows with index[r] < 0 are left as they are
 *   (operands a kind does not name: NULL)
 * surya_op_rec_rope_table: (cos, sin) pairs in fp32. SA_REC_ROPE_VISION: n = patches, d = head_dim; table[p][i] for i < d / 2 is the pair of
 *   pos_hw[2 p] * inv_freq[i] (i < d / 4) or pos_hw[2 p + 1] * inv_freq[i - d / 4]; dtype is not used. SA_REC_ROPE_DECODER: n = max_kv_len, d =
 *   head_dim / 2; table[t][i] = the pair of t * inv_freq[i], rounded to dtype; pos_hw = NULL.
 * surya_op_rec_rope_kv_append: the prefill's RoPE + cache append. qkv [n_tokens][(heads + 2 kv_heads) * head_dim]: q rotated in place; k
 *   rotated and v copied to row tok_pos[t] of slot tok_slot[t] in the caches [slot][kv_head][max_kv_len][head_dim]; rope_cs as above.
 * surya_op_rec_reduce_norm: x[M][H] = T(x + sum of S slabs part[S][M][H]) in place, then y = Qwen2RMSNorm(x) * w; w == NULL skips y. S in
 *   1..8, H % 4 == 0, H <= 4096. Tuning rnorm picks the kernel instance as in the engine.
 * surya_op_rec_decode_embed: row r is slot active_slots[r]: row_len[r] = min(kv_len[slot], max_kv_len - 1), x[r] = table[next_token[slot]],
 *   y[r] = Qwen2RMSNorm(x[r]) * w. Tuning ghead = 2 and H <= 2048, H % 8 == 0: embed_slots_norm2_kernel, else embed_slots_norm_kernel.
 * surya_op_rec_head: the greedy head over the lm_head's partials (surya_op_lm_head_partials) of `rows` rows, row r of slot row_slot[r]:
 *   out_token, out_score, out_bbox [.][6], next_token and kv_len are indexed by slot. table != NULL: the fused next-step embedding (x, y,
 *   row_len and the MXFP8 copy of row r, as surya_op_rec_decode_embed writes them). best_tot [slots][2] or NULL. forced_table != NULL: forced
 *   decoding ([slots][forced_stride] ids, forced_cursor [slots], flogit [rows]; greedy_token, greedy_prob, logprob by slot). pat_tok_class !=
 *   NULL: pattern-guided decoding (pat_tok_class [pat_vocab], pat_next_state [.][pat_n_classes] (the row stride), pat_state_mask [.], pat_slot_state and
 *   pat_slot_mask by slot; not beside forced_table: SA_ERR_ARG): a slot with state >= 0 whose row did not end moves to the next state and
 *   gets that state's mask id; no other output changes. Tuning ghead = 2,
 *   H <= 2048 and tiles_n <= 1536: greedy_head2_kernel, else greedy_head_kernel<T, true>, which has no fused embedding (SA_ERR_STATE). */
enum { SA_REC_CONVERT_TILES = 0, SA_REC_SCATTER_IMAGE, SA_REC_SCATTER_ROWS, SA_REC_EMBED_TOKENS };
enum { SA_REC_ROPE_VISION = 0, SA_REC_ROPE_DECODER };
typedef struct surya_rec_head_args {
    const float* part;                   /* [rows][tiles_n][4] */
    const void *hidden, *wb, *bb;        /* [rows][H], [6][H], [6] */
    const int32_t* row_slot;
    int32_t *out_token; float* out_score; int32_t *out_bbox, *next_token, *kv_len;
    const void *table, *wnorm; void *x, *y; int32_t* row_len; uint8_t *y8, *sy;
    float* best_tot;
    const int32_t* forced_table; int32_t* forced_cursor; const float* flogit; int32_t* greedy_token; float *greedy_prob, *logprob;
    int32_t tiles_n, rows, H, eos_id, pad_id, len_inc, max_kv_len, srows, forced_stride;
    float bbox_size, eps;
    /* pattern-guided decoding (surya_rec_set_patterns); pat_tok_class == NULL: off */
    const uint8_t* pat_tok_class; const uint16_t* pat_next_state; const uint8_t* pat_state_mask; int32_t *pat_slot_state, *pat_slot_mask;
    int32_t pat_n_classes, pat_vocab;
} surya_rec_head_args;
int surya_op_rec_rmsnorm_rows(int dtype, const void* x, long ldx, const void* w, void* y, long ldy, const int32_t* src_row, int rows, int C,
                              float eps, void* stream);
int surya_op_rec_rows(int dtype, int kind, void* dst, const void* src, const void* src2, const void* src3, const int32_t* index,
                      const int32_t* index2, const int32_t* index3, const int32_t* dims, void* stream);
int surya_op_rec_rope_table(int dtype, int kind, const int32_t* pos_hw, const float* inv_freq, float* table, int n, int d, void* stream);
int surya_op_rec_rope_kv_append(int dtype, void* qkv, const int32_t* tok_slot, const int32_t* tok_pos, const float* rope_cs, void* kcache,
                                void* vcache, int n_tokens, int heads, int kv_heads, int head_dim, int max_kv_len, void* stream);
int surya_op_rec_reduce_norm(int dtype, const float* part, int S, int M, void* x, const void* w, void* y, int H, float eps, uint8_t* y8,
                             uint8_t* sy, int srows, void* stream);
int surya_op_rec_decode_embed(int dtype, const void* table, const int32_t* next_token, const int32_t* active_slots, const int32_t* kv_len,
                              int max_kv_len, int32_t* row_len, void* x, const void* w, void* y, int rows, int H, float eps, uint8_t* y8,
                              uint8_t* sy, int srows, void* stream);
int surya_op_rec_head(int dtype, const surya_rec_head_args* args, void* stream);
/* Beam search's two kernels alone (csrc/beam.h), through the launchers the engine uses; device pointers.
 *   beam_select: `n_groups` groups of `width` consecutive slots out of `n_slots`; group g starts at slot lead_slots[g * stride] (NULL:
 *                g * width). In / out per slot: score, finished. In: alt_token / alt_prob [n_slots][SA_MAX_ALTERNATIVES]. Out per slot:
 *                token, parent, rank, prob, logp, next_token (pad for a finished beam), fork_src (absolute source slot or -1). With kv_len
 *                (else all four NULL): a first selection copies the lead's kv_len to the group and into prompt_len; fork_base = prompt_len,
 *                or 0 on a first selection and for a slot whose beam was empty; fork_len = min(the lead's kv_len, max_kv_len).
 *   kv_fork:     caches [layers][slots][kv_heads][max_kv_len][head_dim] of `dtype`; for every slot r < rows with fork_src[r] >= 0, rows
 *                [base[r], len[r]) of every layer, kv head, K and V are copied from slot fork_src[r] to slot r. A source must not be a
 *                destination of the same call. head_dim * sizeof(dtype) must be a multiple of 16 and the caches 16-byte aligned
 *                (SA_ERR_SHAPE). Unknown dtype: SA_ERR_UNSUPPORTED. */
int surya_op_rec_beam_select(const int32_t* lead_slots, int stride, int n_groups, int width, int n_slots, const int32_t* alt_token,
                             const float* alt_prob, float* score, int32_t* finished, int eos_id, int pad_id, int no_output_id, int first,
                             int32_t* token, int32_t* parent, int32_t* rank, float* prob, float* logp, int32_t* next_token, int32_t* fork_src,
                             int32_t* kv_len, int32_t* prompt_len, int32_t* fork_base, int32_t* fork_len, int max_kv_len, void* stream);
int surya_op_rec_kv_fork(int dtype, void* kcache, void* vcache, const int32_t* fork_src, const int32_t* base, const int32_t* len, int rows,
                         int layers, int slots, int kv_heads, int max_kv_len, int head_dim, void* stream);
/* The prompt fan-out of surya_rec_prefill_shared alone (csrc/kv_fanout.h), through the launcher the engine uses; device pointers. Caches as
 * for kv_fork. For every sequence n < n_seqs, rows [0, fan_len[n]) of every layer, kv head, K and V are copied from slot fan_src[n] to the
 * slots fan_dst[fan_off[n] .. fan_off[n + 1]); fan_dst holds n_dst entries. fan_len is clamped to [0, max_kv_len]; a destination out of
 * range or equal to its source is skipped. A source must not be a destination, nor a slot a destination twice, in one call. Shape rules
 * and errors as for kv_fork. */
int surya_op_rec_kv_fanout(int dtype, void* kcache, void* vcache, const int32_t* fan_src, const int32_t* fan_off, const int32_t* fan_dst,
                           const int32_t* fan_len, int n_seqs, int n_dst, int layers, int slots, int kv_heads, int max_kv_len, int head_dim,
                           void* stream);
/* The two kernels of the prompt store alone (csrc/kv_store.h), through the launcher the engine uses; device pointers. Caches as for
 * kv_fork; store_k / store_v are [layers][kv_heads][cap_rows][head_dim] of `dtype`. Entry n is the store rows [first[n], first[n] + len[n]);
 * len is clamped to [0, max_kv_len] and to cap_rows - first[n], and an entry whose first row is outside [0, cap_rows) is skipped.
 *   kv_keep:     rows [0, len[n]) of every layer, kv head, K and V of slot slot[n] go to entry n; a slot out of range is skipped. With x
 *                given (else x, last_row, hid NULL), row last_row[n] of x [x_rows][hidden] also goes to row first[n] of hid
 *                [cap_rows][hidden]; a last_row outside [0, x_rows) copies none. Entries of one call must not overlap.
 *   kv_restore:  entry n goes to rows [0, len[n]) of the slots fan_dst[fan_off[n] .. fan_off[n + 1]); fan_dst holds n_dst entries. A
 *                destination out of range is skipped. A slot must not be a destination twice in one call.
 * Shape rules and errors as for kv_fork; hidden * sizeof(dtype) must be a multiple of 16 as well. */
int surya_op_rec_kv_keep(int dtype, const void* kcache, const void* vcache, void* store_k, void* store_v, const int32_t* slot,
                         const int32_t* first, const int32_t* len, int n, int layers, int slots, int kv_heads, int max_kv_len, int head_dim,
                         int cap_rows, const void* x, const int32_t* last_row, void* hid, int hidden, int x_rows, void* stream);
int surya_op_rec_kv_restore(int dtype, void* kcache, void* vcache, const void* store_k, const void* store_v, const int32_t* first,
                            const int32_t* len, const int32_t* fan_off, const int32_t* fan_dst, int n, int n_dst, int layers, int slots,
                            int kv_heads, int max_kv_len, int head_dim, int cap_rows, void* stream);
/* The two kernels of lexicon-guided decoding (csrc/lexicon.h) on caller-owned DEVICE buffers, through the launch code the engine uses. The
 * tables are read unchecked, as the engine's are after its validation. `table` is a whole mask table of rows of `words` uint32; slot s
 * owns row row_base + s. eos / pad / nop ids outside [0, vocab) have no bit.
 *   lexicon_start: workgroup i gives slot slots[i] the state states[i]: slot_state = it; for a state >= 0 the slot's whole row is zeroed,
 *                the state's bits are set and slot_mask = row_base + slot; -1 leaves mask id and row alone. A slot at most once.
 *   lexicon_step: workgroup r moves slot row_slot[r] behind its token out_token[slot]: no lexicon (-1), eos / pad, an id outside the
 *                vocabulary and an id the state has no edge for touch nothing; else the old state's words are cleared, the new state's
 *                bits set and slot_state updated. A slot at most once per call. */
typedef struct surya_rec_lexicon_args {
    const int32_t *edge_off, *edge_tok, *edge_next; const uint8_t* state_flags;
    uint32_t* table; int32_t *slot_state, *slot_mask;
    int32_t words, row_base, vocab, eos_id, pad_id, nop_id;
} surya_rec_lexicon_args;
int surya_op_rec_lexicon_start(const surya_rec_lexicon_args* args, const int32_t* slots, const int32_t* states, int n, void* stream);
int surya_op_rec_lexicon_step(const surya_rec_lexicon_args* args, const int32_t* row_slot, const int32_t* out_token, int rows, void* stream);
/* The kernels of boosted decoding (csrc/boost.h) on caller-owned DEVICE buffers, through the launch code the engine uses.
 *   boost_step: `lex` as above (state_flags: one zero byte per state; slot_state = the boost states; nop_id unused), slot_root by slot,
 *                out_state and word_row as surya_rec_set_boost. Workgroup r moves slot row_slot[r] behind out_token[slot]: state -1,
 *                eos / pad and an id outside the vocabulary touch nothing; else the edge's target, or out_state for a word unit, or the
 *                slot's root; the slot's row becomes the new state's set. A slot at most once per call.
 *   boost_head: surya_op_rec_head's operands (`head`: part = record A's partials; best_tot, forced_table and pat_tok_class NULL) plus
 *                part_b [rows][tiles_n][4] (record B), slot_beta by slot (+inf = record A alone: the bits of surya_op_rec_head on
 *                `part`), plain_token / plain_prob by slot. Where surya_op_rec_head would run the fallback head: SA_ERR_STATE. */
typedef struct surya_rec_boost_head_args {
    surya_rec_head_args head;
    const float* part_b; const float* slot_beta; int32_t* plain_token; float* plain_prob;
} surya_rec_boost_head_args;
int surya_op_rec_boost_step(const surya_rec_lexicon_args* lex, const int32_t* slot_root, int out_state, int word_row, const int32_t* row_slot,
                            const int32_t* out_token, int rows, void* stream);
int surya_op_rec_boost_head(int dtype, const surya_rec_boost_head_args* args, void* stream);

/* The layout / table-recognition engine's own kernels by themselves (csrc/layout_kernels.h), each through the launch code LayoutModel
 * uses (sa::lay::launch_* of csrc/layout_model.hip: the same grid, block and LDS arithmetic and the same choice of kernel per dtype).
 * dtype SA_DTYPE_F32 or SA_DTYPE_BF16, anything else SA_ERR_UNSUPPORTED: these entries keep their two dtypes. The engine's third dtype has
 * entries of its own, surya_op_lay_<op>_f16 (the same arguments without `dtype`, the same launch code on the fp16 instance; declared below). All pointers are caller-owned device memory
 * unless marked host; enqueue only; nothing is allocated.
 * surya_lay_window_tables (host only, no GPU): what LayoutModel::init builds per (stage, shift) for an h x w token grid.
 *   perm[h * w] (host, may be NULL) = window-order row of every token after padding to whole windows and the cyclic shift by -shift;
 *   pad_rows (host, may be NULL; *n_pad entries, at most padded area - h * w) = the window-order rows of the zero padding, ascending;
 *   padded_hw[2] = the grid in whole windows; *shift_used = 0 when min(h, w) == window (such a stage is never shifted), else shift.
 *   min(h, w) < window: SA_ERR_UNSUPPORTED.
 * surya_lay_cross_plan (host only): for Lk cached keys, the fp32 cross attention's keys per range and ranges (scratch = rows * heads *
 *   ranges * (head_dim + 2) floats) and the bf16 / fp16 kernel's padded key count Lkp (vT = images * kv_heads * head_dim * Lkp elements).
 * surya_op_lay_layernorm: y[dst(r)] = LayerNorm(x[r]) over C channels, dst(r) = (r / rows_per_image) * (rows_per_image_out ?
 *   rows_per_image_out : rows_per_image) + perm[r % rows_per_image], or r when perm == NULL. bf16 / fp16 with C in {128, 256, 512, 1024} run
 *   layernorm_rows_bf16_kernel unless surya_set_tuning("lay_ln", 0), everything else layernorm_kernel. C % 4 == 0.
 * surya_op_lay_window_attn: qkv [windows * 64][(nh + 2 nkv) * 32] in window order -> out [windows * 64][nh * 32]; bias fp32 [nh][64][64];
 *   window index % (nwx * nwy) is its place in the image, shift > 0 masks across the cyclic-shift regions of the last window row / column.
 *   bf16 / fp16 run swin_window_attn_mfma_kernel<T>, fp32 swin_window_attn_kernel. ws must be 8.
 * surya_op_lay_merge_ln: x [B][H][W][C] -> y [B * H/2 * W/2][4C] = LayerNorm of the 2x2 neighbours (0,0), (1,0), (0,1), (1,1). H, W even.
 * surya_op_lay_rows: the encoder's row movers; dims is a HOST array:
 *   SA_LAY_PATCHIFY   dims {B, C, H, W, P, Kpad}: src fp32 pixels [B][C][H][W] -> dst patch rows [B * H/P * W/P][Kpad]
 *   SA_LAY_ADD_ROWS   dims {rows, rows_per_image, C}: dst[r] += src[r % rows_per_image]
 *   SA_LAY_ZERO_ROWS  dims {B, n_pad, rows_per_image, C}: dst[b * rows_per_image + index[i]] = 0
 *   SA_LAY_GATHER_ADD dims {rows, rows_per_image, C, rows_per_image_src}: dst[r] += src[(r / rows_per_image) * (rows_per_image_src ?
 *                     rows_per_image_src : rows_per_image) + index[r % rows_per_image]]
 * surya_op_lay_cross_attn: M query rows, one per decoder row, over the Lk keys of image item_map[row]; kv [n_images][Lk][2 * nkv * head_dim]
 *   (k heads | v heads). S in 1..8: qpart fp32 [S][M][nq * head_dim] split-K slabs, summed and rounded to the compute dtype; S == 0: qpart
 *   is a plain [M][nq * head_dim] matrix of the compute dtype (the prefill path). bf16 / fp16: transpose_cross_v_kernel fills vT, then
 *   cross_attn_mfma_kernel<T>; fp32: cross_attn_split_kernel + cross_attn_merge_kernel through scratch (sizes: surya_lay_cross_plan; the
 *   buffer the dtype does not use may be NULL). head_dim in {32, 64}, nq / nkv <= 8.
 * surya_op_lay_rmsnorm: SuryaADETRDecoderRMSNorm (variance clamped at eps, scale 1 + w, clamp to the dtype's finite range -- +-65504 in
 *   fp16 --, NaN -> 0: a row holding +inf comes out as zeros, as from the reference).
 * surya_op_lay_reduce_norm: x_out = T(res + T(bias + sum of S slabs part[S][M][H])), y = that RMSNorm of x_out. res may alias x_out;
 *   bias may be NULL; w == NULL skips y. H % 4 == 0, H <= 4096, S in 1..8.
 * surya_op_lay_prefill_attn: causal self-attention of B prompts of Tn tokens, qkv [B * Tn][(nq + 2 nkv) * head_dim], RoPE at positions
 *   0 .. Tn - 1 from rope_cs [Tmax][head_dim / 2][2] (cos, sin); writes out [B * Tn][nq * head_dim] and rows 0 .. Tn - 1 of the caches
 *   [B][nkv][Tmax][head_dim]. head_dim in {32, 64}, Tn * head_dim * 8 bytes of LDS.
 * surya_op_lay_embed: family SA_FAMILY_LAYOUT: box_embed_kernel over tokens [rows][7]; SA_FAMILY_TABLE: table_embed_kernel over tokens
 *   [rows][10]; tabs = DEVICE array of 17 device pointers in the order of SA_LW_EMB_TABLES. vocab > bbox_size.
 * surya_op_lay_heads: layout_heads_kernel<T, false>: row b of x starts at element b * ldx; class_logits fp32 [B][label_count], bbox fp32 [B][6]. */
enum { SA_LAY_PATCHIFY = 0, SA_LAY_ADD_ROWS, SA_LAY_ZERO_ROWS, SA_LAY_GATHER_ADD };
int surya_lay_window_tables(int h, int w, int window, int shift, int32_t* perm, int32_t* pad_rows, int32_t* n_pad, int32_t* padded_hw,
                            int32_t* shift_used);
int surya_lay_cross_plan(int Lk, int32_t* chunk, int32_t* ranges, int32_t* Lkp);
int surya_op_lay_layernorm(int dtype, const void* x, const void* w, const void* b, void* y, const int32_t* perm, long rows, int rows_per_image,
                           int C, float eps, int rows_per_image_out, void* stream);
int surya_op_lay_window_attn(int dtype, const void* qkv, const float* bias, void* out, long windows, int nh, int nkv, int nwx, int nwy, int shift,
                             int ws, void* stream);
int surya_op_lay_merge_ln(int dtype, const void* x, const void* w, const void* b, void* y, int B, int H, int W, int C, float eps, void* stream);
int surya_op_lay_rows(int dtype, int kind, void* dst, const void* src, const int32_t* index, const int32_t* dims, void* stream);
int surya_op_lay_cross_attn(int dtype, int head_dim, const void* qpart, int S, int M, const void* kv, int n_images, const int32_t* item_map,
                            void* out, float* scratch, void* vT, int nq, int nkv, int Lk, float scale, void* stream);
int surya_op_lay_rmsnorm(int dtype, const void* x, const void* w, void* y, int rows, int C, float eps, void* stream);
int surya_op_lay_reduce_norm(int dtype, const float* part, int S, int M, const void* res, const void* bias, void* x_out, const void* w, void* y,
                             int H, float eps, void* stream);
int surya_op_lay_prefill_attn(int dtype, int head_dim, const void* qkv, void* out, void* kcache, void* vcache, const float* rope_cs, int B, int Tn,
                              int nq, int nkv, int Tmax, float scale, void* stream);
int surya_op_lay_embed(int dtype, int family, const int32_t* tokens, const void* const* tabs, void* x, int rows, int Hd, int box_embed,
                       int bbox_size, int vocab, int label_count, int category_count, int merge_count, void* stream);
int surya_op_lay_heads(int dtype, const void* x, long ldx, const void* fnorm_w, const void* ln_w, const void* ln_b, const void* lm_w, const void* bb_w,
                       const void* bb_b, float* class_logits, float* bbox, int B, int Hd, int label_count, float rms_eps, float ln_eps, void* stream);

/* The same kernels alone in fp16 (SA_DTYPE_F16, the engine's third compute dtype): the arguments of surya_op_lay_<op> without `dtype`, every
 * pointer of the compute dtype fp16. fp16 takes the kernels bf16 takes (the matrix-core window and cross attention, the rows-in-registers
 * LayerNorm); surya_op_lay_cross_attn_f16 needs vT like bf16 and ignores scratch. surya_op_gemm_geglu_f16 = surya_op_gemm's code 8 (geglu)
 * with fp16 operands and output: X [M][K], W [N][K] rows interleaved (gate_j, up_j), C [M][N / 2]. */
int surya_op_lay_layernorm_f16(const void* x, const void* w, const void* b, void* y, const int32_t* perm, long rows, int rows_per_image, int C, float
        eps, int rows_per_image_out, void* stream);
int surya_op_lay_window_attn_f16(const void* qkv, const float* bias, void* out, long windows, int nh, int nkv, int nwx, int nwy, int shift, int ws,
        void* stream);
int surya_op_lay_merge_ln_f16(const void* x, const void* w, const void* b, void* y, int B, int H, int W, int C, float eps, void* stream);
int surya_op_lay_rows_f16(int kind, void* dst, const void* src, const int32_t* index, const int32_t* dims, void* stream);
int surya_op_lay_cross_attn_f16(int head_dim, const void* qpart, int S, int M, const void* kv, int n_images, const int32_t* item_map, void* out,
        float* scratch, void* vT, int nq, int nkv, int Lk, float scale, void* stream);
int surya_op_lay_rmsnorm_f16(const void* x, const void* w, void* y, int rows, int C, float eps, void* stream);
int surya_op_lay_reduce_norm_f16(const float* part, int S, int M, const void* res, const void* bias, void* x_out, const void* w, void* y, int H, float
        eps, void* stream);
int surya_op_lay_prefill_attn_f16(int head_dim, const void* qkv, void* out, void* kcache, void* vcache, const float* rope_cs, int B, int Tn, int nq,
        int nkv, int Tmax, float scale, void* stream);
int surya_op_lay_embed_f16(int family, const int32_t* tokens, const void* const* tabs, void* x, int rows, int Hd, int box_embed, int bbox_size, int
        vocab, int label_count, int category_count, int merge_count, void* stream);
int surya_op_lay_heads_f16(const void* x, long ldx, const void* fnorm_w, const void* ln_w, const void* ln_b, const void* lm_w, const void* bb_w, const
        void* bb_b, float* class_logits, float* bbox, int B, int Hd, int label_count, float rms_eps, float ln_eps, void* stream);
int surya_op_gemm_geglu_f16(const void* X, long ldx, const void* W, long ldw, void* C, long ldc, int M, int N, int K, void* stream);


/* ------------------------------------------------------------------------------------------------------------
 * Detection model: EfficientViT-L backbone + SegFormer-style decode head + sigmoid + x4 bilinear upsample.
 * Replaces EfficientViTForSemanticSegmentation.forward (surya/detection/model/encoderdecoder.py:734-753) and the
 * interpolate + .float() of DetectionPredictor.batch_detection (surya/detection/__init__.py:119-132).
 * The network is described as a list of ops over NHWC activation buffers (built by surya_amd/detection/plan.py from
 * the reference's state-dict; BatchNorm folded, 3x3 weights as [Cout][ky][kx][Cin] with K padded to x64).
 * ---------------------------------------------------------------------------------------------------------- */
/* What surya_det_create accepts. An op list is either computed correctly or refused on the host before anything is allocated or
 * launched (SA_ERR_ARG: an index; SA_ERR_SHAPE: sizes; SA_ERR_UNSUPPORTED: a parameter no kernel takes). V = elements per 16 bytes of
 * the compute dtype (4 in fp32, 8 in bf16 / fp16), KE = the K-tile (32 / 64 elements). Every op: sizes in [1, 65535], its buffers hold
 * hin * win * cin (in0, in1) and hout * wout * cout (out, res) elements per image, and every buffer it reads was written by an op before it.
 *   INPUT          cin <= cout, cout % V == 0 (one pixel = whole 16-byte stores), hout x wout == hin x win
 *   CONV           cin % V == 0 (a 16-byte gather chunk stays inside one filter tap), cout % 4 == 0 (4-wide epilogue), p1 % KE == 0,
 *                  p1 >= k * k * cin, hout x wout == floor((hin + 2 p0 - k) / stride) + 1, max_batch * hout * wout < 2^31;
 *                  `act` together with `res` is refused: the 1x1 (GEMM) path has a residual epilogue and an activation epilogue, not both
 *   DWCONV         (k, stride) in {3, 5} x {1, 2}, cin == cout, cin % V == 0, hout x wout as for CONV
 *   GROUPED1X1     p0 <= 32 (a group's input row lives in 32 registers), p0 % V == 0, cin % p0 == 0, cin == cout, cin / p0 <= 65535
 *   LITEMLA        p0 in {16, 32}, cout % p0 == 0, cout / p0 heads: even (half from in0, half from in1), cin == 3 * cout / 2
 *   UPCAT          cin % V == 0, p0 % 4 == 0 and cout % 4 == 0 (4-wide stores), p0 + cin <= cout
 *   CLASSIFY       cin % V == 0, 1 <= cout <= 4, bias required, hin * win * cout <= num_labels * (height / 4) * (width / 4) (the planes)
 *   UPSUM_SRC      at most 3 in front of an UPSUM_CLASSIFY, each [hin, win, cin] with the UPSUM_CLASSIFY's cin
 *   UPSUM_CLASSIFY as CLASSIFY
 *   UPSAMPLE_OUT   (hin, win, cout) those of the CLASSIFY / UPSUM_CLASSIFY before it, cout * hout * wout <= num_labels * height * width */
enum { SA_DET_INPUT = 0,       /* fp32 NCHW pixels -> NHWC, channels padded to `cout`                      */
       SA_DET_CONV,            /* dense KxK conv as implicit GEMM: bias, act, optional residual `res`        */
       SA_DET_DWCONV,          /* depthwise KxK: weights [K*K][C], bias, act                                 */
       SA_DET_GROUPED1X1,      /* grouped 1x1, p0 = channels per group (in == out)                           */
       SA_DET_LITEMLA,         /* ReLU linear attention; in0 = qkv conv, in1 = aggregated qkv; p0 = head dim */
       SA_DET_UPCAT,           /* bilinear resize of in0 into channels [p0, p0+cin) of `out` (cout wide)     */
       SA_DET_CLASSIFY,        /* 1x1 conv to `cout` labels + sigmoid -> fp32 planes                         */
       SA_DET_UPSAMPLE_OUT,    /* fp32 planes -> output size, bilinear                                       */
       /* Decode head in its folded form (round 4; surya/detection/model/encoderdecoder.py:699-722 is linear up to the ReLU, and a
        * 1x1 convolution commutes with a bilinear resize): linear_fuse(cat(up(linear_c_s(x_s)))) = sum_s up(A_s x_s) + c with
        * A_s = (bn_scale * W_fuse[:, s]) W_c_s built at load. The 4 x decoder_layer_hidden concat and the K = 4 x 128 GEMM over it
        * never exist: every stage runs ONE 1x1 conv to decoder_hidden channels at its own resolution, and the sum + ReLU + classifier
        * + sigmoid is one pass over the full-resolution stage. */
       SA_DET_UPSUM_SRC,       /* declares in0 ([hin, win, cin] per image) as a low-resolution addend of the next UPSUM_CLASSIFY (<= 3) */
       SA_DET_UPSUM_CLASSIFY };/* planes = sigmoid(classifier(relu(in0 + sum of the bilinearly resized addends))): in0 [hin, win, cin], `cout` labels */
enum { SA_ACT_NONE = 0, SA_ACT_HSWISH = 1, SA_ACT_RELU = 2 };

typedef struct surya_det_op {
    int32_t type;
    int32_t in0, in1, out, res;      /* buffer ids (-1 = none) */
    int32_t cin, cout, k, stride, act;
    int32_t hin, win, hout, wout;
    int32_t w_idx, b_idx;            /* weight-table indices (-1 = none) */
    int32_t p0, p1;                  /* CONV: pad, Kpad; see the enum for others */
} surya_det_op;

typedef struct surya_det_config {
    int32_t n_ops, max_batch, height, width, num_labels, dtype;
} surya_det_config;

typedef struct surya_det surya_det;

/* buf_elems[i] = elements PER IMAGE of activation buffer i (the library allocates max_batch times that). */
int surya_det_create(const surya_det_config* cfg, const surya_det_op* ops, const void* const* weights, int n_weights,
                     const size_t* buf_elems, int n_bufs, surya_det** out);
int surya_det_destroy(surya_det* h);
/* pixel_values: device fp32 [batch, 3, H, W] (rescaled + ImageNet-normalised, surya/detection/processor.py:126-146).
 * heatmaps: device fp32 [batch, labels, H, W] (may be NULL); lowres: device fp32 [batch, labels, H/4, W/4] (may be NULL)
 * = the model's own output before the predictor-side upsample. Enqueue only. */
int surya_det_forward(surya_det* h, const float* pixel_values, int batch, float* heatmaps, float* lowres, void* stream);
/* Measurement support (tools/det_op_times.py, bench.py's detection buckets): the same forward with a hipEvent in front of every op of the
 * list; op_ms[i] (host, n_op_ms >= surya_det_op_count) = milliseconds of op i, 0 for an op folded into a fused form (sa::Tuning det_fuse).
 * Synchronises the stream. Not for timed regions. */
int surya_det_op_count(surya_det* h);
int surya_det_forward_timed(surya_det* h, const float* pixel_values, int batch, float* heatmaps, float* lowres, void* stream, float* op_ms,
                            int n_op_ms);
/* Test and measurement support (tests/test_gpu_det_microplan.py): a device-to-device copy of the first `batch` images of activation
 * buffer `buf` -- batch * buf_elems[buf] elements of the engine's compute dtype, NHWC as the op that wrote it left them -- into dst
 * (device, dst_bytes >= that). SA_ERR_ARG for a bad index, a batch outside [1, max_batch] or a dst_bytes too small. Enqueue only. */
int surya_det_read_buffer(surya_det* h, int buf, int batch, void* dst, size_t dst_bytes, void* stream);
/* Same forward from the resized pages themselves: device uint8 [batch, H, W, pixel_stride], pixel_stride 3 (RGB) or 4 (RGBX =
 * PIL's in-memory layout, uploaded without repacking; the fourth byte is ignored). The rescale
 * (x * 1/255 in fp32) and normalisation ((x - mean) / std) of SegformerImageProcessor._preprocess
 * (surya/detection/processor.py:126-146) run inside the first layout kernel: bit-identical pixel_values, a quarter of the
 * PCIe bytes, no per-pixel host work. */
int surya_det_forward_u8(surya_det* h, const uint8_t* pixels_nhwc, int pixel_stride, const float* mean, const float* std, int batch,
                         float* heatmaps, float* lowres, void* stream);

/* One Pillow `Image.resize(size, LANCZOS)` of an 8-bit RGB page on the device (detection side). Replaces the
 * two host resizes of DetectionPredictor.prepare_image (surya/detection/__init__.py:50-57: img.thumbnail(size, LANCZOS) then
 * img.resize(size, LANCZOS) = two calls here; the sizes and the 22-bit fixed-point coefficient tables of Pillow's resampler come
 * from surya_amd/common/pil_resample.py, which restates Pillow's precompute_coeffs / normalize_coeffs_8bpc). Bit-identical to
 * Pillow: int32 accumulation from 2^21, arithmetic shift by 22, clip to 0..255, horizontal pass first into `tmp`.
 *   src / dst   device uint8 [h][w][pix], pix = 3 (RGB) or 4 (RGBX, fourth byte ignored / written 0)
 *   bounds_*    device int32 [out][2] = (first source index, tap count); taps_* device int32 [out][ksize_*]
 *               (x tables may be NULL when the width does not change, y tables when the height does not)
 *   tmp         device scratch of src_h * dst_w * 4 bytes, needed when both axes change. Enqueue only. */
int surya_resample_lanczos_u8(const uint8_t* src, int src_w, int src_h, int src_pix, uint8_t* dst, int dst_w, int dst_h, int dst_pix,
                              const int32_t* bounds_x, const int32_t* taps_x, int ksize_x, const int32_t* bounds_y,
                              const int32_t* taps_y, int ksize_y, uint8_t* tmp, void* stream);
/* One Pillow `Image.reduce((fx, fy))` of an 8-bit RGB page on the device: the integer box reduction `img.thumbnail(size, LANCZOS)`
 * (reducing_gap = 2.0) runs in front of its LANCZOS passes when an axis shrinks by 4x or more (600-dpi scans, camera photos). The
 * LANCZOS call that follows takes tables built for the source box (0, 0, src_w / fx, src_h / fy) (pil_resample.plan_chain).
 * Bit-identical to Pillow: a pixel = ((sum + n / 2) * (2^24 / n)) >> 24 in uint32 over the n source pixels present in its fx x fy
 * block (the last column / row / corner of a size that is no multiple of the factor average what exists).
 *   src   device uint8 [src_h][src_w][src_pix], dst device uint8 [ceil(src_h / fy)][ceil(src_w / fx)][dst_pix]; pix = 3 (RGB) or
 *         4 (RGBX, fourth byte ignored / written 0; a 4-byte dst must be 4-byte aligned). 1 <= fx, fy <= 255, not both 1; any
 *         height. SA_ERR_ARG otherwise. fx in 2..4 streams through vector loads where the rows are aligned for them (RGBX: 16
 *         or 8 bytes, RGB: 4); every other case runs the generic kernel. Enqueue only. */
int surya_reduce_u8(const uint8_t* src, int src_w, int src_h, int src_pix, uint8_t* dst, int dst_pix, int fx, int fy, void* stream);

/* Heat map -> text boxes on the device. Replaces detect_boxes (surya/detection/heatmap.py:27-107:
 * get_dynamic_thresholds :14-24, cv2.connectedComponentsWithStats, per-component cv2.dilate + cv2.minAreaRect + cv2.boxPoints,
 * corner order, confidence = component max / page max) for `batch` pages at once; what is left for the host is
 * get_and_clean_boxes' rescale / fit_to_bounds / clean_boxes on a few hundred 4-point boxes (heatmap.py:127-136).
 * heat: device fp32; the text heat map of page b starts at heat + b * page_stride (floats) and is [height][width]
 * (width % 4 == 0; values must be non-negative, as sigmoid outputs are). boxes: device fp32 [batch][max_boxes][4][2] (x, y),
 * clockwise from the corner with the smallest x + y, in heat-map pixels; conf: device fp32 [batch][max_boxes]; count: device
 * int32 [batch] = boxes of the page in raster order of their first pixel (the order cv2 labels them), or -1 if the page has
 * more than max_boxes components (nothing else is written for that page). workspace: device, caller-owned,
 * >= surya_det_boxes_workspace_bytes(...). Enqueue only. */
size_t surya_det_boxes_workspace_bytes(int batch, int height, int width, int max_boxes);
int surya_det_boxes(const float* heat, long page_stride, int batch, int height, int width, float text_threshold, float low_text,
                    int max_boxes, float* boxes, float* conf, int32_t* count, void* workspace, size_t workspace_bytes, void* stream);
/* Test and diagnostic surface: where surya_det_boxes keeps its intermediates in the caller's workspace, so that a test can read
 * every stage of one call (tests/test_gpu_det_post_stages.py). Host code only; no effect on any launch. offsets receives
 * SA_DET_BOXES_LAYOUT_WORDS values in this fixed order: the byte offsets of
 *   st (PageState [batch]), hist (uint32 [batch][2048]), psum (double [batch][1024]), pcnt (uint32 [batch][1024]),
 *   label, area, minx, maxx, miny, maxy, maxv (int32 / float bits [batch][height * width] each),
 *   blk (int32 [batch][n_blk][2]), comp (CompStats [batch][max_boxes]), rowoff (int32 [batch][max_boxes]),
 *   rmin, rmax (int32 [batch][row_cap] each), big (scratch of the tall-component launch),
 * then big_stride (bytes of one scratch slice; 0 when the page height needs none), total (= surya_det_boxes_workspace_bytes),
 * sizeof(PageState) and sizeof(CompStats) (csrc/det_post.h, csrc/det_post_core.h) for a caller that mirrors the two structs.
 * n_blk: scan blocks of 4096 pixels per page; row_cap: entries of a page's rmin / rmax (either may be NULL).
 * SA_ERR_ARG for a non-positive size, offsets == NULL or n_offsets < SA_DET_BOXES_LAYOUT_WORDS. */
#define SA_DET_BOXES_LAYOUT_WORDS 21
int surya_det_boxes_workspace_layout(int batch, int height, int width, int max_boxes, size_t* offsets, int n_offsets, int* n_blk,
                                     int* row_cap);

/* Tiled detection (DetectionPredictor.tiling; the grid and the ownership rule: surya_amd/detection/tiling.py): the two copies around
 * the forward of a batch of tiles. Both read a DEVICE table of n descriptors, so one launch serves every tile of a model batch
 * whatever pages they belong to. Enqueue only.
 *
 * surya_det_cut_tiles_u8: descriptor i copies the tile_size x tile_size window at (x0, y0) of its page into tile `tile` of
 * dst, device uint8 [n_tiles][tile_size][tile_size][dst_pix] -- the batch surya_det_forward_u8 reads, written in place. White (255)
 * outside the page (the origin may be negative), the fourth byte 0 when dst_pix is 4. descs: device array of
 *   { uint64 src (device address of the page, uint8 [h][w][pix]); int32 w, h, pix (3 = RGB, 4 = RGBX, fourth byte ignored);
 *     int32 x0, y0; int32 tile }                                                                        -- 32 bytes, C layout.
 * SA_ERR_ARG, with nothing launched, when descs or dst is null, n < 0, n > 65535, n_tiles or tile_size is non-positive or dst_pix
 * is not 3 or 4; n == 0 launches nothing. The table lives on the device, so what IT says is checked there: a descriptor with a
 * null page, a non-positive size, a pix that is not 3 or 4 or a tile outside [0, n_tiles) writes nothing. Two descriptors of one
 * launch must not name the same tile. A lane writes 16 bytes (four RGBX pixels) when tile_size % 4 == 0 and dst is 16-byte aligned
 * (RGB: 12 bytes, dst 4-byte aligned), reading them as one 16-byte / three 4-byte loads where the source address allows it.
 *
 * surya_det_stitch_tiles: descriptor i copies the rectangle its tile OWNS, [ty0, ty0 + th) x [tx0, tx0 + tw) of the first `planes`
 * planes of tile `tile` of heat, device fp32 [n_tiles][labels][tile_size][tile_size] (surya_det_forward_u8's output), to rows
 * dy0.., columns dx0.. of the page map, and writes pad_cols zeros behind the rectangle's last column on each of those rows: the
 * page map is fp32 [planes][rows][pitch] with pitch = the map width rounded up to 4 (surya_det_boxes wants width % 4 == 0), and
 * the descriptors of a page's last tile column carry its pad columns -- zeroing them belongs to THIS entry point, the map needs no
 * memset. Every map pixel has one owner, so a page stitched by several launches (its tiles span several forwards) equals the page
 * stitched by one, in any order; cells no descriptor owns are left as they are. descs: device array of
 *   { uint64 dst (device address of plane 0 of the page map); int64 pitch (floats per row); int64 plane_stride (floats between
 *     planes); int32 tile; int32 tx0, ty0, tw, th; int32 dx0, dy0; int32 planes (1 .. labels); int32 pad_cols (0 .. 3);
 *     int32 reserved }                                                                                  -- 64 bytes, C layout.
 * SA_ERR_ARG, with nothing launched, when heat or descs is null, n < 0, n > 65535 or n_tiles, labels or tile_size is
 * non-positive; n == 0 launches nothing. Checked on the device: a descriptor with a null map, a non-positive pitch, a tile outside
 * [0, n_tiles), a rectangle that is empty or leaves the tile, a negative origin, planes outside 1 .. labels or pad_cols outside
 * 0 .. 3 writes nothing. What a descriptor addresses in the page or the map is not checked against their ends: the caller keeps
 * them inside. Rectangles of one launch must not overlap in a map. */
int surya_det_cut_tiles_u8(const void* descs, int n, uint8_t* dst, int n_tiles, int tile_size, int dst_pix, void* stream);
int surya_det_stitch_tiles(const float* heat, int n_tiles, int labels, int tile_size, const void* descs, int n, void* stream);

/* Page skew from the heat map (DetectionPredictor.skew; the rule: surya_amd/detection/skew.py, the arithmetic: csrc/det_skew_core.h):
 * the projection profile of every page's text pixels under every candidate angle, scored by the sum of squared differences of
 * neighbouring bins. Integers only, so the scores equal the numpy statement bit for bit. Enqueue only.
 * heat is addressed as surya_det_boxes addresses it: page b starts at heat + b * page_stride (floats), is [height][width], width % 4
 * == 0; pixel (x, y) is text iff heat > threshold (strict). cs: device int32 [batch][n_angles][2] = (c, s) = (rint(cos * 65536),
 * rint(sin * 65536)) of the candidate's angle IN THE MAP, every page its own table; a text pixel falls into bin
 * r = (y * c - x * s + (width - 1) * max(s, 0)) >> 16 of height + width bins (int32 arithmetic: c > 0, |s| <= c and sizes <= 8192 keep
 * it below 2^31). scores: device uint64 [batch][n_angles] = sum over r of (P[r + 1] - P[r])^2; n_text: device int32 [batch] = the
 * page's text pixels (it is the compaction's counter: zeroed and counted by the call). A page without text scores 0 everywhere.
 * workspace: device, caller-owned, >= surya_det_skew_workspace_bytes(...) (a word per map pixel: the lists of text pixels).
 * SA_ERR_ARG, with nothing launched, for a null pointer (heat, cs, scores, n_text, workspace), a negative batch, a non-positive
 * height or width, n_angles outside 1 .. 1024, a negative or NaN threshold or a workspace that is too small; SA_ERR_SHAPE for a height
 * or width above 8192, width % 4 != 0, page_stride % 4 != 0 or a heat pointer that is not 16-byte aligned; batch == 0 launches
 * nothing. The coefficient table lives on the device and is read unchecked: the kernel does not count a bin outside
 * [0, height + width), so a table that breaks the bounds above gives wrong scores and touches no memory it should not. */
size_t surya_det_skew_workspace_bytes(int batch, int height, int width);
int surya_det_skew(const float* heat, long page_stride, int batch, int height, int width, float threshold, const int32_t* cs, int n_angles,
                   uint64_t* scores, int32_t* n_text, void* workspace, size_t workspace_bytes, void* stream);

/* Centre-line profiles of the kept text components (DetectionPredictor.centerlines; the rule: surya_amd/detection/centerline.py, the
 * arithmetic: csrc/det_centerline_core.h). Enqueued BEHIND a surya_det_boxes call of the same (batch, height, width, max_boxes) on the
 * same stream: boxes_workspace is that call's workspace, read through its layout (st, label, area and comp of
 * surya_det_boxes_workspace_layout; after the call `area` holds a kept root's compact index and -1 for a dropped one) and never written.
 * Integers only, so the outputs equal the numpy statement bit for bit. Enqueue only.
 * For kept component c of page b, inclusive bounding box x0..x1, y0..y1: axis = 0 (bins along x, perpendicular coordinate p = y) when
 * x1 - x0 >= y1 - y0, else 1 (bins along y, p = x); a pixel of the component at coordinate a along the axis falls into bin
 * k = ((a - origin) * knots) / extent by integer division (origin = x0 or y0, extent = the box length along the axis, <= 8192).
 * cnt: device uint32 [batch][max_boxes][knots] = pixels of the bin; sum: device uint64, same shape = the sum of p; lo / hi: device int32,
 * same shape = min / max of p; an empty bin holds 0, 0, 0x7fffffff, -1. axis: device int32 [batch][max_boxes]. The call initialises all
 * five arrays itself. Components beyond the page's count, and every component of a page whose count is -1 (more than max_boxes
 * components), have empty bins and axis = -1.
 * SA_ERR_ARG, with nothing launched, for a null pointer (boxes_workspace, cnt, sum, lo, hi, axis), a negative batch, a non-positive
 * height, width or max_boxes, knots outside 2 .. 64, batch > 65535, max_boxes > 2^25, or a workspace that is smaller than
 * surya_det_boxes_workspace_bytes(batch, height, width, max_boxes) or not 16-byte aligned; SA_ERR_SHAPE for width % 4 != 0 (as
 * surya_det_boxes) or a height or width above 8192; batch == 0 launches nothing. The workspace is read unchecked but guarded: a label
 * outside the page, a compact index outside the page's count and a pixel outside its component's box are skipped, so a workspace that no
 * surya_det_boxes call filled gives meaningless bins and touches no memory it should not. */
int surya_det_centerlines(int batch, int height, int width, int max_boxes, int knots, const void* boxes_workspace, size_t workspace_bytes,
                          uint32_t* cnt, uint64_t* sum, int32_t* lo, int32_t* hi, int32_t* axis, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Layout model family: Donut-Swin window-attention encoder + ADETR decoder with cross- and self-attention.
 * Replaces DonutSwinLayoutModel.forward (surya/layout/model/encoder.py:36-80, surya/common/donut/encoder.py) and
 * SuryaLayoutDecoder.forward (surya/layout/model/decoder.py:96-131, surya/common/adetr/decoder.py) as
 * LayoutPredictor.batch_layout_detection calls them (surya/layout/__init__.py:95-131): one `encode` per image batch, then one
 * `decode_step` per box until every image emitted its end token (the per-step host round trip is the reference's own).
 * Window 8 (64 tokens), head dim 32 in the encoder; image sides a multiple of patch * 2^(stages-1) (the reference's per-stage sin-cos
 * tables ask for the same), every stage grid at least one window; grids that are not whole windows are zero-padded inside every block
 * as DonutSwinLayer.maybe_pad does (surya/common/donut/encoder.py:588-596, 668).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct surya_layout_config {
    int32_t img_h, img_w, patch, embed_dim, n_stages;
    int32_t depths[8], heads[8], kv_heads[8];
    int32_t window;
    float enc_eps;                    /* layer_norm_eps of the Swin blocks */
    int32_t encoder_length;           /* rows of the learned position_embeddings */
    int32_t dec_layers, dec_hidden, dec_inter, dec_heads, dec_kv_heads;
    int32_t vocab, label_count, bbox_size;
    float rms_eps, ln_eps;
    int32_t max_batch, max_boxes, dtype;
    /* Model family on the same encoder / decoder stack:
     *   SA_FAMILY_LAYOUT (0): surya/layout -- 7-number tokens, BboxEmbedding (15 tables of dec_hidden), double residual flow
     *     (layout/model/config.py:221), heads = lm_head [label_count] + sigmoid(bbox_head + bias);
     *   SA_FAMILY_TABLE (1): surya/table_rec -- 10-number tokens (bbox 6, category, merges, colspan, is_header), LabelEmbedding =
     *     concat(14 box tables of box_embed, category + merge + colspan tables of dec_hidden - box_embed)
     *     (table_rec/model/decoder.py:12-73), the plain residual flow (adetr/decoder.py:395-417), heads = the four non-bbox
     *     box_property_heads stacked [category | merges | colspan | is_header] (label_count rows in all, no bias) + sigmoid(bbox head). */
    int32_t family, box_embed, category_count, merge_count;
} surya_layout_config;
enum { SA_FAMILY_LAYOUT = 0, SA_FAMILY_TABLE = 1 };

/* Weight table (device pointers, compute dtype unless noted; Linear weights [out, in]):
 *   globals SA_LW_*; PATCH_W is [embed_dim][64] = the Conv2d weight flattened (c, ky, kx) and zero padded; DEC_INVFREQ fp32 [hd / 2];
 *   DEC_ZERO_BIAS = zeros [(heads + 2 kv_heads) * hd] (the ADETR attention has no qkv bias; the fused decode-attention kernel takes one);
 *   EMB_TABLES = 17 slots: w, h, cx, cy, xskew, yskew, x1, y1, x2, y2, x3, y3, x4, y4 ([vocab][hidden], table family [vocab][box_embed]), then
 *     layout: label ([label_count][hidden]) + 2 unused; table: category ([category_count][P]), merge ([merge_count][P]), colspan ([vocab][P]),
 *     P = dec_hidden - box_embed;
 *   per stage SA_LS_* (SINCOS = the stage's 2-D sin-cos table [tokens][dim] built as the reference builds it; MERGE_* of the last stage
 *   are ignored), then per block SA_LB_* (QKV fused q | k | v rows; RELBIAS fp32 [heads][64][64] = relative_position_bias_table gathered
 *   through relative_position_index, rounded to the compute dtype first); then per decoder layer SA_LD_* (CKV_W = cross k | v rows fused,
 *   QKV_W = self q | k | v fused, GU_W = gate / up rows interleaved g0, u0, g1, u1 ...). */
enum { SA_LW_PATCH_W = 0, SA_LW_PATCH_B, SA_LW_EMB_LN_W, SA_LW_EMB_LN_B, SA_LW_POS_EMB, SA_LW_DEC_FNORM, SA_LW_DEC_LN_W, SA_LW_DEC_LN_B,
       SA_LW_DEC_LM_W, SA_LW_DEC_BB_W, SA_LW_DEC_BB_B, SA_LW_DEC_INVFREQ, SA_LW_DEC_ZERO_BIAS, SA_LW_EMB_TABLES, SA_LW_GLOBALS = SA_LW_EMB_TABLES + 17 };
enum { SA_LS_SINCOS = 0, SA_LS_MERGE_NORM_W, SA_LS_MERGE_NORM_B, SA_LS_MERGE_RED_W, SA_LS_COUNT };
enum { SA_LB_LN1_W = 0, SA_LB_LN1_B, SA_LB_QKV_W, SA_LB_QKV_B, SA_LB_RELBIAS, SA_LB_PROJ_W, SA_LB_PROJ_B, SA_LB_LN2_W, SA_LB_LN2_B, SA_LB_FC1_W,
       SA_LB_FC1_B, SA_LB_FC2_W, SA_LB_FC2_B, SA_LB_COUNT };
enum { SA_LD_CNORM = 0, SA_LD_CQ_W, SA_LD_CKV_W, SA_LD_CO_W, SA_LD_CO_B, SA_LD_TNORM, SA_LD_QKV_W, SA_LD_TO_W, SA_LD_TO_B, SA_LD_MNORM, SA_LD_GU_W,
       SA_LD_DOWN_W, SA_LD_COUNT };

typedef struct surya_layout surya_layout;
int surya_layout_create(const surya_layout_config* cfg, const void* const* weights, int n_weights, surya_layout** out);
int surya_layout_destroy(surya_layout* h);
/* pixel_values: device fp32 [batch, 3, img_h, img_w] (rescaled + normalised by the processor). Runs the encoder, keeps its output
 * inside the handle and projects every decoder layer's cross-attention keys / values; resets the self-attention caches. Enqueue only. */
int surya_layout_encode(surya_layout* h, const float* pixel_values, int batch, void* stream);
/* One decoder token per image at cache position `position` (0 = the start token): boxes host int32 [batch][7] = (cx, cy, w, h, xskew,
 * yskew, label) as the reference feeds them back (table family: [batch][10] = bbox 6, category, merges, colspan, is_header -- a prompt of
 * T tokens is T calls, which is what a causal prefill computes); class_logits host fp32 [batch][label_count], bbox host fp32 [batch][6] (after the
 * sigmoid). Synchronises the stream (the reference moves both to the host after every step as well). */
int surya_layout_decode_step(surya_layout* h, const int32_t* boxes, int batch, int position, float* class_logits, float* bbox, void* stream);
/* A decoder PROMPT of n_tokens (<= 64) tokens per row in one pass -- the reference's first decoder call, prefill = True
 * (surya/table_rec/__init__.py:60-68; the layout prompt is a single token) -- at positions 0 .. n_tokens - 1; boxes host int32
 * [batch][n_tokens][token width]; outputs as surya_layout_decode_step, for every row's LAST prompt token; the following decode steps
 * continue at position n_tokens. Equivalent to n_tokens decode steps (a causal prefill is the same arithmetic); SA_ERR_ARG when the prompt
 * does not fit the borrowed encoder workspaces -- callers then take the step-by-step route. Synchronises the stream. */
int surya_layout_prefill(surya_layout* h, const int32_t* boxes, int batch, int n_tokens, float* class_logits, float* bbox, void* stream);
/* Device-fed decode steps (round 4). The reference's box loop moves every step's outputs to the host, forms the next token there and sends
 * it back (surya/layout/__init__.py:110-177; surya/table_rec/__init__.py:57-129). Here the heads kernel forms that token itself --
 *   layout: (trunc(bbox * bbox_size) x 6, argmax class), a PageHeader / PageFooter whose polygon (surya/layout/util.py:4-40, float64)
 *           lies in the middle of its page takes the next-best class (__init__.py:158-169);
 *   table:  (trunc(clamp(bbox * bbox_size, 0, bbox_size)) x 6, argmax category, argmax merges, round(max(colspan, 1)), argmax is_header)
 *           = LabelShaper.dict_to_labels of the step's predictions (table_rec/shaper.py:12-51) --
 * embeds it and runs on; the host reads n_steps steps of records at a time and re-derives the tokens as a check.
 *   surya_layout_set_feedback: the constants of the rule (per model) and, for the layout family, the (width, height) of every row's page
 *     slice (host int32 [batch][2]; NULL = rule off). Call after surya_layout_encode / surya_layout_select, before the first run.
 *   surya_layout_decode_steps: enqueue n_steps (<= 16) steps at cache positions position .. position + n_steps - 1 into record ring
 *     `ring` (0 / 1). boxes = host int32 [batch][token width] feeds the first step from the host; NULL continues from the token the
 *     previous run left on the device (its position must be this run's `position`, else SA_ERR_STATE). Enqueue only.
 *   surya_layout_wait_steps: wait for ring `ring` and copy its records: class_logits fp32 [n_steps][batch][label_count], bbox fp32
 *     [n_steps][batch][6], fed_tokens int32 [n_steps][batch][token width] (the token each step fed to the one after it). */
typedef struct surya_layout_feedback {
    int32_t skew_scaler;              /* layout: decoder.skew_scaler (512) */
    int32_t relabel_ids[2];           /* layout: class ids (with the special-token offset) of PageHeader / PageFooter; -1 = none */
    int32_t head_widths[4];           /* table: rows of the category | merges | colspan | is_header heads (their sum = label_count) */
    const int32_t* page_sizes;        /* layout: host [batch][2] = (width, height) of each slice, NULL = no header / footer rule */
} surya_layout_feedback;
int surya_layout_set_feedback(surya_layout* h, const surya_layout_feedback* fb, int batch, void* stream);
int surya_layout_decode_steps(surya_layout* h, const int32_t* boxes, int batch, int position, int n_steps, int ring, void* stream);
int surya_layout_wait_steps(surya_layout* h, int ring, int batch, int n_steps, float* class_logits, float* bbox, int32_t* fed_tokens);
/* Re-batch the decoder after surya_layout_encode: the following decode steps run n rows (n <= max_batch), row i cross-attending the
 * encoder states of image src_index[i] (host array, values < the encoded batch). Table recognition decodes the cells of every detected
 * ROW against its table image (surya/table_rec/__init__.py:196-230: row_encoder_hidden_states = stacked copies); here the copies are an
 * index. Synchronous. */
int surya_layout_select(surya_layout* h, const int32_t* src_index, int n);
/* Test hook: encoder output [batch * tokens, hidden] of the last encode (device, compute dtype). */
int surya_layout_encoder_states(surya_layout* h, void* out, int batch, void* stream);
/* Page pre-processing of the layout family on the device (no handle): uint8 pages -> the pixel_values surya_layout_encode reads.
 * Replaces, per image, the PIL crop of a slicer strip (surya/layout/slicer.py) and SuryaEncoderImageProcessor (surya/common/donut/
 * processor.py:24-126: cv2.resize to the model size with flag 2 = INTER_CUBIC, uint8 result, x * 1/255 in fp64, (x - mean) / std in
 * fp32), bit-identical to the host restatement (surya_amd/layout/predictor.py LayoutImageProcessor).
 *   pages        device uint8, every page HWC at its descriptor's byte offset, pixel_stride bytes per pixel: 3 (RGB) or 4 (RGBX,
 *                the fourth byte ignored); pages_bytes = the size of that buffer (every page must lie inside it)
 *   descs        HOST array of n descriptors, one per output image
 *                { int64 page_off; int32 page_w, page_h; int32 x0, y0, cw, ch (crop rectangle inside the page, >= 1 px) } -- 32 bytes
 *   mean, std    host fp32 [3]
 *   pixel_values device fp32 [n][3][out_h][out_w], written in place
 * SA_ERR_ARG for a NULL pointer, n < 0 or another pixel_stride; SA_ERR_SHAPE for a crop outside its page, a page outside
 * pages_bytes or an empty output size. Enqueue only (the descriptors are read before the call returns). */
int surya_layout_preprocess(const uint8_t* pages, size_t pages_bytes, const void* descs, int n, int pixel_stride, const float* mean,
                            const float* std, int out_h, int out_w, float* pixel_values, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * OCR-error classifier: DistilBERT encoder (post-LayerNorm) + sequence-classification head.
 * Replaces DistilBertForSequenceClassification.forward (surya/ocr_error/model/encoder.py:720-764) as
 * OCRErrorPredictor calls it (surya/ocr_error/__init__.py:19-63). The texts of one call are PACKED: ids holds the
 * sum of text_len tokens back to back ([CLS] ... [SEP] each) and no padded row is computed; a text's logits do not
 * depend on its batch mates (the reference masks padded keys with zero softmax weight and reads only the [CLS] row).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct surya_ocrerr_config {
    int32_t vocab, max_pos, dim, heads, hidden, layers, num_labels;
    float ln_eps;                        /* 1e-12 (encoder.py:54, :417, :420) */
    int32_t max_texts, max_tokens;       /* per forward: texts and packed tokens */
    int32_t dtype;
} surya_ocrerr_config;
/* Weight table: SA_OW_* globals, then SA_OL_COUNT entries per layer. Every entry is in the compute dtype. WORD [vocab][dim],
 * POS [max_pos][dim] (learned, or the sin-cos table built by the caller), PRE [dim][dim], CLS [num_labels][dim]; per layer QKV_W =
 * q_lin | k_lin | v_lin rows fused [3 dim][dim] (q rows and bias already multiplied by 1 / sqrt(head_dim) when that is a power of two and
 * the dtype is fp32 or bf16, see SA_OCRERR_Q_PRESCALED; an fp16 table carries the reference's q rows as they are), OUT [dim][dim], LIN1 [hidden][dim], LIN2 [dim][hidden], LN weights / biases [dim]. */
enum { SA_OW_WORD = 0, SA_OW_POS, SA_OW_EMB_LN_W, SA_OW_EMB_LN_B, SA_OW_PRE_W, SA_OW_PRE_B, SA_OW_CLS_W, SA_OW_CLS_B, SA_OW_GLOBALS };
enum { SA_OL_QKV_W = 0, SA_OL_QKV_B, SA_OL_OUT_W, SA_OL_OUT_B, SA_OL_SA_LN_W, SA_OL_SA_LN_B, SA_OL_LIN1_W, SA_OL_LIN1_B, SA_OL_LIN2_W,
       SA_OL_LIN2_B, SA_OL_OUT_LN_W, SA_OL_OUT_LN_B, SA_OL_COUNT };
/* head_dim 64 in fp32 / bf16: the caller folds the 1 / 8 into the q rows (exact: a power of two, and neither format has a subnormal
 * range a weight reaches). fp16 never folds: a q weight below 8 x 2^-14 = 4.9e-4 would become subnormal and lose significand bits.
 * Unfolded tables (fp16, other head dims) have the engine pass 1 / sqrt(head_dim) to attention, which applies it to the fp32 scores. */
#define SA_OCRERR_Q_PRESCALED(head_dim, dtype) ((head_dim) == 64 && (dtype) != SA_DTYPE_F16)

typedef struct surya_ocrerr surya_ocrerr;
int surya_ocrerr_create(const surya_ocrerr_config* cfg, const void* const* weights, int n_weights, surya_ocrerr** out);
int surya_ocrerr_destroy(surya_ocrerr* h);
/* ids: device int32 [sum text_len] packed token ids; text_len: HOST int32 [n_texts], each in 1 .. max_pos; logits: device fp32
 * [n_texts][num_labels] (rounded to the compute dtype, as the reference's logits are); labels: device int32 [n_texts] (first argmax).
 * Enqueue only (the host arrays are staged before the call returns). */
int surya_ocrerr_forward(surya_ocrerr* h, const int32_t* ids, const int32_t* text_len, int n_texts, float* logits, int32_t* labels,
                         void* stream);
/* The classifier's kernels by themselves (tests/test_gpu_ocr_ops.py), each through the launcher the engine uses (csrc/ocr_error_kernels.h).
 * dtype = SA_DTYPE_F32 / BF16 / F16 (the storage type of every `void*` operand). Device pointers are the caller's; a NULL pointer or a
 * size <= 0 returns SA_ERR_ARG, a size the kernel's vector accesses cannot take (C % 4, head_dim % 8, K not in whole 128-byte chunks)
 * SA_ERR_SHAPE, before anything is launched. Enqueue only, except cls_attn.
 *   embed_ln:    y[r] = LayerNorm(T(word[clamp(ids[r], 0, vocab - 1)] + pos[tok_pos[r]])) over C channels (tok_pos is NOT clamped).
 *   layernorm:   y[r] = LayerNorm(x[r]), fp32 two-pass statistics, eps inside the square root.
 *   gather_rows: out[i] = x[rows_idx[i]], rows of C elements.
 *   cls_attn:    cls_attn_kernel<T, head_dim>: out[t] [dim] = attention of ONE query, row host_starts[t] of the packed qkv rows [.][3 dim]
 *                (q | k | v, head h at columns h * head_dim), over the host_lens[t] rows from there; the LDS is sized for max_len. The two
 *                HOST arrays are copied by the call, which returns after the kernel ran. bf16 and fp16 only (fp32: SA_ERR_UNSUPPORTED);
 *                head_dim in {32, 64, 80, 128}, max_len <= 4096 and the LDS within 64 KB, else SA_ERR_UNSUPPORTED; dim != heads *
 *                head_dim, a start < 0 or a length outside 1 .. max_len: SA_ERR_SHAPE.
 *   cls_head:    logits[t][j] = T(pre[t] . w[j] + b[j]) as fp32, labels[t] = the first argmax (a NaN never wins; all NaN: 0).
 *   gemm:        OcrErrModel's GEMM: C [M][N] = epi(X W^T + bias), X rows ldx elements apart, W [N][K], bias [N], R [M][N]; epi 0 bias,
 *                1 residual (T(T(X W^T + bias) + R), R required), 2 erf GELU, 5 ReLU, others SA_ERR_UNSUPPORTED. pinned = 1: the 64 x 64
 *                tile of the [CLS]-row GEMMs whatever M; 0: launch_gemm's choice. */
int surya_op_ocrerr_embed_ln(int dtype, const int32_t* ids, const int32_t* tok_pos, const void* word, const void* pos, const void* w, const void* b,
                             void* y, int rows, int C, int vocab, float eps, void* stream);
int surya_op_ocrerr_layernorm(int dtype, const void* x, const void* w, const void* b, void* y, int rows, int C, float eps, void* stream);
int surya_op_ocrerr_gather_rows(int dtype, const void* x, const int32_t* rows_idx, void* out, int n, int C, void* stream);
int surya_op_ocrerr_cls_attn(int dtype, int head_dim, const void* qkv, const int32_t* host_starts, const int32_t* host_lens, int n, void* out,
                             int dim, int heads, int max_len, float scale, void* stream);
int surya_op_ocrerr_cls_head(int dtype, const void* pre, const void* w, const void* b, float* logits, int32_t* labels, int n, int dim,
                             int num_labels, void* stream);
int surya_op_ocrerr_gemm(int dtype, int epi, int pinned, const void* X, long ldx, const void* W, const void* bias, void* C, const void* R, int M,
                         int N, int K, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Measurement support (bench.py `roofline`): when enabled every GEMM launch is bracketed by hipEvents on its own
 * stream. surya_prof_read syncs the device and returns, per bucket (0: 128x128 GEMM, 1: tall 256-row GEMM tiles, 2: smaller GEMM tiles,
 * 3: implicit-GEMM convolutions),
 * the number of launches, the summed event time (ms) and the summed ALGORITHMIC flops / bytes
 * (2MNK; X + W + C (+R) once each). Arrays need >= 4 entries; a reader that passes 6 also gets beam search's two launches (4: the selection,
 * 5: the KV fork; launches and time only). Not for use inside timed regions.
 * ---------------------------------------------------------------------------------------------------------- */
int surya_prof_enable(int on);
/* Launch-policy knob for A/B measurements inside one process (tools/microbench/decode_sweep.py; keys = the fields of
 * sa::Tuning in csrc/common.h: "graph", "split_target", "bigtile", "persist", "lmhead", "dattn", ...). Process-wide; results never depend on it
 * beyond fp rounding order. Returns SA_ERR_ARG for an unknown key. */
int surya_set_tuning(const char* key, int value);
/* Synchronous check of the decode GEMM ring's give-up word (csrc/gemm_ring.h): SA_OK while every ring wait of this library's recognition
 * launches was satisfied, SA_ERR_STATE once one gave up (its launch's numbers are then wrong); reset != 0 clears the word. */
int surya_gemm_ring_status(int reset);
int surya_prof_read(int max_cfg, int* launches, double* ms, double* flops, double* bytes);
/* surya_prof_read + slab_bytes[]: the fp32 partial slabs split-K launches wrote (a by-product of the kernel's own decomposition,
 * NOT part of `bytes`: `bytes` counts the result once in the storage type, as an unsplit GEMM would write it). slab_bytes may be NULL. */
int surya_prof_read2(int max_cfg, int* launches, double* ms, double* flops, double* bytes, double* slab_bytes);
/* Median event-pair time (ms) around an empty kernel on `stream`: the fixed cost inside every per-launch figure above. */
int surya_prof_event_overhead(void* stream, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* SURYA_AMD_H */
