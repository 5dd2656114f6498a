// Recognition model on MI355X: host-side planning (window order, segments, slot bookkeeping) + kernel
// sequencing behind the C ABI of include/surya_amd.h.
//
// Design (vs the reference's PyTorch path):
//   * the packed patch sequence is permuted into window order while it is converted to the compute dtype, so
//     `hidden_states[window_index]` (encoder/__init__.py:626) never runs as a separate gather;
//   * prompts are PACKED (no left padding): positions come from per-token (slot, pos), not from a 2-D mask;
//   * the KV cache is slot based, [layer][slot][kv_head][T_max][d], with a per-slot length on the device:
//     ContinuousBatchingCache.merge / pad_left / trim_left (recognition/cache.py:8-105) have no equivalent data
//     movement -- admitting a prompt writes its K/V rows straight into a free slot;
//   * the greedy head keeps next-token / length state on the device, so n decode steps need no host round trip.
// The engine itself, RecModel<T>, is rec_engine.h: this file instantiates it for float and bf16_t, rec_model_f16.hip for fp16_t.
#include "rec_engine.h"
#include "rec_ops.h"
#include "rec_prep.h"
#include "rec_rectify.h"
#include "rec_unroll.h"
#include "page_warp.h"
#include "rec_adjust.h"

namespace sa {

// --------------------------------------------------------------------------------- decode attention launch
// launch_decode_attn (decode_attn.h): every decode-attention launch of the library -- RecModel::decode_layer, LayoutModel::decode_layers
// and surya_op_decode_attn -- is this one, so a kernel tested through the hook is launched exactly as the engines launch it.
template <int D, int MAXG>
static int decode_attn_flash(const DecodeAttnArgs<bf16_t>& a, hipStream_t s) {
    const Tuning& t = tuning();
    if (t.dattn == 3) return decode_attn_as<decode_attn_flash_kernel<D, MAXG>>(a, decode_attn_flash_lds<D, MAXG>(), s, a.out8, a.sout, a.srows);
    // two tile buffers once some row's context exceeds one 128-key tile (Tuning::dattn_db); one workgroup per CU either way
    if (t.dattn_db == 1 || (t.dattn_db == 0 && !t.graph && a.ctx_bound > 128 && a.rows * a.nkv <= 256))
        return decode_attn_as<decode_attn_flash2_kernel<D, MAXG, true>>(a, decode_attn_flash2_lds<D, MAXG, true>(), s, a.out8, a.sout, a.srows);
    return decode_attn_as<decode_attn_flash2_kernel<D, MAXG, false>>(a, decode_attn_flash2_lds<D, MAXG, false>(), s, a.out8, a.sout, a.srows);
}
template <typename T>
int launch_decode_attn(const DecodeAttnArgs<T>& a, hipStream_t s) {
    const int G = a.nq / a.nkv, d = a.d;                     // G <= MAXG on every rung: MAXG sizes the kernels' LDS arrays
    if constexpr (std::is_same<T, bf16_t>::value) {          // bf16: per-wave flash kernels
        if (d == 128 && G <= 5) return decode_attn_flash<128, 5>(a, s);
        if (d == 128 && G <= 8) return decode_attn_flash<128, 8>(a, s);
        if (d == 64 && G <= 8) return decode_attn_flash<64, 8>(a, s);
        if (d == 32 && G <= 8) return decode_attn_flash<32, 8>(a, s);
    }
    if (a.out8) return SA_ERR_UNSUPPORTED;                   // only the flash kernels write the MXFP8 copy of their output
    // fp32 reference mode, and bf16 head shapes the flash ladder lacks (today the two ladders cover the same shapes)
    if (d == 128 && G <= 5) return decode_attn_as<decode_attn_mfma_kernel<T, 128, 5>>(a, decode_attn_mfma_lds<T, 128, 5>(), s);
    if (d == 128 && G <= 8) return decode_attn_as<decode_attn_mfma_kernel<T, 128, 8>>(a, decode_attn_mfma_lds<T, 128, 8>(), s);
    if (d == 64 && G <= 8) return decode_attn_as<decode_attn_mfma_kernel<T, 64, 8>>(a, decode_attn_mfma_lds<T, 64, 8>(), s);
    if (d == 32 && G <= 8) return decode_attn_as<decode_attn_mfma_kernel<T, 32, 8>>(a, decode_attn_mfma_lds<T, 32, 8>(), s);
    return SA_ERR_UNSUPPORTED;
}
template int launch_decode_attn<float>(const DecodeAttnArgs<float>&, hipStream_t);
template int launch_decode_attn<bf16_t>(const DecodeAttnArgs<bf16_t>&, hipStream_t);

static int check_cfg(const surya_rec_config* c) {
    if (!c) return SA_ERR_ARG;
    if (c->dtype != SA_DTYPE_F32 && c->dtype != SA_DTYPE_BF16 && c->dtype != SA_DTYPE_F16) return SA_ERR_UNSUPPORTED;
    if (c->enc_hidden % 64 || c->enc_inter_pad % 64 || c->patch_dim_pad % 64 || c->dec_hidden % 64 || c->dec_inter % 64 ||
        (c->dec_heads * c->dec_head_dim) % 64 || c->vocab % 4)
        return SA_ERR_SHAPE;
    if (c->enc_hidden % c->enc_heads || c->dec_heads % c->dec_kv_heads || c->dec_heads / c->dec_kv_heads > 8) return SA_ERR_SHAPE;
    if (c->merge != 2 || c->window_tokens <= 0 || c->enc_depth > 32) return SA_ERR_UNSUPPORTED;
    if (c->max_slots <= 0 || c->max_kv_len <= 0 || c->max_patches < 4 || c->max_prefill_tokens <= 0) return SA_ERR_ARG;
    return SA_OK;
}

}  // namespace sa

using namespace sa;
struct surya_rec { std::unique_ptr<RecBase> impl; surya_rec_config cfg; };

// ------------------------------------------------------------------------------------------------ op level
namespace sa {
// rec_model_f16.hip: RecModel<fp16_t>
size_t rec_f16_workspace_bytes(const surya_rec_config& cfg);
int rec_f16_create(const surya_rec_config& cfg, const void* const* weights, int n, std::unique_ptr<RecBase>& out);
int rec_f16_ring_error(bool reset);
int op_lm_head_f16(const void* X, const void* W, const void* bias, int M, int N, int K, const TokenMask* tm, float4* amax, float2* alt, int* bn_used,
                   hipStream_t s, const ForcedCols* fc = nullptr);
int op_gemm_rope_f16(const void* X, long ldx, const void* W, long ldw, void* C, long ldc, const void* bias, const float* rope, int rope_cols,
                     int rope_D, int M, int N, int K, hipStream_t s);
// det_model.hip: the fp16 GEMMs of surya_op_gemm
int op_gemm_f16(int epi, const void* X, long ldx, const void* W, long ldw, void* C, long ldc, const void* bias, const void* R, long ldr,
                int M, int N, int K, hipStream_t s);
// ocr_error_model.hip: the fp16 GELU epilogue and fp16 segment attention of the OCR-error classifier
int op_gemm_f16_gelu(const void* X, long ldx, const void* W, long ldw, void* C, long ldc, const void* bias, int M, int N, int K, hipStream_t s);
int op_attn_f16(int D, const void* q, const void* k, const void* v, void* o, const AttnSegs& sg, int n_tiles, int heads, long q_row, long q_head,
                long k_row, long k_head, long o_row, long o_head, int group, int causal, float scale, hipStream_t s);
// layout_model.hip: the ADETR MLP's gated epilogue (gelu_tanh(gate) * up), fp32 and bf16
int op_gemm_geglu(int dtype, const void* X, long ldx, const void* W, long ldw, void* C, long ldc, int M, int N, int K, hipStream_t s);
}
template <typename TI, typename TO>
static int op_gemm_t(int epi, const void* X, long ldx, const void* W, long ldw, void* C, long ldc, const void* bias, const void* R,
                     long ldr, int M, int N, int K, hipStream_t s) {
    GemmArgs<TI, TO> a{(const TI*)X, ldx, (const TI*)W, ldw, (TO*)C, ldc, (const TI*)bias, (const TO*)R, ldr, M, N, K};
    switch (epi) {
        case EPI_BIAS: return launch_gemm<TI, TO, EPI_BIAS>(a, s);
        case EPI_RESIDUAL: return R ? launch_gemm<TI, TO, EPI_RESIDUAL>(a, s) : SA_ERR_ARG;
        case EPI_GELU: return launch_gemm<TI, TO, EPI_GELU>(a, s);
        case EPI_SWIGLU: return launch_gemm<TI, TO, EPI_SWIGLU>(a, s);
        case EPI_HARDSWISH: return launch_gemm<TI, TO, EPI_HARDSWISH>(a, s);
        case EPI_RELU: return launch_gemm<TI, TO, EPI_RELU>(a, s);
    }
    return SA_ERR_ARG;
}

// surya_op_gemm_rope: the vision qkv projection by itself, GemmArgs filled as RecModel<T>::encode fills them (rec_engine.h)
template <typename T>
static int op_gemm_rope_t(const void* X, long ldx, const void* W, long ldw, void* C, long ldc, const void* bias, const float* rope, int rope_cols,
                          int rope_D, int M, int N, int K, hipStream_t s) {
    GemmArgs<T, T> a{(const T*)X, ldx, (const T*)W, ldw, (T*)C, ldc, (const T*)bias, nullptr, 0, M, N, K};
    a.rope = reinterpret_cast<const float2*>(rope); a.rope_cols = rope_cols; a.rope_D = rope_D;
    return launch_gemm<T, T, EPI_ROPE>(a, s);
}

// surya_op_lm_head_partials: the lm_head launch of RecModel<T>::heads for the 16-bit / fp32 operand types built here
template <typename T>
static int op_lm_head_t(const void* X, const void* W, const void* bias, int M, int N, int K, const TokenMask* tm, float4* amax, float2* alt,
                        int* bn_used, hipStream_t s, const ForcedCols* fc = nullptr) {
    GemmArgs<T, float> a{(const T*)X, (long)K, (const T*)W, (long)K, nullptr, (long)N, (const T*)bias, nullptr, 0, M, N, K};
    a.amax = amax;
    int rc;
    if (fc) {                       // surya_op_lm_head_forced
        a.forced = *fc;
        rc = launch_gemm<T, float, EPI_FORCED>(a, s);
    } else if (alt) {                      // surya_op_lm_head_topk: one kernel with or without a table
        if (tm) a.tmask = *tm;
        a.alt = alt;
        rc = launch_gemm<T, float, EPI_TOPK>(a, s);
    } else if (tm) {
        a.tmask = *tm;
        rc = launch_gemm<T, float, EPI_ARGMAX_MASK>(a, s);
    } else {
        rc = launch_gemm<T, float, EPI_ARGMAX>(a, s);
    }
    *bn_used = a.bn_used;
    return rc;
}


extern "C" {

const char* surya_amd_version(void) { return "surya_amd 0.1.0 gfx950"; }

size_t surya_rec_workspace_bytes(const surya_rec_config* cfg) {
    if (check_cfg(cfg)) return 0;
    if (cfg->dtype == SA_DTYPE_F16) return sa::rec_f16_workspace_bytes(*cfg);
    return cfg->dtype == SA_DTYPE_F32 ? RecModel<float>::layout(*cfg, nullptr) : RecModel<bf16_t>::layout(*cfg, nullptr);
}

int surya_rec_create(const surya_rec_config* cfg, const void* const* weights, int n_weights, surya_rec** out) {
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if (!weights || !out || n_weights != SA_RW_TOTAL(cfg->enc_depth, cfg->dec_layers)) return SA_ERR_ARG;
    for (int i = 0; i < n_weights; ++i)
        if (!weights[i]) return SA_ERR_ARG;
    auto* h = new surya_rec();
    h->cfg = *cfg;
    if (cfg->dtype == SA_DTYPE_F32) {
        auto m = std::make_unique<RecModel<float>>();
        rc = m->init(*cfg, weights, n_weights);
        h->impl = std::move(m);
    } else if (cfg->dtype == SA_DTYPE_F16) {
        rc = sa::rec_f16_create(*cfg, weights, n_weights, h->impl);
    } else {
        auto m = std::make_unique<RecModel<bf16_t>>();
        rc = m->init(*cfg, weights, n_weights);
        h->impl = std::move(m);
    }
    if (rc) { delete h; return rc; }
    *out = h;
    return SA_OK;
}

int surya_rec_destroy(surya_rec* h) {
    if (!h) return SA_ERR_ARG;
    (void)hipDeviceSynchronize();
    delete h;
    return SA_OK;
}

int surya_rec_plan_encoder(const surya_rec_config* cfg, const int32_t* grid_hw, int n_images, int32_t* src_row, int32_t* pos_hw,
                           int32_t* cu_window, int32_t* n_windows, int32_t* merged_src) {
    if (!cfg || !grid_hw || n_images <= 0) return SA_ERR_ARG;
    EncPlan pl;
    int rc = plan_encoder(*cfg, grid_hw, n_images, pl);
    if (rc) return rc;
    if (src_row) memcpy(src_row, pl.src_row.data(), pl.src_row.size() * sizeof(int));
    if (pos_hw) memcpy(pos_hw, pl.pos_hw.data(), pl.pos_hw.size() * sizeof(int));
    if (cu_window) memcpy(cu_window, pl.win_cu.data(), pl.win_cu.size() * sizeof(int));
    if (n_windows) *n_windows = (int)pl.win_cu.size() - 1;
    if (merged_src) memcpy(merged_src, pl.merged_src.data(), pl.merged_src.size() * sizeof(int));
    return SA_OK;
}

int surya_rec_prefill(surya_rec* h, const float* tiles, const int32_t* grid_hw, int n_images, const int32_t* input_ids,
                      const int32_t* seq_offsets, const int32_t* slot_ids, int n_seqs, void* stream) {
    if (!h || !input_ids || !seq_offsets || !slot_ids || (n_images > 0 && !grid_hw)) return SA_ERR_ARG;   // tiles == NULL: look-ahead mode
    return h->impl->prefill(tiles, grid_hw, n_images, input_ids, seq_offsets, slot_ids, n_seqs, (hipStream_t)stream);
}
int surya_rec_prefill_shared(surya_rec* h, const float* tiles, const int32_t* grid_hw, int n_images, const int32_t* input_ids,
                             const int32_t* seq_offsets, const int32_t* fan_offsets, const int32_t* fan_slots, int n_seqs, void* stream) {
    if (!h || !input_ids || !seq_offsets || !fan_offsets || !fan_slots || (n_images > 0 && !grid_hw)) return SA_ERR_ARG;
    return h->impl->prefill_shared(tiles, grid_hw, n_images, input_ids, seq_offsets, fan_offsets, fan_slots, n_seqs, (hipStream_t)stream);
}
int surya_rec_copy_kv_rows(surya_rec* h, int slot, int rows, void* k_out, void* v_out, void* stream) {
    if (!h) return SA_ERR_ARG;
    return h->impl->copy_kv_rows(slot, rows, k_out, v_out, (hipStream_t)stream);
}
int surya_rec_reserve_prompts(surya_rec* h, int rows, void* stream) {
    if (!h) return SA_ERR_ARG;
    return h->impl->reserve_prompts(rows, (hipStream_t)stream);
}
int surya_rec_prefill_keep(surya_rec* h, const float* tiles, const int32_t* grid_hw, int n_images, const int32_t* input_ids,
                           const int32_t* seq_offsets, const int32_t* slot_ids, int n_seqs, const int32_t* keep_first, void* stream) {
    if (!h || !input_ids || !seq_offsets || !slot_ids || !keep_first || (n_images > 0 && !grid_hw)) return SA_ERR_ARG;
    return h->impl->prefill_keep(tiles, grid_hw, n_images, input_ids, seq_offsets, slot_ids, n_seqs, keep_first, (hipStream_t)stream);
}
int surya_rec_restore(surya_rec* h, const int32_t* first, const int32_t* fan_offsets, const int32_t* fan_slots, int n, void* stream) {
    if (!h || (n > 0 && (!first || !fan_offsets || !fan_slots))) return SA_ERR_ARG;
    return h->impl->restore(first, fan_offsets, fan_slots, n, (hipStream_t)stream);
}
int surya_rec_drop_prompts(surya_rec* h, const int32_t* first, int n) {
    if (!h || n < 0 || (n > 0 && !first)) return SA_ERR_ARG;
    return h->impl->drop_prompts(first, n);
}
int surya_rec_prompt_store_info(surya_rec* h, int32_t* cap_rows, int32_t* live_entries) {
    if (!h || !cap_rows || !live_entries) return SA_ERR_ARG;
    return h->impl->prompt_store_info(cap_rows, live_entries);
}
int surya_rec_encode_ahead(surya_rec* h, const float* tiles, const int32_t* grid_hw, int n_images, void* stream) {
    if (!h || n_images < 0 || (n_images > 0 && (!tiles || !grid_hw))) return SA_ERR_ARG;      // n_images == 0: discard (see the header)
    return h->impl->encode_ahead(tiles, grid_hw, n_images, (hipStream_t)stream);
}
int surya_rec_set_active(surya_rec* h, const int32_t* slots, int n_active, void* stream) {
    if (!h || (n_active > 0 && !slots)) return SA_ERR_ARG;
    return h->impl->set_active(slots, n_active, (hipStream_t)stream);
}
int surya_rec_decode(surya_rec* h, int n_steps, void* stream) {
    if (!h) return SA_ERR_ARG;
    return h->impl->decode(n_steps, (hipStream_t)stream);
}
int surya_rec_read_outputs(surya_rec* h, int n_steps, int32_t* tokens, float* scores, int32_t* bboxes, void* stream) {
    if (!h || !tokens || !scores || !bboxes) return SA_ERR_ARG;
    return h->impl->read_steps(STEPS_BASE, n_steps, {tokens, scores, bboxes}, (hipStream_t)stream);
}
int surya_rec_decode_async(surya_rec* h, int n_steps, int ring, void* stream) {
    if (!h) return SA_ERR_ARG;
    return h->impl->decode_async(n_steps, ring, (hipStream_t)stream);
}
int surya_rec_wait_outputs(surya_rec* h, int n_steps, int ring, int32_t* tokens, float* scores, int32_t* bboxes) {
    if (!h || !tokens || !scores || !bboxes) return SA_ERR_ARG;
    return h->impl->wait_steps(STEPS_BASE, n_steps, ring, {tokens, scores, bboxes});
}
int surya_rec_encode_only(surya_rec* h, const float* tiles, const int32_t* grid_hw, int n_images, void* out, void* stream) {
    if (!h || !tiles || !grid_hw || !out || n_images <= 0) return SA_ERR_ARG;
    return h->impl->encode_only(tiles, grid_hw, n_images, out, (hipStream_t)stream);
}
int surya_rec_copy_last_logits(surya_rec* h, float* dst, int max_rows, int* rows, void* stream) {
    if (!h || !dst || !rows || max_rows <= 0) return SA_ERR_ARG;
    return h->impl->copy_last_logits(dst, max_rows, rows, (hipStream_t)stream);
}
int surya_rec_set_next_tokens(surya_rec* h, const int32_t* slots, const int32_t* tokens, int n, void* stream) {
    if (!h || !slots || !tokens) return SA_ERR_ARG;
    return h->impl->set_next_tokens(slots, tokens, n, (hipStream_t)stream);
}

int surya_rec_set_mx_weights(surya_rec* h, const void* const* table, int n) {
    if (!h) return SA_ERR_ARG;
    return h->impl->set_mx_weights(table, n);
}

int surya_rec_set_kv_fp8(surya_rec* h, int on) {
    if (!h) return SA_ERR_ARG;
    return h->impl->set_kv_fp8(on);
}

int surya_rec_set_token_masks(surya_rec* h, const uint32_t* masks, int n_masks, void* stream) {
    if (!h) return SA_ERR_ARG;
    return h->impl->set_token_masks(masks, n_masks, (hipStream_t)stream);
}
int surya_rec_set_slot_masks(surya_rec* h, const int32_t* slots, const int32_t* mask_ids, int n, void* stream) {
    if (!h || (n > 0 && (!slots || !mask_ids))) return SA_ERR_ARG;
    return h->impl->set_slot_masks(slots, mask_ids, n, (hipStream_t)stream);
}

int surya_rec_set_alternatives(surya_rec* h, int on) {
    if (!h) return SA_ERR_ARG;
    return h->impl->set_alternatives(on);
}
int surya_rec_read_alternatives(surya_rec* h, int n_steps, int32_t* tokens, float* probs, void* stream) {
    if (!h || !tokens || !probs) return SA_ERR_ARG;
    return h->impl->read_steps(STEPS_ALTS, n_steps, {tokens, probs}, (hipStream_t)stream);
}
int surya_rec_wait_alternatives(surya_rec* h, int n_steps, int ring, int32_t* tokens, float* probs) {
    if (!h || !tokens || !probs) return SA_ERR_ARG;
    return h->impl->wait_steps(STEPS_ALTS, n_steps, ring, {tokens, probs});
}

int surya_rec_set_forced(surya_rec* h, int on) {
    if (!h) return SA_ERR_ARG;
    return h->impl->set_forced(on);
}
int surya_rec_set_forced_tokens(surya_rec* h, const int32_t* slots, const int32_t* tokens, const int32_t* offsets, int n, void* stream) {
    if (!h || (n > 0 && (!slots || !offsets)) || (n > 0 && !tokens && offsets[n] != offsets[0])) return SA_ERR_ARG;
    return h->impl->set_forced_tokens(slots, tokens, offsets, n, (hipStream_t)stream);
}
int surya_rec_read_forced(surya_rec* h, int n_steps, int32_t* greedy_tokens, float* greedy_probs, float* forced_logprobs, void* stream) {
    if (!h || !greedy_tokens || !greedy_probs || !forced_logprobs) return SA_ERR_ARG;
    return h->impl->read_steps(STEPS_FORCED, n_steps, {greedy_tokens, greedy_probs, forced_logprobs}, (hipStream_t)stream);
}
int surya_rec_wait_forced(surya_rec* h, int n_steps, int ring, int32_t* greedy_tokens, float* greedy_probs, float* forced_logprobs) {
    if (!h || !greedy_tokens || !greedy_probs || !forced_logprobs) return SA_ERR_ARG;
    return h->impl->wait_steps(STEPS_FORCED, n_steps, ring, {greedy_tokens, greedy_probs, forced_logprobs});
}

int surya_rec_set_beam(surya_rec* h, int width, int no_output_token_id) {
    if (!h) return SA_ERR_ARG;
    return h->impl->set_beam(width, no_output_token_id);
}
int surya_rec_read_beam(surya_rec* h, int n_steps, int32_t* tokens, int32_t* parents, int32_t* ranks, float* probs, float* logps, void* stream) {
    if (!h || !tokens || !parents || !ranks || !probs || !logps) return SA_ERR_ARG;
    return h->impl->read_steps(STEPS_BEAM, n_steps, {tokens, parents, ranks, probs, logps}, (hipStream_t)stream);
}
int surya_rec_wait_beam(surya_rec* h, int n_steps, int ring, int32_t* tokens, int32_t* parents, int32_t* ranks, float* probs, float* logps) {
    if (!h || !tokens || !parents || !ranks || !probs || !logps) return SA_ERR_ARG;
    return h->impl->wait_steps(STEPS_BEAM, n_steps, ring, {tokens, parents, ranks, probs, logps});
}

int surya_rec_set_patterns(surya_rec* h, const uint8_t* tok_class, const uint16_t* next_state, const uint8_t* state_mask, int n_states,
                           int n_classes, void* stream) {
    if (!h) return SA_ERR_ARG;
    return h->impl->set_patterns(tok_class, next_state, state_mask, n_states, n_classes, (hipStream_t)stream);
}
int surya_rec_set_slot_patterns(surya_rec* h, const int32_t* slots, const int32_t* start_states, int n, void* stream) {
    if (!h || (n > 0 && (!slots || !start_states))) return SA_ERR_ARG;
    return h->impl->set_slot_patterns(slots, start_states, n, (hipStream_t)stream);
}
int surya_rec_copy_slot_states(surya_rec* h, int32_t* dst, void* stream) {
    if (!h || !dst) return SA_ERR_ARG;
    return h->impl->copy_slot_states(dst, (hipStream_t)stream);
}

int surya_rec_set_lexicon(surya_rec* h, const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next, const uint8_t* state_flags,
                          int n_states, int n_edges, int no_output_token_id, void* stream) {
    if (!h) return SA_ERR_ARG;
    return h->impl->set_lexicon(edge_off, edge_tok, edge_next, state_flags, n_states, n_edges, no_output_token_id, (hipStream_t)stream);
}
int surya_rec_set_slot_lexicon(surya_rec* h, const int32_t* slots, const int32_t* start_states, int n, void* stream) {
    if (!h || (n > 0 && (!slots || !start_states))) return SA_ERR_ARG;
    return h->impl->set_slot_lexicon(slots, start_states, n, (hipStream_t)stream);
}
int surya_rec_copy_lexicon_states(surya_rec* h, int32_t* dst, void* stream) {
    if (!h || !dst) return SA_ERR_ARG;
    return h->impl->copy_lexicon_states(dst, (hipStream_t)stream);
}

int surya_rec_set_boost(surya_rec* h, const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next, int n_states, int n_edges,
                        int out_state, int word_row, void* stream) {
    if (!h) return SA_ERR_ARG;
    return h->impl->set_boost(edge_off, edge_tok, edge_next, n_states, n_edges, out_state, word_row, (hipStream_t)stream);
}
int surya_rec_set_slot_boost(surya_rec* h, const int32_t* slots, const int32_t* roots, const float* betas, int n, void* stream) {
    if (!h || (n > 0 && (!slots || !roots || !betas))) return SA_ERR_ARG;
    return h->impl->set_slot_boost(slots, roots, betas, n, (hipStream_t)stream);
}
int surya_rec_copy_boost_states(surya_rec* h, int32_t* dst, void* stream) {
    if (!h || !dst) return SA_ERR_ARG;
    return h->impl->copy_boost_states(dst, (hipStream_t)stream);
}
int surya_rec_read_boost(surya_rec* h, int n_steps, int32_t* plain_tokens, float* plain_probs, void* stream) {
    if (!h || !plain_tokens || !plain_probs) return SA_ERR_ARG;
    return h->impl->read_steps(STEPS_BOOST, n_steps, {plain_tokens, plain_probs}, (hipStream_t)stream);
}
int surya_rec_wait_boost(surya_rec* h, int n_steps, int ring, int32_t* plain_tokens, float* plain_probs) {
    if (!h || !plain_tokens || !plain_probs) return SA_ERR_ARG;
    return h->impl->wait_steps(STEPS_BOOST, n_steps, ring, {plain_tokens, plain_probs});
}

// surya_op_lm_head_topk without a row -> slot map: the identity, for the head kernel (which always reads one)
static __global__ void iota_kernel(int* dst, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = i;
}

// surya_op_lm_head_partials (alt == nullptr) and the lm_head launch of surya_op_lm_head_topk
static int op_lm_head(int dtype, const void* X, const void* SX, const void* W, const void* SW, const void* bias, int M, int N, int K,
                      const uint32_t* masks, const int32_t* slot_mask, const int32_t* row_slot, float* amax, float2* alt, int* bn_used,
                      hipStream_t s, const ForcedCols* fc = nullptr) {
    if (!X || !W || !amax || !bn_used || M <= 0 || N <= 0 || K <= 0 || (masks && !slot_mask)) return SA_ERR_ARG;
    const TokenMask tm{masks, slot_mask, row_slot, cdiv(N, 32)};
    const TokenMask* tp = masks ? &tm : nullptr;
    float4* am = reinterpret_cast<float4*>(amax);
    if (dtype == SA_DTYPE_F32) return op_lm_head_t<float>(X, W, bias, M, N, K, tp, am, alt, bn_used, s, fc);
    if (dtype == SA_DTYPE_BF16) return op_lm_head_t<bf16_t>(X, W, bias, M, N, K, tp, am, alt, bn_used, s, fc);
    if (dtype == SA_DTYPE_F16) return sa::op_lm_head_f16(X, W, bias, M, N, K, tp, am, alt, bn_used, s, fc);
    if (dtype == SA_OP_MXFP8) {
        if (!SX || !SW) return SA_ERR_ARG;
        MxArgs a{(const uint8_t*)X, (long)K, (const uint8_t*)SX, (const uint8_t*)W, (long)K, (const uint8_t*)SW, M, N, K, (long)M, (long)N};
        a.amax = am;
        a.bias = (const bf16_t*)bias;
        int rc;
        if (fc) {
            a.forced = *fc;
            rc = launch_gemm_mx<MX_EPI_FORCED>(a, s);
        } else if (alt) {
            if (tp) a.tmask = tm;
            a.alt = alt;
            rc = launch_gemm_mx<MX_EPI_TOPK>(a, s);
        } else if (tp) {
            a.tmask = tm;
            rc = launch_gemm_mx<MX_EPI_ARGMAX_MASK>(a, s);
        } else {
            rc = launch_gemm_mx<MX_EPI_ARGMAX>(a, s);
        }
        *bn_used = a.bn_used;
        return rc;
    }
    return SA_ERR_UNSUPPORTED;
}

int surya_op_lm_head_partials(int dtype, const void* X, const void* SX, const void* W, const void* SW, const void* bias, int M, int N, int K,
                              const uint32_t* masks, const int32_t* slot_mask, const int32_t* row_slot, float* amax, int* bn_used, void* stream) {
    return op_lm_head(dtype, X, SX, W, SW, bias, M, N, K, masks, slot_mask, row_slot, amax, nullptr, bn_used, (hipStream_t)stream);
}

int surya_op_lm_head_forced(int dtype, const void* X, const void* SX, const void* W, const void* SW, const void* bias, int M, int N, int K,
                            const int32_t* forced_col, float* amax, float* flogit, int* bn_used, void* stream) {
    if (!forced_col || !flogit) return SA_ERR_ARG;
    const ForcedCols fc{forced_col, nullptr, nullptr, 1, flogit};       // one id per row, read at position 0
    return op_lm_head(dtype, X, SX, W, SW, bias, M, N, K, nullptr, nullptr, nullptr, amax, nullptr, bn_used, (hipStream_t)stream, &fc);
}

int surya_op_lm_head_topk(int dtype, const void* X, const void* SX, const void* W, const void* SW, const void* bias, int M, int N, int K,
                          const uint32_t* masks, const int32_t* slot_mask, const int32_t* row_slot, float* amax, float* alt, int* bn_used,
                          int32_t* top_tokens, float* top_probs, int32_t* head_token, float* head_score, float* scratch, void* stream) {
    if (!alt || (top_tokens != nullptr) != (top_probs != nullptr) || (top_tokens && (!head_token || !head_score || !scratch))) return SA_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    float2* al = reinterpret_cast<float2*>(alt);
    int rc = op_lm_head(dtype, X, SX, W, SW, bias, M, N, K, masks, slot_mask, row_slot, amax, al, bn_used, s);
    if (rc || !top_tokens) return rc;
    // the engine's fallback head (greedy_head_kernel<T, true>: the reduction greedy_head2_kernel states) with an empty bbox head, then
    // the combine kernel. scratch: (max, total) [M][2] | bbox [M][6] | next token [M] | kv_len [M] | six zero bbox biases (10 M .. 10 M + 6)
    // | identity row -> slot map [M] from 11 M + 16 on, where the caller gave none
    const int tiles_n = cdiv(N, *bn_used);
    SA_HIP(hipMemsetAsync(scratch, 0, ((size_t)16 * M + 16) * sizeof(float), s));
    float2* bt = reinterpret_cast<float2*>(scratch);
    int* ib = reinterpret_cast<int*>(scratch);
    if (!row_slot) {
        int* ident = ib + (size_t)11 * M + 16;
        hipLaunchKernelGGL(iota_kernel, dim3(cdiv(M, 256)), dim3(256), 0, s, ident, M);
        SA_HIP(hipGetLastError());
        row_slot = ident;
    }
    hipLaunchKernelGGL((greedy_head_kernel<float, true>), dim3(M), dim3(256), 0, s, amax, (long)tiles_n, tiles_n, scratch, 0, scratch,
                       scratch + (size_t)10 * M, row_slot, -1, -1, 1.0f, head_token, head_score, ib + (size_t)2 * M, ib + (size_t)8 * M,
                       ib + (size_t)9 * M, 0, bt);
    SA_HIP(hipGetLastError());
    hipLaunchKernelGGL(topk_combine_kernel, dim3(M), dim3(SA_ALT_THREADS), 0, s, al, tiles_n, row_slot, bt, top_tokens, top_probs);
    return (int)hipGetLastError();
}

int surya_op_gemm(int dtype, int out_f32, int epi, const void* X, long ldx, const void* W, long ldw, void* C, long ldc,
                  const void* bias, const void* R, long ldr, int M, int N, int K, void* stream) {
    if (!X || !W || !C) return SA_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (epi == EPI_GEGLU)                 // no bias, no residual, output in the compute dtype (LayoutModel's only use of it)
        return (bias || R || out_f32 || N % 2 || dtype == SA_DTYPE_F16) ? SA_ERR_UNSUPPORTED       // (fp16: surya_op_gemm_geglu_f16, layout_model.hip)
                                                                         : sa::op_gemm_geglu(dtype, X, ldx, W, ldw, C, ldc, M, N, K, s);
    if (dtype == SA_DTYPE_F32) return op_gemm_t<float, float>(epi, X, ldx, W, ldw, C, ldc, bias, R, ldr, M, N, K, s);
    if (dtype == SA_DTYPE_BF16)
        return out_f32 ? op_gemm_t<bf16_t, float>(epi, X, ldx, W, ldw, C, ldc, bias, R, ldr, M, N, K, s)
                       : op_gemm_t<bf16_t, bf16_t>(epi, X, ldx, W, ldw, C, ldc, bias, R, ldr, M, N, K, s);
    if (dtype == SA_DTYPE_F16) {          // 16-bit output only: the detector's epilogues (bias, residual, Hardswish, ReLU; built in det_model.hip)
        if (out_f32) return SA_ERR_UNSUPPORTED;                       // and the OCR-error classifier's GELU (ocr_error_model.hip)
        if (epi == EPI_GELU) return R ? SA_ERR_UNSUPPORTED : sa::op_gemm_f16_gelu(X, ldx, W, ldw, C, ldc, bias, M, N, K, s);
        return sa::op_gemm_f16(epi, X, ldx, W, ldw, C, ldc, bias, R, ldr, M, N, K, s);
    }
    return SA_ERR_UNSUPPORTED;
}

int surya_op_gemm_rope(int dtype, const void* X, long ldx, const void* W, long ldw, void* C, long ldc, const void* bias, const float* rope,
                       int rope_cols, int rope_D, int M, int N, int K, void* stream) {
    if (!X || !W || !C || !rope) return SA_ERR_ARG;
    if (rope_D <= 0 || rope_cols <= 0 || rope_cols > N || rope_cols % rope_D != 0) return SA_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == SA_DTYPE_F32) return op_gemm_rope_t<float>(X, ldx, W, ldw, C, ldc, bias, rope, rope_cols, rope_D, M, N, K, s);
    if (dtype == SA_DTYPE_BF16) return op_gemm_rope_t<bf16_t>(X, ldx, W, ldw, C, ldc, bias, rope, rope_cols, rope_D, M, N, K, s);
    if (dtype == SA_DTYPE_F16) return sa::op_gemm_rope_f16(X, ldx, W, ldw, C, ldc, bias, rope, rope_cols, rope_D, M, N, K, s);
    return SA_ERR_UNSUPPORTED;
}

// ---- op-level attention hooks (tests of the attention kernels against fp32 PyTorch; synchronous, not for timed code) ---------
namespace {
struct DevSegs {     // device copies of a host segment list for one op-level call
    void* mem = nullptr;
    sa::AttnSegs a{};
    int n_tiles = 0;
    int init(const int32_t* seg_len, const int64_t* q_off, const int64_t* k_off, const int64_t* v_off, const int64_t* o_off, int n_seg) {
        std::vector<int> tile_seg, tile_q0;
        for (int s = 0; s < n_seg; ++s) {
            if (seg_len[s] <= 0) return SA_ERR_ARG;
            for (int q0 = 0; q0 < seg_len[s]; q0 += 64) { tile_seg.push_back(s); tile_q0.push_back(q0); }
        }
        n_tiles = (int)tile_seg.size();
        const size_t ib = ((size_t)(2 * n_tiles + n_seg) * sizeof(int) + 15) & ~(size_t)15, lb = (size_t)n_seg * sizeof(long);
        std::vector<char> host(ib + 4 * lb);
        int* hi = reinterpret_cast<int*>(host.data());
        memcpy(hi, tile_seg.data(), n_tiles * sizeof(int));
        memcpy(hi + n_tiles, tile_q0.data(), n_tiles * sizeof(int));
        memcpy(hi + 2 * n_tiles, seg_len, n_seg * sizeof(int));
        const int64_t* offs[4] = {q_off, k_off, v_off, o_off};
        for (int i = 0; i < 4; ++i) memcpy(host.data() + ib + i * lb, offs[i], lb);
        SA_HIP(hipMalloc(&mem, host.size()));
        SA_HIP(hipMemcpy(mem, host.data(), host.size(), hipMemcpyHostToDevice));
        char* d = reinterpret_cast<char*>(mem);
        a.tile_seg = reinterpret_cast<const int*>(d); a.tile_q0 = a.tile_seg + n_tiles; a.seg_len = a.tile_seg + 2 * n_tiles;
        a.q_off = reinterpret_cast<const long*>(d + ib); a.k_off = a.q_off + n_seg; a.v_off = a.q_off + 2 * n_seg; a.o_off = a.q_off + 3 * n_seg;
        return SA_OK;
    }
    ~DevSegs() { if (mem) (void)hipFree(mem); }
};
}  // namespace

int surya_op_attn(int dtype, int head_dim, const void* q, const void* k, const void* v, void* out, const int32_t* seg_len,
                  const int64_t* q_off, const int64_t* k_off, const int64_t* v_off, const int64_t* o_off, int n_seg, int heads, int group,
                  int causal, float scale, long q_row, long q_head, long k_row, long k_head, long o_row, long o_head, void* stream) {
    if (!q || !k || !v || !out || !seg_len || !q_off || !k_off || !v_off || !o_off || n_seg <= 0 || heads <= 0 || group <= 0) return SA_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    DevSegs sg;
    int rc = sg.init(seg_len, q_off, k_off, v_off, o_off, n_seg);
    if (rc) return rc;
    if (dtype == SA_DTYPE_BF16)
        rc = sa::launch_attn<bf16_t>(head_dim, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)out, sg.a, sg.n_tiles, heads, q_row, q_head,
                                     k_row, k_head, o_row, o_head, group, causal, scale, s);
    else if (dtype == SA_DTYPE_F16)
        rc = sa::op_attn_f16(head_dim, q, k, v, out, sg.a, sg.n_tiles, heads, q_row, q_head, k_row, k_head, o_row, o_head, group, causal, scale, s);
    else if (dtype == SA_DTYPE_F32)
        rc = sa::launch_attn<float>(head_dim, (const float*)q, (const float*)k, (const float*)v, (float*)out, sg.a, sg.n_tiles, heads, q_row, q_head, k_row,
                                    k_head, o_row, o_head, group, causal, scale, s);
    else
        rc = SA_ERR_UNSUPPORTED;
    if (rc) return rc;
    SA_HIP(hipStreamSynchronize(s));          // the segment tables above are freed on return
    return SA_OK;
}

// surya_op_decode_attn and surya_op_decode_attn_mx: the second one also fills the three MXFP8 fields of the args (out8 != NULL)
static int op_decode_attn(int dtype, int head_dim, const float* qkv_part, int n_slabs, const void* qkv_bias, void* out, void* kcache,
                          void* vcache, const int32_t* active_slots, const int32_t* row_len, const float* rope_cs, int rows, int heads,
                          int kv_heads, int max_kv_len, float scale, void* stream, uint8_t* out8, uint8_t* sout, int srows) {
    if (!qkv_part || !qkv_bias || !out || !kcache || !vcache || !active_slots || !row_len || !rope_cs) return SA_ERR_ARG;
    if (rows <= 0 || n_slabs < 1 || n_slabs > 8 || kv_heads <= 0 || heads % kv_heads) return SA_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const float2* cs = reinterpret_cast<const float2*>(rope_cs);
    // no host bound on the contexts at the op level (ctx_bound = 0): the two-buffer kernel runs at dattn_db = 1 only (tests run both)
    if (dtype == SA_DTYPE_BF16) {
        sa::DecodeAttnArgs<bf16_t> a{qkv_part, n_slabs, (const bf16_t*)qkv_bias, (bf16_t*)out, (bf16_t*)kcache, (bf16_t*)vcache, active_slots, row_len,
                                     cs, rows, heads, kv_heads, head_dim, max_kv_len, scale};
        a.out8 = out8; a.sout = sout; a.srows = srows;
        return sa::launch_decode_attn<bf16_t>(a, s);
    }
    if (dtype == SA_DTYPE_F32) {
        sa::DecodeAttnArgs<float> a{qkv_part, n_slabs, (const float*)qkv_bias, (float*)out, (float*)kcache, (float*)vcache, active_slots, row_len, cs,
                                    rows, heads, kv_heads, head_dim, max_kv_len, scale};
        a.out8 = out8; a.sout = sout; a.srows = srows;          // no copy in fp32: the launcher refuses
        return sa::launch_decode_attn<float>(a, s);
    }
    if (dtype == SA_DTYPE_F16) {              // d = 64 / 32 built in layout_model.hip, d = 128 (the recogniser's) in rec_model_f16.hip
        sa::DecodeAttnArgs<sa::fp16_t> a{qkv_part, n_slabs, (const sa::fp16_t*)qkv_bias, (sa::fp16_t*)out, (sa::fp16_t*)kcache, (sa::fp16_t*)vcache,
                                         active_slots, row_len, cs, rows, heads, kv_heads, head_dim, max_kv_len, scale};
        a.out8 = out8; a.sout = sout; a.srows = srows;          // nor in fp16
        return sa::launch_decode_attn<sa::fp16_t>(a, s);
    }
    return SA_ERR_UNSUPPORTED;
}

int surya_op_decode_attn(int dtype, int head_dim, const float* qkv_part, int n_slabs, const void* qkv_bias, void* out, void* kcache,
                         void* vcache, const int32_t* active_slots, const int32_t* row_len, const float* rope_cs, int rows, int heads,
                         int kv_heads, int max_kv_len, float scale, void* stream) {
    return op_decode_attn(dtype, head_dim, qkv_part, n_slabs, qkv_bias, out, kcache, vcache, active_slots, row_len, rope_cs, rows, heads, kv_heads,
                          max_kv_len, scale, stream, nullptr, nullptr, 0);
}

int surya_op_decode_attn_mx(int dtype, int head_dim, const float* qkv_part, int n_slabs, const void* qkv_bias, void* out, void* kcache,
                            void* vcache, const int32_t* active_slots, const int32_t* row_len, const float* rope_cs, int rows, int heads,
                            int kv_heads, int max_kv_len, float scale, void* stream, uint8_t* out8, uint8_t* sout, int srows) {
    if (!out8 || !sout || srows < rows || (heads * head_dim) % 128) return SA_ERR_ARG;
    return op_decode_attn(dtype, head_dim, qkv_part, n_slabs, qkv_bias, out, kcache, vcache, active_slots, row_len, rope_cs, rows, heads, kv_heads,
                          max_kv_len, scale, stream, out8, sout, srows);
}

int surya_op_kv8_quant_rows(int head_dim, const void* kcache, const void* vcache, const int32_t* tok_slot, const int32_t* tok_pos, int n_tokens,
                            void* k8, void* v8t, float* kscale, float* vscale, int kv_heads, int max_kv_len, void* stream) {
    if (!kcache || !vcache || !tok_slot || !tok_pos || !k8 || !v8t || !kscale || !vscale || n_tokens <= 0 || kv_heads <= 0) return SA_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    return sa::launch_kv8_quant_rows(head_dim, (const bf16_t*)kcache, (const bf16_t*)vcache, tok_slot, tok_pos, n_tokens, (uint8_t*)k8, (uint8_t*)v8t, kscale,
                                     vscale, kv_heads, max_kv_len, s);
}

static int op_decode_attn_kv8(int head_dim, const float* qkv_part, int n_slabs, const void* qkv_bias, void* out, void* k8, void* v8t,
                              float* kscale, float* vscale, const int32_t* active_slots, const int32_t* row_len, const float* rope_cs, int rows,
                              int heads, int kv_heads, int max_kv_len, float scale, void* stream, uint8_t* out8, uint8_t* sout, int srows) {
    if (!qkv_part || !qkv_bias || !out || !k8 || !v8t || !kscale || !vscale || !active_slots || !row_len || !rope_cs) return SA_ERR_ARG;
    if (rows <= 0 || n_slabs < 1 || n_slabs > 8 || kv_heads <= 0 || heads % kv_heads) return SA_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    sa::DecodeAttnKv8Args a{qkv_part, n_slabs, (const bf16_t*)qkv_bias, (bf16_t*)out, (uint8_t*)k8, (uint8_t*)v8t, kscale, vscale, active_slots, row_len,
                            reinterpret_cast<const float2*>(rope_cs), rows, heads, kv_heads, head_dim, max_kv_len, scale};
    a.out8 = out8; a.sout = sout; a.srows = srows;
    return sa::launch_decode_attn_kv8(a, s);
}

int surya_op_decode_attn_kv8(int head_dim, const float* qkv_part, int n_slabs, const void* qkv_bias, void* out, void* k8, void* v8t,
                             float* kscale, float* vscale, const int32_t* active_slots, const int32_t* row_len, const float* rope_cs, int rows,
                             int heads, int kv_heads, int max_kv_len, float scale, void* stream) {
    return op_decode_attn_kv8(head_dim, qkv_part, n_slabs, qkv_bias, out, k8, v8t, kscale, vscale, active_slots, row_len, rope_cs, rows, heads, kv_heads,
                              max_kv_len, scale, stream, nullptr, nullptr, 0);
}

int surya_op_decode_attn_kv8_mx(int head_dim, const float* qkv_part, int n_slabs, const void* qkv_bias, void* out, void* k8, void* v8t,
                                float* kscale, float* vscale, const int32_t* active_slots, const int32_t* row_len, const float* rope_cs, int rows,
                                int heads, int kv_heads, int max_kv_len, float scale, void* stream, uint8_t* out8, uint8_t* sout, int srows) {
    if (!out8 || !sout || srows < rows || (heads * head_dim) % 128) return SA_ERR_ARG;
    return op_decode_attn_kv8(head_dim, qkv_part, n_slabs, qkv_bias, out, k8, v8t, kscale, vscale, active_slots, row_len, rope_cs, rows, heads, kv_heads,
                              max_kv_len, scale, stream, out8, sout, srows);
}

__global__ __launch_bounds__(256) void mx_quantize_rows_kernel(const float* __restrict__ x, int K, uint8_t* __restrict__ q,
                                                               uint8_t* __restrict__ sc) {
    const long row = blockIdx.x, rows = gridDim.x;
    for (int c = threadIdx.x * 4; c < K; c += 1024) {            // K % 32 == 0: an 8-lane group is inside the row or outside it
        float v[4];
        load4(x + row * K + c, v);
        int e8;
        const uint32_t pk = mx_quant4_oct(v, e8);
        *reinterpret_cast<uint32_t*>(q + row * K + c) = pk;
        if ((threadIdx.x & 7) == 0) sc[((long)(c >> 7) * rows + row) * 4 + ((c >> 5) & 3)] = (uint8_t)e8;
    }
}

int surya_op_mx_quantize(const float* x, int rows, int K, uint8_t* q, uint8_t* scales, void* stream) {
    if (!x || !q || !scales || rows <= 0 || K <= 0 || K % 128) return SA_ERR_ARG;
    hipLaunchKernelGGL(mx_quantize_rows_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, x, K, q, scales);
    return (int)hipGetLastError();
}

int surya_op_gemm_splitk_bf16(const void* X, long ldx, const void* W, long ldw, float* part, int M, int N, int K, int* splitk, void* stream) {
    if (!X || !W || !part || !splitk) return SA_ERR_ARG;
    GemmArgs<bf16_t, bf16_t> a{reinterpret_cast<const bf16_t*>(X), ldx, reinterpret_cast<const bf16_t*>(W), ldw, nullptr, 0, nullptr, nullptr, 0, M, N, K, 1, part};
    const int rc = launch_gemm_splitk<bf16_t>(a, (hipStream_t)stream);
    *splitk = a.splitk;
    return rc;
}

int surya_op_gemm_mx(int mode, const uint8_t* X, const uint8_t* SX, const uint8_t* W, const uint8_t* SW, int M, int N, int K,
                     float* C, int* splitk, uint8_t* q_out, uint8_t* sq_out, void* stream) {
    if (!X || !SX || !W || !SW) return SA_ERR_ARG;
    MxArgs a{X, (long)K, SX, W, (long)K, SW, M, N, K, (long)M, (long)N};
    hipStream_t s = (hipStream_t)stream;
    if (mode == 0) {
        if (!C) return SA_ERR_ARG;
        a.C = C; a.ldc = N;
        return launch_gemm_mx<MX_EPI_F32>(a, s);
    }
    if (mode == 1) {
        if (!C || !splitk) return SA_ERR_ARG;
        a.part = C;
        int rc = launch_gemm_mx_splitk(a, s);
        *splitk = a.splitk;
        return rc;
    }
    if (mode == 2) {
        if (!q_out || !sq_out) return SA_ERR_ARG;
        a.Q = q_out; a.ldq = N / 2; a.SQ = sq_out; a.sq_rows = M;
        return launch_gemm_mx<MX_EPI_SWIGLU>(a, s);
    }
    return SA_ERR_ARG;
}

int surya_rec_preprocess(const uint8_t* pages, const void* lines, int n_lines, uint8_t* mask_arena, float* mid_arena, float* tiles,
                         int patch_size, int merge_size, float pad_value, const float* mean, const float* std, int any_poly,
                         int max_stage1_width, int pixel_stride, void* stream) {
    if (!pages || !lines || !tiles || !mean || !std || n_lines < 0 || patch_size <= 0 || merge_size <= 0) return SA_ERR_ARG;
    if (pixel_stride != 3 && pixel_stride != 4) return SA_ERR_ARG;
    sa::prep::PrepArgs p;
    p.pages = pages; p.lines = reinterpret_cast<const sa::prep::LineDesc*>(lines); p.n_lines = n_lines;
    p.mask = mask_arena; p.mid = mid_arena; p.tiles = tiles; p.ps = patch_size; p.merge = merge_size; p.pad = pad_value;
    for (int i = 0; i < 3; ++i) { p.mean[i] = mean[i]; p.std[i] = std[i]; }
    p.max_mid_w = max_stage1_width;
    p.pix = pixel_stride;
    return sa::prep::prep_run(p, any_poly, max_stage1_width > 0, (hipStream_t)stream);
}

int surya_rec_rectify(const uint8_t* pages, const void* descs, int n, uint8_t* out, int pixel_stride, int max_w, int max_h, void* stream) {
    return sa::prep::rectify_run(pages, reinterpret_cast<const sa::prep::RectifyDesc*>(descs), n, out, pixel_stride, max_w, max_h,
                                 (hipStream_t)stream);
}

int surya_rec_unroll(const uint8_t* pages, const void* descs, int n, const double* tables, uint8_t* out, int pixel_stride, int max_w,
                     int max_h, void* stream) {
    return sa::prep::unroll_run(pages, reinterpret_cast<const sa::prep::UnrollDesc*>(descs), n, tables, out, pixel_stride, max_w, max_h,
                                (hipStream_t)stream);
}

int surya_warp_mesh(const uint8_t* pages, const void* descs, int n, const double* meshes, uint8_t* out, int pixel_stride, int max_w,
                    int max_h, void* stream) {
    return sa::prep::warp_mesh_run(pages, reinterpret_cast<const sa::pagewarp::MeshDesc*>(descs), n, meshes, out, pixel_stride, max_w, max_h,
                                   (hipStream_t)stream);
}

int surya_rec_adjust_contrast(const uint8_t* pages, const void* descs, int n, uint8_t* out, uint8_t* mask_arena, void* work, int32_t* lo_hi,
                              int pixel_stride, void* stream) {
    return sa::prep::adjust_run(pages, reinterpret_cast<const sa::adjust::AdjustDesc*>(descs), n, out, mask_arena, work, lo_hi, pixel_stride,
                                (hipStream_t)stream);
}

int surya_set_tuning(const char* key, int value) {
    if (!key) return SA_ERR_ARG;
    Tuning& t = tuning();
    struct { const char* k; int* v; } tab[] = {
        {"graph", &t.graph}, {"split_target", &t.split_target}, {"split_min_kt", &t.split_min_kt}, {"split_max", &t.split_max},
        {"bigtile", &t.bigtile}, {"bigtile_any", &t.bigtile_any}, {"conv_lean", &t.conv_lean}, {"conv_persist", &t.conv_persist}, {"dwconv_pipe", &t.dwconv_pipe}, {"bigtile_ratio_pct", &t.bigtile_ratio_pct}, {"gateup_ring", &t.gateup_ring}, {"dring", &t.dring}, {"dring_min_kt", &t.dring_min_kt}, {"big_m_split", &t.big_m_split}, {"big_m_gateup", &t.big_m_gateup}, {"mx_big_m_split", &t.mx_big_m_split}, {"mx_big_m_gateup", &t.mx_big_m_gateup}, {"glds", &t.glds}, {"bigtile_min_k", &t.bigtile_min_k}, {"dattn", &t.dattn}, {"rnorm", &t.rnorm},
        {"ghead", &t.ghead}, {"fuse_embed", &t.fuse_embed}, {"persist", &t.persist}, {"lmhead", &t.lmhead}, {"kvprefetch", &t.kvprefetch},
        {"dattn_db", &t.dattn_db}, {"lay_ln", &t.lay_ln}, {"det_head_blk", &t.det_head_blk}, {"det_fuse", &t.det_fuse}, {"det_up4", &t.det_up4}, {"fmb_chunk", &t.fmb_chunk}, {"ocrerr_cls_only", &t.ocrerr_cls_only}};
    for (auto& e : tab)
        if (!strcmp(e.k, key)) {
            if (*e.v != value) ++tuning_epoch();        // captured decode graphs are stale (RecModel::decode_steps drops them)
            *e.v = value;
            return SA_OK;
        }
    return SA_ERR_ARG;
}

int surya_gemm_ring_status(int reset) {       // every translation unit that runs the ring has a give-up word of its own
    const int a = sa::ring_error(reset != 0), b = sa::rec_f16_ring_error(reset != 0);
    return a ? a : b;
}

int surya_prof_enable(int on) {
    GemmProfiler& pf = gemm_profiler();
    if (on) pf.start(); else pf.enabled = false;
    return SA_OK;
}

__global__ void prof_null_kernel() {}

// Median hipEvent-pair time around an EMPTY one-workgroup kernel, launched back to back like the profiled GEMMs: what an
// event pair costs by itself (dispatch latency + minimal kernel), so a reader can reconcile bench.py's event-bracketed
// per-launch times with rocprofv3's begin->end kernel durations for microsecond-scale kernels.
int surya_prof_event_overhead(void* stream, double* ms) {
    if (!ms) return SA_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    constexpr int N = 201;
    hipEvent_t ev[2 * N];
    for (auto& e : ev) SA_HIP(hipEventCreate(&e));
    for (int i = 0; i < 32; ++i) hipLaunchKernelGGL(prof_null_kernel, dim3(1), dim3(64), 0, s);
    for (int i = 0; i < N; ++i) {
        SA_HIP(hipEventRecord(ev[2 * i], s));
        hipLaunchKernelGGL(prof_null_kernel, dim3(1), dim3(64), 0, s);
        SA_HIP(hipEventRecord(ev[2 * i + 1], s));
    }
    SA_HIP(hipStreamSynchronize(s));
    std::vector<float> t(N);
    for (int i = 0; i < N; ++i) SA_HIP(hipEventElapsedTime(&t[i], ev[2 * i], ev[2 * i + 1]));
    for (auto& e : ev) (void)hipEventDestroy(e);
    std::sort(t.begin(), t.end());
    *ms = t[N / 2];
    return SA_OK;
}

int surya_prof_read2(int max_cfg, int* launches, double* ms, double* flops, double* bytes, double* slab_bytes) {
    GemmProfiler& pf = gemm_profiler();
    if (!launches || !ms || !flops || !bytes || max_cfg < GemmProfiler::NCFG) return SA_ERR_ARG;
    SA_HIP(hipDeviceSynchronize());
    const int ncfg = std::min(max_cfg, (int)GemmProfiler::NCFG_ALL);      // buckets 4 and 5 (beam search) only for a reader with room for them
    for (int c = 0; c < ncfg; ++c) { launches[c] = 0; ms[c] = flops[c] = bytes[c] = 0.0; if (slab_bytes) slab_bytes[c] = 0.0; }
    for (int i = 0; i < pf.n; ++i) {
        const int c = pf.cfg_of[i];
        if (c >= ncfg) continue;
        float t = 0.f;
        SA_HIP(hipEventElapsedTime(&t, pf.ev[2 * i], pf.ev[2 * i + 1]));
        launches[c]++; ms[c] += t; flops[c] += pf.flops_of[i]; bytes[c] += pf.bytes_of[i];
        if (slab_bytes) slab_bytes[c] += pf.slab_of[i];
    }
    pf.n = 0;
    return SA_OK;
}

int surya_prof_read(int max_cfg, int* launches, double* ms, double* flops, double* bytes) {
    return surya_prof_read2(max_cfg, launches, ms, flops, bytes, nullptr);
}

int surya_op_rmsnorm(int dtype, const void* x, long ldx, const void* w, void* y, long ldy, int rows, int C, float eps,
                     void* stream) {
    if (!x || !w || !y || rows <= 0) return SA_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == SA_DTYPE_F32) return sa::launch_rmsnorm<float>((const float*)x, ldx, (const float*)w, (float*)y, ldy, nullptr, rows, C, eps, s);
    if (dtype == SA_DTYPE_BF16) return sa::launch_rmsnorm<bf16_t>((const bf16_t*)x, ldx, (const bf16_t*)w, (bf16_t*)y, ldy, nullptr, rows, C, eps, s);
    return SA_ERR_UNSUPPORTED;
}

// ---- the recogniser's non-GEMM kernels alone (rec_ops.h): one entry per op, the dtype picks the instance
static int rec_dispatch(int dtype, int op, const void* a, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (dtype == SA_DTYPE_F32) return sa::rec_op_any<float>(op, a, s);
    if (dtype == SA_DTYPE_BF16) return sa::rec_op_any<bf16_t>(op, a, s);
    if (dtype == SA_DTYPE_F16) return sa::op_rec_f16(op, a, s);
    return SA_ERR_UNSUPPORTED;
}

int surya_op_rec_rmsnorm_rows(int dtype, const void* x, long ldx, const void* w, void* y, long ldy, const int32_t* src_row, int rows, int C,
                              float eps, void* stream) {
    const sa::RecRmsRowsOp a{x, ldx, w, y, ldy, src_row, rows, C, eps};
    return rec_dispatch(dtype, sa::REC_OP_RMS_ROWS, &a, stream);
}
int surya_op_rec_rows(int dtype, int kind, void* dst, const void* src, const void* src2, const void* src3, const int32_t* index,
                      const int32_t* index2, const int32_t* index3, const int32_t* dims, void* stream) {
    const sa::RecRowsOp a{kind, dst, src, src2, src3, index, index2, index3, dims};
    return rec_dispatch(dtype, sa::REC_OP_ROWS, &a, stream);
}
int surya_op_rec_rope_table(int dtype, int kind, const int32_t* pos_hw, const float* inv_freq, float* table, int n, int d, void* stream) {
    const sa::RecRopeTableOp a{kind, pos_hw, inv_freq, table, n, d};
    return rec_dispatch(dtype, sa::REC_OP_ROPE_TABLE, &a, stream);
}
int surya_op_rec_rope_kv_append(int dtype, void* qkv, const int32_t* tok_slot, const int32_t* tok_pos, const float* rope_cs, void* kcache,
                                void* vcache, int n_tokens, int heads, int kv_heads, int head_dim, int max_kv_len, void* stream) {
    const sa::RecRopeKvOp a{qkv, tok_slot, tok_pos, rope_cs, kcache, vcache, n_tokens, heads, kv_heads, head_dim, max_kv_len};
    return rec_dispatch(dtype, sa::REC_OP_ROPE_KV, &a, stream);
}
int surya_op_rec_reduce_norm(int dtype, const float* part, int S, int M, void* x, const void* w, void* y, int H, float eps, uint8_t* y8,
                             uint8_t* sy, int srows, void* stream) {
    const sa::RecReduceOp a{part, S, M, x, w, y, H, eps, y8, sy, srows};
    return rec_dispatch(dtype, sa::REC_OP_REDUCE, &a, stream);
}
int surya_op_rec_decode_embed(int dtype, const void* table, const int32_t* next_token, const int32_t* active_slots, const int32_t* kv_len,
                              int max_kv_len, int32_t* row_len, void* x, const void* w, void* y, int rows, int H, float eps, uint8_t* y8,
                              uint8_t* sy, int srows, void* stream) {
    const sa::RecEmbedOp a{table, next_token, active_slots, kv_len, max_kv_len, row_len, x, w, y, rows, H, eps, y8, sy, srows};
    return rec_dispatch(dtype, sa::REC_OP_EMBED, &a, stream);
}
int surya_op_rec_head(int dtype, const surya_rec_head_args* args, void* stream) {
    if (!args) return SA_ERR_ARG;
    return rec_dispatch(dtype, sa::REC_OP_HEAD, args, stream);
}
int surya_op_rec_beam_select(const int32_t* lead_slots, int stride, int n_groups, int width, int n_slots, const int32_t* alt_token,
                             const float* alt_prob, float* score, int32_t* finished, int eos_id, int pad_id, int no_output_id, int first,
                             int32_t* token, int32_t* parent, int32_t* rank, float* prob, float* logp, int32_t* next_token, int32_t* fork_src,
                             int32_t* kv_len, int32_t* prompt_len, int32_t* fork_base, int32_t* fork_len, int max_kv_len, void* stream) {
    if (n_groups < 0 || (!lead_slots && (long)n_groups * width > n_slots)) return SA_ERR_ARG;
    const sa::BeamSelectArgs a{lead_slots, stride, n_groups, width, n_slots, alt_token, alt_prob, score, finished, eos_id, pad_id, no_output_id,
                               first ? 1 : 0, token, parent, rank, prob, logp, next_token, fork_src, kv_len, prompt_len, fork_base, fork_len, max_kv_len};
    return sa::launch_beam_select(a, (hipStream_t)stream);
}
int surya_op_rec_kv_fork(int dtype, void* kcache, void* vcache, const int32_t* fork_src, const int32_t* base, const int32_t* len, int rows,
                         int layers, int slots, int kv_heads, int max_kv_len, int head_dim, void* stream) {
    const sa::RecKvForkOp a{kcache, vcache, fork_src, base, len, rows, layers, slots, kv_heads, max_kv_len, head_dim};
    return rec_dispatch(dtype, sa::REC_OP_KV_FORK, &a, stream);
}
int surya_op_rec_kv_fanout(int dtype, void* kcache, void* vcache, const int32_t* fan_src, const int32_t* fan_off, const int32_t* fan_dst,
                           const int32_t* fan_len, int n_seqs, int n_dst, int layers, int slots, int kv_heads, int max_kv_len, int head_dim,
                           void* stream) {
    const sa::RecKvFanoutOp a{kcache, vcache, fan_src, fan_off, fan_dst, fan_len, n_seqs, n_dst, layers, slots, kv_heads, max_kv_len, head_dim};
    return rec_dispatch(dtype, sa::REC_OP_KV_FANOUT, &a, stream);
}
int surya_op_rec_kv_keep(int dtype, const void* kcache, const void* vcache, void* store_k, void* store_v, const int32_t* slot,
                         const int32_t* first, const int32_t* len, int n, int layers, int slots, int kv_heads, int max_kv_len, int head_dim,
                         int cap_rows, const void* x, const int32_t* last_row, void* hid, int hidden, int x_rows, void* stream) {
    const sa::RecKvKeepOp a{kcache, vcache, store_k, store_v, slot, first, len, n, layers, slots, kv_heads, max_kv_len, head_dim, cap_rows,
                            x, last_row, hid, hidden, x_rows};
    return rec_dispatch(dtype, sa::REC_OP_KV_KEEP, &a, stream);
}
int surya_op_rec_kv_restore(int dtype, void* kcache, void* vcache, const void* store_k, const void* store_v, const int32_t* first,
                            const int32_t* len, const int32_t* fan_off, const int32_t* fan_dst, int n, int n_dst, int layers, int slots,
                            int kv_heads, int max_kv_len, int head_dim, int cap_rows, void* stream) {
    const sa::RecKvRestoreOp a{kcache, vcache, store_k, store_v, first, len, fan_off, fan_dst, n, n_dst, layers, slots, kv_heads, max_kv_len,
                               head_dim, cap_rows};
    return rec_dispatch(dtype, sa::REC_OP_KV_RESTORE, &a, stream);
}
static int lexicon_op_args(const surya_rec_lexicon_args* g, sa::LexiconArgs& a) {
    if (!g || !g->edge_off || !g->edge_tok || !g->edge_next || !g->state_flags || !g->table || !g->slot_state || !g->slot_mask || g->words <= 0 ||
        g->row_base < 0 || g->vocab <= 0 || g->vocab > g->words * 32)
        return SA_ERR_ARG;
    a = sa::LexiconArgs{g->edge_off, g->edge_tok, g->edge_next, g->state_flags, g->table, g->words, g->row_base, g->slot_state, g->slot_mask,
                        g->vocab, g->eos_id, g->pad_id, g->nop_id};
    return SA_OK;
}
int surya_op_rec_lexicon_start(const surya_rec_lexicon_args* args, const int32_t* slots, const int32_t* states, int n, void* stream) {
    sa::LexiconArgs a;
    if (lexicon_op_args(args, a) || n < 0 || (n > 0 && (!slots || !states))) return SA_ERR_ARG;
    return sa::launch_lexicon_start(a, slots, states, n, (hipStream_t)stream);
}
int surya_op_rec_lexicon_step(const surya_rec_lexicon_args* args, const int32_t* row_slot, const int32_t* out_token, int rows, void* stream) {
    sa::LexiconArgs a;
    if (lexicon_op_args(args, a) || rows < 0 || (rows > 0 && (!row_slot || !out_token))) return SA_ERR_ARG;
    return sa::launch_lexicon_step(a, row_slot, out_token, rows, (hipStream_t)stream);
}
int surya_op_rec_boost_step(const surya_rec_lexicon_args* lex, const int32_t* slot_root, int out_state, int word_row, const int32_t* row_slot,
                            const int32_t* out_token, int rows, void* stream) {
    sa::BoostArgs b;
    if (lexicon_op_args(lex, b.lx) || !slot_root || out_state < 0 || word_row < 0 || rows < 0 || (rows > 0 && (!row_slot || !out_token))) return SA_ERR_ARG;
    b.slot_root = const_cast<int32_t*>(slot_root); b.out_state = out_state; b.word_row = word_row;
    return sa::launch_boost_step(b, row_slot, out_token, rows, (hipStream_t)stream);
}
int surya_op_rec_boost_head(int dtype, const surya_rec_boost_head_args* args, void* stream) {
    if (!args) return SA_ERR_ARG;
    return rec_dispatch(dtype, sa::REC_OP_BOOST_HEAD, args, stream);
}

}  // extern "C"
