"""ctypes binding of libsurya_amd.so (C ABI: include/surya_amd.h).

The product path has NO fallback: if the HIP library is missing or a call fails this raises -- a silent
PyTorch/CPU path would void every parity and performance claim.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SURYA_AMD_LIB") or os.path.join(HERE, "libsurya_amd.so")   # env: A/B builds of the kernels

SA_MAX_STEPS = 16
SA_MAX_ALTERNATIVES = 4                         # alternatives per token (surya_rec_set_alternatives); top_k < 4 is a slice on the host
SA_MAX_BEAMS = 4                                # widest beam (surya_rec_set_beam): a row reports four candidates
SA_MAX_FORCED_TOKENS = 1024                    # forced ids per slot (surya_rec_set_forced_tokens)
SA_MAX_TOKEN_MASKS = 64                         # rows of a handle's token-mask table (surya_rec_set_token_masks)
SA_MAX_PATTERN_STATES = 4096                    # states of a call's joint automaton (surya_rec_set_patterns)
SA_MAX_PATTERN_CLASSES = 256                    # symbol classes of its alphabet (tok_class is uint8)
SA_MAX_LEXICON_STATES = 1 << 20                 # states of a call's joint lexicon automaton (surya_rec_set_lexicon)
SA_MAX_LEXICON_EDGES = 1 << 21                  # ... and its edges
OP_MXFP8 = 3                                    # SA_OP_MXFP8: the MXFP8 arm of surya_op_lm_head_partials
DTYPE_F32, DTYPE_BF16, DTYPE_F16 = 0, 1, 2      # SA_DTYPE_*; every engine takes all three
(RW_PATCH, RW_MERGER_LN, RW_FC1_W, RW_FC1_B, RW_FC2_W, RW_FC2_B, RW_IMG_H, RW_IMG_W, RW_DEC_NORM, RW_TOK_EMBED, RW_LM_W,
 RW_LM_B, RW_BBOX_W, RW_BBOX_B, RW_ENC_INVFREQ, RW_DEC_INVFREQ, RW_GLOBALS) = range(17)
(RE_NORM1, RE_QKV_W, RE_QKV_B, RE_PROJ_W, RE_PROJ_B, RE_NORM2, RE_GU_W, RE_GU_B, RE_DOWN_W, RE_DOWN_B, RE_COUNT) = range(11)
(RD_LN1, RD_QKV_W, RD_QKV_B, RD_O_W, RD_LN2, RD_GU_W, RD_DOWN_W, RD_COUNT) = range(8)

EPI_BIAS, EPI_RESIDUAL, EPI_GELU, EPI_SWIGLU, EPI_HARDSWISH, EPI_RELU = range(6)
EPI_GEGLU = 8                                   # gelu_tanh(gate) * up (ADETR decoder MLP); surya_op_gemm, fp32 / bf16 (fp16: surya_op_gemm_geglu_f16)
FAMILY_LAYOUT, FAMILY_TABLE = 0, 1              # SA_FAMILY_*
REC_CONVERT_TILES, REC_SCATTER_IMAGE, REC_SCATTER_ROWS, REC_EMBED_TOKENS = range(4)    # SA_REC_*: `kind` of surya_op_rec_rows
REC_ROPE_VISION, REC_ROPE_DECODER = 0, 1        # SA_REC_ROPE_*: `kind` of surya_op_rec_rope_table
LAY_PATCHIFY, LAY_ADD_ROWS, LAY_ZERO_ROWS, LAY_GATHER_ADD = range(4)      # SA_LAY_*: `kind` of surya_op_lay_rows


class RecConfigC(C.Structure):
    _fields_ = [
        ("enc_depth", C.c_int32), ("enc_hidden", C.c_int32), ("enc_inter", C.c_int32), ("enc_inter_pad", C.c_int32),
        ("enc_heads", C.c_int32), ("patch_dim", C.c_int32), ("patch_dim_pad", C.c_int32), ("merge", C.c_int32),
        ("window_tokens", C.c_int32), ("enc_out_hidden", C.c_int32), ("fullatt_mask", C.c_uint32), ("enc_eps", C.c_float),
        ("vocab", C.c_int32), ("dec_hidden", C.c_int32), ("dec_inter", C.c_int32), ("dec_layers", C.c_int32),
        ("dec_heads", C.c_int32), ("dec_kv_heads", C.c_int32), ("dec_head_dim", C.c_int32), ("dec_eps", C.c_float),
        ("bbox_size", C.c_int32), ("embed_multiplier", C.c_int32), ("image_token_id", C.c_int32),
        ("pad_token_id", C.c_int32), ("eos_token_id", C.c_int32), ("max_slots", C.c_int32), ("max_kv_len", C.c_int32),
        ("max_patches", C.c_int32), ("max_prefill_tokens", C.c_int32), ("dtype", C.c_int32),
    ]


class DetConfigC(C.Structure):
    _fields_ = [("n_ops", C.c_int32), ("max_batch", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("num_labels", C.c_int32), ("dtype", C.c_int32)]


class RecHeadArgsC(C.Structure):
    """surya_rec_head_args (include/surya_amd.h): the operands of surya_op_rec_head."""
    _fields_ = ([(n, C.c_void_p) for n in (
        "part", "hidden", "wb", "bb", "row_slot", "out_token", "out_score", "out_bbox", "next_token", "kv_len", "table", "wnorm", "x", "y",
        "row_len", "y8", "sy", "best_tot", "forced_table", "forced_cursor", "flogit", "greedy_token", "greedy_prob", "logprob")] +
                [(n, C.c_int32) for n in ("tiles_n", "rows", "H", "eos_id", "pad_id", "len_inc", "max_kv_len", "srows", "forced_stride")] +
                [("bbox_size", C.c_float), ("eps", C.c_float)] +
                [(n, C.c_void_p) for n in ("pat_tok_class", "pat_next_state", "pat_state_mask", "pat_slot_state", "pat_slot_mask")] +
                [("pat_n_classes", C.c_int32), ("pat_vocab", C.c_int32)])


class RecLexiconArgsC(C.Structure):
    """surya_rec_lexicon_args (include/surya_amd.h): the operands of surya_op_rec_lexicon_start / _step."""
    _fields_ = ([(n, C.c_void_p) for n in ("edge_off", "edge_tok", "edge_next", "state_flags", "table", "slot_state", "slot_mask")] +
                [(n, C.c_int32) for n in ("words", "row_base", "vocab", "eos_id", "pad_id", "nop_id")])


class RecBoostHeadArgsC(C.Structure):
    """surya_rec_boost_head_args (include/surya_amd.h): the operands of surya_op_rec_boost_head."""
    _fields_ = [("head", RecHeadArgsC)] + [(n, C.c_void_p) for n in ("part_b", "slot_beta", "plain_token", "plain_prob")]


class SuryaAmdError(RuntimeError):
    pass


SA_OK, SA_ERR_ARG, SA_ERR_SHAPE, SA_ERR_UNSUPPORTED, SA_ERR_STATE, SA_ERR_NOMEM = 0, -1, -2, -3, -4, -5      # include/surya_amd.h
_ERR = {-1: "SA_ERR_ARG", -2: "SA_ERR_SHAPE", -3: "SA_ERR_UNSUPPORTED", -4: "SA_ERR_STATE", -5: "SA_ERR_NOMEM"}
_lib = None


def lib() -> C.CDLL:
    """Load the HIP library (once). Raises if it has not been built: there is no fallback path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SuryaAmdError(
                f"{LIB_PATH} not found: build it with `python -m surya_amd.build` (hipcc --offload-arch=gfx950). "
                "surya_amd has no CPU/PyTorch fallback for the model path.")
        # torch must load ITS libamdhip64.so.7 first: the library shares device pointers and streams with torch, so both
        # have to bind to one HIP runtime instance (same SONAME -> the loader reuses the copy that is already mapped).
        import torch  # noqa: F401
        _lib = C.CDLL(LIB_PATH)
        _lib.surya_amd_version.restype = C.c_char_p
        _lib.surya_rec_workspace_bytes.restype = C.c_size_t
        _lib.surya_det_boxes_workspace_bytes.restype = C.c_size_t
        _lib.surya_det_boxes_workspace_layout.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.c_int,
                                                          C.POINTER(C.c_int), C.POINTER(C.c_int)]
        _lib.surya_det_boxes_workspace_layout.restype = C.c_int
        _bind_lay_ops(_lib)
    return _lib


def _bind_lay_ops(lib):
    """Argument types of the layout family's op-level entry points (include/surya_amd.h): Python ints and floats convert themselves."""
    i, l, f, p = C.c_int, C.c_long, C.c_float, C.c_void_p
    ip = C.POINTER(C.c_int32)
    sig = {
        "surya_lay_window_tables": [i, i, i, i, ip, ip, ip, ip, ip],
        "surya_lay_cross_plan": [i, ip, ip, ip],
        "surya_op_lay_layernorm": [i, p, p, p, p, p, l, i, i, f, i, p],
        "surya_op_lay_window_attn": [i, p, p, p, l, i, i, i, i, i, i, p],
        "surya_op_lay_merge_ln": [i, p, p, p, p, i, i, i, i, f, p],
        "surya_op_lay_rows": [i, i, p, p, p, ip, p],
        "surya_op_lay_cross_attn": [i, i, p, i, i, p, i, p, p, p, p, i, i, i, f, p],
        "surya_op_lay_rmsnorm": [i, p, p, p, i, i, f, p],
        "surya_op_lay_reduce_norm": [i, p, i, i, p, p, p, p, p, i, f, p],
        "surya_op_lay_prefill_attn": [i, i, p, p, p, p, p, i, i, i, i, i, f, p],
        "surya_op_lay_embed": [i, i, p, p, p, i, i, i, i, i, i, i, i, p],
        "surya_op_lay_heads": [i, p, l, p, p, p, p, p, p, p, p, i, i, i, f, f, p],
    }
    for name, args in sig.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, C.c_int
        if name.startswith("surya_op_lay_"):                     # the fp16 entry of the same op: the same arguments without `dtype`
            f16 = getattr(lib, name + "_f16")
            f16.argtypes, f16.restype = args[1:], C.c_int
    lib.surya_op_gemm_geglu_f16.argtypes, lib.surya_op_gemm_geglu_f16.restype = [p, l, p, l, p, l, i, i, i, p], C.c_int
    lib.surya_op_gemm_rope.argtypes, lib.surya_op_gemm_rope.restype = [i, p, l, p, l, p, l, p, p, i, i, i, i, i, p], C.c_int
    # the fp16 recogniser's GEMMs (csrc/rec_model_f16.hip)
    lib.surya_op_rec_gemm_f16.argtypes, lib.surya_op_rec_gemm_f16.restype = [i, i, p, l, p, l, p, l, p, p, l, i, i, i, p, ip, p], C.c_int
    lib.surya_op_gemm_splitk_f16.argtypes, lib.surya_op_gemm_splitk_f16.restype = [p, l, p, l, p, i, i, i, ip, p], C.c_int
    # constrained output (token masks of the lm_head's greedy epilogues) and the lm_head launch by itself
    lib.surya_rec_set_token_masks.argtypes, lib.surya_rec_set_token_masks.restype = [p, C.POINTER(C.c_uint32), i, p], C.c_int
    lib.surya_rec_set_slot_masks.argtypes, lib.surya_rec_set_slot_masks.restype = [p, ip, ip, i, p], C.c_int
    lib.surya_op_lm_head_partials.argtypes, lib.surya_op_lm_head_partials.restype = [i, p, p, p, p, p, i, i, i, p, p, p, p, ip, p], C.c_int
    # alternatives (the k most likely tokens of every step) and the *_TOPK lm_head launch by itself
    lib.surya_rec_set_alternatives.argtypes, lib.surya_rec_set_alternatives.restype = [p, i], C.c_int
    lib.surya_rec_read_alternatives.argtypes, lib.surya_rec_read_alternatives.restype = [p, i, ip, C.POINTER(C.c_float), p], C.c_int
    lib.surya_rec_wait_alternatives.argtypes, lib.surya_rec_wait_alternatives.restype = [p, i, i, ip, C.POINTER(C.c_float)], C.c_int
    lib.surya_op_lm_head_topk.argtypes = [i, p, p, p, p, p, i, i, i, p, p, p, p, p, ip, p, p, p, p, p, p]
    lib.surya_op_lm_head_topk.restype = C.c_int
    # forced decoding (align a known transcription) and the *_FORCED lm_head launch by itself
    fp = C.POINTER(C.c_float)
    lib.surya_rec_set_forced.argtypes, lib.surya_rec_set_forced.restype = [p, i], C.c_int
    lib.surya_rec_set_forced_tokens.argtypes, lib.surya_rec_set_forced_tokens.restype = [p, ip, ip, ip, i, p], C.c_int
    lib.surya_rec_read_forced.argtypes, lib.surya_rec_read_forced.restype = [p, i, ip, fp, fp, p], C.c_int
    lib.surya_rec_wait_forced.argtypes, lib.surya_rec_wait_forced.restype = [p, i, i, ip, fp, fp], C.c_int
    lib.surya_op_lm_head_forced.argtypes, lib.surya_op_lm_head_forced.restype = [i, p, p, p, p, p, i, i, i, p, p, p, ip, p], C.c_int
    # beam search (the n best readings of a line) and its two kernels by themselves
    lib.surya_rec_set_beam.argtypes, lib.surya_rec_set_beam.restype = [p, i, i], C.c_int
    lib.surya_rec_read_beam.argtypes, lib.surya_rec_read_beam.restype = [p, i, ip, ip, ip, fp, fp, p], C.c_int
    lib.surya_rec_wait_beam.argtypes, lib.surya_rec_wait_beam.restype = [p, i, i, ip, ip, ip, fp, fp], C.c_int
    lib.surya_op_rec_beam_select.argtypes = [p, i, i, i, i, p, p, p, p, i, i, i, i, p, p, p, p, p, p, p, p, p, p, p, i, p]
    lib.surya_op_rec_beam_select.restype = C.c_int
    lib.surya_op_rec_kv_fork.argtypes, lib.surya_op_rec_kv_fork.restype = [i, p, p, p, p, p, i, i, i, i, i, i, p], C.c_int
    # one prefill shared by many slots (rank candidate texts) and its fan-out kernel by itself
    lib.surya_rec_prefill_shared.argtypes, lib.surya_rec_prefill_shared.restype = [p, p, ip, i, ip, ip, ip, ip, i, p], C.c_int
    lib.surya_rec_copy_kv_rows.argtypes, lib.surya_rec_copy_kv_rows.restype = [p, i, i, p, p, p], C.c_int
    lib.surya_op_rec_kv_fanout.argtypes, lib.surya_op_rec_kv_fanout.restype = [i, p, p, p, p, p, p, i, i, i, i, i, i, i, p], C.c_int
    # the prompt store (prompts kept across calls: encode once, read / rank / align as often as asked) and its two kernels by themselves
    lib.surya_rec_reserve_prompts.argtypes, lib.surya_rec_reserve_prompts.restype = [p, i, p], C.c_int
    lib.surya_rec_prefill_keep.argtypes, lib.surya_rec_prefill_keep.restype = [p, p, ip, i, ip, ip, ip, i, ip, p], C.c_int
    lib.surya_rec_restore.argtypes, lib.surya_rec_restore.restype = [p, ip, ip, ip, i, p], C.c_int
    lib.surya_rec_drop_prompts.argtypes, lib.surya_rec_drop_prompts.restype = [p, ip, i], C.c_int
    lib.surya_rec_prompt_store_info.argtypes, lib.surya_rec_prompt_store_info.restype = [p, ip, ip], C.c_int
    lib.surya_op_rec_kv_keep.argtypes, lib.surya_op_rec_kv_keep.restype = [i, p, p, p, p, p, p, p, i, i, i, i, i, i, i, p, p, p, i, i, p], C.c_int
    lib.surya_op_rec_kv_restore.argtypes, lib.surya_op_rec_kv_restore.restype = [i, p, p, p, p, p, p, p, p, i, i, i, i, i, i, i, i, p], C.c_int
    # pattern-guided decoding (a slot's mask id follows an automaton over its tokens; recognition/pattern.py compiles the tables)
    lib.surya_rec_set_patterns.argtypes = [p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint16), C.POINTER(C.c_uint8), i, i, p]
    lib.surya_rec_set_patterns.restype = C.c_int
    lib.surya_rec_set_slot_patterns.argtypes, lib.surya_rec_set_slot_patterns.restype = [p, ip, ip, i, p], C.c_int
    lib.surya_rec_copy_slot_states.argtypes, lib.surya_rec_copy_slot_states.restype = [p, p, p], C.c_int
    # lexicon-guided decoding (every slot's own mask row follows a sparse automaton; recognition/lexicon.py compiles the tables)
    lib.surya_rec_set_lexicon.argtypes, lib.surya_rec_set_lexicon.restype = [p, ip, ip, ip, C.POINTER(C.c_uint8), i, i, i, p], C.c_int
    lib.surya_rec_set_slot_lexicon.argtypes, lib.surya_rec_set_slot_lexicon.restype = [p, ip, ip, i, p], C.c_int
    lib.surya_rec_copy_lexicon_states.argtypes, lib.surya_rec_copy_lexicon_states.restype = [p, p, p], C.c_int
    for name in ("surya_op_rec_lexicon_start", "surya_op_rec_lexicon_step"):
        getattr(lib, name).argtypes, getattr(lib, name).restype = [C.POINTER(RecLexiconArgsC), p, p, i, p], C.c_int
    # boosted decoding (a slot's own mask row is its preferred set; recognition/boost.py compiles the tables) and its kernels by themselves
    lib.surya_rec_set_boost.argtypes, lib.surya_rec_set_boost.restype = [p, ip, ip, ip, i, i, i, i, p], C.c_int
    lib.surya_rec_set_slot_boost.argtypes, lib.surya_rec_set_slot_boost.restype = [p, ip, ip, fp, i, p], C.c_int
    lib.surya_rec_copy_boost_states.argtypes, lib.surya_rec_copy_boost_states.restype = [p, p, p], C.c_int
    lib.surya_rec_read_boost.argtypes, lib.surya_rec_read_boost.restype = [p, i, ip, fp, p], C.c_int
    lib.surya_rec_wait_boost.argtypes, lib.surya_rec_wait_boost.restype = [p, i, i, ip, fp], C.c_int
    lib.surya_op_rec_boost_step.argtypes, lib.surya_op_rec_boost_step.restype = [C.POINTER(RecLexiconArgsC), p, i, i, p, p, i, p], C.c_int
    lib.surya_op_rec_boost_head.argtypes, lib.surya_op_rec_boost_head.restype = [i, C.POINTER(RecBoostHeadArgsC), p], C.c_int
    # rectification of rotated line quads in front of surya_rec_preprocess (csrc/rec_rectify.h); `descs` is a host array
    lib.surya_rec_rectify.argtypes, lib.surya_rec_rectify.restype = [p, p, i, p, i, i, i, p], C.c_int
    # unrolling of bent lines along their centre lines, likewise (csrc/rec_unroll.h); `descs` is a host array, `tables` a device one
    lib.surya_rec_unroll.argtypes, lib.surya_rec_unroll.restype = [p, p, i, p, p, i, i, i, p], C.c_int
    # flattening of whole pages through a warp mesh (csrc/page_warp.h; detection/dewarp.py); `descs` is a host array, `meshes` a device one
    lib.surya_warp_mesh.argtypes, lib.surya_warp_mesh.restype = [p, p, i, p, p, i, i, i, p], C.c_int
    # contrast adjustment of line crops in front of surya_rec_preprocess (csrc/rec_adjust.h); `descs` is a host array
    lib.surya_rec_adjust_contrast.argtypes, lib.surya_rec_adjust_contrast.restype = [p, p, i, p, p, p, p, i, p], C.c_int
    # the recogniser's non-GEMM kernels alone (csrc/rec_ops.h): one entry per op, `dtype` first
    rec = {
        "surya_op_rec_rmsnorm_rows": [i, p, l, p, p, l, p, i, i, f, p],
        "surya_op_rec_rows": [i, i, p, p, p, p, p, p, p, ip, p],
        "surya_op_rec_rope_table": [i, i, p, p, p, i, i, p],
        "surya_op_rec_rope_kv_append": [i, p, p, p, p, p, p, i, i, i, i, i, p],
        "surya_op_rec_reduce_norm": [i, p, i, i, p, p, p, i, f, p, p, i, p],
        "surya_op_rec_decode_embed": [i, p, p, p, p, i, p, p, p, p, i, i, f, p, p, i, p],
        "surya_op_rec_head": [i, C.POINTER(RecHeadArgsC), p],
    }
    for name, args in rec.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, C.c_int
    # the OCR-error classifier's kernels alone (csrc/ocr_error_kernels.h): `dtype` first; cls_attn's starts / lengths are host arrays
    ocr = {
        "surya_op_ocrerr_embed_ln": [i, p, p, p, p, p, p, p, i, i, i, f, p],
        "surya_op_ocrerr_layernorm": [i, p, p, p, p, i, i, f, p],
        "surya_op_ocrerr_gather_rows": [i, p, p, p, i, i, p],
        "surya_op_ocrerr_cls_attn": [i, i, p, ip, ip, i, p, i, i, i, f, p],
        "surya_op_ocrerr_cls_head": [i, p, p, p, p, p, i, i, i, p],
        "surya_op_ocrerr_gemm": [i, i, i, p, l, p, p, p, p, i, i, i, p],
    }
    for name, args in ocr.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, C.c_int
    # decode attention with the MXFP8 copy of its output (csrc/rec_model.hip): surya_op_decode_attn / _kv8 + (out8, sout, srows)
    lib.surya_op_decode_attn_mx.argtypes = [i, i, p, i, p, p, p, p, p, p, p, i, i, i, i, f, p, p, p, i]
    lib.surya_op_decode_attn_mx.restype = C.c_int
    lib.surya_op_decode_attn_kv8_mx.argtypes = [i, p, i, p, p, p, p, p, p, p, p, p, i, i, i, i, f, p, p, p, i]
    lib.surya_op_decode_attn_kv8_mx.restype = C.c_int


def bind_det_tile(lib):
    """Tiled detection (csrc/det_tile.h): the cut in front of a forward of tiles and the stitch behind it; `descs` is a DEVICE table.
    Bound by HipDetTiler, not at load: an A/B build from before these entries (SURYA_AMD_LIB) still serves every other path."""
    i, p = C.c_int, C.c_void_p
    lib.surya_det_cut_tiles_u8.argtypes, lib.surya_det_cut_tiles_u8.restype = [p, i, p, i, i, i, p], C.c_int
    lib.surya_det_stitch_tiles.argtypes, lib.surya_det_stitch_tiles.restype = [p, i, i, i, p, i, p], C.c_int
    return lib


def bind_det_skew(lib):
    """Page skew from the heat map (csrc/det_skew.h); `cs` is a DEVICE table. Bound by HipDetSkew, not at load, as bind_det_tile is."""
    i, l, f, p = C.c_int, C.c_long, C.c_float, C.c_void_p
    lib.surya_det_skew_workspace_bytes.argtypes, lib.surya_det_skew_workspace_bytes.restype = [i, i, i], C.c_size_t
    lib.surya_det_skew.argtypes, lib.surya_det_skew.restype = [p, l, i, i, i, f, p, i, p, p, p, C.c_size_t, p], C.c_int
    return lib


def bind_det_centerlines(lib):
    """Centre-line profiles of the kept components (csrc/det_centerline.h), behind surya_det_boxes on its workspace. Bound by
    HipDetCenterlines, not at load, as bind_det_skew is."""
    i, p = C.c_int, C.c_void_p
    lib.surya_det_centerlines.argtypes, lib.surya_det_centerlines.restype = [i, i, i, i, i, p, C.c_size_t, p, p, p, p, p, p], C.c_int
    return lib


def check(rc: int, what: str):
    if rc != 0:
        raise SuryaAmdError(f"{what} failed: {_ERR.get(rc, 'hipError ' + str(rc))} ({rc})")


def ptr(t):
    """Device/host pointer of a torch tensor (or None) as c_void_p."""
    if t is None:
        return C.c_void_p(0)
    return C.c_void_p(t.data_ptr())


def np_ptr(a, ctype=C.c_int32):
    return a.ctypes.data_as(C.POINTER(ctype))
