"""HipRecModel: the recognition model behind libsurya_amd.so.

Python here is plumbing only (device memory via torch, stream handle, ctypes marshalling); all arithmetic runs
in the HIP library. There is no fallback: constructing this without the built library or without a GPU raises.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np
import torch

from .. import _lib as L
from ..config import RecConfig
from .weights import repack_rec_weights, pad64


class _StepBufs:
    """Host arrays of one step-output set (outputs / alternatives / forced / beam: csrc/rec_engine.h, StepOutputs) and its two calls,
    surya_rec_read_<name> and surya_rec_wait_<name>. One array [SA_MAX_STEPS, slots, *tail] per field, made by `ensure` when the set is
    first switched on; ring half r is rows r * SA_MAX_STEPS / 2 onwards, so a wait never overwrites what the other half returned."""

    def __init__(self, name, fields, slots):
        self.name, self.fields, self.slots, self.bufs = name, fields, slots, None       # fields: (dtype, tail shape) per argument

    def ensure(self):
        if self.bufs is None:
            self.bufs = tuple(np.zeros((L.SA_MAX_STEPS, self.slots) + tail, dt) for dt, tail in self.fields)

    def _call(self, model, what, first, n_steps, before, after):
        """what(handle, n_steps, *before, one pointer per field, *after), into rows first.. of the arrays; -> the first n_steps of them."""
        bufs = self.bufs
        if bufs is None:                # never switched on: the library refuses below, with buffers it may not write to anyway
            bufs = tuple(np.zeros((1, 1) + tail, dt) for dt, tail in self.fields)
        views = tuple(b[first:] for b in bufs)
        ptrs = [L.np_ptr(v, C.c_float if v.dtype == np.float32 else C.c_int32) for v in views]
        L.check(getattr(model.lib, what)(model.handle, C.c_int(n_steps), *before, *ptrs, *after), what)
        return tuple(v[:n_steps] for v in views)

    def read(self, model, n_steps):
        return self._call(model, "surya_rec_read_" + self.name, 0, n_steps, (), (model._stream,))

    def wait(self, model, n_steps, ring):
        return self._call(model, "surya_rec_wait_" + self.name, ring * (L.SA_MAX_STEPS // 2), n_steps, (C.c_int(ring),), ())


class HipRecModel:
    def __init__(self, cfg: RecConfig, state_dict, *, image_token_id: int, pad_token_id: int, eos_token_id: int,
                 dtype: torch.dtype = torch.bfloat16, device="cuda:0", max_slots: int = 256, max_kv_len: int = 512,
                 max_patches: int = 65536, max_prefill_tokens: Optional[int] = None, broadcast_weights: bool = False,
                 process_group=None, decode_fp8: Optional[bool] = None):
        if not torch.cuda.is_available():
            raise L.SuryaAmdError("HipRecModel needs a GPU (MI355X); there is no CPU fallback")
        self.lib = L.lib()
        self.cfg = cfg
        self.device = torch.device(device)
        self.dtype = dtype
        torch.cuda.set_device(self.device)
        if dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise ValueError("dtype must be float32 (reference mode), bfloat16 or float16")
        e, d = cfg.encoder, cfg.decoder
        self.max_slots = max_slots
        self.vocab = d.vocab_size
        if max_prefill_tokens is None:
            max_prefill_tokens = max_slots * 96
        if broadcast_weights:
            # rank 0 repacks; the other ranks (state_dict may be None there) receive the kernel-layout tensors over RCCL
            from .. import dist as sdist
            rank, _ = sdist.world_info(process_group)
            mine = repack_rec_weights(cfg, state_dict, dtype, self.device) if rank == 0 else None
            self.weights = sdist.share_weights(mine, self.device, src=0, group=process_group)
        else:
            self.weights = repack_rec_weights(cfg, state_dict, dtype, self.device)   # keeps tensors alive
        mask = 0
        for i in e.fullatt_block_indexes:
            mask |= 1 << i
        c = L.RecConfigC(
            enc_depth=e.depth, enc_hidden=e.hidden_size, enc_inter=e.intermediate_size,
            enc_inter_pad=pad64(e.intermediate_size), enc_heads=e.num_heads, patch_dim=e.patch_dim,
            patch_dim_pad=pad64(e.patch_dim), merge=e.spatial_merge_size,
            window_tokens=e.window_size // e.spatial_merge_size // e.patch_size, enc_out_hidden=e.out_hidden_size,
            fullatt_mask=mask, enc_eps=e.rms_norm_eps, vocab=d.vocab_size, dec_hidden=d.hidden_size,
            dec_inter=pad64(d.intermediate_size), dec_layers=d.num_hidden_layers, dec_heads=d.num_attention_heads,
            dec_kv_heads=d.num_key_value_heads, dec_head_dim=d.head_dim, dec_eps=d.rms_norm_eps,
            bbox_size=cfg.bbox_size, embed_multiplier=cfg.image_embed_encoding_multiplier,
            image_token_id=image_token_id, pad_token_id=pad_token_id, eos_token_id=eos_token_id, max_slots=max_slots,
            max_kv_len=max_kv_len, max_patches=max_patches, max_prefill_tokens=max_prefill_tokens,
            dtype={torch.float32: L.DTYPE_F32, torch.bfloat16: L.DTYPE_BF16, torch.float16: L.DTYPE_F16}[dtype])
        self.c = c
        table = (C.c_void_p * len(self.weights))(*[t.data_ptr() for t in self.weights])
        self.handle = C.c_void_p()
        L.check(self.lib.surya_rec_create(C.byref(c), table, len(self.weights), C.byref(self.handle)), "surya_rec_create")
        i32, f32, A = np.int32, np.float32, (L.SA_MAX_ALTERNATIVES,)
        self._out = _StepBufs("outputs", [(i32, ()), (f32, ()), (i32, (6,))], max_slots)
        self._out.ensure()
        self._alt = _StepBufs("alternatives", [(i32, A), (f32, A)], max_slots)               # the other sets: made on first switch-on
        self._forced = _StepBufs("forced", [(i32, ()), (f32, ()), (f32, ())], max_slots)
        self._beam = _StepBufs("beam", [(i32, ()), (i32, ()), (i32, ()), (f32, ()), (f32, ())], max_slots)
        self._boost = _StepBufs("boost", [(i32, ()), (f32, ())], max_slots)
        self.mx_weights = None
        self.n_token_masks = 0
        self.n_pattern_states = 0
        self.n_lexicon_states = 0
        self.n_boost_states = 0
        self.alternatives = False
        self.forced = False
        self.beam = 0
        self.decode_fp8 = False
        if decode_fp8 is None:
            from ..settings import settings
            decode_fp8 = settings.RECOGNITION_DECODE_FP8
        if decode_fp8:
            self.set_decode_fp8(True)
        self.kv_fp8 = False
        from ..settings import settings as _settings
        if _settings.RECOGNITION_KV_FP8:
            self.set_kv_fp8(True)

    def set_decode_fp8(self, on: bool):
        """Decode steps on MXFP8 weights and activations (surya_rec_set_mx_weights; bf16 models only). The e4m3 / e8m0 twins
        of the decoder projections and lm_head are quantised once from the kernel-layout bf16 table and stay resident next to
        it (prefill keeps using the bf16 weights). Holds at every slot count: above 256 active slots the MXFP8 GEMMs take larger tiles
        (csrc/gemm_mx.h) with the same split-K slices and K order, so a line's results do not depend on recognition_batch_size."""
        if on and self.dtype != torch.bfloat16:
            raise ValueError("the fp8 decode path exists for bfloat16 models only")
        if on:
            if self.mx_weights is None:
                from ..mx import repack_rec_mx_weights
                self.mx_weights = repack_rec_mx_weights(self.cfg, self.weights, self.device)
            table = (C.c_void_p * len(self.mx_weights))(*[t.data_ptr() for t in self.mx_weights])
            L.check(self.lib.surya_rec_set_mx_weights(self.handle, table, C.c_int(len(self.mx_weights))), "surya_rec_set_mx_weights")
        else:
            L.check(self.lib.surya_rec_set_mx_weights(self.handle, None, C.c_int(0)), "surya_rec_set_mx_weights")
        torch.cuda.synchronize(self.device)
        self.decode_fp8 = bool(on)

    def set_kv_fp8(self, on: bool):
        """Decode steps on an FP8 (e4m3 + one power-of-two scale per token and kv head) KV cache (surya_rec_set_kv_fp8,
        csrc/decode_attn_kv8.h; bf16 models only). Prefill still attends over the bf16 cache; lines prefilled after the call decode
        from the fp8 arrays. Switch while no line is in flight. One workgroup per (row, kv head): no slot limit, alone or together with
        set_decode_fp8 (tests/test_gpu_fp8_slots.py runs both at 512 slots)."""
        if on and self.dtype != torch.bfloat16:
            raise ValueError("the fp8 KV cache exists for bfloat16 models only")
        L.check(self.lib.surya_rec_set_kv_fp8(self.handle, C.c_int(1 if on else 0)), "surya_rec_set_kv_fp8")
        self.kv_fp8 = bool(on)

    def set_token_masks(self, masks):
        """The call's allowed-id sets (surya_rec_set_token_masks): uint32 [n_masks, ceil(vocab / 32)], bit (c & 31) of word (c >> 5) set =
        id c allowed (OCRTokenizer.token_mask builds a row). None or an empty table switches back to the unmasked lm_head kernels. A new
        table sets every slot back to unconstrained; set_slot_masks names the rows of the slots about to be prefilled."""
        words = (self.vocab + 31) // 32
        if masks is None or len(masks) == 0:
            L.check(self.lib.surya_rec_set_token_masks(self.handle, None, C.c_int(0), self._stream), "surya_rec_set_token_masks")
            self.n_token_masks = self.n_pattern_states = self.n_lexicon_states = self.n_boost_states = 0      # (a new or dropped table switches patterns, the lexicon and boosting off)
            return
        m = np.ascontiguousarray(np.asarray(masks, np.uint32))
        if m.ndim != 2 or m.shape[1] != words:
            raise ValueError(f"token masks must be [n, {words}] uint32 for a vocabulary of {self.vocab}, got {m.shape}")
        L.check(self.lib.surya_rec_set_token_masks(self.handle, L.np_ptr(m, C.c_uint32), C.c_int(m.shape[0]), self._stream),
                "surya_rec_set_token_masks")
        self.n_token_masks, self.n_pattern_states, self.n_lexicon_states, self.n_boost_states = int(m.shape[0]), 0, 0, 0

    def _set_slots(self, name, slots, values):
        """surya_rec_<name>(slots, values): one int32 per slot about to be prefilled."""
        s = np.ascontiguousarray(np.asarray(slots, np.int32))
        v = np.ascontiguousarray(np.asarray(values, np.int32))
        assert s.shape == v.shape and s.ndim == 1
        L.check(getattr(self.lib, "surya_rec_" + name)(self.handle, L.np_ptr(s), L.np_ptr(v), C.c_int(len(s)), self._stream), "surya_rec_" + name)

    def _read_states(self, name) -> np.ndarray:
        """Sync; surya_rec_<name>: one int32 per slot."""
        buf = torch.empty(self.max_slots, dtype=torch.int32, device=self.device)
        L.check(getattr(self.lib, "surya_rec_" + name)(self.handle, L.ptr(buf), self._stream), "surya_rec_" + name)
        return buf.cpu().numpy()

    @staticmethod
    def _csr_arrays(tables):
        """edge_off / edge_tok / edge_next of a sparse automaton as contiguous int32 arrays, and whether their shapes fit each other."""
        eo, et, en = (np.ascontiguousarray(np.asarray(a, np.int32)) for a in (tables.edge_off, tables.edge_tok, tables.edge_next))
        return eo, et, en, eo.ndim == 1 and et.ndim == 1 and en.shape == et.shape

    def set_slot_masks(self, slots, mask_ids):
        """Mask id (row of the table, -1 = unconstrained) of the slots about to be prefilled; a slot keeps it until it is set again."""
        self._set_slots("set_slot_masks", slots, mask_ids)

    def set_patterns(self, tables):
        """The call's pattern automaton (surya_rec_set_patterns; recognition/pattern.py::PatternTables, or anything with its tok_class /
        next_state / state_mask arrays), uploaded behind the token-mask table its state_mask names rows of. None switches the feature
        off. New tables set every slot back to "no pattern"; set_slot_patterns names the start states of the slots about to be prefilled."""
        if tables is None:
            L.check(self.lib.surya_rec_set_patterns(self.handle, None, None, None, C.c_int(0), C.c_int(0), self._stream), "surya_rec_set_patterns")
            self.n_pattern_states = 0
            return
        tc = np.ascontiguousarray(np.asarray(tables.tok_class, np.uint8))
        ns = np.ascontiguousarray(np.asarray(tables.next_state, np.uint16))
        sm = np.ascontiguousarray(np.asarray(tables.state_mask, np.uint8))
        if tc.shape != (self.vocab,) or ns.ndim != 2 or sm.shape != (ns.shape[0],):
            raise ValueError(f"pattern tables must be tok_class [{self.vocab}], next_state [n_states, n_classes], state_mask [n_states], got "
                             f"{tc.shape}, {ns.shape}, {sm.shape}")
        L.check(self.lib.surya_rec_set_patterns(self.handle, L.np_ptr(tc, C.c_uint8), L.np_ptr(ns, C.c_uint16), L.np_ptr(sm, C.c_uint8),
                                                C.c_int(ns.shape[0]), C.c_int(ns.shape[1]), self._stream), "surya_rec_set_patterns")
        self.n_pattern_states = int(ns.shape[0])

    def set_slot_patterns(self, slots, start_states):
        """Start state (-1 = no pattern: the slot keeps its mask id) of the slots about to be prefilled, after set_slot_masks; a state
        >= 0 also sets the slot's mask id to the state's row. A slot's state then follows its tokens on the device."""
        self._set_slots("set_slot_patterns", slots, start_states)

    def slot_states(self) -> np.ndarray:
        """Sync; the automaton state of every slot, int32 [max_slots] (-1 = no pattern). A test hook, like last_logits."""
        return self._read_states("copy_slot_states")

    def set_lexicon(self, tables):
        """The call's lexicon automaton (surya_rec_set_lexicon; recognition/lexicon.py::LexiconTables, or anything with its edge_off /
        edge_tok / edge_next / state_flags arrays and `nop`), uploaded behind the token-mask table: every slot then owns a row of that
        table, which the device rewrites behind each token. None switches the feature off. New tables set every slot back to "no
        lexicon"; set_slot_lexicon names the start states of the slots about to be prefilled."""
        if tables is None:
            L.check(self.lib.surya_rec_set_lexicon(self.handle, None, None, None, None, C.c_int(0), C.c_int(0), C.c_int(-1), self._stream),
                    "surya_rec_set_lexicon")
            self.n_lexicon_states = 0
            return
        eo, et, en, ok = self._csr_arrays(tables)
        fl = np.ascontiguousarray(np.asarray(tables.state_flags, np.uint8))
        if not ok or fl.shape != (len(eo) - 1,):
            raise ValueError(f"lexicon tables must be edge_off [n_states + 1], edge_tok / edge_next [n_edges], state_flags [n_states], got "
                             f"{eo.shape}, {et.shape}, {en.shape}, {fl.shape}")
        L.check(self.lib.surya_rec_set_lexicon(self.handle, L.np_ptr(eo), L.np_ptr(et), L.np_ptr(en), L.np_ptr(fl, C.c_uint8), C.c_int(len(fl)),
                                               C.c_int(len(et)), C.c_int(int(tables.nop)), self._stream), "surya_rec_set_lexicon")
        self.n_lexicon_states = int(len(fl))

    def set_slot_lexicon(self, slots, start_states):
        """Start state (-1 = no lexicon: the slot keeps its mask id) of the slots about to be prefilled, after set_slot_masks; a state
        >= 0 makes the slot's own row its mask id. The slot's state and row then follow its tokens on the device."""
        self._set_slots("set_slot_lexicon", slots, start_states)

    def copy_lexicon_states(self) -> np.ndarray:
        """Sync; the lexicon state of every slot, int32 [max_slots] (-1 = no lexicon). A test hook, like slot_states."""
        return self._read_states("copy_lexicon_states")

    def set_boost(self, tables):
        """The call's boost automaton (surya_rec_set_boost; recognition/boost.py::BoostTables, or anything with its edge_off / edge_tok /
        edge_next arrays, `out_state` and `word_row`, the row of the uploaded token-mask table that holds the word-unit set), uploaded
        behind the token-mask table. None switches the feature off. New tables set every slot back to "not boosted"; set_slot_boost
        names root and beta of the slots about to be prefilled."""
        if tables is None:
            L.check(self.lib.surya_rec_set_boost(self.handle, None, None, None, C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), self._stream),
                    "surya_rec_set_boost")
            self.n_boost_states = 0
            return
        eo, et, en, ok = self._csr_arrays(tables)
        if not ok or len(eo) < 2:
            raise ValueError(f"boost tables must be edge_off [n_states + 1], edge_tok / edge_next [n_edges], got {eo.shape}, {et.shape}, {en.shape}")
        L.check(self.lib.surya_rec_set_boost(self.handle, L.np_ptr(eo), L.np_ptr(et), L.np_ptr(en), C.c_int(len(eo) - 1), C.c_int(len(et)),
                                             C.c_int(int(tables.out_state)), C.c_int(int(tables.word_row)), self._stream), "surya_rec_set_boost")
        self.n_boost_states = int(len(eo) - 1)
        self._boost.ensure()

    def set_slot_boost(self, slots, roots, betas):
        """Root state (-1 = not boosted: the slot keeps its mask id) and beta (logit units, finite, >= 0; a scalar or one per slot) of the
        slots about to be prefilled, after set_slot_masks. The slot's state and row then follow its tokens on the device."""
        s = np.ascontiguousarray(np.asarray(slots, np.int32))
        r = np.ascontiguousarray(np.asarray(roots, np.int32))
        b = np.ascontiguousarray(np.broadcast_to(np.asarray(betas, np.float32), s.shape))
        assert s.shape == r.shape and s.ndim == 1
        L.check(self.lib.surya_rec_set_slot_boost(self.handle, L.np_ptr(s), L.np_ptr(r), L.np_ptr(b, C.c_float), C.c_int(len(s)), self._stream),
                "surya_rec_set_slot_boost")

    def copy_boost_states(self) -> np.ndarray:
        """Sync; the boost state of every slot, int32 [max_slots] (-1 = not boosted). A test hook, like slot_states."""
        return self._read_states("copy_boost_states")

    def read_boost(self, n_steps: int = 1):
        """Sync; (plain_tokens [n_steps, slots] int32, plain_probs [n_steps, slots] float32) of the steps read_outputs returns: the token
        the model would have emitted without the boost, and the emitted token's probability without the boost."""
        return self._boost.read(self, n_steps)

    def wait_boost(self, n_steps: int, ring: int):
        """The boost outputs of the decode_async call on `ring`, parallel to wait_outputs."""
        return self._boost.wait(self, n_steps, ring)

    def set_alternatives(self, on: bool):
        """Report the SA_MAX_ALTERNATIVES most likely (allowed) tokens of every step beside the token itself (surya_rec_set_alternatives).
        Off (the default) the handle launches the kernels it always launched; tokens, scores and boxes are the same either way."""
        L.check(self.lib.surya_rec_set_alternatives(self.handle, C.c_int(1 if on else 0)), "surya_rec_set_alternatives")
        self.alternatives = bool(on)
        if on:
            self._alt.ensure()

    def read_alternatives(self, n_steps: int = 1):
        """Sync; (tokens [n_steps, slots, 4] int32, -1 = fewer ids allowed; probs [n_steps, slots, 4]) of the steps read_outputs returns,
        best first: entry 0 is the emitted token."""
        return self._alt.read(self, n_steps)

    def wait_alternatives(self, n_steps: int, ring: int):
        """The alternatives of the decode_async call on `ring`, parallel to wait_outputs."""
        return self._alt.wait(self, n_steps, ring)

    def set_forced(self, on: bool):
        """Forced decoding (surya_rec_set_forced): slots with forced ids (set_forced_tokens) emit them instead of the greedy token and
        report the ids' probabilities. Off (the default) the handle launches the kernels it always launched. Not together with token
        masks or alternatives."""
        L.check(self.lib.surya_rec_set_forced(self.handle, C.c_int(1 if on else 0)), "surya_rec_set_forced")
        self.forced = bool(on)
        if on:
            self._forced.ensure()

    def set_forced_tokens(self, slots, ids):
        """ids[i]: the token ids slot slots[i] is forced to from its next prefill on, one per head pass, the prefill's included (an
        empty list: the slot free-runs). Call for the slots about to be prefilled."""
        s = np.ascontiguousarray(slots, np.int32)
        offs = np.zeros(len(ids) + 1, np.int32)
        np.cumsum([len(x) for x in ids], out=offs[1:])
        flat = np.ascontiguousarray([t for x in ids for t in x], np.int32) if offs[-1] else np.zeros(1, np.int32)
        if len(s) != len(ids):
            raise ValueError("set_forced_tokens: one id list per slot")
        L.check(self.lib.surya_rec_set_forced_tokens(self.handle, L.np_ptr(s), L.np_ptr(flat), L.np_ptr(offs), C.c_int(len(s)), self._stream),
                "surya_rec_set_forced_tokens")

    def read_forced(self, n_steps: int = 1):
        """Sync; (greedy_tokens [n_steps, slots] int32, greedy_probs, forced_logprobs [n_steps, slots] float32) of the steps read_outputs
        returns: the model's own argmax and its probability, and the log-probability of the token that was emitted."""
        return self._forced.read(self, n_steps)

    def wait_forced(self, n_steps: int, ring: int):
        """The forced-decoding outputs of the decode_async call on `ring`, parallel to wait_outputs."""
        return self._forced.wait(self, n_steps, ring)

    def set_beam(self, width: Optional[int], no_output_token_id: int = -1):
        """Beam search (surya_rec_set_beam): `width` in 2..SA_MAX_BEAMS keeps the `width` best readings of every line in a group of `width`
        consecutive slots (prefill names lead slots, set_active whole groups); None or 0 switches it off, and the handle launches the
        kernels it always launched. Not together with forced decoding, the fp8 KV cache or MXFP8 decode weights."""
        w = int(width or 0)
        L.check(self.lib.surya_rec_set_beam(self.handle, C.c_int(w), C.c_int(no_output_token_id)), "surya_rec_set_beam")
        self.beam = w
        if w:
            self._beam.ensure()
            self._alt.ensure()                              # read_alternatives works in beam mode

    def read_beam(self, n_steps: int = 1):
        """Sync; (tokens, parents, ranks [n_steps, slots] int32, probs, logps [n_steps, slots] float32) of the steps read_outputs returns:
        per slot the beam placed there by the step's selection -- its token (pad: frozen or empty), the slot index inside the group it came
        from (own index: stayed in place, -1: empty), which alternative of the parent it took, that token's probability and the cumulative
        log-probability. The box of a beam is read_outputs' box of its parent's slot."""
        return self._beam.read(self, n_steps)

    def wait_beam(self, n_steps: int, ring: int):
        """The beam outputs of the decode_async call on `ring`, parallel to wait_outputs."""
        return self._beam.wait(self, n_steps, ring)

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            self.lib.surya_rec_destroy(h)
            self.handle = None

    @property
    def config(self):
        """The reference reads `model.config.bbox_size` (recognition/__init__.py:315) and friends off the module."""
        return self.cfg

    def to(self, device_dtype=None):
        """BasePredictor.to calls model.to(...) (surya/common/predictor.py:31-35). Weights, KV slots and workspaces of a
        handle live on the device it was created on, in the dtype it was created with; asking for the same placement is
        a no-op, anything else needs a new handle (construct a new predictor) -- refuse loudly rather than pretend."""
        if device_dtype is None:
            return self
        want_dev, want_dt = None, None
        if isinstance(device_dtype, torch.dtype):
            want_dt = device_dtype
        else:
            want_dev = torch.device("cuda:0" if device_dtype == "cuda" else device_dtype)
        if (want_dt is not None and want_dt != self.dtype) or (want_dev is not None and want_dev != self.device):
            raise NotImplementedError(f"HipRecModel lives on {self.device} as {self.dtype}; create a new predictor for "
                                      f"{device_dtype} (the HIP handle owns device memory; there is no CPU path)")
        return self

    def eval(self):
        return self

    @property
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ---------------------------------------------------------------------------------------------- calls
    def prefill(self, tiles: torch.Tensor, grid_hw, input_ids: Sequence[Sequence[int]], slot_ids: Sequence[int]):
        """tiles: cuda fp32 [P, patch_dim], or None to consume embeddings queued by encode_ahead; grid_hw: [n_images, 2];
        input_ids: per-sequence prompt ids."""
        torch.cuda.set_device(self.device)
        grid = np.ascontiguousarray(np.asarray(grid_hw, np.int32).reshape(-1, 2))
        offs = np.zeros(len(input_ids) + 1, np.int32)
        offs[1:] = np.cumsum([len(s) for s in input_ids])
        flat = np.ascontiguousarray(np.concatenate([np.asarray(s, np.int32) for s in input_ids]))
        slots = np.ascontiguousarray(np.asarray(slot_ids, np.int32))
        if tiles is not None:
            assert tiles.is_cuda and tiles.dtype == torch.float32 and tiles.is_contiguous()
            assert tiles.shape[0] == int((grid[:, 0] * grid[:, 1]).sum()) and tiles.shape[1] == self.cfg.encoder.patch_dim
        L.check(self.lib.surya_rec_prefill(self.handle, L.ptr(tiles), L.np_ptr(grid), C.c_int(len(grid)), L.np_ptr(flat),
                                           L.np_ptr(offs), L.np_ptr(slots), C.c_int(len(slots)), self._stream),
                "surya_rec_prefill")

    def prefill_shared(self, tiles: torch.Tensor, grid_hw, input_ids: Sequence[Sequence[int]], fan_slots: Sequence[Sequence[int]]):
        """`prefill` with one prompt shared by several slots (surya_rec_prefill_shared): fan_slots[i] holds the slots of sequence i, any
        distinct ones, at least one. The sequence is encoded and prefilled once, into fan_slots[i][0]; every slot of the list then holds
        its prompt rows, its length and a first token of its own (with forced decoding on: its own forced id). Not with beam search or
        the fp8 KV cache."""
        torch.cuda.set_device(self.device)
        grid = np.ascontiguousarray(np.asarray(grid_hw, np.int32).reshape(-1, 2))
        if len(fan_slots) != len(input_ids):
            raise ValueError("prefill_shared: one slot list per sequence")
        offs = np.zeros(len(input_ids) + 1, np.int32)
        offs[1:] = np.cumsum([len(s) for s in input_ids])
        flat = np.ascontiguousarray(np.concatenate([np.asarray(s, np.int32) for s in input_ids]))
        foffs = np.zeros(len(fan_slots) + 1, np.int32)
        foffs[1:] = np.cumsum([len(f) for f in fan_slots])
        slots = np.ascontiguousarray([s for f in fan_slots for s in f], np.int32) if foffs[-1] else np.zeros(1, np.int32)
        if tiles is not None:
            assert tiles.is_cuda and tiles.dtype == torch.float32 and tiles.is_contiguous()
            assert tiles.shape[0] == int((grid[:, 0] * grid[:, 1]).sum()) and tiles.shape[1] == self.cfg.encoder.patch_dim
        L.check(self.lib.surya_rec_prefill_shared(self.handle, L.ptr(tiles), L.np_ptr(grid), C.c_int(len(grid)), L.np_ptr(flat), L.np_ptr(offs),
                                                  L.np_ptr(foffs), L.np_ptr(slots), C.c_int(len(fan_slots)), self._stream),
                "surya_rec_prefill_shared")

    # ---- the prompt store (surya_rec_reserve_prompts ...): prompts kept on the device across calls; EncodedLines (encoded.py) hands out its rows
    def reserve_prompts(self, rows: int):
        """The store holds at least `rows` rows afterwards; growing keeps the live entries' bytes."""
        torch.cuda.set_device(self.device)
        L.check(self.lib.surya_rec_reserve_prompts(self.handle, C.c_int(int(rows)), self._stream), "surya_rec_reserve_prompts")

    def prefill_keep(self, tiles: torch.Tensor, grid_hw, input_ids: Sequence[Sequence[int]], slot_ids: Sequence[int], keep_first: Sequence[int]):
        """`prefill` that also keeps prompts (surya_rec_prefill_keep): sequence i with keep_first[i] >= 0 leaves its prompt rows and its last
        hidden row in the store at rows [keep_first[i], keep_first[i] + len(input_ids[i])). Not with the fp8 KV cache."""
        torch.cuda.set_device(self.device)
        grid = np.ascontiguousarray(np.asarray(grid_hw, np.int32).reshape(-1, 2))
        offs = np.zeros(len(input_ids) + 1, np.int32)
        offs[1:] = np.cumsum([len(s) for s in input_ids])
        flat = np.ascontiguousarray(np.concatenate([np.asarray(s, np.int32) for s in input_ids]))
        slots = np.ascontiguousarray(np.asarray(slot_ids, np.int32))
        keep = np.ascontiguousarray(np.asarray(keep_first, np.int32))
        if keep.shape != slots.shape:
            raise ValueError("prefill_keep: one store row (or -1) per sequence")
        if tiles is not None:
            assert tiles.is_cuda and tiles.dtype == torch.float32 and tiles.is_contiguous()
            assert tiles.shape[0] == int((grid[:, 0] * grid[:, 1]).sum()) and tiles.shape[1] == self.cfg.encoder.patch_dim
        L.check(self.lib.surya_rec_prefill_keep(self.handle, L.ptr(tiles), L.np_ptr(grid), C.c_int(len(grid)), L.np_ptr(flat), L.np_ptr(offs),
                                                L.np_ptr(slots), C.c_int(len(slots)), L.np_ptr(keep), self._stream), "surya_rec_prefill_keep")

    def restore(self, first: Sequence[int], fan_slots: Sequence[Sequence[int]]):
        """Land kept prompts in slots (surya_rec_restore): entry first[i] goes to every slot of fan_slots[i], each of which then holds the
        prompt's rows, its length and a first token of its own, as after `prefill` / `prefill_shared`. With beam search on every list is
        one lead slot. Not with the fp8 KV cache."""
        torch.cuda.set_device(self.device)
        if len(fan_slots) != len(first):
            raise ValueError("restore: one slot list per entry")
        f = np.ascontiguousarray(np.asarray(first, np.int32))
        foffs = np.zeros(len(fan_slots) + 1, np.int32)
        foffs[1:] = np.cumsum([len(x) for x in fan_slots])
        slots = np.ascontiguousarray([s for x in fan_slots for s in x], np.int32) if foffs[-1] else np.zeros(1, np.int32)
        L.check(self.lib.surya_rec_restore(self.handle, L.np_ptr(f), L.np_ptr(foffs), L.np_ptr(slots), C.c_int(len(f)), self._stream),
                "surya_rec_restore")

    def drop_prompts(self, first: Sequence[int]):
        """Forget entries (host bookkeeping only)."""
        f = np.ascontiguousarray(np.asarray(first, np.int32))
        L.check(self.lib.surya_rec_drop_prompts(self.handle, L.np_ptr(f), C.c_int(len(f))), "surya_rec_drop_prompts")

    def prompt_store_info(self):
        """(capacity in rows, live entries) of the store. A test hook."""
        cap, live = C.c_int32(0), C.c_int32(0)
        L.check(self.lib.surya_rec_prompt_store_info(self.handle, C.byref(cap), C.byref(live)), "surya_rec_prompt_store_info")
        return int(cap.value), int(live.value)

    def encode_ahead(self, tiles: torch.Tensor, grid_hw):
        """Encode the images of the next prompts on the library's low-priority stream (overlaps with decode steps); the
        following prefill(None, ...) calls consume the embeddings in this order."""
        torch.cuda.set_device(self.device)
        grid = np.ascontiguousarray(np.asarray(grid_hw, np.int32).reshape(-1, 2))
        assert tiles.is_cuda and tiles.dtype == torch.float32 and tiles.is_contiguous()
        assert tiles.shape[0] == int((grid[:, 0] * grid[:, 1]).sum()) and tiles.shape[1] == self.cfg.encoder.patch_dim
        L.check(self.lib.surya_rec_encode_ahead(self.handle, L.ptr(tiles), L.np_ptr(grid), C.c_int(len(grid)), self._stream),
                "surya_rec_encode_ahead")

    def discard_ahead(self):
        """Forget look-ahead embeddings nobody consumed (a loop that ended early, e.g. on an exception): the next encode_ahead starts clean."""
        L.check(self.lib.surya_rec_encode_ahead(self.handle, None, None, C.c_int(0), self._stream), "surya_rec_encode_ahead(discard)")

    def set_active(self, slots: Sequence[int]):
        a = np.ascontiguousarray(np.asarray(slots, np.int32))
        L.check(self.lib.surya_rec_set_active(self.handle, L.np_ptr(a), C.c_int(len(a)), self._stream), "surya_rec_set_active")

    def decode(self, n_steps: int = 1):
        L.check(self.lib.surya_rec_decode(self.handle, C.c_int(n_steps), self._stream), "surya_rec_decode")

    def read_outputs(self, n_steps: int = 1):
        """Sync; returns (tokens [n_steps, slots], scores, bboxes [n_steps, slots, 6]) numpy views."""
        return self._out.read(self, n_steps)

    def decode_async(self, n_steps: int, ring: int):
        """Enqueue n_steps (<= SA_MAX_STEPS / 2) decode steps whose outputs land in ring half `ring`; no sync."""
        L.check(self.lib.surya_rec_decode_async(self.handle, C.c_int(n_steps), C.c_int(ring), self._stream), "surya_rec_decode_async")

    def wait_outputs(self, n_steps: int, ring: int):
        """Block until the decode_async call on `ring` finished (later calls may still be queued); copies of the outputs."""
        return self._out.wait(self, n_steps, ring)

    def set_next_tokens(self, slots, tokens):
        s = np.ascontiguousarray(np.asarray(slots, np.int32))
        t = np.ascontiguousarray(np.asarray(tokens, np.int32))
        L.check(self.lib.surya_rec_set_next_tokens(self.handle, L.np_ptr(s), L.np_ptr(t), C.c_int(len(s)), self._stream),
                "surya_rec_set_next_tokens")

    def encode_only(self, tiles: torch.Tensor, grid_hw) -> torch.Tensor:
        grid = np.ascontiguousarray(np.asarray(grid_hw, np.int32).reshape(-1, 2))
        ntok = int((grid[:, 0] * grid[:, 1]).sum()) // (self.cfg.encoder.spatial_merge_size ** 2)
        out = torch.empty((ntok, self.cfg.decoder.hidden_size), dtype=self.dtype, device=self.device)
        L.check(self.lib.surya_rec_encode_only(self.handle, L.ptr(tiles), L.np_ptr(grid), C.c_int(len(grid)), L.ptr(out),
                                               self._stream), "surya_rec_encode_only")
        return out

    def kv_rows(self, slot: int, rows: int):
        """Sync; (K, V) [layers, kv_heads, rows, head_dim] of the first `rows` cache rows of `slot`, in the model's dtype. A test hook, like
        last_logits."""
        d = self.cfg.decoder
        shape = (d.num_hidden_layers, d.num_key_value_heads, rows, d.head_dim)
        k, v = torch.empty(shape, dtype=self.dtype, device=self.device), torch.empty(shape, dtype=self.dtype, device=self.device)
        L.check(self.lib.surya_rec_copy_kv_rows(self.handle, C.c_int(slot), C.c_int(rows), L.ptr(k), L.ptr(v), self._stream), "surya_rec_copy_kv_rows")
        torch.cuda.synchronize(self.device)
        return k, v

    def last_logits(self) -> torch.Tensor:
        """fp32 logits of the last prefill / decode step, recomputed; with token masks set these are still the UNMASKED logits."""
        buf = torch.empty((self.max_slots, self.vocab), dtype=torch.float32, device=self.device)
        rows = C.c_int(0)
        L.check(self.lib.surya_rec_copy_last_logits(self.handle, L.ptr(buf), C.c_int(self.max_slots), C.byref(rows),
                                                    self._stream), "surya_rec_copy_last_logits")
        return buf[: rows.value]
