"""GPU: every decoding mode of one recognition handle switched on, used and switched off again, through HipRecModel's own setters, on
REC-TINY with four slots and two short synthetic lines.

Each mode allocates its device block on its first switch-on (csrc/rec_state.h, DevBlock) and the first lexicon moves the mask arena. In
an order that respects the exclusions -- masks, patterns, lexicon, boost, alternatives, beam, forced, and on bfloat16 the fp8 KV cache and
the MXFP8 decode weights -- each mode runs one prefill and two decode steps. Afterwards, with everything off, tokens, scores and boxes of
a prefill and four steps are bit-identical to those of a handle that never switched anything on. Then the handle is destroyed and two
more are created, used and destroyed. Nothing is asserted about free device memory: other work on the card moves that number."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from util import make_prompts

pytestmark = pytest.mark.gpu
GRIDS = [(6, 38), (10, 18)]


@functools.lru_cache(maxsize=None)
def _inputs():
    from surya_amd.config import rec_config
    from surya_amd.synth import make_rec_weights
    cfg = rec_config("REC-TINY")
    tiles, seqs = make_prompts(cfg, GRIDS)
    special = {cfg.eos_token_id, cfg.pad_token_id, cfg.nop_token_id, cfg.image_token_id}
    toks = [t for t in range(300, 320) if t not in special][:3]                  # three ordinary ids, ascending
    return cfg, make_rec_weights(cfg, 0), tiles, seqs, toks


def _handle(dtype):
    from surya_amd.recognition.model import HipRecModel
    cfg, sd = _inputs()[:2]
    return HipRecModel(cfg, sd, image_token_id=cfg.image_token_id, pad_token_id=cfg.pad_token_id, eos_token_id=cfg.eos_token_id, dtype=dtype,
                       device="cuda:0", max_slots=4, max_kv_len=128, max_patches=1024, max_prefill_tokens=512, decode_fp8=False)


def _run(m, steps, slots=(0, 1), active=None):
    """One prefill of the two lines into `slots` and `steps` decode steps: [(tokens, scores, boxes) of the prefill, ... of the steps]."""
    _, _, tiles, seqs, _ = _inputs()
    slots = list(slots)
    m.prefill(tiles.cuda(), GRIDS, seqs, slots)
    out = [tuple(a[:1, slots].copy() for a in m.read_outputs(1))]
    m.set_active(sorted(active or slots))
    m.decode(steps)
    out.append(tuple(a[:steps, slots].copy() for a in m.read_outputs(steps)))
    return out


def _same_bits(a, b):
    return all(np.array_equal(x.view(np.int32), y.view(np.int32)) for p, q in zip(a, b) for x, y in zip(p, q))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
def test_modes_on_and_off_leave_the_handle_as_new(dtype):
    cfg, _, _, _, toks = _inputs()
    V = cfg.decoder.vocab_size
    fresh = _run(_handle(dtype), 4)

    m = _handle(dtype)
    masks = np.full((2, (V + 31) // 32), 0xffffffff, np.uint32)
    masks[1, toks[0] >> 5] &= ~np.uint32(1 << (toks[0] & 31))                   # row 1: everything but one id
    m.set_token_masks(masks)                                                     # allowed sets
    m.set_slot_masks([0, 1], [1, -1])
    _run(m, 2)
    m.set_patterns(SimpleNamespace(tok_class=np.zeros(V, np.uint8), next_state=np.zeros((1, 1), np.uint16),      # one state, one class, row 0
                                   state_mask=np.zeros(1, np.uint8)))
    m.set_slot_masks([0, 1], [-1, 1])
    m.set_slot_patterns([0, 1], [0, -1])
    _run(m, 2)
    assert list(m.slot_states()[:2]) == [0, -1]
    m.set_patterns(None)
    loop = SimpleNamespace(edge_off=[0, 3], edge_tok=toks, edge_next=[0, 0, 0], state_flags=[1], nop=-1)      # one terminal state, three ids
    m.set_lexicon(loop)                                                          # the first lexicon moves the mask arena
    m.set_slot_masks([0, 1], [-1, 1])
    m.set_slot_lexicon([0, 1], [0, -1])
    out = _run(m, 2)
    assert all(int(t) in toks + [cfg.eos_token_id, cfg.pad_token_id] for p in out for t in p[0][:, 0])      # slot 0 stayed inside the lexicon
    m.set_lexicon(None)
    m.set_boost(SimpleNamespace(edge_off=[0, 1, 1], edge_tok=toks[:1], edge_next=[1], out_state=1, word_row=0))
    m.set_slot_masks([0, 1], [-1, 1])
    m.set_slot_boost([0, 1], [0, -1], 1.5)
    _run(m, 2)
    m.read_boost(2)
    m.set_boost(None)
    m.set_token_masks(None)
    m.set_alternatives(True)
    _run(m, 2)
    m.read_alternatives(2)
    m.set_alternatives(False)
    m.set_beam(2, cfg.pad_token_id)                                              # two groups of two slots
    _run(m, 2, slots=(0, 2), active=(0, 1, 2, 3))
    m.read_beam(2)
    m.set_beam(None)
    m.set_forced(True)
    m.set_forced_tokens([0, 1], [toks, []])
    out = _run(m, 2)
    assert [int(out[0][0][0, 0])] + [int(t) for t in out[1][0][:, 0]] == toks    # slot 0 emitted its forced ids
    m.read_forced(2)
    m.set_forced(False)
    if dtype == torch.bfloat16:
        m.set_kv_fp8(True)
        _run(m, 2)
        m.set_kv_fp8(False)
        m.set_decode_fp8(True)
        _run(m, 2)
        m.set_decode_fp8(False)

    assert _same_bits(_run(m, 4), fresh)
    del m
    for _ in range(2):                                                           # destroy, create, use, destroy
        assert _same_bits(_run(_handle(dtype), 4), fresh)
