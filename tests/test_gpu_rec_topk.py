"""GPU: alternatives through the recognition engine (surya_rec_set_alternatives / surya_rec_read_alternatives / surya_rec_wait_alternatives)
and through RecognitionPredictor.top_k, on REC-SMALL (vocabulary 69 632: the 256 x 320 lm_head tile with a partial last tile).

The reference for a step's alternatives is the engine's own UNMASKED logits of that step (surya_rec_copy_last_logits), masked in torch and
ordered by a stable sort on (-value, column); ids must be equal, probabilities within the rtol = 2e-3 of the other recognition tests
against float64. Tokens, scores and boxes must be BIT-identical to a run with the feature off.
"""
import ctypes as C

import numpy as np
import pytest
import torch
from PIL import Image

from surya_amd import _lib as L
from surya_amd.synth import make_line_crops

from test_gpu_rec_allowlist import (DIGITS, GRIDS, _allowed_rows, _cfg_sd, _max_tokens, _model, _predictor, _run, _table)   # noqa: F401
from util import make_prompts

pytestmark = pytest.mark.gpu
A = L.SA_MAX_ALTERNATIVES
SLOTS, IDS = [0, 1, 2, 3, 4, 5], [0, 1, -1, 0, 1, -1]


def _check_alts(m, cfg, tok, score, at, ap, slots, allowed, what):
    """at / ap [max_slots, 4] of one step against the stable top four of that step's logits over `allowed` (row r = slots[r])."""
    lg = m.last_logits()
    assert lg.shape == (len(slots), cfg.decoder.vocab_size)
    ml = lg.masked_fill(~allowed, float("-inf"))
    order = torch.sort(-ml, dim=1, stable=True).indices[:, :A]
    v = torch.gather(ml, 1, order).double()
    ref_tok = torch.where(torch.isinf(v), torch.full_like(order, -1), order).cpu().numpy()
    tot = torch.exp(ml.double() - v[:, :1]).sum(1, keepdim=True)
    ref_p = torch.where(torch.isinf(v), torch.zeros_like(v), torch.exp(v - v[:, :1]) / tot).cpu().numpy()
    got_tok, got_p = np.asarray(at)[slots], np.asarray(ap)[slots].astype(np.float64)
    assert np.array_equal(got_tok, ref_tok), (what, got_tok.tolist(), ref_tok.tolist())
    rel = np.abs(got_p - ref_p)[ref_tok >= 0] / ref_p[ref_tok >= 0]
    print(f"{what}: max relative probability error {rel.max():.3e}")
    assert (rel <= 2e-3).all(), (what, rel.max())
    assert (got_p[ref_tok < 0] == 0).all()
    # entry 0 is the emitted token, and on rows that go on its probability is the emitted score, bit for bit
    t, s = np.asarray(tok)[slots], np.asarray(score)[slots]
    assert np.array_equal(got_tok[:, 0], t)
    live = ~np.isin(t, [cfg.eos_token_id, cfg.pad_token_id])
    assert np.array_equal(np.asarray(ap)[slots][live, 0].view(np.int32), s[live].view(np.int32)), what
    assert (s[~live] == 0).all() and (got_p[~live, 0] > 0).all()                  # done rows: score 0, alternatives reported all the same
    assert (np.diff(got_p, axis=1) <= 0).all() and (got_p.sum(1) <= 1 + 1e-6).all()


def _steps(m, cfg, allowed, what, steps=6):
    tiles, seqs = make_prompts(cfg, GRIDS, seed=9)
    m.prefill(tiles.cuda(), GRIDS, seqs, SLOTS)
    t, s, _ = m.read_outputs(1)
    at, ap = m.read_alternatives(1)
    _check_alts(m, cfg, t[0], s[0], at[0], ap[0], SLOTS, allowed, f"{what} prefill")
    m.set_active(SLOTS)
    for step in range(steps):
        m.decode(1)
        t, s, _ = m.read_outputs(1)
        at, ap = m.read_alternatives(1)
        _check_alts(m, cfg, t[0], s[0], at[0], ap[0], SLOTS, allowed, f"{what} step {step}")


@pytest.mark.parametrize("dtype,fp8", [(torch.float32, False), (torch.bfloat16, False), (torch.float16, False), (torch.bfloat16, True)])
@pytest.mark.parametrize("masked", [False, True])
def test_every_step_equals_the_recomputation(hip_lib, dtype, fp8, masked):
    """After the prefill and after each of 6 single steps; without a table, and with one on mixed slots (digits / blocklist / -1)."""
    cfg = _cfg_sd()[0]
    m = _model(dtype, decode_fp8=True) if fp8 else _model(dtype)
    m.set_alternatives(True)
    if masked:
        table = _table()
        m.set_token_masks(table)
        m.set_slot_masks(SLOTS, IDS)
        allowed = _allowed_rows(table, IDS, cfg.decoder.vocab_size)
    else:
        allowed = torch.ones(len(SLOTS), cfg.decoder.vocab_size, dtype=torch.bool, device="cuda")
    _steps(m, cfg, allowed, f"{dtype} fp8={fp8} masked={masked}")


def _run_alts(m, slots, steps, single=False):
    """_run of the allowlist tests plus the alternatives [1 + steps, len(slots), 4] x 2."""
    lines = list(range(len(slots)))
    from test_gpu_rec_allowlist import N_LINES, _line
    tiles, seqs = torch.cat([_line(i)[0] for i in lines]), [_line(i)[1] for i in lines]
    m.prefill(tiles.cuda(), [GRIDS[i % N_LINES] for i in lines], seqs, slots)
    t, s, b = m.read_outputs(1)
    at, ap = m.read_alternatives(1)
    out = [(t[0, slots].copy(), s[0, slots].copy(), b[0, slots].copy(), at[0, slots].copy(), ap[0, slots].copy())]
    m.set_active(sorted(slots))
    for k in range(steps if single else 1):
        n = 1 if single else steps
        m.decode(n)
        t, s, b = m.read_outputs(n)
        at, ap = m.read_alternatives(n)
        out += [(t[j, slots].copy(), s[j, slots].copy(), b[j, slots].copy(), at[j, slots].copy(), ap[j, slots].copy()) for j in range(n)]
    return tuple(np.stack([o[i] for o in out]) for i in range(5))


@pytest.mark.parametrize("masked", [False, True])
def test_outputs_are_bit_identical_with_the_feature_on_and_off(hip_lib, masked):
    m = _model(torch.bfloat16)
    if masked:
        m.set_token_masks(_table())
        m.set_slot_masks(SLOTS, IDS)
    off = _run(m, SLOTS, 6)
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.read_alternatives(1)                                                  # read while off
    m.set_alternatives(True)
    if masked:
        m.set_slot_masks(SLOTS, IDS)
    on = _run_alts(m, SLOTS, 6)
    for a, b in zip(off, on[:3]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert np.array_equal(on[3][..., 0], on[0])
    m.set_alternatives(False)
    if masked:
        m.set_slot_masks(SLOTS, IDS)
    again = _run(m, SLOTS, 6)
    for a, b in zip(off, again):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.wait_alternatives(1, 0)


def test_eight_steps_in_one_call_equal_eight_calls(hip_lib):
    m = _model(torch.bfloat16)
    m.set_alternatives(True)
    one = _run_alts(m, SLOTS, 8, single=True)
    eight = _run_alts(m, SLOTS, 8)
    for a, b in zip(one, eight):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_alternatives_do_not_depend_on_the_slot_count(hip_lib):
    """The same 64 lines alone and as the first 64 of 320 active slots (the grouped 256 x 320 launch above 256 rows)."""
    m = _model(torch.bfloat16, max_slots=320)
    m.set_alternatives(True)
    few = _run_alts(m, list(range(64)), 4)
    many = _run_alts(m, list(range(320)), 4)
    for a, b in zip(few, many):
        assert np.array_equal(a.view(np.int32), b[:, :64].view(np.int32))
    assert (few[3] >= 0).all()


def test_decode_async_ring_equals_read(hip_lib):
    m = _model(torch.bfloat16)
    m.set_alternatives(True)
    ref = _run_alts(m, SLOTS, 8)
    from test_gpu_rec_allowlist import N_LINES, _line
    lines = list(range(len(SLOTS)))
    tiles, seqs = torch.cat([_line(i)[0] for i in lines]), [_line(i)[1] for i in lines]
    m.prefill(tiles.cuda(), [GRIDS[i % N_LINES] for i in lines], seqs, SLOTS)
    m.read_outputs(1)
    m.set_active(SLOTS)
    m.decode_async(4, 0)
    m.decode_async(4, 1)
    got_t, got_a, got_p = [], [], []
    for ring in (0, 1):
        t, _, _ = m.wait_outputs(4, ring)
        at, ap = m.wait_alternatives(4, ring)
        got_t.append(t[:, SLOTS].copy()); got_a.append(at[:, SLOTS].copy()); got_p.append(ap[:, SLOTS].copy())
    assert np.array_equal(np.concatenate(got_t), ref[0][1:])
    assert np.array_equal(np.concatenate(got_a), ref[3][1:])
    assert np.array_equal(np.concatenate(got_p).view(np.int32), ref[4][1:].view(np.int32))


def test_a_ring_half_filled_while_off_is_refused(hip_lib):
    """decode_async ran with the feature off, then it is switched on: that ring half mirrored no alternatives, and says so."""
    m = _model(torch.bfloat16)
    _run(m, SLOTS, 0)
    m.decode_async(2, 0)
    m.wait_outputs(2, 0)
    m.set_alternatives(True)
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.wait_alternatives(2, 0)
    m.decode_async(2, 1)
    m.wait_outputs(2, 1)
    at, _ = m.wait_alternatives(2, 1)
    assert (at[:, SLOTS, 0] >= 0).all()


def test_captured_steps_toggled_on_off_on(hip_lib):
    """hipGraph replay on: switching drops the captured steps, so on / off / on give the arrays the eager runs give."""
    m = _model(torch.bfloat16)
    m.set_alternatives(True)
    eager_on = _run_alts(m, SLOTS, 4)
    m.set_alternatives(False)
    eager_off = _run(m, SLOTS, 4)
    L.check(m.lib.surya_set_tuning(b"graph", C.c_int(1)), "surya_set_tuning(graph)")
    try:
        for rnd in range(2):
            m.set_alternatives(True)
            for rep in range(3):                                                # eager, capture, replay
                got = _run_alts(m, SLOTS, 4)
                for a, b in zip(eager_on, got):
                    assert np.array_equal(a.view(np.int32), b.view(np.int32)), (rnd, rep)
            m.set_alternatives(False)
            for rep in range(3):
                got = _run(m, SLOTS, 4)
                for a, b in zip(eager_off, got):
                    assert np.array_equal(a.view(np.int32), b.view(np.int32)), (rnd, rep)
    finally:
        L.check(m.lib.surya_set_tuning(b"graph", C.c_int(0)), "surya_set_tuning(graph)")


def test_refusals(hip_lib):
    m = _model(torch.bfloat16)
    assert m.lib.surya_rec_set_alternatives(m.handle, C.c_int(2)) == L.SA_ERR_ARG
    assert m.lib.surya_rec_set_alternatives(m.handle, C.c_int(-1)) == L.SA_ERR_ARG
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.read_alternatives(1)
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.wait_alternatives(1, 0)


# ------------------------------------------------------------------------------------------------------------------ the predictor
def _chars(results):
    return [c for r in results for ln in r.text_lines for c in ln.chars]


def test_predictor_top_k(hip_lib, _max_tokens):
    pred = _predictor()
    crops = make_line_crops(4, seed=4)
    imgs = [Image.fromarray(c) for c in crops]
    boxes = [[[0, 0, im.size[0], im.size[1]]] for im in imgs]                    # four synthetic lines
    plain = pred(imgs, bboxes=boxes)
    pred.top_k = 3
    out = pred(imgs, bboxes=boxes)
    assert not pred.model.alternatives                                           # switched off on the way out
    chars = _chars(out)
    assert len(chars) > 8
    own = [c for c in chars if c.alternatives is not None]
    assert len(own) >= len(chars) - 8 and own                                    # (None: closing tags the tag fixer inserted)
    for c in own:
        assert len(c.alternatives) == 3
        assert c.alternatives[0].confidence == c.confidence                       # the token the character takes its confidence from
        assert c.alternatives[0].confidence >= c.alternatives[1].confidence >= c.alternatives[2].confidence > 0
    # ... which is the character's own token, exactly, on every line's prefix of plain characters: line_runs maps character i of a UTF-16
    # run to token i, so up to the first surrogate (a pair is one non-BMP character; a dropped lone one shows as an entry 0 without text) or
    # special / math run (bbox_valid False) entry 0 must read what the character reads
    checked = 0
    for ln in (ln for r in out for ln in r.text_lines):
        for c in ln.chars:
            if c.alternatives is None or not c.bbox_valid or len(c.text) != 1 or ord(c.text) > 0xFFFF or c.alternatives[0].text == "":
                break
            assert c.alternatives[0].text == c.text, (ln.text, c.text, c.alternatives[0])
            checked += 1
    print(f"entry 0 == char.text checked on {checked} of {len(own)} characters")
    assert checked >= len(own) // 2, (checked, len(own))
    # texts, confidences and boxes are those of the plain call
    strip = lambda rs: [[{k: v for k, v in ch.items() if k != "alternatives"} for ch in ln["chars"]] for r in rs for ln in r.model_dump()["text_lines"]]
    assert strip(out) == strip(plain) and [ln.text for r in out for ln in r.text_lines] == [ln.text for r in plain for ln in r.text_lines]
    # with an allowlist every alternative is in the list (or a lone surrogate / eos-like id without text)
    pred.top_k = 4
    lim = pred(imgs, bboxes=boxes, allowlist=DIGITS)
    alts = [a for c in _chars(lim) if c.alternatives for a in c.alternatives]
    assert alts and all(a.text == "" or set(a.text) <= set(DIGITS) for a in alts)
    # top_k=None afterwards: today's objects
    pred.top_k = None
    assert [r.model_dump() for r in pred(imgs, bboxes=boxes)] == [r.model_dump() for r in plain]
    pred.top_k = 5
    with pytest.raises(ValueError, match="top_k"):
        pred(imgs, bboxes=boxes)


def test_streamed_call_with_top_k_equals_the_serial_one(hip_lib, _max_tokens):
    from surya_amd.synth import make_pages_with_lines
    from test_gpu_predictors import _det_with_drawn_rows
    size = 256
    pages_np, rows = make_pages_with_lines(3, size, seed=99)
    pages = [Image.fromarray(p) for p in pages_np]
    det = _det_with_drawn_rows(pages, rows, size, 2)
    pred = _predictor(max_slots=8, max_tokens=7)
    pred.stream_detection = False
    pred.top_k = 2
    serial = pred(pages, det_predictor=det)
    assert "streamed" not in pred.last_timing
    pred.stream_detection = True
    streamed = pred(pages, det_predictor=det)
    assert pred.last_timing.get("streamed") == 1.0
    assert [r.model_dump() for r in serial] == [r.model_dump() for r in streamed] and len(streamed) == 3
    assert any(c.alternatives and len(c.alternatives) == 2 for c in _chars(streamed))
