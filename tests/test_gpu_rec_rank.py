"""GPU: one prefill shared by many slots (surya_rec_prefill_shared, csrc/kv_fanout.h) through the recognition engine and through
RecognitionPredictor.rank, on REC-SMALL, six slots in use.

The reference is what exists without the feature: surya_rec_prefill of the same lines REPEATED into the same slots. Nothing in a row of
the prefill or of a decode step depends on which other rows its launch holds (the "8 x 1 = 8" tests pin that), and the fan-out moves
bytes, so the two arrangements must agree bit for bit: tokens, score bits, boxes, and under forcing the greedy tokens, their
probabilities and the forced log-probabilities, at the prefill's outputs and at every step, for every slot."""
import ctypes as C

import numpy as np
import pytest
import torch
from PIL import Image

from surya_amd import _lib as L
from surya_amd.settings import settings
from surya_amd.synth import make_line_crops

from test_gpu_rec_allowlist import GRIDS, N_LINES, _cfg_sd, _line, _max_tokens, _model, _predictor, _run   # noqa: F401
from test_gpu_rec_forced import ARITH, _bits, _forced_mask, _ids

pytestmark = pytest.mark.gpu
FANS = [[0, 2, 5], [3, 1]]                  # line 0 into slots 0 (lead), 2, 5; line 1 into 3 (lead), 1; slot 4 in no fan
NAMED = [s for f in FANS for s in f]
LINES = [0, 1]
LENS = [5, 7, 1, 3, 6]                      # forced ids per named slot, in NAMED's order; the second list ends in eos


def _make(dtype, fp8, **kw):
    return _model(dtype, decode_fp8=True, **kw) if fp8 else _model(dtype, **kw)


def _forced_lists():
    return [_ids(40 + r, n, end_eos=(r == 1)) for r, n in enumerate(LENS)]


def _tiles(lines):
    return torch.cat([_line(i)[0] for i in lines]).cuda()


def _prefill_shared(m, fans=FANS, lines=LINES, ids=None, ahead=False):
    if ids is not None:
        m.set_forced_tokens([s for f in fans for s in f], ids)
    grids, seqs = [GRIDS[i % N_LINES] for i in lines], [_line(i)[1] for i in lines]
    if ahead:
        m.encode_ahead(_tiles(lines), grids)
    m.prefill_shared(None if ahead else _tiles(lines), grids, seqs, fans)


def _prefill_repeated(m, fans=FANS, lines=LINES, ids=None):
    """What the engine offers without the feature: every line once per slot of its fan."""
    rep = [ln for ln, f in zip(lines, fans) for _ in f]
    named = [s for f in fans for s in f]
    if ids is not None:
        m.set_forced_tokens(named, ids)
    m.prefill(_tiles(rep), [GRIDS[i % N_LINES] for i in rep], [_line(i)[1] for i in rep], named)


def _outs(m, slots, n, forced):
    t, s, b = m.read_outputs(n)
    f = m.read_forced(n) if forced else ()
    return [tuple(a[j, slots].copy() for a in (t, s, b) + tuple(f)) for j in range(n)]


def _arrange(m, prefill, steps, ids=None, slots=NAMED, **kw):
    """prefill(m, ids=ids, ...), then `steps` decode steps of `slots` in one call -> (tokens, scores, boxes[, greedy tokens, greedy
    probabilities, log-probabilities]), each [1 + steps, len(slots)(, 6)]."""
    prefill(m, ids=ids, **kw)
    out = _outs(m, slots, 1, ids is not None)
    m.set_active(sorted(slots))
    m.decode(steps)
    out += _outs(m, slots, steps, ids is not None)
    return tuple(np.stack([o[i] for o in out]) for i in range(len(out[0])))


def _same_bits(a, b, what):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y)), f"{what}: output {k} differs in some bit"


@pytest.mark.parametrize("dtype,fp8", ARITH)
def test_shared_prefill_equals_the_repeated_prefill_forcing_off(hip_lib, dtype, fp8):
    """(a) Two lines into fans [0, 2, 5] and [3, 1], six decode steps: every slot of a fan runs the greedy stream of its line, with the bits
    of the arrangement that prefills the line once per slot."""
    m = _make(dtype, fp8)
    got = _arrange(m, _prefill_shared, 6)
    ref = _arrange(m, _prefill_repeated, 6)
    _same_bits(got, ref, "shared vs repeated prefill")
    tok = got[0]
    assert np.array_equal(tok[:, 0], tok[:, 1]) and np.array_equal(tok[:, 0], tok[:, 2]) and np.array_equal(tok[:, 3], tok[:, 4])
    assert not np.array_equal(tok[:, 0], tok[:, 3]), "the two lines read the same: the test distinguishes nothing"
    assert (got[1] > 0).any()


@pytest.mark.parametrize("dtype,fp8", ARITH)
def test_shared_prefill_equals_the_repeated_prefill_forcing_on(hip_lib, dtype, fp8):
    """(b) The same two arrangements with a forced list of its own per slot (5, 7, 1, 3 and 6 ids, one ending in eos), seven steps, so
    every list runs out: forced log-probabilities, greedy tokens and greedy probabilities are bit-equal, every forced position emitted
    its id, and past its list a slot goes on as a slot of the repeated arrangement does."""
    m = _make(dtype, fp8)
    ids, steps = _forced_lists(), 7
    m.set_forced(True)
    got = _arrange(m, _prefill_shared, steps, ids=ids)
    ref = _arrange(m, _prefill_repeated, steps, ids=ids)
    m.set_forced(False)
    _same_bits(got, ref, "shared vs repeated prefill, forced")
    on, val = _forced_mask(ids, steps)
    assert on.any() and (~on).any() and np.array_equal(got[0][on], val[on]), "a forced position did not emit its id"
    lp = got[5]
    assert (lp <= 0).all() and np.isfinite(lp).all()
    # slots of one fan share the prompt, so the FIRST token's greedy reading is one per line, whatever each slot is forced to
    assert len(set(got[3][0, :3].tolist())) == 1 and len(set(got[3][0, 3:].tolist())) == 1


def test_a_slot_in_no_fan_is_untouched(hip_lib):
    """(c) Slot 4 holds another line, two steps in, when the shared prefill runs: its cache rows are byte-equal before and after, and its
    stream before and after equals the run of a handle on which the shared prefill never happened. The fan slots hold the lead's rows."""
    def slot4(m, between):
        m.prefill(_tiles([5]), [GRIDS[5 % N_LINES]], [_line(5)[1]], [4])
        out = _outs(m, [4], 1, False)
        m.set_active([4])
        m.decode(2)
        out += _outs(m, [4], 2, False)
        between(m)
        m.set_active([4])
        m.decode(3)
        out += _outs(m, [4], 3, False)
        return tuple(np.stack([o[i] for o in out]) for i in range(3))

    rows = len(_line(5)[1]) + 2
    seen = {}

    def shared(m):
        seen["before"] = m.kv_rows(4, rows)
        _prefill_shared(m)
        m.read_outputs(1)
        seen["after"] = m.kv_rows(4, rows)
        for lead, others, line in ((0, (2, 5), 0), (3, (1,), 1)):
            n = len(_line(line)[1])
            k0, v0 = m.kv_rows(lead, n)
            for s in others:
                k, v = m.kv_rows(s, n)
                assert torch.equal(k.view(torch.int16), k0.view(torch.int16)) and torch.equal(v.view(torch.int16), v0.view(torch.int16))
        assert not torch.equal(m.kv_rows(0, 4)[0].view(torch.int16), m.kv_rows(3, 4)[0].view(torch.int16))
    got = slot4(_model(torch.bfloat16), shared)
    ref = slot4(_model(torch.bfloat16), lambda m: None)
    _same_bits(got, ref, "slot 4 with and without a shared prefill beside it")
    for a, b in zip(seen["before"], seen["after"]):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and a.view(torch.int16).any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_encoded_ahead_equals_tiles_given(hip_lib, dtype):
    """(d) tiles = None after encode_ahead gives the outputs of the call that brings its tiles."""
    m = _model(dtype)
    given = _arrange(m, _prefill_shared, 3)
    ahead = _arrange(m, _prefill_shared, 3, ahead=True)
    _same_bits(given, ahead, "tiles given vs encoded ahead")


def test_refusals_change_nothing(hip_lib):
    """(e) Every SA_ERR_ARG case comes back before anything is enqueued or changed: six lines two steps in go on, and a plain prefill +
    decode afterwards runs, with the bits of a fresh handle. SA_ERR_STATE with beam search and with the fp8 KV cache."""
    cfg = _cfg_sd()[0]
    m, fresh = _model(torch.bfloat16), _model(torch.bfloat16)
    slots = [0, 1, 2, 3, 4, 5]
    a, b = _run(m, slots, 2), _run(fresh, slots, 2)
    _same_bits(a, b, "two handles")
    for fans in ([[0, 2], []], [[], [0]], [[0, 8]], [[0, -1]], [[0, 2], [2]], [[0, 0]], [[0, 1, 2, 3, 4], [5, 6, 7, 0]]):
        with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
            _prefill_shared(m, fans=fans, lines=LINES[:len(fans)])
    # offsets that do not start at 0, or go back: only the C call can say that
    grids = np.ascontiguousarray(np.asarray([GRIDS[i % N_LINES] for i in LINES], np.int32))
    seqs = [_line(i)[1] for i in LINES]
    offs = np.zeros(3, np.int32)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    flat = np.ascontiguousarray(np.concatenate([np.asarray(s, np.int32) for s in seqs]))
    fslots = np.asarray([0, 2, 5, 3, 1], np.int32)
    t = _tiles(LINES)
    for foffs in ([0, 3, 2], [1, 3, 5], [0, 3, 3], [0, 5, 9]):
        fo = np.asarray(foffs, np.int32)
        rc = m.lib.surya_rec_prefill_shared(m.handle, L.ptr(t), L.np_ptr(grids), C.c_int(2), L.np_ptr(flat), L.np_ptr(offs), L.np_ptr(fo),
                                            L.np_ptr(fslots), C.c_int(2), m._stream)
        assert rc == L.SA_ERR_ARG, foffs
    for mm in (m, fresh):
        mm.decode(2)
    stack = lambda outs: tuple(np.stack([o[i] for o in outs]) for i in range(3))
    _same_bits(stack(_outs(m, slots, 2, False)), stack(_outs(fresh, slots, 2, False)), "the lines in flight after the refused calls")
    _same_bits(_run(m, slots, 3), _run(fresh, slots, 3), "a plain prefill and decode after the refused calls")
    m.set_beam(2, cfg.pad_token_id)
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        _prefill_shared(m)
    m.set_beam(None)
    m.set_kv_fp8(True)
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        _prefill_shared(m)
    m.set_kv_fp8(False)
    _same_bits(_arrange(m, _prefill_shared, 2), _arrange(fresh, _prefill_shared, 2), "a shared prefill after the refusals")


def test_plain_calls_after_shared_prefills_equal_a_fresh_handle(hip_lib):
    """(f) Shared prefills, forced and free, single-slot fans included, leave nothing behind: prefill + decode on the same handle has the
    bits of a fresh one."""
    m, fresh = _model(torch.bfloat16), _model(torch.bfloat16)
    _arrange(m, _prefill_shared, 4)
    m.set_forced(True)
    _arrange(m, _prefill_shared, 4, ids=_forced_lists())
    m.set_forced(False)
    one = _arrange(m, _prefill_shared, 2, fans=[[4], [1]], slots=[4, 1])      # fans of one slot: nothing to copy
    ref = _arrange(fresh, lambda mm, ids=None: mm.prefill(_tiles(LINES), [GRIDS[i % N_LINES] for i in LINES], [_line(i)[1] for i in LINES], [4, 1]),
                   2, slots=[4, 1])
    _same_bits(one, ref, "single-slot fans vs the plain prefill")
    slots = [0, 1, 2, 3, 4, 5]
    _same_bits(_run(m, slots, 6), _run(fresh, slots, 6), "plain prefill + decode after shared prefills")


# ------------------------------------------------------------------------------------------------------------------ the predictor
def _dump(results):
    return [r.model_dump() for r in results]


def test_predictor_rank_equals_align_and_leaves_call_unchanged(hip_lib, _max_tokens):
    """(g) 2 images x 2 lines with 3 / 1 / 4 / 2 candidates, one of them a duplicate: every candidate's log_prob IS align's
    TextLine.log_prob for that line and text (a float64 sum of bit-equal terms: exact equality, bf16 being bit-equal in (b)), the order is
    the sorted one, and __call__ gives the same results before and after."""
    pred = _predictor(max_tokens=10)
    imgs = [Image.fromarray(c) for c in make_line_crops(2, seed=4)]
    boxes = [[[0, 0, im.size[0], im.size[1]], [0, 0, im.size[0] // 2, im.size[1]]] for im in imgs]
    before = pred(imgs, bboxes=boxes)
    settings.RECOGNITION_MAX_TOKENS = 24
    cands = [[["Invoice 2024", "lnvoice 2024", "Invoice 2024"], ["x"]], [["a", "", "The quick brown fox", "1234"], ["left", "right"]]]
    ranked = pred.rank(imgs, cands, bboxes=boxes)
    assert not pred.model.forced and [len(r.lines) for r in ranked] == [2, 2]
    aligned = [pred.align(imgs, [[line[min(c, len(line) - 1)] for line in page] for page in cands], bboxes=boxes) for c in range(4)]
    for i, page in enumerate(cands):
        for j, texts in enumerate(page):
            ln = ranked[i].lines[j]
            assert ln.bbox == [float(v) for v in boxes[i][j]]
            assert sorted(c.index for c in ln.candidates) == list(range(len(texts)))
            key = [(-c.log_prob, c.index) for c in ln.candidates]
            assert key == sorted(key) and ln.best == ln.candidates[0].index
            for c in ln.candidates:
                want = aligned[c.index][i].text_lines[j]
                assert want.text == texts[c.index] == c.text
                assert c.log_prob == want.log_prob and c.log_prob < 0, (i, j, c, want.log_prob)
                assert c.n_tokens == len(pred.forced_ids(c.text, "ocr_with_boxes"))
            distinct = {c.text: c.log_prob for c in ln.candidates}
            lp = np.asarray(list(distinct.values()), np.float64)
            e = np.exp(lp - lp.max())
            for c in ln.candidates:
                assert c.probability == float(e[list(distinct).index(c.text)] / e.sum())
    dup = [c for c in ranked[0].lines[0].candidates if c.text == "Invoice 2024"]
    assert [c.index for c in dup] == [0, 2] and dup[0].log_prob == dup[1].log_prob
    settings.RECOGNITION_MAX_TOKENS = 10
    after = pred(imgs, bboxes=boxes)
    assert before == after and _dump(before) == _dump(after)
