"""GPU: prompts kept on the device (surya_rec_prefill_keep / surya_rec_restore, csrc/kv_store.h) through the recognition engine and
through RecognitionPredictor.encode / EncodedLines, on REC-SMALL in fp32, bf16, fp16 and bf16 with MXFP8 decode weights.

The reference is what exists without the feature: a fresh surya_rec_prefill of the same lines, and the direct `__call__` / `rank` /
`align`. The store moves bytes and the head pass of a restore runs the prefill's kernels on the prefill's row values, so the requirement
is bit equality: cache rows byte for byte, token, score bits and box of step 0 and of every decode step, and every field of every result
object. Both arms of a comparison run with the same recognition_batch_size."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
from PIL import Image

from surya_amd import _lib as L
from surya_amd.settings import settings
from surya_amd.synth import make_line_crops

from test_gpu_rec_allowlist import DIGITS, GRIDS, N_LINES, _cfg_sd, _line, _max_tokens, _model, _run   # noqa: F401
from test_gpu_rec_forced import ARITH, _bits
from test_gpu_rec_rank import _outs, _same_bits, _tiles

pytestmark = pytest.mark.gpu
KEPT = [0, 1, 2, 3]                          # the lines that are kept ...
FIRST = [40, 0, 8, 100]                      # ... at these store rows (the prompts are 7, 8, 9 and 10 rows long: the entries at 0 and 8 touch)
CAP = 120


def _make(dtype, fp8, **kw):
    return _model(dtype, decode_fp8=True, **kw) if fp8 else _model(dtype, **kw)


def _len(i):
    return len(_line(i)[1])


def _keep(m, slots, lines=KEPT, first=FIRST):
    m.prefill_keep(_tiles(lines), [GRIDS[i % N_LINES] for i in lines], [_line(i)[1] for i in lines], slots, first)


def _stack(outs):
    return tuple(np.stack([o[i] for o in outs]) for i in range(len(outs[0])))


def _decode(m, slots, steps):
    m.set_active(sorted(slots))
    m.decode(steps)
    return _outs(m, slots, steps, False)


def _kv_equal(a, b, slot_a, slot_b, rows):
    for x, y in zip(a.kv_rows(slot_a, rows), b.kv_rows(slot_b, rows)):
        if not torch.equal(x.view(torch.uint8), y.view(torch.uint8)):
            return False
    return True


@pytest.mark.parametrize("dtype,fp8", ARITH)
def test_restored_slots_equal_freshly_prefilled_ones(hip_lib, dtype, fp8):
    """Slots 4-7 hold the longest lines, three steps in; lines 0-3 are prefilled into slots 0-3 and kept, everything decodes two steps;
    then the entries land in slots 4-7. Their cache rows are byte-equal to a fresh handle's prefill of lines 0-3 into slots 4-7, step 0
    is bit-equal, and so are six decode steps. The keeping prefill itself has the bits of the plain one."""
    m, fresh = _make(dtype, fp8), _make(dtype, fp8)
    assert m.prompt_store_info() == (0, 0)                                   # a handle that never keeps a prompt allocates nothing
    m.reserve_prompts(CAP)
    _run(m, [4, 5, 6, 7], 3, lines=[4, 4, 4, 4])                             # grid (2, 10): longer prompts than any kept line's
    _keep(m, [0, 1, 2, 3])
    kept0 = _outs(m, [0, 1, 2, 3], 1, False)
    assert m.prompt_store_info() == (CAP, 4)
    _decode(m, list(range(8)), 2)
    m.restore(FIRST, [[4], [5], [6], [7]])
    got = _outs(m, [4, 5, 6, 7], 1, False)
    fresh.prefill(_tiles(KEPT), [GRIDS[i % N_LINES] for i in KEPT], [_line(i)[1] for i in KEPT], [4, 5, 6, 7])
    ref = _outs(fresh, [4, 5, 6, 7], 1, False)
    _same_bits(_stack(got), _stack(ref), "step 0 of restored slots vs a fresh prefill")
    _same_bits(_stack(kept0), _stack(ref), "step 0 of the keeping prefill vs a plain one")
    for s, i in zip([4, 5, 6, 7], KEPT):
        assert _kv_equal(m, fresh, s, s, _len(i)), f"cache rows of slot {s} differ from a fresh prefill's"
    got += _decode(m, [4, 5, 6, 7], 6)
    ref += _decode(fresh, [4, 5, 6, 7], 6)
    _same_bits(_stack(got), _stack(ref), "restored slots vs freshly prefilled ones, six steps")
    assert len({tuple(t) for t in _stack(got)[0].T.tolist()}) > 1, "every line reads the same: the test distinguishes nothing"


def test_one_entry_lands_in_a_fan_and_twice(hip_lib):
    """An entry restored into a fan of three and, in the same call, once more into a fan of one: all four slots hold the lead's rows and
    run its greedy stream; slot 7, in no fan, keeps its line."""
    m, fresh = _model(torch.bfloat16), _model(torch.bfloat16)
    m.reserve_prompts(CAP)
    _keep(m, [0, 1, 2, 3])
    m.read_outputs(1)
    _run(m, [7], 2, lines=[5])
    before = m.kv_rows(7, _len(5) + 2)
    m.restore([FIRST[2], FIRST[0], FIRST[2]], [[5, 0, 3], [1], [6]])
    got = _outs(m, [5, 0, 3, 1, 6], 1, False) + _decode(m, [5, 0, 3, 1, 6], 4)
    rep = [2, 2, 2, 0, 2]
    fresh.prefill(_tiles(rep), [GRIDS[i % N_LINES] for i in rep], [_line(i)[1] for i in rep], [5, 0, 3, 1, 6])
    ref = _outs(fresh, [5, 0, 3, 1, 6], 1, False) + _decode(fresh, [5, 0, 3, 1, 6], 4)
    _same_bits(_stack(got), _stack(ref), "fans out of the store vs one prefill per slot")
    for x, y in zip(before, m.kv_rows(7, _len(5) + 2)):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16))


def test_captured_steps_replay_correctly_after_a_restore(hip_lib):
    """hipGraph replay on: the decode call of four rows x four steps runs eagerly, is captured, and is replayed, each time on slots that
    a restore just filled (the first time: the keeping prefill). No captured launch holds an address of the store: all three streams
    are the stream of an engine without graphs."""
    m, plain = _model(torch.bfloat16), _model(torch.bfloat16)
    ref = _run(plain, [0, 1, 2, 3], 4, lines=KEPT)
    m.reserve_prompts(CAP)
    L.check(m.lib.surya_set_tuning(b"graph", C.c_int(1)), "surya_set_tuning(graph)")
    try:
        for k in range(4):                                                   # eager, capture, replay, replay behind a grown store
            if k == 0:
                _keep(m, [0, 1, 2, 3])
            else:
                if k == 3:
                    m.reserve_prompts(3 * CAP)
                m.restore(FIRST, [[0], [1], [2], [3]])
            got = _stack(_outs(m, [0, 1, 2, 3], 1, False) + _decode(m, [0, 1, 2, 3], 4))
            _same_bits(got, ref, f"round {k} with graphs vs an engine without")
    finally:
        L.check(m.lib.surya_set_tuning(b"graph", C.c_int(0)), "surya_set_tuning(graph)")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_store_growth_keeps_live_entries(hip_lib, dtype):
    """Two entries in a store of 30 rows, one of them dropped; the store grows to 200 and to 700 rows while the other is live: it lands
    with the bytes it was kept with, and its freed neighbour's rows take a new entry."""
    m = _model(dtype)
    m.reserve_prompts(30)
    _keep(m, [0, 1], lines=[3, 1], first=[17, 2])
    m.read_outputs(1)
    want = m.kv_rows(0, _len(3))
    m.drop_prompts([2])
    assert m.prompt_store_info() == (30, 1)
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
        _keep(m, [4], lines=[2], first=[30 - _len(2) + 1])                   # reaches past the reserved rows
    m.reserve_prompts(200)
    m.reserve_prompts(100)                                                   # never shrinks
    assert m.prompt_store_info() == (200, 1)
    _keep(m, [4], lines=[2], first=[150])
    m.reserve_prompts(700)
    m.restore([17, 150], [[5, 6], [7]])
    got = _outs(m, [5, 6, 7], 1, False)
    for s in (5, 6):
        for x, y in zip(want, m.kv_rows(s, _len(3))):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), "an entry's bytes changed while the store grew"
    fresh = _model(dtype)
    fresh.prefill(_tiles([3, 3, 2]), [GRIDS[3], GRIDS[3], GRIDS[2]], [_line(3)[1], _line(3)[1], _line(2)[1]], [5, 6, 7])
    _same_bits(_stack(got + _decode(m, [5, 6, 7], 3)), _stack(_outs(fresh, [5, 6, 7], 1, False) + _decode(fresh, [5, 6, 7], 3)),
               "entries restored behind two growths vs a fresh prefill")


def test_refusals_leave_the_handle_usable(hip_lib):
    """Every refused call comes back before anything is enqueued or changed: lines in flight go on with the bits of a fresh handle's,
    and so does a plain prefill + decode afterwards."""
    m, fresh = _model(torch.bfloat16), _model(torch.bfloat16)
    slots = [0, 1, 2, 3, 4, 5]
    _same_bits(_run(m, slots, 2), _run(fresh, slots, 2), "two handles")
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
        _keep(m, [6], lines=[0], first=[0])                                  # nothing reserved yet
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
        m.restore([0], [[6]])                                                # an unknown entry, no store at all
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
        m.reserve_prompts(-1)
    m.reserve_prompts(CAP)
    _keep(m, [6], lines=[0], first=[20])
    m.read_outputs(1)
    n0 = _len(0)
    for first in ([-2], [CAP - _len(1) + 1], [20], [20 + n0 - 1], [20 - _len(1) + 1]):      # below -1, past the rows, over the live entry
        with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
            _keep(m, [7], lines=[1], first=first)
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
        _keep(m, [6, 7], lines=[1, 1], first=[40, 40 + _len(1) - 1])         # two ranges of one call overlap
    assert m.prompt_store_info() == (CAP, 1)
    for first, fans in (([21], [[7]]), ([20], [[8]]), ([20], [[-1]]), ([20], [[]]), ([20, 20], [[7], [7]]), ([20], [[6, 6]])):
        with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
            m.restore(first, fans)
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
        m.drop_prompts([20, 20])
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
        m.drop_prompts([20, 21])
    m.set_kv_fp8(True)                                                       # the store holds bf16 / fp16 / fp32 rows only
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.restore([20], [[7]])
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        _keep(m, [7], lines=[1], first=[40])
    m.set_kv_fp8(False)
    m.set_beam(2, _cfg_sd()[0].pad_token_id)                                 # beam search: lead slots of whole groups, one per entry
    for fans in ([[7]], [[6, 7]]):
        with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
            m.restore([20], fans)
    m.set_beam(None)
    assert m.prompt_store_info() == (CAP, 1)
    for mm in (m, fresh):
        mm.decode(2)
    _same_bits(_stack(_outs(m, slots, 2, False)), _stack(_outs(fresh, slots, 2, False)), "the lines in flight after the refused calls")
    m.restore([20], [[7]])
    m.read_outputs(1)
    m.drop_prompts([20])
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
        m.restore([20], [[7]])                                               # a dropped entry is unknown
    _same_bits(_run(m, slots, 3), _run(fresh, slots, 3), "a plain prefill and decode after the refused calls")


def test_beam_groups_out_of_the_store_equal_prefilled_ones(hip_lib):
    """Beam search on (width 2): entries land in lead slots of whole groups and the first selection follows, as in the prefill."""
    cfg = _cfg_sd()[0]
    m, fresh = _model(torch.bfloat16), _model(torch.bfloat16)
    m.reserve_prompts(CAP)
    _keep(m, [0, 1, 2, 3])
    m.read_outputs(1)

    def beams(mm, land):
        mm.set_beam(2, cfg.pad_token_id)
        try:
            land(mm)
            out = [tuple(a[0].copy() for a in tuple(mm.read_outputs(1)) + tuple(mm.read_beam(1)))]
            mm.set_active([0, 1, 4, 5])
            mm.decode(4)
            o, b = tuple(mm.read_outputs(4)), tuple(mm.read_beam(4))
            out += [tuple(a[k].copy() for a in o + b) for k in range(4)]
        finally:
            mm.set_beam(None)
        # (token, score and box of step 0 are written for the lead slots only: the other slots' cells hold whatever ran there before)
        lead0 = tuple(out[0][i][[0, 4]] for i in range(3))
        return lead0 + tuple(np.stack([x[i][[0, 1, 4, 5]] for x in out[1 if i < 3 else 0:]]) for i in range(len(out[0])))
    got = beams(m, lambda mm: mm.restore([FIRST[1], FIRST[3]], [[4], [0]]))
    ref = beams(fresh, lambda mm: mm.prefill(_tiles([1, 3]), [GRIDS[1], GRIDS[3]], [_line(1)[1], _line(3)[1]], [4, 0]))
    _same_bits(got, ref, "beam groups out of the store vs prefilled ones")


# ------------------------------------------------------------------------------------------------------------------ the predictor
SLOTS = 8


@functools.lru_cache(maxsize=None)
def _pred_of(dtype, fp8):
    from test_gpu_predictors import make_rec_predictor
    pred = make_rec_predictor("REC-SMALL", dtype, max_slots=16, max_tokens=10)[2]
    if fp8:
        pred.model.set_decode_fp8(True)
    return pred


def _predictor(dtype=torch.bfloat16, fp8=False):
    settings.RECOGNITION_MAX_TOKENS = 10
    return _pred_of(dtype, fp8)


def _inputs(n=4, seed=4):
    imgs = [Image.fromarray(c) for c in make_line_crops(n, seed=seed)]
    return imgs, [[[0, 0, im.size[0], im.size[1]], [0, 0, im.size[0] // 2, im.size[1]]] for im in imgs]      # two lines per image


def _dump(results):
    return [r.model_dump() for r in results]


def _options(pred):
    """The decoding options a read runs under, each as (name, attributes to set, keywords of the call)."""
    from test_gpu_rec_boost import WORDS5
    from test_gpu_rec_lexicon import WORDS
    from test_gpu_rec_pattern import DATE
    opts = [("plain", {}, {}), ("allowlist", {}, {"allowlist": DIGITS}), ("top_k", {"top_k": 3}, {}), ("pattern", {"pattern": DATE}, {}),
            ("lexicon", {"lexicon": WORDS}, {}), ("boost", {"boost_words": WORDS5, "boost_weight": 1e4}, {}),
            ("words", {}, {"return_words": True, "sort_lines": True})]
    if not pred.model.decode_fp8:                             # (beam search excludes MXFP8 decode weights)
        opts.append(("beam", {"beam_width": 2}, {}))
    return opts


@pytest.mark.parametrize("dtype,fp8", ARITH)
def test_read_equals_the_call_under_every_option(hip_lib, _max_tokens, dtype, fp8):
    """enc.read() is pred(images, bboxes=...) field for field -- texts, confidences, character boxes, alternatives, pattern_matched,
    lexicon_index, boost_matches and plain readings, hypotheses and log_prob -- under each decoding option, from ONE encode."""
    pred = _predictor(dtype, fp8)
    imgs, boxes = _inputs()
    with pred.encode(imgs, bboxes=boxes, recognition_batch_size=SLOTS) as enc:
        assert pred.model.prompt_store_info()[1] == 8
        for name, attrs, kw in _options(pred):
            try:
                for k, v in attrs.items():
                    setattr(pred, k, v)
                want = pred(imgs, bboxes=boxes, recognition_batch_size=SLOTS, **kw)
                got = enc.read(recognition_batch_size=SLOTS, **kw)
            finally:
                for k in attrs:
                    setattr(pred, k, None)
            assert len(got) == 4 and sum(len(r.text_lines) for r in got) == 8
            assert _dump(got) == _dump(want), f"{name}: a read of kept lines differs from the call"
            if name == "beam":
                assert all(ln.hypotheses and ln.log_prob is not None for r in got for ln in r.text_lines)
            if name == "top_k":
                assert any(c.alternatives for r in got for ln in r.text_lines for c in ln.chars)
        assert any(ln.text for r in enc.read(recognition_batch_size=SLOTS) for ln in r.text_lines), "every line came out empty"
    assert pred.model.prompt_store_info()[1] == 0


@pytest.mark.parametrize("dtype,fp8", ARITH)
def test_rank_and_align_equal_the_direct_calls(hip_lib, _max_tokens, dtype, fp8):
    """enc.rank(c) is pred.rank(c) and enc.align(t) is pred.align(t): the maximum difference in log_prob is 0.0."""
    pred = _predictor(dtype, fp8)
    imgs, boxes = _inputs(2)
    settings.RECOGNITION_MAX_TOKENS = 24
    cands = [[["Invoice 2024", "lnvoice 2024", "Invoice 2024"], ["x"]], [["a", "", "The quick brown fox", "1234"], ["left", "right"]]]
    texts = [[line[0] for line in page] for page in cands]
    with pred.encode(imgs, bboxes=boxes, recognition_batch_size=SLOTS) as enc:
        want, got = pred.rank(imgs, cands, bboxes=boxes, recognition_batch_size=SLOTS), enc.rank(cands, recognition_batch_size=SLOTS)
        diff = max(abs(a.log_prob - b.log_prob) for x, y in zip(got, want) for la, lb in zip(x.lines, y.lines)
                   for a, b in zip(sorted(la.candidates, key=lambda c: c.index), sorted(lb.candidates, key=lambda c: c.index)))
        print("max |log_prob difference| rank:", diff)
        assert diff == 0.0 and _dump(got) == _dump(want)
        want, got = pred.align(imgs, texts, bboxes=boxes, recognition_batch_size=SLOTS), enc.align(texts, recognition_batch_size=SLOTS)
        assert max(abs(a.log_prob - b.log_prob) for x, y in zip(got, want) for a, b in zip(x.text_lines, y.text_lines)) == 0.0
        assert _dump(got) == _dump(want) and all(ln.log_prob < 0 for r in got for ln in r.text_lines)
        want = pred.align(imgs, texts, bboxes=boxes, recognition_batch_size=SLOTS, return_words=True)
        assert _dump(enc.align(texts, return_words=True, recognition_batch_size=SLOTS)) == _dump(want)
        assert not pred.model.forced


def test_one_set_read_rank_read_and_sets_side_by_side(hip_lib, _max_tokens):
    """One EncodedLines: a read, a rank, a second read equal to the first. Two live sets interleaved; one released, a third encoded into
    the freed rows, and the other still intact. `lines=` subsets hold those lines, in that order."""
    pred = _predictor()
    imgs_a, boxes_a = _inputs(4, seed=4)
    imgs_b, boxes_b = _inputs(3, seed=9)
    want_a, want_b = pred(imgs_a, bboxes=boxes_a, recognition_batch_size=SLOTS), pred(imgs_b, bboxes=boxes_b, recognition_batch_size=SLOTS)
    cands = [[["ab", "abc"], ["7"]] for _ in imgs_a]
    want_rank = pred.rank(imgs_a, cands, bboxes=boxes_a, recognition_batch_size=SLOTS)
    a = pred.encode(imgs_a, bboxes=boxes_a, recognition_batch_size=SLOTS)
    first = a.read(recognition_batch_size=SLOTS)
    assert _dump(first) == _dump(want_a)
    assert _dump(a.rank(cands, recognition_batch_size=SLOTS)) == _dump(want_rank)
    assert _dump(a.read(recognition_batch_size=SLOTS)) == _dump(first)
    b = pred.encode(imgs_b, bboxes=boxes_b, recognition_batch_size=SLOTS)
    assert pred.model.prompt_store_info()[1] == 14
    for _ in range(2):
        assert _dump(b.read(recognition_batch_size=SLOTS)) == _dump(want_b) and _dump(a.read(recognition_batch_size=SLOTS)) == _dump(want_a)
    # subsets: only those lines, in that order; candidates per selected line
    sub = a.read(lines=[[1, 0], [], [1], None], recognition_batch_size=SLOTS)
    lines_of = lambda r, idx: [r.text_lines[i].model_dump() for i in idx]
    assert [[ln.model_dump() for ln in r.text_lines] for r in sub] == [lines_of(want_a[0], [1, 0]), [], lines_of(want_a[2], [1]),
                                                                      lines_of(want_a[3], [0, 1])]
    sub = a.rank([[["7"]], [], [["ab", "abc"], ["7"]], []], lines=[[1], [], [0, 1], []], recognition_batch_size=SLOTS)
    assert [ln.model_dump() for ln in sub[0].lines] == [want_rank[0].lines[1].model_dump()] and _dump(sub[2:3]) == _dump(want_rank[2:3])
    rows_a = sorted(a._first)
    a.release()
    with pytest.raises(ValueError, match="released"):
        a.read()
    assert pred.model.prompt_store_info()[1] == 6
    c = pred.encode(imgs_a, bboxes=boxes_a, recognition_batch_size=SLOTS)
    assert sorted(c._first) == rows_a, "the freed rows are handed out again"
    assert _dump(b.read(recognition_batch_size=SLOTS)) == _dump(want_b), "a live set changed when its neighbour's rows were reused"
    assert _dump(c.read(recognition_batch_size=SLOTS)) == _dump(want_a)
    # another predictor's lines are refused
    with pytest.raises(ValueError, match="another predictor"):
        c.read(predictor=_predictor(torch.float16))
    b.release()
    c.release()
    assert pred.model.prompt_store_info()[1] == 0


def test_a_rectified_line_comes_back_with_its_tilted_quads(hip_lib, _max_tokens):
    """`rectify` is read at encode time: tilted polygon lines are warped upright then, and every later read reports them as the direct
    call does -- the same tilted character quads, `rectified` set -- whatever `rectify` says by then."""
    from test_gpu_predictors import make_rec_predictor
    from test_gpu_rectify import _five_lines
    pages, polys = _five_lines()
    pred = make_rec_predictor(max_slots=8, max_tokens=8)[2]
    try:
        pred.rectify = True
        want = pred(pages, polygons=polys, recognition_batch_size=8)
        enc = pred.encode(pages, polygons=polys, recognition_batch_size=8)
        pred.rectify = None
        got = enc.read(recognition_batch_size=8)
        assert _dump(got) == _dump(want)
        lines = [ln for r in got for ln in r.text_lines]
        assert [ln.rectified for ln in lines] == [True, True, True, False, False] and sum(len(ln.chars) for ln in lines[:3]) > 0
        pred.rectify = True
        texts = [["12", "ab", "x"], ["7", "left"]]
        assert _dump(enc.align(texts, recognition_batch_size=8)) == _dump(pred.align(pages, texts, polygons=polys, recognition_batch_size=8))
        enc.release()
    finally:
        pred.rectify = None


def test_the_fp8_kv_cache_is_refused_and_the_predictor_stays_usable(hip_lib, _max_tokens):
    pred = _predictor()
    imgs, boxes = _inputs(2)
    want = pred(imgs, bboxes=boxes, recognition_batch_size=SLOTS)
    enc = pred.encode(imgs, bboxes=boxes, recognition_batch_size=SLOTS)
    pred.model.set_kv_fp8(True)
    try:
        with pytest.raises(ValueError, match="fp8 KV cache"):
            pred.encode(imgs, bboxes=boxes)
        with pytest.raises(ValueError, match="fp8 KV cache"):
            enc.read()
    finally:
        pred.model.set_kv_fp8(False)
    assert _dump(enc.read(recognition_batch_size=SLOTS)) == _dump(want) == _dump(pred(imgs, bboxes=boxes, recognition_batch_size=SLOTS))
    enc.release()
