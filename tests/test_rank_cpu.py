"""CPU: ranking candidate texts (RecognitionPredictor.rank) -- the device loop's candidate fans against a fake model that ENFORCES the
contract of surya_rec_prefill_shared (include/surya_amd.h), `rank` itself on that fake, and the serialised form of its three schema classes.

The fake's scores are a function of the forced id alone, so what a candidate must score is known from its text: a wrong slot, a wrong
index or a lost step shows as a wrong number."""
import inspect
import json
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
from PIL import Image

from surya_amd import _lib as L
from surya_amd.recognition.loop import DeviceLoop
from surya_amd.recognition.predictor import RecognitionPredictor
from surya_amd.recognition.processor import SuryaOCRProcessor
from surya_amd.recognition.schema import LineRanking, RankedCandidate, RankResult
from surya_amd.recognition.tokenizer import ByteMathTokenizer, OCRTokenizer
from surya_amd.settings import settings
from test_forced_cpu import FakeForcedModel
from test_scheduler_cpu import EOS, NOP, PAD, FakeModel, make


def logp_of(tid):
    """The log-probability the fake reports for forced id `tid`: a multiple of 1/16, so sums are exact in any order."""
    return np.float32(-((int(tid) * 7) % 64) / 16.0)


def greedy_of(tid):
    """The fake's own reading where `tid` is forced: it disagrees on every id divisible by 5."""
    return int(tid) + 1 if int(tid) % 5 == 0 else int(tid)


class FakeFanModel(FakeForcedModel):
    """FakeForcedModel + prefill_shared with the rules of surya_rec_prefill_shared: forcing on, nothing in flight, one non-empty slot list
    per sequence, every slot in range, named once in the call and not busy (active), look-ahead images consumed ONCE per sequence. Every
    fan slot gets the sequence, position 1 and a first token of its own; the forced outputs follow the slot's own ids."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.shared_calls, self.active_at_call = [], []
        self.vocab, self.device = 70000, "cpu"

    def _step(self, s):
        c, ids = self.cursor[s], self.slot_ids[s]
        self.cursor[s] = c + 1
        t = ids[c] if c < len(ids) else 7                               # (past its list a slot only rides along: the loop drops it)
        return t, greedy_of(t), np.float32(0.5), logp_of(t)

    def prefill(self, *a, **k):
        raise AssertionError("a loop with candidate fans prefills through prefill_shared only")

    def prefill_shared(self, tiles, grid_hw, input_ids, fan_slots):
        assert self.forced, "the loop forces every fan slot"
        assert not self.inflight, "prefill while decode calls are in flight"
        assert len(grid_hw) == len(input_ids) == len(fan_slots) > 0
        named = [s for f in fan_slots for s in f]
        assert all(len(f) > 0 for f in fan_slots), "SA_ERR_ARG: an empty fan"
        assert len(set(named)) == len(named) <= self.max_slots, "SA_ERR_ARG: a slot named twice / too many"
        assert all(0 <= s < self.max_slots for s in named), "SA_ERR_ARG: a slot out of range"
        assert not set(named) & set(self.active), "a named slot is busy"
        assert sum(len(p) for p in input_ids) <= self.c.max_prefill_tokens, "SA_ERR_SHAPE: prompt tokens, once per sequence"
        lines = [ids[0] - 1000 for ids in input_ids]
        if tiles is None:
            for ln in lines:
                assert self.ahead and self.ahead.popleft() == ln, "look-ahead images consumed out of order"
        else:
            assert tiles.shape[0] == sum(h * w for h, w in grid_hw)
        S = self.max_slots
        tok, sc, bb = np.zeros((1, S), np.int32), np.zeros((1, S), np.float32), np.zeros((1, S, 6), np.int32)
        f = (np.full((1, S), -9, np.int32), np.zeros((1, S), np.float32), np.zeros((1, S), np.float32))
        for ln, fan in zip(lines, fan_slots):
            for s in fan:
                self.slot_line[s], self.slot_pos[s] = ln, 1
                tok[0, s], f[0][0, s], f[1][0, s], f[2][0, s] = self._step(s)
                sc[0, s], bb[0, s] = 0.5, ln
        self.prefill_out, self.prefill_forced = (tok, sc, bb), f
        self.shared_calls.append((lines, [list(fan) for fan in fan_slots]))
        self.active_at_call.append(sorted(self.active))
        self.stats["prefills"] += 1

    def decode_async(self, n, ring):
        FakeModel.decode_async(self, n, ring)
        tok = self.inflight[-1][2][0]
        S = self.max_slots
        f = (np.full((n, S), -9, np.int32), np.zeros((n, S), np.float32), np.zeros((n, S), np.float32))
        for k in range(n):
            for s in self.active:
                tok[k, s], f[0][k, s], f[1][k, s], f[2][k, s] = self._step(s)
        self.forced_inflight[ring] = (n, f)


def cand_ids(line, j, n):
    """Candidate j of `line`: n ids that name line, candidate and position; none is EOS, PAD or NOP."""
    return [5000 + line * 1000 + j * 100 + k for k in range(n)]


# lines of 3, 1, 2, 4 candidates; a one-id list in line 0 and in line 3
LENS = [[5, 1, 20], [3], [2, 24], [4, 1, 6, 2]]


def _run_loop(lens, slots, ahead, sps, max_prefill=None):
    old = (settings.RECOGNITION_STEPS_PER_SYNC, settings.RECOGNITION_ENCODE_AHEAD)
    settings.RECOGNITION_STEPS_PER_SYNC, settings.RECOGNITION_ENCODE_AHEAD = sps, ahead
    try:
        _, prep = make(len(lens), 48, slots)
        prep["forced_ids"] = [[cand_ids(i, j, n) for j, n in enumerate(line)] for i, line in enumerate(lens)]
        model = FakeFanModel(slots)
        if max_prefill is not None:
            model.c.max_prefill_tokens = max_prefill
        done = {}

        def on_done(line, results):
            assert line not in done, "on_done fired twice for a line"
            done[line] = results
        loop = DeviceLoop(model, EOS, PAD, NOP, slots, 48, 0.2, forced=True, fan=True, on_done=on_done)
        loop.run(prep)
    finally:
        settings.RECOGNITION_STEPS_PER_SYNC, settings.RECOGNITION_ENCODE_AHEAD = old
    return model, loop, done, prep


def _check_results(done, forced_ids):
    assert sorted(done) == list(range(len(forced_ids)))
    for i, line in enumerate(forced_ids):
        assert len(done[i]) == len(line)
        for ids, (gt, gp, lp) in zip(line, done[i]):
            assert gt.tolist() == [greedy_of(t) for t in ids], (i, ids)
            assert lp.dtype == np.float32 and lp.tolist() == [float(logp_of(t)) for t in ids], (i, ids)
            assert gp.shape == lp.shape == (len(ids),)


@pytest.mark.parametrize("ahead", [True, False])
@pytest.mark.parametrize("sps", [1, 4])
def test_loop_fans_lines_over_slots_and_frees_them_per_candidate(ahead, sps):
    """6 slots, lines of 3 / 1 / 2 / 4 candidates: the first three lines fill the slots in ONE shared prefill whose nine prompt tokens
    are counted once per line (max_prefill is 9; counted per candidate they would be 18); the fourth waits until four slots have
    drained, and is admitted while candidates of lines 0 and 2 still decode -- a candidate frees its slot on its own."""
    model, loop, done, prep = _run_loop(LENS, 6, ahead, sps, max_prefill=9)
    _check_results(done, prep["forced_ids"])
    assert model.switches == [True, False]
    (l0, f0), (l1, f1) = model.shared_calls
    assert l0 == [0, 1, 2] and f0 == [[0, 1, 2], [3], [4, 5]]             # lead first: the empty slots ascending, a line's run together
    assert l1 == [3] and len(f1[0]) == 4
    busy = model.active_at_call[1]
    assert busy == [2, 5] and not set(f1[0]) & set(busy)                   # the twenty- and the twenty-four-id candidates still run
    assert model.token_calls == 2 and model.stats["prefills"] == 2
    assert loop.tok_mat.shape[0] == sum(len(x) for x in LENS) and loop.predicted_tokens == [[] for _ in LENS]
    assert not model.inflight and not model.ahead


def test_a_line_waits_for_slots_and_nothing_overtakes_it():
    """4 slots: line 0 takes three, line 1 (three candidates) does not fit the one slot left and waits; line 2 (one candidate) would
    fit but stays behind it. Admission order is queue order."""
    model, _, done, prep = _run_loop([[6, 6, 6], [2, 2, 2], [1]], 4, True, 2)
    _check_results(done, prep["forced_ids"])
    assert [c[0] for c in model.shared_calls] == [[0], [1, 2]]
    assert model.active_at_call[1] == []


def test_a_line_of_one_id_lists_never_takes_a_slot():
    model, _, done, prep = _run_loop([[1, 1], [1]], 2, False, 4)
    _check_results(done, prep["forced_ids"])
    assert model.stats["decode_calls"] == 0


def test_the_loop_refuses_fans_it_cannot_run():
    _, prep = make(1, 48, 2)
    prep["forced_ids"] = [[cand_ids(0, j, 2) for j in range(3)]]             # three candidates, two slots
    with pytest.raises(AssertionError, match="candidates"):
        DeviceLoop(FakeFanModel(2), EOS, PAD, NOP, 2, 48, 0.2, forced=True, fan=True).run(prep)
    prep["forced_ids"] = [[cand_ids(0, 0, 2), []]]
    with pytest.raises(AssertionError, match="candidates"):
        DeviceLoop(FakeFanModel(2), EOS, PAD, NOP, 2, 48, 0.2, forced=True, fan=True).run(prep)
    with pytest.raises(AssertionError, match="forced"):
        DeviceLoop(FakeFanModel(2), EOS, PAD, NOP, 2, 48, 0.2, fan=True)


def test_a_loop_without_fans_never_calls_prefill_shared():
    class NoShared(FakeForcedModel):
        def prefill_shared(self, *a, **k):
            raise AssertionError("prefill_shared without fan=True")
    _, prep = make(5, 12, 3)
    prep["forced_ids"] = [[200 + i, 300 + i] for i in range(5)]
    done = {}
    DeviceLoop(NoShared(3), EOS, PAD, NOP, 3, 12, 0.2, forced=True, on_done=lambda k, toks, *r: done.__setitem__(k, list(toks))).run(prep)
    assert done == {i: [200 + i, 300 + i] for i in range(5)}
    DeviceLoop(NoShared(3), EOS, PAD, NOP, 3, 12, 0.2).run(make(5, 12, 3)[1])


# ------------------------------------------------------------------------------------------------- rank on the fake
@pytest.fixture(scope="module")
def proc():
    return SuryaOCRProcessor(OCRTokenizer(None, ByteMathTokenizer(256), reserve_special=64))


def _key(ln):
    return (int(ln.y0) * 131 + int(ln.x0)) % 997


def _pred(proc, slots=8):
    pred = object.__new__(RecognitionPredictor)
    pred.processor = proc
    pred.model = FakeFanModel(slots)
    pred.model.cfg = SimpleNamespace(encoder=SimpleNamespace(spatial_merge_size=2), bbox_size=1024)
    pred.device_preprocess = True

    def fake_preprocess(prompts, pages):
        grids = [(2, 2 + 2 * (_key(p.image) % 3)) for p in prompts]
        offs = np.cumsum([0] + [h * w for h, w in grids])
        tiles = np.zeros((offs[-1], 3), np.float32)
        for i, p in enumerate(prompts):
            tiles[offs[i]:offs[i + 1], 0] = _key(p.image)
        return tiles, offs, grids, [[1000 + _key(p.image), 5, 6] for p in prompts]
    pred.preprocess_prompts_device = fake_preprocess
    return pred


def _want(pred, text, task="ocr_with_boxes"):
    ids = pred.forced_ids(text, task)
    return float(np.sum(np.asarray([logp_of(t) for t in ids], np.float64))), len(ids), all(greedy_of(t) == t for t in ids)


BOXES = [[[2, 3, 60, 14], [4, 20, 40, 31]], [[1, 5, 30, 15]]]
CANDS = [[["ab", "ba", "abc", "ab"], ["x"]], [["hello", "help", ""]]]


@pytest.fixture
def fake_loop_settings():
    old = (settings.RECOGNITION_STEPS_PER_SYNC, settings.RECOGNITION_ENCODE_AHEAD, settings.RECOGNITION_MAX_TOKENS)
    settings.RECOGNITION_STEPS_PER_SYNC, settings.RECOGNITION_ENCODE_AHEAD, settings.RECOGNITION_MAX_TOKENS = 4, True, 12
    yield
    settings.RECOGNITION_STEPS_PER_SYNC, settings.RECOGNITION_ENCODE_AHEAD, settings.RECOGNITION_MAX_TOKENS = old


def test_rank_scores_sorts_and_reports_duplicates(proc, fake_loop_settings):
    pred = _pred(proc)
    pred.top_k, pred.beam_width = 3, 2                                      # parked for the call
    imgs = [Image.new("RGB", (64, 40)), Image.new("RGB", (64, 40))]
    res = pred.rank(imgs, CANDS, bboxes=BOXES, recognition_batch_size=8)
    assert pred._top_k is None and pred._beam is None and pred.top_k == 3
    assert [type(r) for r in res] == [RankResult, RankResult] and [len(r.lines) for r in res] == [2, 1]
    assert res[0].image_bbox == [0, 0, 64, 40]
    # the model scored DISTINCT id lists only: 3 + 1 + 3 slots in all
    assert sorted(len(f) for _, fans in pred.model.shared_calls for f in fans) == [1, 3, 3]
    for i, (page, boxes) in enumerate(zip(CANDS, BOXES)):
        for j, (texts, box) in enumerate(zip(page, boxes)):
            ln = res[i].lines[j]
            assert isinstance(ln, LineRanking) and ln.bbox == [float(v) for v in box]
            assert sorted(c.index for c in ln.candidates) == list(range(len(texts)))
            key = [(-c.log_prob, c.index) for c in ln.candidates]
            assert key == sorted(key) and ln.best == ln.candidates[0].index
            distinct = {}
            for c in ln.candidates:
                assert isinstance(c, RankedCandidate) and c.text == texts[c.index]
                assert (c.log_prob, c.n_tokens, c.greedy_match) == _want(pred, c.text), (i, j, c)
                distinct[c.text] = c.log_prob
            lp = np.asarray(list(distinct.values()), np.float64)
            e = np.exp(lp - lp.max())
            for c in ln.candidates:
                assert c.probability == float(e[list(distinct).index(c.text)] / e.sum())
            assert abs(sum(dict((c.text, c.probability) for c in ln.candidates).values()) - 1.0) < 1e-12
    first = res[0].lines[0].candidates
    # "ab" and "ba" hold the same ids in another order: the same score, so the lower index goes first; "ab" is reported at 0 and at 3
    ab = [c for c in first if c.text == "ab"]
    assert [c.index for c in ab] == [0, 3] and ab[0].log_prob == ab[1].log_prob and ab[0].probability == ab[1].probability
    ba = next(c for c in first if c.text == "ba")
    assert ba.log_prob == ab[0].log_prob and [c.index for c in first if c.text in ("ab", "ba")] == [0, 1, 3]
    assert any(c.greedy_match for r in res for ln in r.lines for c in ln.candidates)
    assert not all(c.greedy_match for r in res for ln in r.lines for c in ln.candidates)
    assert pred.model.switches == [True, False]


def test_rank_refuses_before_any_model_call(proc, fake_loop_settings):
    img, box = Image.new("RGB", (64, 16)), [0, 0, 64, 16]

    def refused(exc, match, *a, setup=None, slots=8, **k):
        pred = _pred(proc, slots)
        if setup:
            setup(pred)
        with pytest.raises(exc, match=match):
            pred.rank(*a, **k)
        m = pred.model
        assert m.switches == [] and m.stats["prefills"] == 0 and m.stats["encode_ahead"] == 0 and not m.shared_calls

    refused(ValueError, "bboxes or polygons", [img], [[["a"]]])
    refused(ValueError, "1 images, 2 candidate lists", [img], [[["a"]], [["b"]]], bboxes=[[box]])
    refused(ValueError, "image 1 has 2 lines but 1 candidate lists", [img, img], [[["a"]], [["b"]]], bboxes=[[box], [box, box]])
    refused(ValueError, "image 0, line 1: the candidates must be a non-empty list", [img], [[["a"], []]], bboxes=[[box, box]])
    refused(ValueError, "image 0, line 0: the candidates must be a non-empty list", [img], [["a"]], bboxes=[[box]])
    refused(ValueError, r"image 0, line 0, candidate 1: 13 tokens \(eos included\) exceed the token budget 12", [img], [[["a", "x" * 12]]], bboxes=[[box]])
    refused(ValueError, "image 0, line 0, candidate 0: the text must be a str", [img], [[[None]]], bboxes=[[box]])
    refused(ValueError, "not supported", [img], [[["a"]]], bboxes=[[box]], task_names=["nonsense"])
    refused(ValueError, "3 distinct candidates exceed the 2 slots in use", [img], [[["a", "b", "c", "a"]]], bboxes=[[box]], recognition_batch_size=2)
    refused(ValueError, "3 distinct candidates exceed the 2 slots in use", [img], [[["a", "b", "c"]]], bboxes=[[box]], recognition_batch_size=64, slots=2)
    for attr, val in (("pattern", r"\d+"), ("lexicon", ["a"]), ("boost_words", ["a"])):
        refused(ValueError, "do(es)? not apply to rank", [img], [[["a"]]], bboxes=[[box]], setup=lambda p: setattr(p, attr, val))
    for attr, val in (("shard_lines", True), ("process_group", object())):
        refused(NotImplementedError, "one rank", [img], [[["a"]]], bboxes=[[box]], setup=lambda p: setattr(p, attr, val))
    old = settings.RECOGNITION_MAX_TOKENS
    try:
        settings.RECOGNITION_MAX_TOKENS = 4096
        refused(ValueError, f"candidate 0: 1201 tokens exceed SA_MAX_FORCED_TOKENS = {L.SA_MAX_FORCED_TOKENS}", [img], [[["x" * 1200]]], bboxes=[[box]])
    finally:
        settings.RECOGNITION_MAX_TOKENS = old

    def small(p):
        p.model.vocab = proc.ocr_tokenizer.special_token_offset + 100
    refused(ValueError, "image 0, line 0, candidate 1: token id .* outside the model's vocabulary", [img], [[["A", "é"]]], bboxes=[[box]], setup=small)
    # four duplicates of two texts fit two slots
    pred = _pred(proc, 2)
    res = pred.rank([img], [[["a", "b", "a", "b"]]], bboxes=[[box]], recognition_batch_size=2)
    assert len(res[0].lines[0].candidates) == 4


def test_rank_has_the_stated_signature_and_align_keeps_its_messages(proc):
    assert list(inspect.signature(RecognitionPredictor.rank).parameters) == [
        "self", "images", "candidates", "task_names", "bboxes", "polygons", "recognition_batch_size", "math_mode"]
    assert list(inspect.signature(DeviceLoop.__init__).parameters)[-1] == "fan"
    pred = _pred(proc)
    with pytest.raises(ValueError, match=r"align\(\) needs bboxes or polygons: the lines the texts belong to"):
        pred.align([Image.new("RGB", (8, 8))], [["a"]])


# ------------------------------------------------------------------------------------------------- schema, bindings
def test_serialised_form_of_the_three_classes():
    poly = [[0, 0], [8, 0], [8, 10], [0, 10]]
    a = RankedCandidate(index=1, text="ab", log_prob=-1.5, n_tokens=3, probability=0.75, greedy_match=True)
    b = RankedCandidate(index=0, text="ba", log_prob=-2.5, n_tokens=3, probability=0.25, greedy_match=False)
    ln = LineRanking(polygon=poly, candidates=[a, b], best=1)
    r = RankResult(lines=[ln], image_bbox=[0, 0, 64, 40])
    assert a.model_dump() == {"index": 1, "text": "ab", "log_prob": -1.5, "n_tokens": 3, "probability": 0.75, "greedy_match": True}
    d = r.model_dump()
    assert set(d) == {"lines", "image_bbox"} and d["image_bbox"] == [0, 0, 64, 40]
    assert set(d["lines"][0]) == {"polygon", "confidence", "bbox", "candidates", "best"}
    assert d["lines"][0]["bbox"] == [0, 0, 8, 10] and d["lines"][0]["best"] == 1 and d["lines"][0]["candidates"][1] == b.model_dump()
    back = json.loads(r.model_dump_json())
    assert back["lines"][0]["candidates"][0]["log_prob"] == -1.5 and back["lines"][0]["polygon"] == [[float(v) for v in p] for p in poly]
    assert RankResult.model_validate(json.loads(r.model_dump_json())).lines[0].candidates == [a, b]
    for cls, fields in ((RankedCandidate, {"index", "text", "log_prob", "n_tokens", "probability", "greedy_match"}),
                        (LineRanking, {"polygon", "candidates", "best"}), (RankResult, {"lines", "image_bbox"})):
        assert fields <= set(cls.model_json_schema()["properties"])


def test_bindings_and_header_agree():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "surya_amd.h")).read()
    for name in ("surya_rec_prefill_shared", "surya_op_rec_kv_fanout"):
        assert re.search(r"\bint " + name + r"\(", hdr), name
    if os.path.exists(L.LIB_PATH):
        lib = L.lib()
        assert len(lib.surya_rec_prefill_shared.argtypes) == 10 and len(lib.surya_op_rec_kv_fanout.argtypes) == 15
