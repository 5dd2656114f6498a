"""CPU: lines kept on the device (RecognitionPredictor.encode / recognition/encoded.py) without a GPU: the row allocator, the device
loop's store modes on the contract-checking fake models of the scheduler, forced, rank and beam tests, EncodedLines on a fake predictor
(`lines=` selection, result order, every refusal), and the bindings against the header."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
from PIL import Image

from surya_amd import _lib as L
from surya_amd.recognition.encoded import EncodedLines, RowAllocator
from surya_amd.recognition.loop import DeviceLoop
from surya_amd.recognition.predictor import RecognitionPredictor
from surya_amd.recognition.schema import TextLine
from surya_amd.settings import settings
from test_beam_cpu import FakeBeamModel, pure_beam_search
from test_forced_cpu import FakeForcedModel
from test_rank_cpu import BOXES, CANDS, FakeFanModel, _check_results, _key, _pred, cand_ids, fake_loop_settings, proc  # noqa: F401
from test_scheduler_cpu import EOS, NOP, PAD, FakeModel, expected, make, script


# ---------------------------------------------------------------------------------------------------------- the row allocator
def test_allocator_first_fit_free_and_coalesce():
    grown = []
    a = RowAllocator(grown.append, capacity=100)
    r = [a.alloc(n) for n in (10, 20, 30, 40)]
    assert r == [0, 10, 30, 60] and a.free_list == [] and a.used == 100 and not grown
    a.free(10)
    a.free(60)
    assert a.free_list == [[10, 20], [60, 40]]
    assert a.alloc(15) == 10                                  # first fit: the lower hole, though the upper one is larger
    assert a.alloc(30) == 60 and a.free_list == [[25, 5], [90, 10]]
    a.free(30)                                                # joins the free block below it ([25, 5]); rows 60.. above it are live
    assert a.free_list == [[25, 35], [90, 10]]
    a.free(60)                                                # joins both neighbours
    assert a.free_list == [[25, 75]]
    a.free(0)
    a.free(10)
    assert a.free_list == [[0, 100]] and a.used == 0 and a.live == {}
    with pytest.raises(KeyError):
        a.free(10)                                            # not a live range


def test_allocator_exhaustion_leads_to_a_reserve_call():
    grown = []
    a = RowAllocator(grown.append, chunk=64)
    assert a.capacity == 0 and a.alloc(10) == 0 and grown == [64]      # lazily: nothing is reserved before the first range
    assert a.alloc(50) == 10 and grown == [64]
    assert a.alloc(10) == 60 and grown == [64, 128]           # 4 rows were left: the tail grows, doubling
    assert a.free_list == [[70, 58]]
    assert a.alloc(300) == 70 and grown == [64, 128, 370]     # more than double: what is missing
    assert a.capacity == 370 and a.free_list == []
    a.free(10)
    assert a.alloc(51) == 370 and grown[-1] == 740 and a.free_list == [[10, 50], [421, 319]]      # a hole that is too small stays a hole

    def refuse(rows):
        raise MemoryError("no room")
    b = RowAllocator(refuse, capacity=8)
    assert b.alloc(8) == 0
    with pytest.raises(MemoryError):
        b.alloc(1)
    assert b.capacity == 8 and b.free_list == [] and b.live == {0: 8}      # a failed reserve changed nothing


# ------------------------------------------------------------------------------------------------ the loop's store modes on fakes
class StoreFake(FakeFanModel):
    """FakeFanModel + the prompt store with the rules of surya_rec_prefill_keep / surya_rec_restore / surya_rec_drop_prompts: ranges inside
    the reserved rows and free, entries known, fans of distinct, free slots, nothing in flight. `log` keeps the order of the calls."""

    def __init__(self, slots):
        super().__init__(slots)
        self.cap, self.entries, self.log = 0, {}, []
        self.dtype, self.handle = "fake", SimpleNamespace(value=7)

    def prefill(self, *a, **k):
        self.log.append(("prefill",))
        return FakeForcedModel.prefill(self, *a, **k)

    def encode_ahead(self, *a, **k):
        self.log.append(("encode_ahead",))
        return super().encode_ahead(*a, **k)

    def decode_async(self, n, ring):
        return FakeFanModel.decode_async(self, n, ring) if self.forced else FakeModel.decode_async(self, n, ring)

    def reserve_prompts(self, rows):
        assert rows > self.cap
        self.cap = rows
        self.log.append(("reserve", rows))

    def prefill_keep(self, tiles, grid_hw, input_ids, slot_ids, keep_first):
        assert len(keep_first) == len(input_ids)
        taken = {r for f, n in self.entries.items() for r in range(f, f + n[1])}
        for ids, f in zip(input_ids, keep_first):
            rows = set(range(f, f + len(ids)))
            assert f >= 0 and f + len(ids) <= self.cap and not rows & taken, "SA_ERR_ARG: past the reserved rows, or over a live entry"
            taken |= rows
        FakeForcedModel.prefill(self, tiles, grid_hw, input_ids, slot_ids)
        for ids, f in zip(input_ids, keep_first):
            self.entries[f] = (ids[0] - 1000, len(ids))
        self.log.append(("prefill_keep", list(slot_ids), list(keep_first)))

    def restore(self, first, fan_slots):
        assert not self.inflight, "restore while decode calls are in flight"
        assert len(first) == len(fan_slots) > 0 and all(f in self.entries for f in first), "SA_ERR_ARG: an unknown entry"
        named = [s for f in fan_slots for s in f]
        assert all(len(f) > 0 for f in fan_slots) and len(set(named)) == len(named) <= self.max_slots, "SA_ERR_ARG: an empty fan / a slot twice"
        assert all(0 <= s < self.max_slots for s in named) and not set(named) & set(self.active), "a named slot is out of range or busy"
        S = self.max_slots
        tok, sc, bb = np.zeros((1, S), np.int32), np.zeros((1, S), np.float32), np.zeros((1, S, 6), np.int32)
        f = (np.full((1, S), -9, np.int32), np.zeros((1, S), np.float32), np.zeros((1, S), np.float32))
        for e, fan in zip(first, fan_slots):
            ln = self.entries[e][0]
            for s in fan:
                self.slot_line[s], self.slot_pos[s] = ln, 1
                tok[0, s], sc[0, s], bb[0, s] = script(ln, 0), 0.5, ln
                if self.forced:
                    tok[0, s], f[0][0, s], f[1][0, s], f[2][0, s] = self._step(s)
        self.prefill_out, self.prefill_forced = (tok, sc, bb), (f if self.forced else None)
        self.log.append(("restore", list(first), [list(x) for x in fan_slots], sorted(self.active)))
        self.stats["prefills"] += 1

    def drop_prompts(self, first):
        assert all(f in self.entries for f in first) and len(set(first)) == len(first), "SA_ERR_ARG: not a live entry"
        for f in first:
            del self.entries[f]
        self.log.append(("drop", list(first)))

    def set_token_masks(self, table):
        self.log.append(("set_token_masks", None if table is None else len(table)))

    def set_slot_masks(self, slots, ids):
        self.log.append(("set_slot_masks", list(slots), list(ids)))

    def set_forced_tokens(self, slots, ids):
        self.log.append(("set_forced_tokens", list(slots)))
        return super().set_forced_tokens(slots, ids)


def _restored(prep, first, **more):
    """`prep` of fresh lines as the dict of the same lines restored from store rows `first`: no tiles."""
    d = dict(prep, tiles=None, tile_offs=None, store_first=list(first), **more)
    return d


@pytest.fixture
def loop_settings():
    old = (settings.RECOGNITION_STEPS_PER_SYNC, settings.RECOGNITION_ENCODE_AHEAD)
    settings.RECOGNITION_STEPS_PER_SYNC, settings.RECOGNITION_ENCODE_AHEAD = 4, True
    yield
    settings.RECOGNITION_STEPS_PER_SYNC, settings.RECOGNITION_ENCODE_AHEAD = old


def _keep_all(model, n_lines, slots):
    """A keep run of n_lines lines of three prompt ids each at rows 3 * i; -> the fresh lines' dict."""
    _, prep = make(n_lines, 12, slots)
    model.reserve_prompts(3 * n_lines + 5)
    done = []
    DeviceLoop(model, EOS, PAD, NOP, slots, 1, 0.2, store="keep", on_done=lambda k, toks, *r: done.append((k, list(toks)))).run(
        dict(prep, max_tokens={i: 1 for i in range(n_lines)}, store_first=[3 * i for i in range(n_lines)]))
    assert sorted(done) == [(i, [script(i, 0)]) for i in range(n_lines)]      # the prefill's token, then the line stopped
    return prep


def test_a_keep_run_encodes_every_line_and_decodes_nothing(loop_settings):
    model = StoreFake(4)
    _keep_all(model, 11, 4)
    assert model.entries == {3 * i: (i, 3) for i in range(11)} and model.stats["decode_calls"] == 0
    assert not [c for c in model.log if c[0] in ("prefill", "restore")] and [c for c in model.log if c[0] == "encode_ahead"]
    keeps = [c for c in model.log if c[0] == "prefill_keep"]
    assert [f for c in keeps for f in c[2]] == [3 * i for i in range(11)] and all(len(c[1]) <= 4 for c in keeps)


def test_a_restore_run_reads_the_lines_without_tiles_encoder_or_prefill(loop_settings):
    """23 lines through 4 slots with a mask table: the streams are the fresh lines' streams; every restore comes behind its set_slot_masks
    call for the same slots, names free slots only and as many lines as there are, refills a slot as soon as one is free (no
    min_prefill_ratio wait), and the table is switched off on the way out."""
    model = StoreFake(4)
    prep = _keep_all(model, 23, 4)
    model.log.clear()
    table = np.ones((2, 4), np.uint32)
    done = {}
    loop = DeviceLoop(model, EOS, PAD, NOP, 4, 12, 0.9, on_done=lambda k, toks, *r: done.__setitem__(k, list(toks)), store="restore")
    loop.run(_restored(prep, [3 * i for i in range(23)], token_masks=table, mask_ids=[i % 2 - 1 for i in range(23)]))
    assert done == {i: expected(i, prep["max_tokens"][i]) for i in range(23)}
    assert not [c for c in model.log if c[0] in ("prefill", "prefill_keep", "encode_ahead")] and not model.ahead and not model.inflight
    assert model.log[0] == ("set_token_masks", 2) and model.log[-1] == ("set_token_masks", None)
    calls = model.log[1:-1]
    assert len(calls) % 2 == 0 and len(calls) >= 2 * 6
    restored = []
    for setter, rest in zip(calls[::2], calls[1::2]):
        assert setter[0] == "set_slot_masks" and rest[0] == "restore"                   # call order: set_slot_* -> restore
        slots = [f[0] for f in rest[2]]
        assert all(len(f) == 1 for f in rest[2]) and setter[1] == slots and not set(slots) & set(rest[3])
        lines = [f // 3 for f in rest[1]]
        assert setter[2] == [i % 2 - 1 for i in lines]                                   # a line's mask id goes where the line goes
        assert len(slots) == min(4 - len(rest[3]), 23 - len(restored))                   # every free slot is refilled, at a ratio of 0.9 too
        restored += lines
    assert restored == list(range(23))                                                   # every line once, in queue order


def test_a_restore_run_lands_candidate_fans(loop_settings):
    """rank's loop on restored lines: 6 slots, lines of 3 / 1 / 2 / 4 candidates: a line lands in as many slots as it has candidates,
    behind set_forced_tokens for those slots; the fourth line waits for four free slots."""
    lens = [[5, 1, 20], [3], [2, 24], [4, 1, 6, 2]]
    model = StoreFake(6)
    prep = _keep_all(model, 4, 6)
    model.log.clear()
    forced = [[cand_ids(i, j, n) for j, n in enumerate(line)] for i, line in enumerate(lens)]
    done = {}
    loop = DeviceLoop(model, EOS, PAD, NOP, 6, 48, 0.2, forced=True, fan=True, store="restore", on_done=done.__setitem__)
    loop.run(_restored(dict(prep, max_tokens={i: 48 for i in range(4)}), [0, 3, 6, 9], forced_ids=forced))
    _check_results(done, forced)
    assert model.switches == [True, False] and not [c for c in model.log if c[0] in ("prefill", "prefill_keep", "encode_ahead")]
    (t0, r0), (t1, r1) = [(model.log[i], model.log[i + 1]) for i in range(0, len(model.log), 2)]
    assert t0[0] == t1[0] == "set_forced_tokens" and r0[0] == r1[0] == "restore"
    assert r0[1:3] == ([0, 3, 6], [[0, 1, 2], [3], [4, 5]]) and t0[1] == [0, 1, 2, 3, 4, 5]      # fan sizes = candidate counts
    assert r1[1] == [9] and len(r1[2][0]) == 4 and t1[1] == r1[2][0] and not set(r1[2][0]) & set(r1[3])


class StoreBeamFake(FakeBeamModel):
    """FakeBeamModel + restore: every fan is the lead slot of one free group."""

    def __init__(self, slots, entries):
        super().__init__(slots)
        self.entries, self.restores = entries, []

    def restore(self, first, fan_slots):
        assert all(len(f) == 1 for f in fan_slots) and all(e in self.entries for e in first), "SA_ERR_ARG"
        self.restores.append((list(first), [f[0] for f in fan_slots]))
        FakeBeamModel.prefill(self, np.zeros((0, 1)), [(2, 2)] * len(first), [[1000 + self.entries[e]] for e in first], [f[0] for f in fan_slots])


def test_a_restore_run_lands_lines_in_lead_slots_of_whole_groups(loop_settings):
    B, slots, n = 3, 7, 9
    model = StoreBeamFake(slots, {10 * i: i for i in range(n)})
    _, prep = make(n, 9, slots)
    done = {}
    DeviceLoop(model, EOS, PAD, NOP, slots, 9, 0.2, beam=B, store="restore", on_done=done.__setitem__).run(
        _restored(prep, [10 * i for i in range(n)]))
    assert model.switches == [B, 0] and sorted(done) == list(range(n))
    for k in range(n):
        want = pure_beam_search(k, B, prep["max_tokens"][k])
        assert [h.tokens for h in done[k]] == [w[0] for w in want]
    assert all(s % B == 0 and s + B <= slots for _, leads in model.restores for s in leads)       # two groups in seven slots
    assert [e for firsts, _ in model.restores for e in firsts] == [10 * i for i in range(n)] and max(len(l) for _, l in model.restores) <= 2


def test_a_store_row_is_admitted_once_and_modes_are_refused(loop_settings):
    model = StoreFake(4)
    prep = _keep_all(model, 3, 4)
    with pytest.raises(AssertionError, match="once per run"):
        DeviceLoop(model, EOS, PAD, NOP, 4, 12, 0.2, store="restore").run(_restored(prep, [0, 3, 3]))
    loop = DeviceLoop(model, EOS, PAD, NOP, 4, 12, 0.2, store="restore")
    loop.admit(_restored(make(2, 12, 4)[1], [0, 3]))
    with pytest.raises(AssertionError):                       # (fed lines continue the ids: the third line of the run)
        loop.admit(dict(_restored(make(3, 12, 4)[1], [3]), prompts=make(3, 12, 4)[1]["prompts"][2:], grids=[(2, 2)], prompt_ids=[[1002, 5, 6]]))
    with pytest.raises(AssertionError, match="store_first"):
        DeviceLoop(model, EOS, PAD, NOP, 4, 12, 0.2, store="restore").run(_restored(prep, [0, 3]))
    with pytest.raises(AssertionError, match="None, 'keep' or 'restore'"):
        DeviceLoop(model, EOS, PAD, NOP, 4, 12, 0.2, store="both")
    with pytest.raises(AssertionError, match="kept by plain greedy prefills"):
        DeviceLoop(model, EOS, PAD, NOP, 4, 12, 0.2, forced=True, fan=True, store="keep")
    with pytest.raises(AssertionError, match="kept by plain greedy prefills"):
        DeviceLoop(model, EOS, PAD, NOP, 4, 12, 0.2, beam=2, store="keep")


def test_the_mode_switch_off_runs_after_an_exception(loop_settings):
    model = StoreFake(4)
    prep = _keep_all(model, 5, 4)
    model.log.clear()

    def boom(first, fan_slots):
        raise RuntimeError("restore failed")
    model.restore = boom
    with pytest.raises(RuntimeError, match="restore failed"):
        DeviceLoop(model, EOS, PAD, NOP, 4, 12, 0.2, forced=True, store="restore").run(
            _restored(prep, [0, 3, 6, 9, 12], forced_ids=[[200 + i, 300 + i] for i in range(5)]))
    assert model.switches == [True, False]
    with pytest.raises(RuntimeError, match="restore failed"):
        DeviceLoop(model, EOS, PAD, NOP, 4, 12, 0.2, store="restore").run(
            _restored(prep, [0, 3, 6, 9, 12], token_masks=np.ones((1, 4), np.uint32), mask_ids=[0] * 5))
    assert [c for c in model.log if c[0] == "set_token_masks"] == [("set_token_masks", 1), ("set_token_masks", None)]


def test_a_loop_without_a_store_never_touches_the_entry_points(loop_settings):
    class NoStore(FakeModel):
        def prefill_keep(self, *a, **k):
            raise AssertionError("prefill_keep without store='keep'")
        restore = reserve_prompts = drop_prompts = prefill_keep
    pred, prep = make(9, 12, 3)
    pred.model = NoStore(3)
    toks, _, _ = pred.generate(prep, 3)
    assert toks == [expected(i, prep["max_tokens"][i]) for i in range(9)]


# ----------------------------------------------------------------------------------------------- EncodedLines on a fake predictor
def _enc_pred(proc, slots=8):
    pred = _pred(proc, slots)
    pred.model = StoreFake(slots)
    pred.model.cfg = SimpleNamespace(encoder=SimpleNamespace(spatial_merge_size=2), bbox_size=1024)
    pred.last_timing = {}

    def fake_assemble(flat, items, drop_repeated_text, return_words, bbox_size):
        return [TextLine(text=",".join(map(str, it[2])), polygon=flat["polygons"][it[1]], confidence=1.0, chars=[]) for it in items]
    pred._assemble_batch = fake_assemble
    return pred


IMAGES = [Image.new("RGB", (64, 40)), Image.new("RGB", (48, 32))]
BOXES3 = [[[2, 3, 60, 14], [4, 20, 40, 31], [1, 1, 20, 9]], [[1, 5, 30, 15]]]


def _texts(results):
    return [[ln.text for ln in r.text_lines] for r in results]


def _stream_of(box, budget=12):
    """The text the fake predictor gives the line cut at `box`: the scripted stream of the line's key, which ends at the budget or at
    the PROCESSOR's eos (the script's own EOS is an ordinary id to it)."""
    ln = SimpleNamespace(x0=box[0], y0=box[1])
    return ",".join(str(script(_key(ln), t)) for t in range(budget))


def test_encoded_read_equals_the_call_and_lines_select_and_order(proc, fake_loop_settings):
    pred = _enc_pred(proc)
    direct = pred(IMAGES, bboxes=BOXES3, recognition_batch_size=8)
    assert _texts(direct) == [[_stream_of(b) for b in page] for page in BOXES3]
    with pred.encode(IMAGES, bboxes=BOXES3, recognition_batch_size=8) as enc:
        assert len(enc) == 4 and enc.line_counts == [3, 1] and len(pred.model.entries) == 4 and not enc.released
        calls = len(pred.model.log)
        got = enc.read(recognition_batch_size=8)
        assert [r.model_dump() for r in got] == [r.model_dump() for r in direct]
        after = pred.model.log[calls:]
        assert {c[0] for c in after} == {"restore"}, "a read of kept lines runs no encoder and no prefill"
        # subsets: only those lines, in that order; a page may select nothing
        sub = enc.read(lines=[[2, 0], []], recognition_batch_size=8)
        assert _texts(sub) == [[_stream_of(BOXES3[0][2]), _stream_of(BOXES3[0][0])], []]
        assert [ln.polygon for ln in sub[0].text_lines] == [direct[0].text_lines[2].polygon, direct[0].text_lines[0].polygon]
        assert sub[1].image_bbox == direct[1].image_bbox
        assert _texts(enc.read(lines=[None, [0]], recognition_batch_size=8)) == _texts(direct)
        assert enc.read(lines=[[], []], recognition_batch_size=8) == []                  # no line at all: the call's contract
        for bad in ([[0]], [[3], []], [[0, 0], []], [[-1], []], [[True], []], "all"):
            with pytest.raises(ValueError):
                enc.read(lines=bad, recognition_batch_size=8)
        assert _texts(enc.read(recognition_batch_size=8)) == _texts(direct)              # ... and a second read equals the first
        first = sorted(pred.model.entries)
    assert enc.released and pred.model.entries == {} and [sorted(c[1]) for c in pred.model.log if c[0] == "drop"] == [first]
    enc.release()                                             # idempotent


def test_encoded_rank_and_align_equal_the_direct_calls(proc, fake_loop_settings):
    pred = _enc_pred(proc)
    want_rank = pred.rank(IMAGES, CANDS, bboxes=BOXES, recognition_batch_size=8)
    want_align = pred.align(IMAGES, [[c[0] for c in page] for page in CANDS], bboxes=BOXES, recognition_batch_size=8)
    enc = pred.encode(IMAGES, bboxes=BOXES, recognition_batch_size=8)
    got = enc.rank(CANDS, recognition_batch_size=8)
    assert [r.model_dump() for r in got] == [r.model_dump() for r in want_rank]
    fans = [c for c in pred.model.log if c[0] == "restore"][-1][2]
    assert sorted(len(f) for f in fans) == [1, 3, 3]          # distinct candidates per line: "ab" twice counts once
    got = enc.align([[c[0] for c in page] for page in CANDS], recognition_batch_size=8)
    assert [r.model_dump() for r in got] == [r.model_dump() for r in want_align]
    # a subset: candidates and texts have one entry per SELECTED line
    sub = enc.rank([[CANDS[0][1]], CANDS[1]], lines=[[1], [0]], recognition_batch_size=8)
    assert [r.model_dump() for r in sub] == [RankSlice(want_rank[0], [1]).model_dump(), want_rank[1].model_dump()]
    with pytest.raises(ValueError, match="image 0 has 1 lines but 2 candidate lists"):
        enc.rank(CANDS, lines=[[1], [0]], recognition_batch_size=8)
    enc.release()


def RankSlice(result, idx):
    return type(result)(lines=[result.lines[i] for i in idx], image_bbox=result.image_bbox)


def test_every_refusal_comes_before_any_model_call(proc, fake_loop_settings):
    pred = _enc_pred(proc)
    enc = pred.encode(IMAGES, bboxes=BOXES, recognition_batch_size=8)
    calls = len(pred.model.log)

    def refused(exc, match, fn, *a, **k):
        with pytest.raises(exc, match=match):
            fn(*a, **k)
        assert len(pred.model.log) == calls and not pred.model.inflight, "a refused call reached the model"
    refused(ValueError, "det_predictor", pred.encode, IMAGES, det_predictor=object())
    refused(ValueError, "bboxes or polygons", pred.encode, IMAGES)
    refused(ValueError, "task", pred.encode, IMAGES, task_names=["nope", "nope"], bboxes=BOXES)
    refused(ValueError, "2 images, 1 bbox", pred.encode, IMAGES, bboxes=BOXES[:1])
    for attr, value in (("shard_lines", True), ("shard_pages", True), ("process_group", object())):
        setattr(pred, attr, value)
        refused(NotImplementedError, "one rank", pred.encode, IMAGES, bboxes=BOXES)
        refused(NotImplementedError, "one rank", enc.read)
        refused(NotImplementedError, "one rank", enc.rank, CANDS)
        refused(NotImplementedError, "one rank", enc.align, [["a", "b"], ["c"]])
        setattr(pred, attr, False if attr != "process_group" else None)
    pred.model.kv_fp8 = True
    refused(ValueError, "fp8 KV cache", pred.encode, IMAGES, bboxes=BOXES)
    refused(ValueError, "fp8 KV cache", enc.read)
    refused(ValueError, "fp8 KV cache", enc.rank, CANDS)
    pred.model.kv_fp8 = False
    other = _enc_pred(proc)
    refused(ValueError, "another predictor", enc.read, predictor=other)
    refused(ValueError, "another predictor", enc.rank, CANDS, predictor=other)
    refused(ValueError, "another predictor", enc.align, [["a", "b"], ["c"]], predictor=other)
    mine, pred.model = pred.model, other.model                # the predictor's model was replaced: the prompts live in the old one
    with pytest.raises(ValueError, match="another predictor"):
        enc.read()
    assert len(mine.log) == calls and other.model.log == []
    pred.model = mine
    pred.top_k = 7                                            # what __call__ refuses, read refuses
    refused(ValueError, "top_k", enc.read)
    pred.top_k = None
    pred.pattern = r"\d+"
    refused(ValueError, "pattern does not apply", enc.rank, CANDS)
    pred.pattern = None
    assert _texts(enc.read(recognition_batch_size=8)) == [[_stream_of(b) for b in page] for page in BOXES]
    enc.release()
    calls = len(pred.model.log)
    refused(ValueError, "released", enc.read)
    refused(ValueError, "released", enc.rank, CANDS)
    refused(ValueError, "released", enc.align, [["a", "b"], ["c"]])


def test_several_encoded_sets_share_the_store_and_a_finaliser_releases(proc, fake_loop_settings):
    pred = _enc_pred(proc)
    a = pred.encode(IMAGES, bboxes=BOXES3, recognition_batch_size=8)
    b = pred.encode(IMAGES[:1], bboxes=[BOXES[0]], recognition_batch_size=8)
    alloc = pred.model._prompt_rows
    assert len(pred.model.entries) == 6 and alloc.used == 18 and [c for c in pred.model.log if c[0] == "reserve"] == [("reserve", 4096)]
    rows_a = sorted(a._first)
    a.release()
    assert sorted(pred.model.entries) == sorted(b._first) and alloc.used == 6
    c = pred.encode(IMAGES, bboxes=BOXES3, recognition_batch_size=8)
    assert sorted(c._first) == rows_a, "the freed rows are handed out again, first fit"
    assert _texts(b.read(recognition_batch_size=8)) == [[_stream_of(x) for x in BOXES[0]]]
    assert _texts(c.read(recognition_batch_size=8)) == [[_stream_of(x) for x in page] for page in BOXES3]
    del b                                                     # collected: the finaliser drops its entries
    import gc
    gc.collect()
    assert sorted(pred.model.entries) == rows_a and alloc.used == 12
    # an encode that fails half-way gives its rows back
    def boom(*a_, **k):
        raise RuntimeError("prefill_keep failed")
    keep, pred.model.prefill_keep = pred.model.prefill_keep, boom
    with pytest.raises(RuntimeError, match="prefill_keep failed"):
        pred.encode(IMAGES[:1], bboxes=[BOXES[0]], recognition_batch_size=8)
    pred.model.prefill_keep = keep
    assert alloc.used == 12 and sorted(pred.model.entries) == rows_a
    c.release()
    assert alloc.used == 0 and alloc.free_list == [[0, 4096]]
    assert pred.encode([], bboxes=[], recognition_batch_size=8).read() == []      # no images: no lines, no rows


# --------------------------------------------------------------------------------------------------------------- the bindings
def test_bindings_and_header_agree():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "surya_amd.h")).read()
    want = {"surya_rec_reserve_prompts": 3, "surya_rec_prefill_keep": 10, "surya_rec_restore": 6, "surya_rec_drop_prompts": 3,
            "surya_rec_prompt_store_info": 3, "surya_op_rec_kv_keep": 21, "surya_op_rec_kv_restore": 18}
    for name, n in want.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == n, name                 # the declaration's argument count ...
    if os.path.exists(L.LIB_PATH):
        lib = L.lib()
        for name, n in want.items():
            assert len(getattr(lib, name).argtypes) == n, name       # ... is the binding's
    # the model's methods exist under the names the loop calls
    from surya_amd.recognition.model import HipRecModel
    for name in ("reserve_prompts", "prefill_keep", "restore", "drop_prompts", "prompt_store_info"):
        assert callable(getattr(HipRecModel, name)), name
