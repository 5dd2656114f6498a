"""CPU: the host side of RecognitionPredictor.align: the device loop's forced-decoding contract (against the fake model of
test_scheduler_cpu.py, extended here with the four entry points and the ABI rules of include/surya_amd.h), the assembly of `greedy` and
`log_prob`, align's validation and id building, the schema, and the bindings."""
from types import SimpleNamespace

import numpy as np
import pytest
from PIL import Image

from surya_amd import _lib as L
from surya_amd.recognition import assemble
from surya_amd.recognition.loop import DeviceLoop
from surya_amd.recognition.predictor import RecognitionPredictor
from surya_amd.recognition.processor import SuryaOCRProcessor
from surya_amd.recognition.schema import CharAlternative, TextChar, TextLine
from surya_amd.recognition.tokenizer import ByteMathTokenizer, OCRTokenizer
from surya_amd.settings import settings
from test_scheduler_cpu import EOS, NOP, PAD, FakeModel, expected, make, script


def forced_ids_of(line):
    """The forced ids of `line`: mixed lengths, ending in EOS on even lines; line % 5 == 3 has none (it free-runs); line % 10 == 6 is forty-five
    equal ids -- a repetition that would trip detect_repeat_token."""
    if line % 5 == 3:
        return []
    if line % 10 == 6:
        return [777] * 45
    n = 1 + (line * 3) % 7
    ids = [5000 + line * 10 + k for k in range(n)]
    if line % 2 == 0:
        ids[-1] = EOS
    return ids


def outs_of(line, pos):
    """(greedy token, greedy probability, log-probability) the fake reports for token `pos` of `line`."""
    return script(line, pos), np.float32(0.5 + 0.001 * (pos % 50)), np.float32(-0.25 * (pos + 1) - line)


class FakeForcedModel(FakeModel):
    """FakeModel + set_forced / set_forced_tokens / read_forced / wait_forced with the contracts of surya_amd.h: tokens only while on, no
    slot twice, slots in range, at most SA_MAX_FORCED_TOKENS ids, a slot's ids and cursor last until they are set again (so a loop that
    forgets a reused slot emits the previous line's ids), outputs only while on and laid out like the outputs they run beside."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.forced, self.switches = False, []
        self.slot_ids = {s: [] for s in range(self.max_slots)}
        self.cursor = {s: 0 for s in range(self.max_slots)}
        self.prefill_forced, self.forced_inflight, self.token_calls = None, {}, 0

    def set_forced(self, on):
        assert not self.inflight, "switched while decode calls are in flight"
        self.forced = bool(on)
        self.switches.append(bool(on))
        if not on:
            self.slot_ids = {s: [] for s in range(self.max_slots)}

    def set_forced_tokens(self, slots, ids):
        assert self.forced, "SA_ERR_STATE: set_forced_tokens while off"
        assert not self.inflight and len(slots) == len(ids) and len(set(slots)) == len(slots), "SA_ERR_ARG"
        for s, seq in zip(slots, ids):
            assert 0 <= s < self.max_slots and len(seq) <= L.SA_MAX_FORCED_TOKENS and all(0 <= t < 70000 for t in seq), "SA_ERR_ARG"
            self.slot_ids[s], self.cursor[s] = list(seq), 0
        self.token_calls += 1

    def _emit(self, s, ln, pos):
        c = self.cursor[s]
        self.cursor[s] = c + 1
        return self.slot_ids[s][c] if c < len(self.slot_ids[s]) else script(ln, pos)

    def prefill(self, tiles, grid_hw, input_ids, slot_ids):
        super().prefill(tiles, grid_hw, input_ids, slot_ids)
        if not self.forced:
            return
        tok, sc, bb = self.prefill_out
        f = (np.full((1, self.max_slots), -9, np.int32), np.zeros((1, self.max_slots), np.float32), np.zeros((1, self.max_slots), np.float32))
        for ids, s in zip(input_ids, slot_ids):
            ln = ids[0] - 1000
            tok[0, s] = self._emit(s, ln, 0)
            f[0][0, s], f[1][0, s], f[2][0, s] = outs_of(ln, 0)
        self.prefill_forced = f

    def read_forced(self, n):
        assert self.forced and n == 1 and self.prefill_forced is not None, "SA_ERR_STATE"
        out, self.prefill_forced = self.prefill_forced, None
        return out

    def decode_async(self, n, ring):
        pos0 = {s: self.slot_pos[s] for s in self.active}
        super().decode_async(n, ring)
        if not self.forced:
            return
        tok = self.inflight[-1][2][0]
        f = (np.full((n, self.max_slots), -9, np.int32), np.zeros((n, self.max_slots), np.float32), np.zeros((n, self.max_slots), np.float32))
        for k in range(n):
            for s in self.active:
                ln = self.slot_line[s]
                tok[k, s] = self._emit(s, ln, pos0[s] + k)
                f[0][k, s], f[1][k, s], f[2][k, s] = outs_of(ln, pos0[s] + k)
        self.forced_inflight[ring] = (n, f)

    def wait_forced(self, n, ring):
        assert self.forced, "SA_ERR_STATE"
        m, f = self.forced_inflight.pop(ring)
        assert m == n
        return f


def _loop(model, slots, max_tokens, **kw):
    return DeviceLoop(model, EOS, PAD, NOP, slots, max_tokens, 0.2, **kw)


def want_stream(line, budget):
    ids = forced_ids_of(line)
    return ids if ids else expected(line, budget)


@pytest.mark.parametrize("n_lines,max_tokens,slots,sps", [(23, 48, 4, 4), (40, 48, 7, 1), (9, 48, 16, 8)])
def test_loop_forces_every_line_on_whatever_slot_it_gets(n_lines, max_tokens, slots, sps):
    """More lines than slots (slot reuse): every line emits its own ids -- budget = their number, no early stop on forty-five equal ids --
    and on_done gets its greedy tokens, probabilities and log-probabilities position by position; a line without ids free-runs."""
    old = settings.RECOGNITION_STEPS_PER_SYNC
    settings.RECOGNITION_STEPS_PER_SYNC = sps
    try:
        _, prep = make(n_lines, max_tokens, slots)
        prep["forced_ids"] = [forced_ids_of(i) for i in range(n_lines)]
        model = FakeForcedModel(slots)
        done = {}
        loop = _loop(model, slots, max_tokens, forced=True,
                     on_done=lambda k, toks, sc, bb, gt, gp, lp: done.__setitem__(k, (list(toks), gt, gp, lp)))
        loop.run(prep)
    finally:
        settings.RECOGNITION_STEPS_PER_SYNC = old
    assert model.switches == [True, False] and not model.forced
    assert model.token_calls == model.stats["prefills"]                     # set beside every prefill
    assert sorted(done) == list(range(n_lines))
    for k, (toks, gt, gp, lp) in done.items():
        assert toks == want_stream(k, prep["max_tokens"][k]), (k, toks)
        assert gt.shape == gp.shape == lp.shape == (len(toks),) and gt.dtype == np.int32 and lp.dtype == np.float32
        for pos in range(len(toks)):
            g, p, l = outs_of(k, pos)
            assert (gt[pos], gp[pos], lp[pos]) == (g, p, l), (k, pos)
    assert len(done[6][0]) == 45                                            # the repeat rule did not cut the forty-five equal ids
    assert loop.greedy_tok_mat.shape == loop.greedy_p_mat.shape == loop.logp_mat.shape == (n_lines, loop.cap)


def test_the_repeat_rule_still_stops_a_free_running_loop():
    """Line 6 of the scripted streams is a 3-cycle: without forcing it stops at the rule (test_scheduler_cpu pins the streams)."""
    _, prep = make(9, 90, 4)
    loop = _loop(FakeModel(4), 4, 90)
    loop.run(prep)
    assert loop.predicted_tokens[6] == expected(6, prep["max_tokens"][6]) and len(loop.predicted_tokens[6]) < prep["max_tokens"][6]


def test_loop_switches_off_after_an_exception():
    _, prep = make(9, 48, 4)
    prep["forced_ids"] = [forced_ids_of(i) for i in range(9)]
    model = FakeForcedModel(4)
    calls = []

    def boom(*a):
        calls.append(a)
        raise RuntimeError("consumer failed")

    with pytest.raises(RuntimeError, match="consumer failed"):
        _loop(model, 4, 48, forced=True, on_done=boom).run(prep)
    assert calls and model.switches == [True, False]


def test_loop_without_the_request_never_touches_the_entry_points():
    """The plain FakeModel has none of the four methods; on_done keeps its four arguments; no arrays are kept."""
    _, prep = make(9, 12, 4)
    seen = []
    loop = _loop(FakeModel(4), 4, 12, on_done=lambda *a: seen.append(len(a)))
    loop.run(prep)
    assert seen == [4] * 9 and loop.greedy_tok_mat is None and loop.logp_mat is None
    model = FakeForcedModel(4)
    _loop(model, 4, 12).run(prep)
    assert model.switches == [] and model.token_calls == 0
    with pytest.raises(AssertionError, match="exclude"):
        _loop(model, 4, 12, forced=True, alternatives=True)


def test_generate_requests_forcing_only_for_a_prep_with_forced_ids():
    pred, prep = make(9, 48, 4)
    pred.model = FakeForcedModel(4)
    pred.generate(prep, 4)
    assert pred.model.switches == []
    prep["forced_ids"] = [forced_ids_of(i) for i in range(9)]
    toks, _, _ = pred.generate(prep, 4)
    assert pred.model.switches == [True, False] and toks[0] == forced_ids_of(0)
    gt, gp, lp = pred.last_forced
    assert gt[1] == [outs_of(1, p)[0] for p in range(len(toks[1]))] and len(lp[1]) == len(toks[1])


# ------------------------------------------------------------------------------------------------- assembly
@pytest.fixture(scope="module")
def proc():
    return SuryaOCRProcessor(OCRTokenizer(None, ByteMathTokenizer(256), reserve_special=64))


def _flat(n):
    return {"polygons": [[5, 5, 600, 60]] * n, "res_scales": [(1.0, 1.0)] * n, "slices": [np.zeros((40, 300, 3), np.uint8)] * n, "forced": True}


def _item(proc, k, text, rng):
    tk = proc.ocr_tokenizer
    ids = tk(text, "ocr_with_boxes")["input_ids"][0] + [proc.eos_token_id]
    T = len(ids)
    rows = (np.arange(T)[:, None] * 10 + np.arange(6)[None, :]).astype(np.float32)         # every box far from the one before
    sc = rng.random(T).astype(np.float32).tolist()
    gt = np.asarray(ids, np.int32)
    gt[1::2] = tk("Z", "ocr_with_boxes")["input_ids"][0][0]                    # the model disagrees on every other token
    forced = (gt, rng.random(T).astype(np.float32), -rng.random(T).astype(np.float32))
    return (k, k, ids, sc, rows, forced)


def test_assembly_attaches_greedy_and_log_prob(proc):
    rng = np.random.default_rng(3)
    texts = ["hello", "", "a \U0001F600 b", "-" * 40]
    items = [_item(proc, k, t, rng) for k, t in enumerate(texts)]
    flat = _flat(len(texts))
    lines = assemble.assemble_batch(proc, flat, items, False, False, 1025)
    single = [assemble.assemble_line(proc, flat, *it[:5], False, False, 1025, alts=it[5]) for it in items]
    for ln, one, it, text in zip(lines, single, items, texts):
        assert ln.text == text and one.model_dump() == ln.model_dump()
        assert ln.log_prob == float(np.sum(np.asarray(it[5][2], np.float64))) and "log_prob" in ln.model_dump()
        assert len(ln.chars) == len(text)
        gt, gp = it[5][0].tolist(), it[5][1].tolist()
        for c in ln.chars:
            assert isinstance(c.greedy, CharAlternative) and c.alternatives is None and "alternatives" not in c.model_dump()
            assert c.greedy.token_id in gt and c.greedy.confidence in gp
        if text == "hello":                                                   # one UTF-16 run, boxes far apart: character i <- token i
            assert [c.greedy.text for c in ln.chars] == ["h", "Z", "l", "Z", "o"]
            assert [c.greedy.confidence for c in ln.chars] == gp[:5] and [c.confidence for c in ln.chars] == [float(np.float32(s)) for s in it[3][:5]]
    # without the flag the same items (five fields) assemble as they always did
    plain = assemble.assemble_batch(proc, {**flat, "forced": False}, [it[:5] for it in items], False, False, 1025)
    for ln, p in zip(lines, plain):
        assert p.log_prob is None and all(c.greedy is None for c in p.chars) and "log_prob" not in p.model_dump()
        d = ln.model_dump()
        d.pop("log_prob")
        for c in d["chars"]:
            c.pop("greedy")
        assert d == p.model_dump()


# ------------------------------------------------------------------------------------------------- align
def _pred(proc, vocab=70000):
    pred = object.__new__(RecognitionPredictor)
    pred.processor = proc
    pred.model = SimpleNamespace(vocab=vocab)
    return pred


def test_forced_ids_for_ocr_and_block_tasks(proc):
    pred, tk = _pred(proc), proc.ocr_tokenizer
    ids = pred.forced_ids("ab", "ocr_with_boxes")
    assert ids == [ord("a") + tk.special_token_offset, ord("b") + tk.special_token_offset, proc.eos_token_id]
    assert pred.forced_ids("", "ocr_without_boxes") == [proc.eos_token_id]
    assert len(pred.forced_ids("\U0001F600", "ocr_with_boxes")) == 3            # a surrogate pair and eos
    blk = pred.forced_ids("x+1", "block_without_boxes")
    assert blk == list(tk.math_tokenizer("x+1")["input_ids"]) + [proc.eos_token_id] and all(t < tk.qwen_offset for t in blk[:-1])
    assert all(type(t) is int for t in ids + blk)


def test_align_validation_names_the_image_and_the_line(proc):
    pred = _pred(proc)
    img = Image.new("RGB", (64, 16))
    box = [0, 0, 64, 16]
    old = settings.RECOGNITION_MAX_TOKENS
    try:
        settings.RECOGNITION_MAX_TOKENS = 8
        with pytest.raises(ValueError, match="bboxes or polygons"):
            pred.align([img], [["a"]])
        with pytest.raises(ValueError, match="1 images, 2 text lists"):
            pred.align([img], [["a"], ["b"]], bboxes=[[box]])
        with pytest.raises(ValueError, match="image 1 has 2 lines but 1 texts"):
            pred.align([img, img], [["a"], ["b"]], bboxes=[[box], [box, box]])
        with pytest.raises(ValueError, match=r"image 0, line 1: 9 tokens \(eos included\) exceed the token budget 8"):
            pred.align([img], [["a", "12345678"]], bboxes=[[box, box]])
        with pytest.raises(ValueError, match="image 0, line 0: the text must be a str"):
            pred.align([img], [[None]], bboxes=[[box]])
        with pytest.raises(ValueError, match="not supported"):
            pred.align([img], [["a"]], bboxes=[[box]], task_names=["nonsense"])
        settings.RECOGNITION_MAX_TOKENS = 4096
        with pytest.raises(ValueError, match=f"image 0, line 0: 1201 tokens exceed SA_MAX_FORCED_TOKENS = {L.SA_MAX_FORCED_TOKENS}"):
            pred.align([img], [["x" * 1200]], bboxes=[[box]])
        small = _pred(proc, vocab=proc.ocr_tokenizer.special_token_offset + 100)
        with pytest.raises(ValueError, match="image 1, line 0: token id .* outside the model's vocabulary"):
            small.align([img, img], [["A"], ["é"]], polygons=[[[[0, 0], [64, 0], [64, 16], [0, 16]]]] * 2)
        for attr, val in (("shard_lines", True), ("process_group", object())):
            p = _pred(proc)
            setattr(p, attr, val)
            with pytest.raises(NotImplementedError, match="one rank"):
                p.align([img], [["a"]], bboxes=[[box]])
    finally:
        settings.RECOGNITION_MAX_TOKENS = old


def test_call_keeps_its_signature_and_align_has_the_stated_one():
    import inspect
    assert list(inspect.signature(RecognitionPredictor.__call__).parameters)[-2:] == ["allowlist", "blocklist"]
    assert list(inspect.signature(RecognitionPredictor.align).parameters) == [
        "self", "images", "texts", "task_names", "bboxes", "polygons", "recognition_batch_size", "math_mode", "return_words"]


# ------------------------------------------------------------------------------------------------- schema, bindings
def test_new_fields_are_absent_from_the_serialised_form_while_none():
    poly = [[0, 0], [8, 0], [8, 10], [0, 10]]
    c = TextChar(text="a", polygon=poly, confidence=0.5)
    ln = TextLine(text="a", polygon=poly, confidence=0.5, chars=[c])
    assert c.greedy is None and ln.log_prob is None
    assert "greedy" not in c.model_dump() and "log_prob" not in ln.model_dump() and "greedy" not in ln.model_dump()["chars"][0]
    assert "greedy" not in c.model_dump_json() and "log_prob" not in ln.model_dump_json()
    assert "greedy" not in c.model_fields_set and "log_prob" not in ln.model_fields_set
    c2 = TextChar(text="a", polygon=poly, confidence=0.5, greedy=CharAlternative(text="b", confidence=0.75, token_id=7))
    l2 = TextLine(text="a", polygon=poly, confidence=0.5, chars=[c2], log_prob=-1.5)
    assert c2.model_dump()["greedy"] == {"text": "b", "confidence": 0.75, "token_id": 7}
    assert l2.model_dump()["log_prob"] == -1.5 and '"log_prob":-1.5' in l2.model_dump_json()
    assert TextLine.model_validate_json(l2.model_dump_json()) == l2
    assert "greedy" in TextChar.model_json_schema()["properties"] and "log_prob" in TextLine.model_json_schema()["properties"]


def test_bindings_and_header_agree():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "surya_amd.h")).read()
    assert int(re.search(r"#define SA_MAX_FORCED_TOKENS (\d+)", hdr).group(1)) == L.SA_MAX_FORCED_TOKENS == 1024
    for name in ("surya_rec_set_forced", "surya_rec_set_forced_tokens", "surya_rec_read_forced", "surya_rec_wait_forced", "surya_op_lm_head_forced"):
        assert re.search(r"\bint " + name + r"\(", hdr), name
    if os.path.exists(L.LIB_PATH):
        lib = L.lib()
        assert len(lib.surya_rec_set_forced_tokens.argtypes) == 6 and len(lib.surya_op_lm_head_forced.argtypes) == 14
        assert len(lib.surya_rec_read_forced.argtypes) == 6 and len(lib.surya_rec_wait_forced.argtypes) == 6
