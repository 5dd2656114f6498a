"""CPU: beam search without a GPU. (1) surya_amd/csrc/beam_core.h -- the selection and placement rules the device kernel runs -- compiled
with g++ and checked against their plain-Python restatement (tests/beam_ref.py) on random groups; (2) DeviceLoop(beam=B) against a fake
model that reports what the device would and a pure-Python beam search over the same scoring function; (3) the predictor's argument
checks, the schema, and the ctypes declarations of the new C entries."""
import re
from collections import deque
from types import SimpleNamespace

import numpy as np
import pytest

import beam_ref as br
from surya_amd.recognition.loop import BeamHypothesis, DeviceLoop
from surya_amd.recognition.postprocess import detect_repeat_token
from surya_amd.settings import settings
from test_scheduler_cpu import EOS, NOP, PAD, FakeModel, make

A = br.A
KEYS = ("token", "parent", "rank", "finished", "fork_src", "prob", "logp")


# ------------------------------------------------------------------------------------------------- (1) the core
@pytest.mark.parametrize("B", [2, 3, 4])
@pytest.mark.parametrize("first", [False, True])
def test_core_matches_the_python_statement_of_the_rules(B, first):
    rng = np.random.default_rng(100 * B + first)
    G = 400
    score, fin, ids, ps = br.random_groups(rng, G, B, EOS, PAD, NOP, first)
    got = br.native_select(G, B, score, fin, ids, ps, EOS, PAD, NOP, first)
    seen = dict(tie=0, frozen=0, short=0, one_parent=0, moved=0)
    for g in range(G):
        s = slice(g * B, g * B + B)
        want = br.select_group(B, g * B, score[s], fin[s], ids[s], ps[s], EOS, PAD, NOP, first)
        for k in KEYS:
            w = np.asarray(want[k], got[k].dtype)
            assert got[k][s].tobytes() == w.tobytes(), (g, k, got[k][s], w)          # logp / prob: bit for bit
        par, src, lp = got["parent"][s], got["fork_src"][s], got["logp"][s]
        # no fork source is a destination of the same step
        dests = {g * B + b for b in range(B) if src[b] >= 0}
        assert not dests & {int(x) for x in src if x >= 0}
        for b in range(B):
            assert (src[b] == -1) == (par[b] in (b, -1))                             # a copy exactly where a beam came from another slot
            if par[b] >= 0 and par[b] != b:
                assert par[par[b]] == par[b], "a parent with a moved child kept its best child in place"
        # a surviving parent's best child sits in the parent's slot
        for p in set(par[par >= 0].tolist()):
            kids = [b for b in range(B) if par[b] == p]
            assert p in kids and lp[p] == max(lp[b] for b in kids)
        alive = lp[par >= 0]
        seen["tie"] += len(set(alive.tolist())) < alive.size
        seen["frozen"] += bool(((got["prob"][s] == 0) & (par >= 0)).any())
        seen["short"] += bool((par < 0).any())
        seen["one_parent"] += alive.size == B and len(set(par.tolist())) == 1
        seen["moved"] += bool((src >= 0).any())
    want_seen = ("tie", "short", "one_parent", "moved") if first else tuple(seen)
    assert all(seen[k] > 0 for k in want_seen), seen                                   # the corners were really there


def test_core_log_prob_is_the_rounded_double_logarithm():
    ps = np.asarray([[1.0, 0.5, 1e-30, 3e-5]], np.float32).repeat(2, 0)
    got = br.native_select(1, 2, np.zeros(2, np.float32), np.zeros(2, np.int32), np.arange(8, dtype=np.int32).reshape(2, 4) + 10, ps, EOS, PAD,
                           NOP, True)
    assert got["logp"].tolist() == [np.float32(0.0), np.float32(np.log(0.5))] and got["token"].tolist() == [10, 11]


# ------------------------------------------------------------------------------------------------- (2) the device loop
def alts_of(line, prefix):
    """The four alternatives after `prefix` of `line`, a deterministic function computed in float64: distinct ids, probabilities
    descending. eos becomes likelier with length; some lines offer few first tokens, one cycles, one may open with the no-output id."""
    rng = np.random.default_rng([7, line, len(prefix)] + [int(t) for t in prefix[-6:]])
    p = np.sort(rng.dirichlet([1.2, 1.0, 0.8, 0.6, 2.0]).astype(np.float64)[:A])[::-1]
    ids = (100 + rng.choice(30, size=A, replace=False)).astype(np.int64)
    if line % 10 == 6:                                  # a 3-cycle far ahead of the rest: the repeat rule fires on the best beam
        ids[0], p[0] = 200 + len(prefix) % 3, 0.9
        p[1:] *= 0.1 / 3
    elif rng.random() < 0.08 + 0.04 * len(prefix):
        ids[int(rng.integers(0, A))] = EOS
    if len(prefix) and rng.random() < 0.03:
        ids[int(rng.integers(0, A))] = PAD
    if not prefix and line % 4 == 1:
        ids[1] = NOP
    if not prefix and line % 5 == 0:
        ids[1 + line % 2:], p[1 + line % 2:] = -1, 0.0   # one or two first tokens only: fewer candidates than beams
    return ids, p


def pure_beam_search(line, B, max_tokens):
    """Textbook beam search over alts_of with the engine's score arithmetic -> [(tokens, probs, log_prob, finished)] in the final order."""
    beams = [((), (), np.float32(0), False)]
    n = 0
    while True:
        cands = []
        for toks, pr, sc, fin in beams:
            if fin:
                cands.append((sc, toks, pr, True))
                continue
            ids, p = alts_of(line, toks)
            for t, q in zip(ids.tolist(), p.astype(np.float32).tolist()):
                if t >= 0 and q > 0:
                    done = t in (EOS, PAD) or (n == 0 and t == NOP)
                    cands.append((np.float32(sc + br.log_prob(q)), toks + (t,), pr + (np.float32(q),), done))
        scores = [float(c[0]) for c in cands]
        assert len(set(scores)) == len(scores), "alts_of is built so that no two candidates tie"
        cands.sort(key=lambda c: -float(c[0]))
        beams = [(c[1], c[2], c[0], c[3]) for c in cands[:B]]
        n += 1
        live = [b for b in beams if not b[3]]
        if not live or n >= max_tokens or detect_repeat_token(list(live[0][0])):
            break
    fin = [b for b in beams if b[3]]
    return [(list(b[0]), list(b[1]), float(b[2]), b[3]) for b in fin + live]


class FakeBeamModel:
    """The HipRecModel surface a beam run uses, with the contracts of include/surya_amd.h enforced: lead slots only in prefill, whole
    ascending groups in set_active, beam outputs only while the mode is on. Per slot it tracks the beam's prefix, score and finished flag
    the way the device does (selection: beam_ref.select_group) and reports, per step and slot, the box of the prefix BEFORE the selection."""

    def __init__(self, max_slots):
        self.max_slots = max_slots
        self.c = SimpleNamespace(max_prefill_tokens=10 ** 6, max_slots=max_slots)
        self.cfg = SimpleNamespace(encoder=SimpleNamespace(spatial_merge_size=2))
        self.beam, self.switches = 0, []
        self.line, self.prefix, self.score, self.fin = {}, {}, {}, {}
        self.active, self.inflight, self.ahead = [], deque(), deque()
        self.prefill_out = None
        self.masks = {}

    def set_beam(self, width, nop=-1):
        self.beam = int(width or 0)
        if self.beam:                                   # (the switch-off of a loop that died may find a call in flight)
            assert nop == NOP and not self.inflight, "switched on while decode calls are in flight"
        self.switches.append(self.beam)

    def encode_ahead(self, tiles, grid_hw):
        assert not self.ahead
        self.ahead.extend(int(tiles[off, 0]) for off in np.cumsum([0] + [h * w for h, w in grid_hw])[:-1])

    def discard_ahead(self):
        self.ahead.clear()

    def _blank(self, n):
        S = self.max_slots
        return [np.full((n, S), -7, np.int32), np.full((n, S), -7, np.int32), np.zeros((n, S), np.int32), np.zeros((n, S), np.float32),
                np.zeros((n, S), np.float32), np.full((n, S, 6), -5, np.int32)]

    def _select(self, out, k, lead, first):
        B = self.beam
        sl = list(range(lead, lead + B))
        ids, ps = np.full((B, A), -1, np.int64), np.zeros((B, A), np.float32)
        for b, s in enumerate(sl):
            if (first and b == 0) or (not first and not self.fin[s]):
                pre = self.prefix[s]
                i, p = alts_of(self.line[lead], pre)
                ids[b], ps[b] = i, p.astype(np.float32)
                out[5][k, s] = (self.line[lead], len(pre), pre[-1] if pre else -1, 0, 0, 0)
        r = br.select_group(B, lead, [self.score[s] for s in sl], [self.fin[s] for s in sl], ids, ps, EOS, PAD, NOP, first)
        old = {s: self.prefix[s] for s in sl}
        for b, s in enumerate(sl):
            par = r["parent"][b]
            frozen = par >= 0 and r["prob"][b] == 0
            self.prefix[s] = () if par < 0 else old[lead + par] + (() if frozen else (r["token"][b],))
            self.score[s], self.fin[s] = r["logp"][b], bool(r["finished"][b])
            for j, key in enumerate(("token", "parent", "rank", "prob", "logp")):
                out[j][k, s] = r[key][b]

    def prefill(self, tiles, grid_hw, input_ids, slot_ids):
        assert self.beam and not self.inflight and len(grid_hw) == len(input_ids) == len(slot_ids) > 0
        lines = [ids[0] - 1000 for ids in input_ids]
        if tiles is None:
            for ln in lines:
                assert self.ahead.popleft() == ln
        out = self._blank(1)
        for ln, s in zip(lines, slot_ids):
            assert s % self.beam == 0 and s + self.beam <= self.max_slots and s not in self.active, "SA_ERR_ARG: a lead slot of a free group"
            for b in range(self.beam):
                self.line[s + b], self.prefix[s + b], self.score[s + b], self.fin[s + b] = ln, (), br.NEG, True
            self._select(out, 0, s, True)
        self.prefill_out = out

    def read_outputs(self, n):
        assert n == 1 and self.prefill_out is not None
        return np.full((1, self.max_slots), -9, np.int32), np.zeros((1, self.max_slots), np.float32), self.prefill_out[5]

    def read_beam(self, n):
        assert self.beam and n == 1
        out, self.prefill_out = self.prefill_out, None
        return tuple(out[:5])

    def set_active(self, slots):
        B = self.beam
        assert len(slots) % B == 0 and list(slots) == sorted(slots), "SA_ERR_ARG: whole groups, ascending"
        for g in range(0, len(slots), B):
            assert slots[g] % B == 0 and list(slots[g:g + B]) == list(range(slots[g], slots[g] + B)), "SA_ERR_ARG: a partial group"
            assert slots[g] in self.line
        self.active = list(slots)

    def decode_async(self, n, ring):
        assert self.beam and 1 <= n <= 8 and len(self.inflight) < 2 and self.active
        out = self._blank(n)
        for k in range(n):
            for lead in self.active[::self.beam]:
                self._select(out, k, lead, False)
        self.inflight.append((n, ring, out))

    def wait_outputs(self, n, ring):
        assert self.inflight[0][:2] == (n, ring)
        out = self.inflight[0][2]
        return np.full((n, self.max_slots), -9, np.int32), np.zeros((n, self.max_slots), np.float32), out[5]

    def wait_beam(self, n, ring):
        assert self.beam
        m, r, out = self.inflight.popleft()
        assert (m, r) == (n, ring)
        return tuple(out[:5])


def _run_beam(n_lines, max_tokens, slots, B, sps, ahead=True):
    old = settings.RECOGNITION_STEPS_PER_SYNC, settings.RECOGNITION_ENCODE_AHEAD
    settings.RECOGNITION_STEPS_PER_SYNC, settings.RECOGNITION_ENCODE_AHEAD = sps, ahead
    try:
        _, prep = make(n_lines, max_tokens, slots)
        model = FakeBeamModel(slots)
        done, calls = {}, []
        loop = DeviceLoop(model, EOS, PAD, NOP, slots, max_tokens, 0.2, beam=B,
                          on_done=lambda k, hyps: (calls.append(k), done.__setitem__(k, hyps)))
        loop.run(prep)
    finally:
        settings.RECOGNITION_STEPS_PER_SYNC, settings.RECOGNITION_ENCODE_AHEAD = old
    return model, prep, done, calls


@pytest.mark.parametrize("n_lines,max_tokens,slots,B,sps,ahead", [(23, 12, 8, 2, 4, True), (17, 9, 7, 3, 1, True), (30, 16, 16, 4, 8, False),
                                                                   (11, 1, 6, 3, 4, True), (8, 64, 8, 4, 3, True), (9, 12, 3, 3, 2, False)])
def test_device_loop_equals_a_pure_python_beam_search(n_lines, max_tokens, slots, B, sps, ahead):
    model, prep, done, calls = _run_beam(n_lines, max_tokens, slots, B, sps, ahead)
    assert sorted(calls) == list(range(n_lines)), "on_done once per line"
    assert model.switches == [B, 0] and not model.inflight
    for k in range(n_lines):
        budget = prep["max_tokens"][k]
        want = pure_beam_search(k, B, budget)
        got = done[k]
        assert all(isinstance(h, BeamHypothesis) for h in got) and len(got) == len(want) <= B, (k, got, want)
        for h, (toks, probs, lp, fin) in zip(got, want):
            assert h.tokens == toks and h.finished == fin, (k, h, toks)
            assert np.float32(h.log_prob) == np.float32(lp) and np.asarray(h.scores, np.float32).tolist() == probs
            assert 1 <= len(toks) <= budget
            # the box of token t is the one predicted from the prefix before it: the parent's slot, also after a fork
            want_box = [[k, t, toks[t - 1] if t else -1, 0, 0, 0] for t in range(len(toks))]
            assert h.bboxes.astype(np.int64).tolist() == want_box
        lps = [h.log_prob for h in got if h.finished], [h.log_prob for h in got if not h.finished]
        assert all(x == sorted(x, reverse=True) for x in lps) and [h.finished for h in got] == sorted((h.finished for h in got), reverse=True)


def test_the_repeat_rule_ends_a_cycling_line_on_its_best_live_beam():
    _, prep, done, _ = _run_beam(8, 64, 8, 4, 3)
    best = [h for h in done[6] if not h.finished][0]     # (finished readings come first in the result)
    assert 40 <= len(best.tokens) < 64 and detect_repeat_token(best.tokens)


def test_loop_switches_beam_mode_off_after_an_exception():
    _, prep = make(9, 12, 8)
    model = FakeBeamModel(8)

    def boom(*a):
        raise RuntimeError("consumer failed")

    with pytest.raises(RuntimeError, match="consumer failed"):
        DeviceLoop(model, EOS, PAD, NOP, 8, 12, 0.2, beam=2, on_done=boom).run(prep)
    assert model.switches == [2, 0] and model.beam == 0


def test_loop_without_beam_never_touches_the_entry_points():
    """The plain FakeModel has none of set_beam / read_beam / wait_beam; on_done keeps its four arguments."""
    _, prep = make(9, 12, 4)
    seen = []
    DeviceLoop(FakeModel(4), EOS, PAD, NOP, 4, 12, 0.2, on_done=lambda *a: seen.append(len(a))).run(prep)
    assert seen == [4] * 9


# ------------------------------------------------------------------------------------------------- (3) predictor, assembly, schema, bindings
class _UntouchedModel:
    """A model a refused call must not reach: only the two mode flags the check reads may be asked for."""

    def __init__(self, **flags):
        self.__dict__.update(flags)

    def __getattr__(self, name):
        if name in ("decode_fp8", "kv_fp8"):
            return False
        raise AssertionError(f"the model was touched ({name}) by a call that must be refused before any device work")


def _pred(**flags):
    from surya_amd.recognition.predictor import RecognitionPredictor
    pred = object.__new__(RecognitionPredictor)
    pred.model = _UntouchedModel(**flags)
    pred.processor = None
    return pred


def test_predictor_refuses_a_bad_beam_width_before_any_model_call():
    from PIL import Image
    img, box = [Image.new("RGB", (64, 16))], [[[0, 0, 64, 16]]]
    for bad in (1, 5, 0, True, 2.0, "3"):
        p = _pred()
        p.beam_width = bad
        with pytest.raises(ValueError, match="beam_width must be None or an integer in 2..4"):
            p(img, bboxes=box)
    p = _pred()
    p.beam_width, p.top_k = 3, 2
    with pytest.raises(ValueError, match="beam_width and top_k exclude each other"):
        p(img, bboxes=box)
    for attr, val in (("shard_lines", True), ("shard_pages", True), ("process_group", object())):
        p = _pred()
        p.beam_width = 2
        setattr(p, attr, val)
        with pytest.raises(NotImplementedError, match="one rank"):
            p(img, bboxes=box)
    for flag, word in (("decode_fp8", "MXFP8"), ("kv_fp8", "fp8 KV cache")):
        p = _pred(**{flag: True})
        p.beam_width = 4
        with pytest.raises(ValueError, match=word):
            p(img, bboxes=box)
    from surya_amd.recognition.predictor import RecognitionPredictor
    assert RecognitionPredictor.beam_width is None and RecognitionPredictor._beam is None
    import inspect
    assert list(inspect.signature(RecognitionPredictor.__call__).parameters)[-2:] == ["allowlist", "blocklist"]      # the signature stays


def test_a_beam_call_takes_the_serial_detect_then_recognise_path():
    from surya_amd.detection.predictor import DetectionPredictor
    p = _pred()
    det = object.__new__(DetectionPredictor)
    p._beam = 3
    assert p._can_stream(det) is False


def test_generate_asks_the_loop_for_beams_only_in_a_beam_call(monkeypatch):
    from surya_amd.recognition import predictor as P
    seen = []

    class Loop:
        def __init__(self, *a, **kw):
            seen.append(kw)
            self.tok_mat = self.sc_mat = self.greedy_tok_mat = self.greedy_p_mat = self.logp_mat = np.zeros((0, 1))
            self.line_len = np.zeros(0, np.int64)
            self.predicted_tokens, self.scores, self.batch_bboxes = [], [], np.zeros((0, 1, 6), np.float32)

        def run(self, prep):
            pass

    monkeypatch.setattr(P, "DeviceLoop", Loop)
    p = object.__new__(P.RecognitionPredictor)
    p.model = SimpleNamespace(max_slots=8)
    p.processor = SimpleNamespace(eos_token_id=EOS, pad_token_id=PAD, no_output_token=NOP)
    prep = {"max_tokens": {0: 5}}
    p.generate(prep, 8)
    p._beam = 3
    p.generate(prep, 8)
    p.generate({**prep, "forced_ids": [[1]]}, 8)                    # an aligned call inside: forcing wins (align sets _beam None anyway)
    assert ["beam" in kw for kw in seen] == [False, True, False] and seen[1]["beam"] == 3


def test_assembly_makes_every_hypothesis_a_line_and_the_line_hypothesis_0():
    from surya_amd.recognition import assemble
    from surya_amd.recognition.processor import SuryaOCRProcessor
    from surya_amd.recognition.schema import LineHypothesis
    from surya_amd.recognition.tokenizer import ByteMathTokenizer, OCRTokenizer
    proc = SuryaOCRProcessor(OCRTokenizer(None, ByteMathTokenizer(256), reserve_special=64))
    tk = proc.ocr_tokenizer

    def hyp(text, lp, fin):
        ids = tk(text, "ocr_with_boxes")["input_ids"][0] + ([proc.eos_token_id] if fin else [])
        T = len(ids)
        rows = (np.arange(T)[:, None] * 10 + np.arange(6)[None, :]).astype(np.float32)
        return BeamHypothesis(ids, [0.5] * T, rows, lp, fin)

    flat = {"polygons": [[5, 5, 600, 60]] * 2, "res_scales": [(1.0, 1.0)] * 2, "slices": [np.zeros((40, 300, 3), np.uint8)] * 2}
    items = [(0, 0, [hyp("rn", -1.0, True), hyp("m", -1.5, True), hyp("rnx", -0.5, False)]), (1, 1, [hyp("10", -2.0, True)])]
    lines = assemble.assemble_beam_batch(proc, flat, items, False, False, 1000)
    assert [ln.text for ln in lines] == ["rn", "10"] and lines[0].log_prob == -1.0 and lines[1].log_prob == -2.0
    h = lines[0].hypotheses
    assert all(isinstance(x, LineHypothesis) for x in h) and [x.text for x in h] == ["rn", "m", "rnx"]
    assert [x.finished for x in h] == [True, True, False] and [x.log_prob for x in h] == [-1.0, -1.5, -0.5]
    assert h[0].text == lines[0].text and h[0].confidence == lines[0].confidence and [c.text for c in h[1].chars] == ["m"]
    d = lines[0].model_dump()
    assert d["log_prob"] == -1.0 and [x["text"] for x in d["hypotheses"]] == ["rn", "m", "rnx"]
    assert set(d["hypotheses"][0]) == {"text", "confidence", "log_prob", "finished", "chars", "words"}
    # a line without any candidate: the empty line, an empty list
    empty = assemble.assemble_beam_batch(proc, flat, [(0, 0, [])], False, False, 1000)[0]
    assert empty.text == "" and empty.hypotheses == [] and empty.log_prob is None


def test_hypotheses_are_absent_from_the_serialised_form_while_none():
    from surya_amd.recognition.schema import LineHypothesis, TextChar, TextLine
    poly = [[0, 0], [8, 0], [8, 10], [0, 10]]
    c = TextChar(text="a", polygon=poly, confidence=0.5)
    ln = TextLine(text="a", polygon=poly, confidence=0.5, chars=[c])
    assert ln.hypotheses is None and "hypotheses" not in ln.model_dump() and "hypotheses" not in ln.model_dump_json()
    assert "hypotheses" not in ln.model_fields_set and "log_prob" not in ln.model_dump()
    hy = LineHypothesis(text="a", confidence=0.5, log_prob=-0.25, finished=True, chars=[c])
    l2 = TextLine(text="a", polygon=poly, confidence=0.5, chars=[c], log_prob=-0.25, hypotheses=[hy])
    d = l2.model_dump()
    assert d["hypotheses"][0]["log_prob"] == -0.25 and d["hypotheses"][0]["finished"] is True and d["hypotheses"][0]["chars"][0]["text"] == "a"
    assert TextLine.model_validate_json(l2.model_dump_json()) == l2
    assert "hypotheses" in TextLine.model_json_schema()["properties"]


def test_bindings_and_header_agree():
    import os
    from surya_amd import _lib as L
    hdr = open(os.path.join(br.ROOT, "include", "surya_amd.h")).read()
    assert int(re.search(r"#define SA_MAX_BEAMS (\d+)", hdr).group(1)) == L.SA_MAX_BEAMS == 4
    core = open(os.path.join(br.ROOT, "surya_amd", "csrc", "beam_core.h")).read()
    assert int(re.search(r"#define SA_BEAM_MAX (\d+)", core).group(1)) == L.SA_MAX_BEAMS
    assert int(re.search(r"#define SA_BEAM_ALTS (\d+)", core).group(1)) == L.SA_MAX_ALTERNATIVES
    want = {"surya_rec_set_beam": 3, "surya_rec_read_beam": 8, "surya_rec_wait_beam": 8, "surya_op_rec_beam_select": 26, "surya_op_rec_kv_fork": 13}
    for name, n in want.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == n, name                 # the declaration's argument count ...
    if os.path.exists(L.LIB_PATH):
        lib = L.lib()
        for name, n in want.items():
            assert len(getattr(lib, name).argtypes) == n, name       # ... is the binding's
