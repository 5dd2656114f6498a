"""CPU: the host side of RecognitionPredictor.top_k: the device loop's bookkeeping of the alternatives (against the fake model of
test_scheduler_cpu.py, extended here with the three entry points), the token -> character mapping of the assembly, the line gather
(PackedLines, shard_lines, gloo world 2), the schema and the argument check."""
import multiprocessing as mp
import os
import socket
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from surya_amd import dist as sd
from surya_amd.recognition import assemble
from surya_amd.recognition.loop import DeviceLoop
from surya_amd.recognition.processor import SuryaOCRProcessor
from surya_amd.recognition.schema import CharAlternative, TextChar
from surya_amd.recognition.tokenizer import ByteMathTokenizer, OCRTokenizer
from surya_amd.settings import settings
from test_scheduler_cpu import EOS, NOP, PAD, FakeModel, expected, make, script

A = 4


def alt_of(line, pos):
    """The scripted alternatives of token `pos` of `line`: entry 0 is the token itself, entry 3 is missing on odd lines."""
    t = script(line, pos)
    ids = [t, 100000 + line, 200000 + pos, -1 if line % 2 else 300000 + line + pos]
    p = [0.5, 0.25, 0.125, 0.0 if line % 2 else 0.0625]
    return ids, p


class FakeAltModel(FakeModel):
    """FakeModel + set_alternatives / read_alternatives / wait_alternatives, laid out like the outputs they run beside."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.alternatives, self.switches = False, []
        self.prefill_alt, self.alt_inflight = None, {}

    def set_alternatives(self, on):
        assert not self.inflight, "switched while decode calls are in flight"
        self.alternatives = bool(on)
        self.switches.append(bool(on))

    def prefill(self, tiles, grid_hw, input_ids, slot_ids):
        super().prefill(tiles, grid_hw, input_ids, slot_ids)
        at, ap = np.full((1, self.max_slots, A), -9, np.int32), np.zeros((1, self.max_slots, A), np.float32)
        for ids, s in zip(input_ids, slot_ids):
            at[0, s], ap[0, s] = alt_of(ids[0] - 1000, 0)
        self.prefill_alt = (at, ap)

    def read_alternatives(self, n):
        assert self.alternatives and n == 1 and self.prefill_alt is not None
        out, self.prefill_alt = self.prefill_alt, None
        return out

    def decode_async(self, n, ring):
        pos0 = {s: self.slot_pos[s] for s in self.active}
        super().decode_async(n, ring)
        at, ap = np.full((n, self.max_slots, A), -9, np.int32), np.zeros((n, self.max_slots, A), np.float32)
        for k in range(n):
            for s in self.active:
                at[k, s], ap[k, s] = alt_of(self.slot_line[s], pos0[s] + k)
        self.alt_inflight[ring] = (n, at, ap)

    def wait_alternatives(self, n, ring):
        assert self.alternatives
        m, at, ap = self.alt_inflight.pop(ring)
        assert m == n
        return at, ap


def _loop(model, prep, slots, max_tokens, **kw):
    return DeviceLoop(model, EOS, PAD, NOP, slots, max_tokens, 0.2, **kw)


@pytest.mark.parametrize("n_lines,max_tokens,slots,sps", [(23, 12, 4, 4), (40, 6, 7, 1), (9, 40, 16, 8)])
def test_loop_hands_aligned_alternatives_to_on_done(n_lines, max_tokens, slots, sps):
    """More lines than slots (slot reuse): every line's arrays are its own tokens' alternatives, position by position."""
    old = settings.RECOGNITION_STEPS_PER_SYNC
    settings.RECOGNITION_STEPS_PER_SYNC = sps
    try:
        _, prep = make(n_lines, max_tokens, slots)
        model = FakeAltModel(slots)
        done = {}
        loop = _loop(model, prep, slots, max_tokens, alternatives=True,
                     on_done=lambda k, toks, sc, bb, at, ap: done.__setitem__(k, (list(toks), at, ap)))
        loop.run(prep)
    finally:
        settings.RECOGNITION_STEPS_PER_SYNC = old
    assert model.switches == [True, False] and not model.alternatives
    assert sorted(done) == list(range(n_lines))
    for k, (toks, at, ap) in done.items():
        assert toks == expected(k, prep["max_tokens"][k])
        assert at.shape == (len(toks), A) and ap.shape == (len(toks), A) and at.dtype == np.int32 and ap.dtype == np.float32
        for pos in range(len(toks)):
            ids, p = alt_of(k, pos)
            assert at[pos].tolist() == ids and ap[pos].tolist() == p, (k, pos)
        assert at[:, 0].tolist() == toks                                    # entry 0 is the emitted token
    assert loop.alt_tok_mat.shape == (n_lines, loop.cap, A)
    assert (loop.alt_tok_mat[np.arange(loop.cap)[None, :] >= loop.line_len[:, None]] == -1).all()     # past a line's end: no entry


def test_loop_switches_off_after_an_exception():
    _, prep = make(9, 12, 4)
    model = FakeAltModel(4)
    calls = []

    def boom(*a):
        calls.append(a)
        raise RuntimeError("consumer failed")

    with pytest.raises(RuntimeError, match="consumer failed"):
        _loop(model, prep, 4, 12, alternatives=True, on_done=boom).run(prep)
    assert calls and model.switches == [True, False]


def test_loop_without_the_request_never_touches_the_entry_points():
    """The plain FakeModel has none of the three methods; on_done keeps its four arguments; no arrays are kept."""
    _, prep = make(9, 12, 4)
    model = FakeModel(4)
    seen = []
    loop = _loop(model, prep, 4, 12, on_done=lambda *a: seen.append(len(a)))
    loop.run(prep)
    assert seen == [4] * 9 and loop.alt_tok_mat is None and loop.alt_p_mat is None
    model = FakeAltModel(4)
    _loop(model, prep, 4, 12).run(prep)
    assert model.switches == []


# ------------------------------------------------------------------------------------------------- assembly
@pytest.fixture(scope="module")
def proc():
    return SuryaOCRProcessor(OCRTokenizer(None, ByteMathTokenizer(256), reserve_special=64))


def _units(tok, text):
    raw = text.encode("utf-16le")
    return [raw[i] + (raw[i + 1] << 8) + tok.special_token_offset for i in range(0, len(raw), 2)]


def _alts_for(tokens, rng):
    """Random alternatives whose entry 0 is the token; some entries missing."""
    T = len(tokens)
    at = rng.integers(0, 60000, size=(T, A)).astype(np.int32)
    at[:, 0] = tokens
    ap = np.sort(rng.random((T, A)).astype(np.float32), axis=1)[:, ::-1].copy()
    at[::3, 3] = -1
    ap[::3, 3] = 0
    return at, ap


def test_alt_decoder(proc):
    tk = proc.ocr_tokenizer
    dec = assemble.AltDecoder(proc)
    assert dec(_units(tk, "A")[0]) == "A" and dec(_units(tk, "漢")[0]) == "漢"
    hi, lo = _units(tk, "😀")
    assert dec(hi) == "" and dec(lo) == ""                                 # a lone surrogate has no text of its own
    sp = next(v for k, v in tk.SPECIAL_TOKEN_MAPPING.items() if k not in tk.system_tokens)
    from surya_amd.recognition.schema import TaskNames
    assert dec(sp) == tk.decode([sp], task=TaskNames.ocr_without_boxes) and dec(sp)
    assert dec(65) == tk.decode([65], task=TaskNames.block_without_boxes)
    assert dec(65) is dec(65)                                              # cached
    assert dec(proc.eos_token_id) == dec(proc.pad_token_id) == dec(proc.no_output_token) == ""


def test_line_runs_mapping(proc):
    """Every character takes the alternatives of the token it takes its confidence from (csrc of line_runs): surrogate pairs, a math
    run, a special tag, a character that repeats its run's last box."""
    tk = proc.ocr_tokenizer
    sp = next(v for k, v in tk.SPECIAL_TOKEN_MAPPING.items() if k not in tk.system_tokens)
    tokens = _units(tk, "a😀b") + [sp] + [40, 41, 42] + _units(tk, "xyz")
    T = len(tokens)
    rows = (np.arange(T)[:, None] * 10 + np.arange(6)[None, :]).astype(np.float32)
    rows[-1] = rows[-2]                                                    # 'z' repeats the box of 'y'
    rng = np.random.default_rng(5)
    at, ap = _alts_for(tokens, rng)
    flat = {"polygons": [[5, 5, 600, 60]], "res_scales": [(1.0, 1.0)], "slices": [np.zeros((40, 300, 3), np.uint8)], "top_k": 3}
    sc = rng.random(T).astype(np.float32).tolist()
    line = assemble.assemble_line(proc, flat, 0, 0, tokens, sc, rows, False, False, 1025, alts=(at, ap))
    P = np.asarray(assemble.prediction_to_polygon_batch(rows[None], [(40, 300, 3)], 1025, 512), np.float64)[0]
    far = (np.abs(P[1:] - P[:-1]).reshape(T - 1, 8).max(axis=1) > 0.1).tolist()
    texts, src, csrc, valid = assemble.line_runs(proc, tokens, far)
    own, added = line.chars[:len(texts)], line.chars[len(texts):]         # (the lone opening tag gets its closing tag appended)
    assert [c.text for c in own] == texts and len(texts) == len(csrc)
    assert all(c.alternatives is None and c.text.startswith("</") for c in added)       # inserted characters keep None
    assert csrc[:3] == [0, 1, 2] and texts[1] == "😀"                       # the pair's character reads token 1, a lone surrogate
    dec = assemble.AltDecoder(proc)
    for ch, j in zip(own, csrc):
        want = [(dec(int(t)), float(p), int(t)) for t, p in zip(at[j][:3], ap[j][:3]) if t >= 0]
        assert [(a.text, a.confidence, a.token_id) for a in ch.alternatives] == want
        assert len(ch.alternatives) == 3 and ch.alternatives[0].token_id == tokens[j]
        assert ch.confidence == pytest.approx(sc[j])
    assert line.chars[1].alternatives[0].text == ""                        # token 1 is the high surrogate
    i_sp = texts.index(tk.decode([sp], task="ocr_without_boxes"))
    assert line.chars[i_sp].alternatives[0].text == texts[i_sp] and not valid[i_sp]
    assert csrc[-1] == csrc[-2] or src[-1] == src[-2]                      # the repeated box
    d = line.model_dump()
    assert d["chars"][0]["alternatives"][0] == {"text": "a", "confidence": float(ap[0, 0]), "token_id": tokens[0]}


@pytest.mark.parametrize("top_k", [2, 4])
def test_assemble_line_equals_assemble_batch(proc, top_k):
    tk = proc.ocr_tokenizer
    rng = np.random.default_rng(top_k)
    specials = [v for k, v in tk.SPECIAL_TOKEN_MAPPING.items() if k not in tk.system_tokens]
    flat = {"polygons": [], "res_scales": [], "slices": [], "top_k": top_k}
    items = []
    for li in range(24):
        toks = []
        for _ in range(int(rng.integers(1, 9))):
            r = rng.random()
            if r < 0.6:
                toks += _units(tk, "".join(rng.choice(list("ab Ä漢😀"), size=int(rng.integers(1, 5)))))
            elif r < 0.8:
                toks.append(int(rng.choice(specials)))                       # unbalanced tags: fix_unbalanced_tags inserts characters
            else:
                toks += [int(x) for x in rng.integers(32, 127, size=int(rng.integers(1, 4)))]
        if li % 7 == 3:
            toks.append(proc.eos_token_id)
            toks += _units(tk, "zz")
        if li % 11 == 5:
            toks[0] = proc.no_output_token
        T = len(toks)
        rows = np.sort(rng.integers(0, 1025, size=(T, 6)), axis=0).astype(np.float32)
        flat["polygons"].append([7, 9, 300, 52])
        flat["res_scales"].append((1.0, 1.0))
        flat["slices"].append(np.zeros((30, 200, 3), np.uint8))
        items.append((li, li, toks, rng.random(T).astype(np.float32).tolist(), rows, _alts_for(toks, rng)))
    got = assemble.assemble_batch(proc, flat, items, False, False, 1025)
    some = inserted = 0
    for it, g in zip(items, got):
        ref = assemble.assemble_line(proc, flat, *it[:5], False, False, 1025, alts=it[5])
        assert g.model_dump() == ref.model_dump(), it[0]
        for c in g.chars:
            if c.alternatives is None:
                inserted += 1                                                # only characters the tag fixer inserted
                assert c.text.startswith("</") and c.confidence == 0
            else:
                some += 1
                assert 1 <= len(c.alternatives) <= top_k and all(a.token_id >= 0 for a in c.alternatives)
    assert some > 50 and inserted > 0
    # without alternatives the same items give today's objects: no `alternatives` key in the serialised form
    flat.pop("top_k")
    plain = assemble.assemble_batch(proc, flat, [it[:5] for it in items], False, False, 1025)
    for g, p in zip(got, plain):
        assert all(c.alternatives is None for c in p.chars)
        assert all("alternatives" not in c for c in p.model_dump()["chars"])
        gd = g.model_dump()
        for c in gd["chars"]:
            c.pop("alternatives", None)
        assert gd == p.model_dump()


def test_schema_defaults():
    c = TextChar(text="a", polygon=[0, 0, 1, 1], confidence=0.5)
    assert c.alternatives is None and "alternatives" not in c.model_dump() and "alternatives" not in c.model_fields_set
    c2 = TextChar(text="a", polygon=[0, 0, 1, 1], confidence=0.5, alternatives=[CharAlternative(text="a", confidence=0.5, token_id=7)])
    assert c2.model_dump()["alternatives"] == [{"text": "a", "confidence": 0.5, "token_id": 7}]
    assert TextChar(**c2.model_dump()) == c2
    fast = assemble._text_char(c.polygon, 0.5, "a", True)
    assert fast == c and fast.model_dump() == c.model_dump()


@pytest.mark.parametrize("bad", [0, 1, 5, -1, 2.0, "3", True])
def test_top_k_is_validated(bad):
    from surya_amd.recognition.predictor import RecognitionPredictor
    pred = object.__new__(RecognitionPredictor)
    pred.top_k = bad
    with pytest.raises(ValueError, match="top_k"):
        pred([])
    assert pred._top_k is None and RecognitionPredictor.top_k is None        # off by default


# ------------------------------------------------------------------------------------------------- gather
def test_packed_lines_round_trip_with_alternatives():
    rng = np.random.default_rng(0)
    n, T = 7, 12
    lens = rng.integers(1, T + 1, size=n)
    at = rng.integers(0, 70000, size=(n, T + 1, A)).astype(np.int32)
    ap = rng.random((n, T + 1, A)).astype(np.float32)
    toks = [rng.integers(0, 70000, size=L).tolist() for L in lens]
    scs = [rng.random(L).astype(np.float32).tolist() for L in lens]
    bbs = rng.integers(0, 1025, size=(n, T, 6)).astype(np.float32)
    out = sd.gather_line_outputs(toks, scs, bbs, list(range(n)), n, T, alts=(sd.PackedLines(at, lens), sd.PackedLines(ap, lens)))
    assert len(out) == 5
    plain = sd.gather_line_outputs(toks, scs, bbs, list(range(n)), n, T)
    assert len(plain) == 3 and out[0] == plain[0] and out[1] == plain[1] and np.array_equal(out[2], plain[2])
    for i in range(n):
        assert np.array_equal(out[3].row(i), at[i, :lens[i]]) and np.array_equal(out[4].row(i), ap[i, :lens[i]])
        assert (out[3].data[i, lens[i]:] == -1).all() and (out[4].data[i, lens[i]:] == 0).all()
        assert out[3][i] == at[i, :lens[i]].tolist()


def _shard_worker(rank, world, port, n_lines, max_tokens, slots, q):
    import sys
    import torch.distributed as dist
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import test_scheduler_cpu as ts
    import test_topk_cpu as me
    from surya_amd.recognition.predictor import RecognitionPrompt
    if world > 1:
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
    settings.RECOGNITION_MAX_TOKENS = max_tokens
    pred, _ = ts.make(1, max_tokens, slots)
    pred.model = me.FakeAltModel(slots)
    pred.model.device = torch.device("cpu")
    pred.process_group = None

    def prepare_lines(flat, math_mode=True):
        ids = [int(s[0, 0, 0]) for s in flat["slices"]]
        grids = [(2, 2 + 2 * (i % 3)) for i in ids]
        offs = np.cumsum([0] + [h * w for h, w in grids])
        tiles = np.zeros((offs[-1], 3), np.float32)
        for k, i in enumerate(ids):
            tiles[offs[k]:offs[k + 1], 0] = i
        return {"prompts": [RecognitionPrompt(k, "ocr_with_boxes", None, None, True) for k in range(len(ids))],
                "max_tokens": {k: max_tokens for k in range(len(ids))}, "tiles": tiles, "tile_offs": offs, "grids": grids,
                "prompt_ids": [[1000 + i, 5, 6] for i in ids]}

    pred.prepare_lines = prepare_lines
    flat = {"slices": [np.full((8, 40 + (i * 7) % 23, 3), i, np.float32) for i in range(n_lines)], "input_text": [None] * n_lines,
            "task_names": ["ocr_with_boxes"] * n_lines}
    pred._top_k = 3
    toks, boxes, scores = pred.sharded_prediction_loop(flat, slots, True)
    la = pred.last_alternatives
    q.put((rank, list(toks), [la[0].row(i).copy() for i in range(n_lines)], [la[1].row(i).copy() for i in range(n_lines)]))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def test_shard_lines_gathers_the_alternatives_over_two_gloo_ranks():
    n_lines, max_tokens, slots = 11, 12, 3
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_shard_worker, args=(r, 2, port, n_lines, max_tokens, slots, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = [q.get(timeout=180) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, toks, at, ap in results:
        for i in range(n_lines):
            exp = expected(i, max_tokens)
            assert toks[i] == exp
            assert at[i].shape == (len(exp), A)
            for pos in range(len(exp)):
                ids, p = alt_of(i, pos)
                assert at[i][pos].tolist() == ids and ap[i][pos].tolist() == p, (rank, i, pos)
