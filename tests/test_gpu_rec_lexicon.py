"""GPU: lexicon-guided decoding through the recognition engine (surya_rec_set_lexicon / surya_rec_set_slot_lexicon /
surya_rec_copy_lexicon_states) and through RecognitionPredictor.lexicon, on REC-SMALL with synthetic weights.

The engine is checked step by step as tests/test_gpu_rec_allowlist.py checks token masks, with that file's `_check_step` and score
tolerance: at every step a lexicon slot's token is the first argmax of the engine's own unmasked logits (surya_rec_copy_last_logits)
masked by allowed(state before the step) of the HOST replay (LexiconTables), the score is the softmax over that set, and the device's
states equal the replay's. Lines without a lexicon must be bit-identical to the same call without the lexicon lines' constraint."""
import ctypes as C
import functools
import random
import string

import numpy as np
import pytest
import torch
from PIL import Image

from surya_amd import _lib as L
from surya_amd.synth import make_line_crops

from test_gpu_rec_allowlist import (DIGITS, GRIDS, _allowed_rows, _cfg_sd, _check_step, _lines_of, _max_tokens, _model, _predictor, _run,  # noqa: F401
                                    _tokenizer)
from util import make_prompts

pytestmark = pytest.mark.gpu
DATE = r"\d{2}/\d{2}/\d{4}"
_r2, _r1 = random.Random(2), random.Random(1)
CODES = ["%05d" % _r2.randrange(100000) for _ in range(2000)]                      # the list the pattern compiler refuses
WORDS = ["".join(_r1.choice(string.ascii_lowercase) for _ in range(_r1.randint(4, 9))) for _ in range(200)]
SHORT = ["a", "ab", "abc", "b", "7", "77"]                                         # entries that are prefixes of others: terminal inner states
LEXICONS = [CODES, WORDS, SHORT]
SLOTS = [0, 1, 2, 3, 4, 5]
LINE_LEX = [0, 1, 2, 0, 1, None]                                                   # index into LEXICONS per line, None = no lexicon


@functools.lru_cache(maxsize=None)
def _tables(which=(0, 1, 2)):
    from surya_amd.recognition.lexicon import compile_lexicons
    return compile_lexicons(_tokenizer(), [LEXICONS[i] for i in which], _cfg_sd()[0].decoder.vocab_size)


@functools.lru_cache(maxsize=None)
def _mask_table(with_date=False):
    """(the call's mask table as an array -- a lexicon needs one --, digits row id, PatternTables or None)."""
    from surya_amd.recognition.pattern import compile_patterns
    from surya_amd.recognition.tokenizer import MaskTable
    tk, V = _tokenizer(), _cfg_sd()[0].decoder.vocab_size
    tb = MaskTable(tk, V, L.SA_MAX_TOKEN_MASKS)
    dig = tb.id_for(DIGITS, None)
    pt = compile_patterns(tk, [DATE], V, extra_mask_rows=tb) if with_date else None
    return tb.array(), dig, pt


def _arm(m, lt, slots=SLOTS, line_lex=LINE_LEX, mask_ids=None):
    m.set_token_masks(_mask_table()[0])
    m.set_lexicon(lt)
    return _start(m, lt, slots, line_lex, mask_ids)


def _start(m, lt, slots=SLOTS, line_lex=LINE_LEX, mask_ids=None):
    states = [-1 if k is None else lt.starts[k] for k in line_lex]
    m.set_slot_masks(slots, [-1] * len(slots) if mask_ids is None else mask_ids)
    m.set_slot_lexicon(slots, states)
    return states


def _rows(lt, states, mask_ids=None):
    """bool [rows, V] on the GPU: allowed(state) of a lexicon row, the mask row (or everything) of the others."""
    V = _cfg_sd()[0].decoder.vocab_size
    rows = _allowed_rows(_mask_table()[0], [-1 if s >= 0 or mask_ids is None else mask_ids[r] for r, s in enumerate(states)], V).cpu().numpy()
    for r, s in enumerate(states):
        if s >= 0:
            rows[r] = False
            rows[r, sorted(lt.allowed(s))] = True
    return torch.from_numpy(rows).cuda()


def _replay_ok(lt, k, tokens):
    """Host replay of one stream of lexicon k: (every token allowed where it stood, entry index or -1, state at the end)."""
    st = lt.starts[k]
    for t in tokens:
        t = int(t)
        if t not in lt.allowed(st):
            return False, -1, st
        if t in (lt.eos, lt.pad, lt.nop):
            break
        st = lt.advance(st, t)
    return True, lt.entry_of(k, tokens), st


def _stepwise(m, lt, n_steps, what, mask_ids=None):
    """Prefill six lines and decode one step at a time, checking token, score and device state against the host replay every step."""
    cfg = _cfg_sd()[0]
    states = _arm(m, lt, mask_ids=mask_ids)
    tiles, seqs = make_prompts(cfg, GRIDS, seed=9)
    m.prefill(tiles.cuda(), GRIDS, seqs, SLOTS)
    moved = 0
    for step in range(n_steps + 1):
        if step:
            m.decode(1)
        t, s, _ = m.read_outputs(1)
        _check_step(m, cfg, t[0], s[0], SLOTS, _rows(lt, states, mask_ids), f"{what} step {step}")
        new = [lt.advance(st, int(t[0, sl])) for st, sl in zip(states, SLOTS)]
        moved += sum(a != b for a, b in zip(new, states))
        states = new
        assert m.copy_lexicon_states()[SLOTS].tolist() == states, (what, step)
        if step == 0:
            m.set_active(SLOTS)
    assert moved >= n_steps, "the automata hardly moved: the test shows nothing"
    return states


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_every_step_follows_the_host_replay(hip_lib, dtype):
    _stepwise(_model(dtype), _tables(), 6, str(dtype))


def test_lines_end_on_an_entry_or_are_a_proper_prefix(hip_lib):
    """12 steps: a line that ended is exactly one entry of its own lexicon; every other line took only its state's children."""
    lt = _tables()
    m = _model(torch.bfloat16)
    lex = [0, 1, 2, 0, 1, 2]
    _arm(m, lt, line_lex=lex)
    toks = _run(m, SLOTS, 12)[0]
    sto, done = _tokenizer().special_token_offset, 0
    for r, k in enumerate(lex):
        stream = toks[:, r].tolist()
        if stream[0] == lt.nop:
            continue                                                    # a blank crop: the line ends at its first token
        ok, idx, st = _replay_ok(lt, k, stream)
        assert ok, (k, stream)
        if idx >= 0:
            done += 1
            n = next(i for i, t in enumerate(stream) if t in (lt.eos, lt.pad))
            assert "".join(chr(t - sto) for t in stream[:n]) == LEXICONS[k][idx] and lt.accepts(st)
    assert done >= 3, "five-character codes and short entries end within 12 steps"


def test_mixed_batch_leaves_the_other_rows_bit_identical(hip_lib):
    """Lexicon, pattern, allowlist and unconstrained slots together: the rows without a lexicon equal, bit for bit, the same call without the
    lexicon lines' constraint."""
    lt = _tables()
    table, dig, pt = _mask_table(with_date=True)
    m = _model(torch.bfloat16)
    m.set_token_masks(table)
    m.set_patterns(pt)
    mask_ids = [-1, -1, dig, -1, -1, -1]
    pat_states = [-1, pt.starts[0], -1, -1, -1, -1]

    def go(line_lex):
        m.set_slot_masks(SLOTS, mask_ids)
        m.set_slot_patterns(SLOTS, pat_states)
        if line_lex is not None:
            m.set_slot_lexicon(SLOTS, [-1 if k is None else lt.starts[k] for k in line_lex])
        return _run(m, SLOTS, 6)
    without = go(None)
    m.set_lexicon(lt)
    assert m.n_pattern_states > 0                                       # a lexicon may be on together with patterns
    mixed = go([0, None, None, None, 1, None])
    for a, b in zip(without, mixed):
        assert np.array_equal(a[:, [1, 2, 3, 5]].view(np.int32), b[:, [1, 2, 3, 5]].view(np.int32))
    assert _replay_ok(lt, 0, mixed[0][:, 0].tolist())[0] and _replay_ok(lt, 1, mixed[0][:, 4].tolist())[0]
    assert not np.array_equal(without[0][:, [0, 4]], mixed[0][:, [0, 4]]), "the lexicon rows were not constrained at all"
    st = m.copy_lexicon_states()
    assert st[1] == -1 and st[2] == -1 and st[3] == -1 and m.slot_states()[1] >= 0
    m.set_lexicon(None)
    m.set_slot_masks(SLOTS, mask_ids)
    m.set_slot_patterns(SLOTS, pat_states)
    off = _run(m, SLOTS, 6)                                             # and switched off again: the first call, every row
    for a, b in zip(without, off):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_eight_steps_in_one_call_equal_eight_calls(hip_lib):
    lt = _tables()
    m = _model(torch.bfloat16)
    _arm(m, lt)
    one = _run(m, SLOTS, 8, single=True)
    s1 = m.copy_lexicon_states()[SLOTS].tolist()
    _start(m, lt)
    eight = _run(m, SLOTS, 8)
    for a, b in zip(one, eight):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert m.copy_lexicon_states()[SLOTS].tolist() == s1


def test_streams_do_not_depend_on_the_slot_count(hip_lib):
    """The same 8 lines against 8 and against 64 slots: identical streams and states."""
    lt = _tables()
    lex = [i % 3 for i in range(64)]
    m8 = _model(torch.bfloat16, max_slots=8)
    _arm(m8, lt, slots=list(range(8)), line_lex=lex[:8])
    few = _run(m8, list(range(8)), 5)
    s_few = m8.copy_lexicon_states()[:8].tolist()
    m = _model(torch.bfloat16, max_slots=64)
    _arm(m, lt, slots=list(range(8)), line_lex=lex[:8])
    alone = _run(m, list(range(8)), 5)
    _start(m, lt, slots=list(range(64)), line_lex=lex)
    many = _run(m, list(range(64)), 5)
    for a, b, c in zip(few, alone, many):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)) and np.array_equal(a.view(np.int32), c[:, :8].view(np.int32))
    assert m.copy_lexicon_states()[:8].tolist() == s_few
    for r in range(64):
        assert _replay_ok(lt, lex[r], many[0][:, r].tolist())[0], r


def test_a_reused_slot_starts_anew_and_a_plain_mask_id_stops_it(hip_lib):
    lt = _tables()
    dig = _mask_table()[1]
    m = _model(torch.bfloat16)
    _arm(m, lt, slots=[0, 1], line_lex=[0, 1])
    ref = _run(m, [0, 1], 4, lines=[2, 3])
    _start(m, lt, slots=[0, 1], line_lex=[1, 2])                         # other lines, other lexicons: their bits are anywhere in the rows
    _run(m, [0, 1], 3, lines=[0, 1])
    assert (m.copy_lexicon_states()[[0, 1]] >= 0).all()
    _start(m, lt, slots=[0, 1], line_lex=[0, 1])
    again = _run(m, [0, 1], 4, lines=[2, 3])
    for a, b in zip(ref, again):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    # a slot given a plain mask id afterwards stops moving and rewrites no row
    m.set_slot_masks([0], [dig])
    assert m.copy_lexicon_states()[0] == -1
    toks = _run(m, [0, 1], 4, lines=[2, 3])[0]
    assert m.copy_lexicon_states()[0] == -1
    digits = set(np.flatnonzero(_allowed_rows(_mask_table()[0], [dig], _cfg_sd()[0].decoder.vocab_size)[0].cpu().numpy()).tolist())
    assert set(toks[:, 0].tolist()) <= digits


def test_mxfp8_head_with_a_lexicon(hip_lib):
    _stepwise(_model(torch.bfloat16, decode_fp8=True), _tables(), 4, "mxfp8")


def test_every_alternative_is_a_child_of_the_state(hip_lib):
    cfg = _cfg_sd()[0]
    lt = _tables()
    m = _model(torch.bfloat16)
    m.set_alternatives(True)
    states = _arm(m, lt)
    tiles, seqs = make_prompts(cfg, GRIDS, seed=9)
    m.prefill(tiles.cuda(), GRIDS, seqs, SLOTS)
    for step in range(5):
        if step:
            m.decode(1)
        t, _, _ = m.read_outputs(1)
        at, _ = m.read_alternatives(1)
        for r, sl in enumerate(SLOTS):
            assert int(at[0, sl, 0]) == int(t[0, sl])
            if states[r] >= 0:
                assert all(int(a) in lt.allowed(states[r]) for a in at[0, sl] if a >= 0), (step, r)
        states = [lt.advance(st, int(t[0, sl])) for st, sl in zip(states, SLOTS)]
        if step == 0:
            m.set_active(SLOTS)
    m.set_alternatives(False)


def test_captured_steps_follow_new_table_contents(hip_lib):
    """hipGraph replay on: tables of the same capacity live at the same addresses, so steps captured under one automaton obey the next
    one's contents; a larger automaton moves them and is followed just the same."""
    big, small, other = _tables(), _tables((1, 2)), _tables((2, 1))
    assert small.n_states != other.n_states or not np.array_equal(small.edge_tok, other.edge_tok)
    m = _model(torch.bfloat16)
    m.set_token_masks(_mask_table()[0])
    L.check(m.lib.surya_set_tuning(b"graph", C.c_int(1)), "surya_set_tuning(graph)")
    try:
        streams = []
        for tables in (small, small, small, other, big, big, big, small):      # eager, capture, replay, new contents; grown; ...; smaller again
            n = len(tables.starts)
            lex = [i % n for i in range(4)]
            m.set_lexicon(tables)
            _start(m, tables, slots=[0, 1, 2, 3], line_lex=lex)
            toks = _run(m, [0, 1, 2, 3], 4)[0]
            for r in range(4):
                assert _replay_ok(tables, lex[r], toks[:, r].tolist())[0], r
            streams.append(toks)
        assert np.array_equal(streams[0], streams[1]) and np.array_equal(streams[0], streams[2]) and np.array_equal(streams[0], streams[7])
        assert np.array_equal(streams[4], streams[5]) and np.array_equal(streams[4], streams[6])
    finally:
        L.check(m.lib.surya_set_tuning(b"graph", C.c_int(0)), "surya_set_tuning(graph)")


def test_entry_points_refuse_bad_tables_and_modes(hip_lib):
    from types import SimpleNamespace
    lt = _tables()
    V = _cfg_sd()[0].decoder.vocab_size
    m = _model(torch.bfloat16)

    def variant(**kw):
        d = dict(edge_off=lt.edge_off.copy(), edge_tok=lt.edge_tok.copy(), edge_next=lt.edge_next.copy(), state_flags=lt.state_flags.copy(),
                 nop=lt.nop)
        d.update(kw)
        return SimpleNamespace(**d)
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.set_lexicon(lt)                                               # no mask table yet
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.set_slot_lexicon([0], [0])                                    # the lexicon is off
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.copy_lexicon_states()                                         # ... and never was on
    m.set_token_masks(_mask_table()[0])
    root = lt.starts[0]
    a, b = int(lt.edge_off[root]), int(lt.edge_off[root + 1])
    assert b - a >= 2
    i = int(np.flatnonzero(np.diff(lt.edge_off) > 0)[1])
    off = lt.edge_off.copy(); off[i + 1] = off[i] - 1                   # not monotone
    end = lt.edge_off.copy(); end[-1] -= 1                              # does not end at n_edges
    tok_hi = lt.edge_tok.copy(); tok_hi[b - 1] = V                      # outside the vocabulary
    tok_eq = lt.edge_tok.copy(); tok_eq[a + 1] = tok_eq[a]              # not strictly ascending
    nxt = lt.edge_next.copy(); nxt[5] = lt.n_states                     # a target that is no state
    leaf = int(np.flatnonzero(np.diff(lt.edge_off) == 0)[0])
    fl = lt.state_flags.copy(); fl[leaf] = 0                            # a state without an allowed id
    many = np.zeros(L.SA_MAX_LEXICON_STATES + 2, np.int32)
    bad = [variant(edge_off=off), variant(edge_off=end), variant(edge_tok=tok_hi), variant(edge_tok=tok_eq), variant(edge_next=nxt),
           variant(state_flags=fl), variant(nop=V), variant(nop=-1),
           variant(edge_off=many, state_flags=np.ones(L.SA_MAX_LEXICON_STATES + 1, np.uint8), edge_tok=many[:0], edge_next=many[:0])]
    for k, v in enumerate(bad):
        with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
            m.set_lexicon(v)
        assert m.n_lexicon_states == 0, k
    # a refused call changes nothing: the next run is the one of the good tables
    _arm(m, lt)
    ref = _run(m, SLOTS, 3)
    _start(m, lt)
    for v in bad[:6]:
        with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
            m.set_lexicon(v)
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
        m.set_slot_lexicon([0, 0], [0, 0])                              # a slot named twice
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
        m.set_slot_lexicon([0], [lt.n_states])
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
        m.set_slot_lexicon([8], [0])
    again = _run(m, SLOTS, 3)
    for x, y in zip(ref, again):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    # beam search and forced decoding, both orders
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.set_beam(2)
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.set_forced(True)
    m.set_lexicon(None)
    m.set_beam(2)
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.set_lexicon(lt)
    m.set_beam(None)
    m.set_token_masks(None)
    m.set_forced(True)
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.set_lexicon(lt)                                               # (forced decoding admits no mask table either)
    m.set_forced(False)
    # a new mask table switches the lexicon off
    m.set_token_masks(_mask_table()[0])
    m.set_lexicon(lt)
    m.set_token_masks(_mask_table()[0])
    assert m.n_lexicon_states == 0
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.set_slot_lexicon([0], [0])
    m.set_token_masks(None)


# ------------------------------------------------------------------------------------------------------------------ the predictor
def _crops(n, seed=4):
    imgs = [Image.fromarray(c) for c in make_line_crops(n, seed=seed)]
    return imgs, [[[0, 0, im.size[0], im.size[1]]] for im in imgs]


def test_two_thousand_codes_end_to_end_and_not_vacuous(hip_lib, _max_tokens):
    """8 lines under the 2000 five-digit codes, token budget 8: every line reads exactly one code -- the mask only permits trie paths and
    ends a line only at a terminal. Unconstrained, the same crops land on a code on no line."""
    pred = _predictor(max_tokens=8)
    imgs, boxes = _crops(8)
    plain = pred(imgs, bboxes=boxes)
    assert all(ln.lexicon_index is None and "lexicon_index" not in ln.model_dump() for ln in _lines_of(plain))
    hits = [ln.text for ln in _lines_of(plain) if ln.text in set(CODES)]
    print("unconstrained lines that are a code:", hits)
    assert not hits
    try:
        pred.lexicon = CODES
        lines = _lines_of(pred(imgs, bboxes=boxes))
        assert pred.model.n_lexicon_states == 0 and pred.model.n_token_masks == 0      # switched off on the way out
    finally:
        pred.lexicon = None
    print("read:", [(ln.lexicon_index, ln.text) for ln in lines])
    assert len(lines) == 8
    for ln in lines:
        assert ln.lexicon_index is not None and ln.lexicon_index >= 0, (ln.lexicon_index, ln.text)
        assert ln.text == CODES[ln.lexicon_index] and CODES.index(ln.text) == ln.lexicon_index
    # a call with lexicon = None dumps exactly what it dumped before
    assert [r.model_dump() for r in pred(imgs, bboxes=boxes)] == [r.model_dump() for r in plain]


def test_predictor_lexicon_forms(hip_lib, _max_tokens):
    pred = _predictor(max_tokens=12)
    crops = make_line_crops(8, seed=4)
    imgs = [Image.fromarray(c) for c in crops[:4]]
    boxes = [[[0, 0, im.size[0], im.size[1]], [0, 0, im.size[0] // 2, im.size[1]]] for im in imgs]        # two lines per image
    plain = pred(imgs, bboxes=boxes)
    try:
        pred.lexicon = WORDS
        every = _lines_of(pred(imgs, bboxes=boxes))
        assert len(every) == 8
        for ln in every:
            assert ln.lexicon_index is not None and (ln.lexicon_index < 0 or ln.text == WORDS[ln.lexicon_index])
            assert any(w.startswith(ln.text) for w in WORDS), ln.text           # a cut line keeps a prefix of an entry
        # per image: none / words / per line (codes, none) / none, beside an allowlist on the last image and a pattern on the first
        pred.lexicon, pred.pattern = [None, WORDS, [CODES, None], None], [DATE, None, None, None]
        out = pred(imgs, bboxes=boxes, allowlist=[None, None, None, DIGITS])
        assert all(ln.pattern_matched is not None and ln.lexicon_index is None for ln in out[0].text_lines)
        assert [ln.model_dump() for ln in out[1].text_lines] == [ln.model_dump() for ln in every[2:4]]      # a line does not depend on its batch mates
        assert out[2].text_lines[0].lexicon_index >= 0 and out[2].text_lines[0].text in CODES
        assert out[2].text_lines[1].model_dump() == plain[2].text_lines[1].model_dump()
        assert all(ln.lexicon_index is None and set(ln.text) <= set(DIGITS) for ln in out[3].text_lines)
        pred.pattern = None
        # top_k: every alternative is a character some entry continues with
        pred.lexicon, pred.top_k = SHORT, 3
        for ln in _lines_of(pred(imgs, bboxes=boxes)):
            for ch in ln.chars:
                assert ch.alternatives and set("".join(a.text for a in ch.alternatives)) <= set("abc7")
        pred.top_k = None
        # malformed arguments raise before any device work
        for bad, err in (([WORDS], ValueError), ([[WORDS], None, None, None], ValueError), (7, TypeError), ("abc", TypeError), ([], ValueError),
                         (["ok", ""], ValueError), ([None, [], None, None], ValueError), ([None, [3], None, None], TypeError)):
            pred.lexicon = bad
            with pytest.raises(err):
                pred(imgs, bboxes=boxes)
        pred.lexicon = WORDS
        with pytest.raises(ValueError, match="never two"):
            pred(imgs, bboxes=boxes, allowlist=DIGITS)
        pred.pattern = DATE
        with pytest.raises(ValueError, match="never two"):
            pred(imgs, bboxes=boxes)
        pred.pattern = None
        pred.beam_width = 2
        with pytest.raises(ValueError, match="beam_width"):
            pred(imgs, bboxes=boxes)
        pred.beam_width = None
        with pytest.raises(ValueError, match="align"):
            pred.align(imgs, [["1", "2"]] * 4, bboxes=boxes)
    finally:
        pred.lexicon = pred.pattern = pred.top_k = pred.beam_width = None
    assert [r.model_dump() for r in pred(imgs, bboxes=boxes)] == [r.model_dump() for r in plain]


def test_streamed_call_with_a_lexicon_equals_the_serial_one(hip_lib, _max_tokens):
    from surya_amd.synth import make_pages_with_lines
    from test_gpu_predictors import _det_with_drawn_rows
    size = 256
    pages_np, rows = make_pages_with_lines(5, size, seed=99)
    pages = [Image.fromarray(p) for p in pages_np]
    det = _det_with_drawn_rows(pages, rows, size, 2)
    pred = _predictor(max_slots=8, max_tokens=8)
    try:
        for lexicon in (CODES, [CODES, None, SHORT, None, CODES]):
            pred.lexicon = lexicon
            pred.stream_detection = False
            serial = pred(pages, det_predictor=det)
            pred.stream_detection = True
            streamed = pred(pages, det_predictor=det)
            assert pred.last_timing.get("streamed") == 1.0
            assert [r.model_dump() for r in serial] == [r.model_dump() for r in streamed] and len(streamed) == 5
            assert sum(len(r.text_lines) for r in streamed) > 8
            assert all(ln.lexicon_index >= 0 and ln.text == CODES[ln.lexicon_index] for ln in streamed[0].text_lines)
            assert lexicon is CODES or all(ln.lexicon_index is None for ln in streamed[1].text_lines)
        pred.lexicon = [[CODES], None, None, None, None]
        with pytest.raises(ValueError, match="not known yet"):
            pred(pages, det_predictor=det)
    finally:
        pred.lexicon = None
