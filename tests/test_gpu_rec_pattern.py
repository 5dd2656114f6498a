"""GPU: pattern-guided decoding through the recognition engine (surya_rec_set_patterns / surya_rec_set_slot_patterns /
surya_rec_copy_slot_states) and through RecognitionPredictor.pattern, on REC-SMALL with synthetic weights.

The engine is checked step by step as tests/test_gpu_rec_allowlist.py checks token masks, with that file's `_check_step` and score
tolerance: at every step the token is the first argmax of the engine's own unmasked logits (surya_rec_copy_last_logits) masked by the row
of the state the HOST replay (PatternTables.advance) says the slot is in, the score is the softmax over that set, and the device's states
equal the replay's. Rows without a pattern must be bit-identical to an engine that never saw a mask."""
import ctypes as C
import functools
import re

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
DATE, AMOUNT, IBAN = r"\d{2}/\d{2}/\d{4}", r"-?\d{1,3}(,\d{3})*\.\d{2}", r"[A-Z]{2}\d{2}( ?[A-Z0-9]{4}){2,7}"
PATS = [DATE, AMOUNT, IBAN]
SLOTS = [0, 1, 2, 3, 4, 5]
LINE_PATS = [DATE, AMOUNT, IBAN, DATE, AMOUNT, None]


@functools.lru_cache(maxsize=None)
def _tables(pats=tuple(PATS), with_digits=False):
    """(PatternTables, id of the digits allowlist row or None): one mask table for both kinds of constraint."""
    from surya_amd.recognition.pattern import compile_patterns
    from surya_amd.recognition.tokenizer import MaskTable
    tk, V = _tokenizer(), _cfg_sd()[0].decoder.vocab_size
    tb = MaskTable(tk, V, L.SA_MAX_TOKEN_MASKS)
    dig = tb.id_for(DIGITS, None) if with_digits else None
    return compile_patterns(tk, list(pats), V, extra_mask_rows=tb), dig


def _arm(m, pt, slots=SLOTS, line_pats=LINE_PATS, mask_ids=None):
    """Upload the tables and put every slot at its line's start state (-1 = no pattern); -> the start states."""
    m.set_token_masks(pt.table.array())
    m.set_patterns(pt)
    return _start(m, pt, slots, line_pats, mask_ids)


def _start(m, pt, slots=SLOTS, line_pats=LINE_PATS, mask_ids=None):
    states = [-1 if p is None else pt.start_of(p) for p in line_pats]
    m.set_slot_masks(slots, [-1] * len(slots) if mask_ids is None else mask_ids)
    m.set_slot_patterns(slots, states)
    return states


def _rows(pt, states, mask_ids=None):
    ids = [int(pt.state_mask[s]) if s >= 0 else (-1 if mask_ids is None else mask_ids[r]) for r, s in enumerate(states)]
    return _allowed_rows(pt.table.array(), ids, _cfg_sd()[0].decoder.vocab_size)


def _text(tokens):
    sto = _tokenizer().special_token_offset
    return "".join(chr(int(t) - sto) for t in tokens)


def _replay_ok(pt, pat, tokens):
    """Host replay of one stream: (every token allowed where it stood, text before eos or None, state at the end)."""
    cfg = _cfg_sd()[0]
    st = pt.start_of(pat)
    for k, t in enumerate(tokens):
        t = int(t)
        if t == cfg.eos_token_id:
            return True, _text(tokens[:k]), st
        if t == cfg.pad_token_id:
            return pt.accepts(st), None, st
        if not pt.allowed(st, t):
            return False, None, st
        st = pt.advance(st, t)
    return True, None, st


def _stepwise(m, pt, n_steps, what, mask_ids=None):
    """Prefill six lines and decode one step at a time, checking token, score and device state against the host replay every step."""
    cfg = _cfg_sd()[0]
    states = _arm(m, pt, mask_ids=mask_ids)
    tiles, seqs = make_prompts(cfg, GRIDS, seed=9)
    m.prefill(tiles.cuda(), GRIDS, seqs, SLOTS)
    moved = 0
    for step in range(n_steps + 1):
        if step:
            m.decode(1)
        t, s, _ = m.read_outputs(1)
        _check_step(m, cfg, t[0], s[0], SLOTS, _rows(pt, states, mask_ids), f"{what} step {step}")
        new = [pt.advance(st, int(t[0, sl])) for st, sl in zip(states, SLOTS)]
        moved += sum(a != b for a, b in zip(new, states))
        states = new
        assert m.slot_states()[SLOTS].tolist() == states, (what, step)
        if step == 0:
            m.set_active(SLOTS)
    assert moved >= n_steps, "the automata hardly moved: the test shows nothing"
    return states


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_every_step_follows_the_host_replay(hip_lib, dtype):
    _stepwise(_model(dtype), _tables()[0], 6, str(dtype))


def test_lines_end_in_a_match_or_are_a_live_prefix(hip_lib):
    """12 steps: a line that reached eos fullmatches its pattern; every other line took only allowed tokens, so its state is one of the
    trimmed automaton's, from which a match can still be completed."""
    cfg = _cfg_sd()[0]
    pt = _tables()[0]
    m = _model(torch.bfloat16)
    pats = [DATE, AMOUNT, IBAN, DATE, AMOUNT, DATE]
    _arm(m, pt, line_pats=pats)
    toks = _run(m, SLOTS, 12)[0]
    done = 0
    for r, pat in enumerate(pats):
        stream = toks[:, r].tolist()
        if stream[0] == pt.nop:
            continue                                                    # a blank crop: the line ends at its first token
        ok, text, st = _replay_ok(pt, pat, stream)
        assert ok, (pat, stream)
        if text is not None:
            done += 1
            assert re.fullmatch(pat, text), (pat, text)
            assert pt.accepts(st)
        else:
            assert 0 <= st < pt.n_states
    print("lines that reached eos:", done)


def test_mixed_batch_leaves_unconstrained_rows_bit_identical(hip_lib):
    """Pattern, allowlist and unconstrained slots together: the unconstrained rows equal an engine that never saw a mask, bit for bit."""
    pt, dig = _tables(with_digits=True)
    m = _model(torch.bfloat16)
    plain = _run(m, SLOTS, 6)
    line_pats = [DATE, None, None, AMOUNT, None, None]
    mask_ids = [-1, dig, -1, -1, dig, -1]
    _arm(m, pt, line_pats=line_pats, mask_ids=mask_ids)
    mixed = _run(m, SLOTS, 6)
    for a, b in zip(plain, mixed):
        assert np.array_equal(a[:, [2, 5]].view(np.int32), b[:, [2, 5]].view(np.int32))
    digits = set(np.flatnonzero(_allowed_rows(pt.table.array(), [dig], _cfg_sd()[0].decoder.vocab_size)[0].cpu().numpy()).tolist())
    assert set(mixed[0][:, [1, 4]].reshape(-1).tolist()) <= digits
    assert _replay_ok(pt, DATE, mixed[0][:, 0].tolist())[0] and _replay_ok(pt, AMOUNT, mixed[0][:, 3].tolist())[0]
    assert not np.array_equal(plain[0][:, [0, 3]], mixed[0][:, [0, 3]]), "the pattern rows were not constrained at all"
    states = m.slot_states()
    assert states[1] == -1 and states[2] == -1 and states[0] >= 0
    # the stepwise check with an allowlist row beside the patterns
    _stepwise(_model(torch.bfloat16), pt, 3, "mixed", mask_ids=[-1, -1, -1, -1, -1, dig])


def test_eight_steps_in_one_call_equal_eight_calls(hip_lib):
    """decode(8): the head that advances the automaton also writes the next step's embedding; against 8 x decode(1)."""
    pt = _tables()[0]
    m = _model(torch.bfloat16)
    _arm(m, pt)
    one = _run(m, SLOTS, 8, single=True)
    s1 = m.slot_states()[SLOTS].tolist()
    _start(m, pt)
    eight = _run(m, SLOTS, 8)
    for a, b in zip(one, eight):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert m.slot_states()[SLOTS].tolist() == s1


def test_streams_do_not_depend_on_the_slot_count(hip_lib):
    """The same 8 lines alone and as the first 8 of 64 active slots: identical streams and states."""
    pt = _tables()[0]
    m = _model(torch.bfloat16, max_slots=64)
    pats = [PATS[i % 3] for i in range(64)]
    _arm(m, pt, slots=list(range(8)), line_pats=pats[:8])
    few = _run(m, list(range(8)), 5)
    s_few = m.slot_states()[:8].tolist()
    _start(m, pt, slots=list(range(64)), line_pats=pats)
    many = _run(m, list(range(64)), 5)
    for a, b in zip(few, many):
        assert np.array_equal(a.view(np.int32), b[:, :8].view(np.int32))
    assert m.slot_states()[:8].tolist() == s_few
    for r in range(64):
        assert _replay_ok(pt, pats[r], many[0][:, r].tolist())[0], r


def test_a_reused_slot_starts_at_its_new_lines_state(hip_lib):
    pt, dig = _tables(with_digits=True)
    m = _model(torch.bfloat16)
    _arm(m, pt, slots=[0, 1], line_pats=[DATE, AMOUNT])
    ref = _run(m, [0, 1], 4, lines=[2, 3])
    _start(m, pt, slots=[0, 1], line_pats=[AMOUNT, DATE])
    _run(m, [0, 1], 3, lines=[0, 1])
    assert (m.slot_states()[[0, 1]] >= 0).all()
    _start(m, pt, slots=[0, 1], line_pats=[DATE, AMOUNT])
    again = _run(m, [0, 1], 4, lines=[2, 3])
    for a, b in zip(ref, again):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    # a slot given a plain mask afterwards follows no automaton any more
    m.set_slot_masks([0], [dig])
    assert m.slot_states()[0] == -1
    toks = _run(m, [0, 1], 4, lines=[2, 3])[0]
    assert m.slot_states()[0] == -1
    digits = set(np.flatnonzero(_allowed_rows(pt.table.array(), [dig], _cfg_sd()[0].decoder.vocab_size)[0].cpu().numpy()).tolist())
    assert set(toks[:, 0].tolist()) <= digits


def test_mxfp8_head_with_patterns(hip_lib):
    _stepwise(_model(torch.bfloat16, decode_fp8=True), _tables()[0], 4, "mxfp8")


def test_every_alternative_is_allowed_in_the_steps_state(hip_lib):
    cfg = _cfg_sd()[0]
    pt = _tables()[0]
    m = _model(torch.bfloat16)
    m.set_alternatives(True)
    states = _arm(m, pt)
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
                assert all(pt.allowed(states[r], int(a)) for a in at[0, sl] if a >= 0), (step, r)
        states = [pt.advance(st, int(t[0, sl])) for st, sl in zip(states, SLOTS)]
        if step == 0:
            m.set_active(SLOTS)
    m.set_alternatives(False)


def test_captured_steps_follow_new_table_contents(hip_lib):
    """hipGraph replay on: the tables live at fixed addresses with a fixed row stride, so steps captured under one set of patterns obey
    the next set's contents."""
    from surya_amd.recognition.pattern import compile_patterns
    from surya_amd.recognition.tokenizer import MaskTable
    tk, V = _tokenizer(), _cfg_sd()[0].decoder.vocab_size
    tb = MaskTable(tk, V, L.SA_MAX_TOKEN_MASKS)                         # one mask table for both automata: replacing IT would drop the captures
    pt = compile_patterns(tk, PATS, V, extra_mask_rows=tb)
    other = compile_patterns(tk, [r"[a-f]{3}-\d+", r"(yes|no)( sir)?"], V, extra_mask_rows=tb)
    assert other.n_classes != pt.n_classes and other.n_states != pt.n_states
    m = _model(torch.bfloat16)
    m.set_token_masks(tb.array())
    L.check(m.lib.surya_set_tuning(b"graph", C.c_int(1)), "surya_set_tuning(graph)")
    try:
        streams = []
        for tables in (pt, pt, pt, other):                              # eager, capture, replay, replay under new contents
            pats = [tables.patterns[i % len(tables.patterns)] for i in range(4)]
            m.set_patterns(tables)
            _start(m, tables, slots=[0, 1, 2, 3], line_pats=pats)
            toks = _run(m, [0, 1, 2, 3], 4)[0]
            for r in range(4):
                assert _replay_ok(tables, pats[r], toks[:, r].tolist())[0], (tables.patterns, r)
            streams.append(toks)
        assert np.array_equal(streams[0], streams[1]) and np.array_equal(streams[0], streams[2])
    finally:
        L.check(m.lib.surya_set_tuning(b"graph", C.c_int(0)), "surya_set_tuning(graph)")


def test_entry_points_refuse_bad_tables_and_modes(hip_lib):
    pt = _tables()[0]
    m = _model(torch.bfloat16)
    from types import SimpleNamespace

    def variant(**kw):
        d = dict(tok_class=pt.tok_class.copy(), next_state=pt.next_state.copy(), state_mask=pt.state_mask.copy())
        d.update(kw)
        return SimpleNamespace(**d)
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.set_patterns(pt)                                              # no mask table yet
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.set_slot_patterns([0], [0])                                   # patterns are off
    m.set_token_masks(pt.table.array())
    sm = pt.state_mask.copy(); sm[3] = len(pt.table)
    ns = pt.next_state.copy(); ns[2, 1] = pt.n_states
    tc = pt.tok_class.copy(); tc[70] = pt.n_classes
    for bad in (variant(state_mask=sm), variant(next_state=ns), variant(tok_class=tc),
                variant(next_state=np.zeros((L.SA_MAX_PATTERN_STATES + 1, 2), np.uint16), state_mask=np.zeros(L.SA_MAX_PATTERN_STATES + 1, np.uint8)),
                variant(next_state=np.zeros((pt.n_states, L.SA_MAX_PATTERN_CLASSES + 1), np.uint16))):
        with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
            m.set_patterns(bad)
    # a refused call changes nothing: the next run is the one of the good tables
    _arm(m, pt)
    ref = _run(m, SLOTS, 3)
    _start(m, pt)
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
        m.set_patterns(variant(state_mask=sm))
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
        m.set_slot_patterns([0, 0], [0, 0])                             # a slot named twice
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
        m.set_slot_patterns([0], [pt.n_states])
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
        m.set_slot_patterns([8], [0])
    again = _run(m, SLOTS, 3)
    for a, b in zip(ref, again):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    # beam search and forced decoding, both orders
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.set_beam(2)
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.set_forced(True)
    m.set_patterns(None)
    m.set_beam(2)
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.set_patterns(pt)
    m.set_beam(None)
    m.set_token_masks(None)
    m.set_forced(True)
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.set_patterns(pt)                                              # (forced decoding admits no mask table either)
    m.set_forced(False)
    # a new mask table switches patterns off
    m.set_token_masks(pt.table.array())
    m.set_patterns(pt)
    m.set_token_masks(pt.table.array())
    assert m.n_pattern_states == 0
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.set_slot_patterns([0], [0])
    m.set_token_masks(None)


# ------------------------------------------------------------------------------------------------------------------ the predictor
def _pages(n=4):
    crops = make_line_crops(2 * n, seed=4)
    imgs = [Image.fromarray(c) for c in crops[:n]]
    boxes = [[[0, 0, im.size[0], im.size[1]], [0, 0, im.size[0] // 2, im.size[1]]] for im in imgs]        # two lines per image
    return imgs, boxes


def test_predictor_pattern_forms(hip_lib, _max_tokens):
    pred = _predictor(max_tokens=14)
    imgs, boxes = _pages()
    plain = pred(imgs, bboxes=boxes)
    assert all(ln.pattern_matched is None for ln in _lines_of(plain))
    try:
        pred.pattern = DATE                                             # one str for every line of the call
        out = pred(imgs, bboxes=boxes)
        lines = _lines_of(out)
        assert len(lines) == 8 and all(ln.pattern_matched is not None for ln in lines)
        for ln in lines:                                                # (a line that ended with pad, not eos, reports False whatever it reads)
            assert not ln.pattern_matched or re.fullmatch(DATE, ln.text), ln.text
            assert re.fullmatch(r"[\d/]*", ln.text), ln.text                 # (\d is re's: every Unicode decimal digit)
        assert pred.model.n_pattern_states == 0 and pred.model.n_token_masks == 0      # switched off on the way out
        # per image: none / date / per line (amount, none) / none, beside an allowlist on the last image
        pred.pattern = [None, DATE, [AMOUNT, None], None]
        out = pred(imgs, bboxes=boxes, allowlist=[None, None, None, DIGITS])
        assert [r.model_dump() for r in out[:1]] == [r.model_dump() for r in plain[:1]]
        assert [ln.model_dump() for ln in out[1].text_lines] == [ln.model_dump() for ln in lines[2:4]]      # a line does not depend on its batch mates
        assert out[2].text_lines[0].pattern_matched is not None and re.fullmatch(r"[\d,.-]*", out[2].text_lines[0].text)
        assert out[2].text_lines[1].model_dump() == plain[2].text_lines[1].model_dump()
        assert all(ln.pattern_matched is None and set(ln.text) <= set(DIGITS) for ln in out[3].text_lines)
        # top_k: every alternative is a character the pattern allows at that place
        pred.pattern, pred.top_k = DATE, 3
        for ln in _lines_of(pred(imgs, bboxes=boxes)):
            for ch in ln.chars:
                assert ch.alternatives and re.fullmatch(r"[\d/]*", "".join(a.text for a in ch.alternatives))
        pred.top_k = None
        # malformed arguments raise before any device work
        for bad, err in (([DATE], ValueError), ([[DATE], None, None, None], ValueError), (7, TypeError), (r"\d+$", ValueError), (r"(?i)a", ValueError)):
            pred.pattern = bad
            with pytest.raises(err):
                pred(imgs, bboxes=boxes)
        pred.pattern = DATE
        with pytest.raises(ValueError, match="not both"):
            pred(imgs, bboxes=boxes, allowlist=DIGITS)
        pred.beam_width = 2
        with pytest.raises(ValueError, match="beam_width"):
            pred(imgs, bboxes=boxes)
        pred.beam_width = None
        with pytest.raises(ValueError, match="align"):
            pred.align(imgs, [["1", "2"]] * 4, bboxes=boxes)
    finally:
        pred.pattern = pred.top_k = pred.beam_width = None
    assert [r.model_dump() for r in pred(imgs, bboxes=boxes)] == [r.model_dump() for r in plain]


def test_streamed_call_with_a_pattern_equals_the_serial_one(hip_lib, _max_tokens):
    from surya_amd.synth import make_pages_with_lines
    from test_gpu_predictors import _det_with_drawn_rows
    size = 256
    pages_np, rows = make_pages_with_lines(5, size, seed=99)
    pages = [Image.fromarray(p) for p in pages_np]
    det = _det_with_drawn_rows(pages, rows, size, 2)
    pred = _predictor(max_slots=8, max_tokens=12)
    try:
        for pattern in (DATE, [DATE, None, AMOUNT, None, DATE]):
            pred.pattern = pattern
            pred.stream_detection = False
            serial = pred(pages, det_predictor=det)
            pred.stream_detection = True
            streamed = pred(pages, det_predictor=det)
            assert pred.last_timing.get("streamed") == 1.0
            assert [r.model_dump() for r in serial] == [r.model_dump() for r in streamed] and len(streamed) == 5
            assert sum(len(r.text_lines) for r in streamed) > 8
            assert all(ln.pattern_matched is not None and (not ln.pattern_matched or re.fullmatch(DATE, ln.text)) for ln in streamed[0].text_lines)
            assert isinstance(pattern, str) or all(ln.pattern_matched is None for ln in streamed[1].text_lines)
        pred.pattern = [[DATE], None, None, None, None]
        with pytest.raises(ValueError, match="not known yet"):
            pred(pages, det_predictor=det)
    finally:
        pred.pattern = None


def test_date_pattern_end_to_end_and_not_vacuous(hip_lib, _max_tokens):
    """Synthetic weights know no dates: unconstrained, no line of the crops reads as one; under the date pattern every line that reports
    pattern_matched is a date by re.fullmatch, and some line does."""
    pred = _predictor(max_tokens=14)
    crops = make_line_crops(12, seed=11)
    imgs = [Image.fromarray(c) for c in crops]
    boxes = [[[0, 0, im.size[0], im.size[1]]] for im in imgs]
    plain = _lines_of(pred(imgs, bboxes=boxes))
    assert not any(re.fullmatch(DATE, ln.text) for ln in plain)
    try:
        pred.pattern = DATE
        lines = _lines_of(pred(imgs, bboxes=boxes))
    finally:
        pred.pattern = None
    assert len(lines) == 12
    matched = [ln for ln in lines if ln.pattern_matched]
    print("lines that matched:", len(matched), [ln.text for ln in lines])
    assert matched, "no line completed its date within the token budget"
    assert all(re.fullmatch(DATE, ln.text) for ln in matched)
    assert all(ln.pattern_matched is False for ln in lines if ln not in matched)
