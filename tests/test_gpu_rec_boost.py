"""GPU: boosted decoding through the recognition engine (surya_rec_set_boost / surya_rec_set_slot_boost / surya_rec_read_boost /
surya_rec_copy_boost_states) and through RecognitionPredictor.boost_words, on REC-SMALL with synthetic weights.

The reference for a step is that step's own unmasked logits (surya_rec_copy_last_logits): beta * [in S] is added to them in float32, the
token is the first argmax, the score its softmax value in float64; plain_token is the plain argmax and plain_prob the emitted token's
plain softmax value. S per row is the preferred set of the HOST replay (BoostTables) over the row's tokens so far. Tokens must be equal,
scores within the rtol = 2e-3 of tests/test_gpu_rec_allowlist.py. beta is derived inside the test from an unboosted run of the same lines
so that some rows flip and some do not. Rows that are not boosted must be bit-identical to a handle that never saw a boost table."""
import ctypes as C
import functools
import random
import string
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

from surya_amd import _lib as L
from surya_amd.synth import make_line_crops

from test_gpu_rec_allowlist import (DIGITS, GRIDS, _allowed_rows, _cfg_sd, _line, _lines_of, _max_tokens, _model, _predictor, _run,  # noqa: F401
                                    _tokenizer)
from util import make_prompts

pytestmark = pytest.mark.gpu
_r1 = random.Random(1)
WORDS5 = sorted({"".join(_r1.choice(string.ascii_lowercase) for _ in range(5)) for _ in range(220)})[:200]      # 200 five-letter words
PLACES = ["New York", "New Jersey", "Co-op", "York", "Ab", "b", "x y z", "Zürich", "éa"]
LISTS = [WORDS5, PLACES]
SLOTS = [0, 1, 2, 3, 4, 5]
LINE_LIST = [0, 1, 0, 1, None, None]                      # index into LISTS per line; None = not boosted
MASK_IDS = [-1, -1, -1, -1, 0, -1]                        # ... where line 4 carries the digits allowlist and line 5 nothing


@functools.lru_cache(maxsize=None)
def _setup(which=(0, 1)):
    """(BoostTables with word_row set, the call's mask table: digits, then the word-unit row)."""
    from surya_amd.recognition.boost import compile_boost
    from surya_amd.recognition.tokenizer import MaskTable
    tk, V = _tokenizer(), _cfg_sd()[0].decoder.vocab_size
    tb = MaskTable(tk, V, L.SA_MAX_TOKEN_MASKS)
    assert tb.id_for(DIGITS, None) == 0
    bt = compile_boost(tk, [LISTS[i] for i in which], V)
    bt.word_row = tb.add_row(bt.word_mask)
    return bt, tb.array()


def _roots(bt, line_list=LINE_LIST):
    return [-1 if k is None else bt.roots[k] for k in line_list]


def _arm(m, bt, table, beta, slots=SLOTS, line_list=LINE_LIST, mask_ids=MASK_IDS):
    m.set_token_masks(table)
    m.set_boost(bt)
    return _start(m, bt, beta, slots, line_list, mask_ids)


def _start(m, bt, beta, slots=SLOTS, line_list=LINE_LIST, mask_ids=MASK_IDS):
    m.set_slot_masks(slots, mask_ids)
    m.set_slot_boost(slots, _roots(bt, line_list), beta)
    return _roots(bt, line_list)


def _brun(m, slots, steps, single=False, lines=None):
    """_run of tests/test_gpu_rec_allowlist.py with the boost outputs: (tokens, scores, boxes, plain tokens, plain probabilities)."""
    lines = list(range(len(slots))) if lines is None else lines
    tiles, seqs = torch.cat([_line(i)[0] for i in lines]), [_line(i)[1] for i in lines]
    m.prefill(tiles.cuda(), [GRIDS[i % len(GRIDS)] for i in lines], seqs, slots)

    def take(k):
        (t, s, b), (pt, pp) = m.read_outputs(k), m.read_boost(k)
        return [(t[j, slots].copy(), s[j, slots].copy(), b[j, slots].copy(), pt[j, slots].copy(), pp[j, slots].copy()) for j in range(k)]
    out = take(1)
    m.set_active(sorted(slots))
    if single:
        for _ in range(steps):
            m.decode(1)
            out += take(1)
    elif steps:
        m.decode(steps)
        out += take(steps)
    return tuple(np.stack([o[i] for o in out]) for i in range(5))


def _replay(bt, root, tokens):
    """The states before each token of a stream, and the state behind the last one."""
    st, before = root, []
    for t in tokens:
        before.append(st)
        st = bt.advance(st, int(t), root)
    return before, st


def _sets(bt, states, V):
    S = np.zeros((len(states), V), bool)
    for r, st in enumerate(states):
        S[r, sorted(bt.preferred(st))] = True
    return torch.from_numpy(S).cuda()


def _first_argmax(x):
    best = x.max(1, keepdim=True).values
    cols = torch.arange(x.shape[1], device=x.device).expand_as(x)
    return torch.where(x == best, cols, torch.full_like(cols, 2 ** 31 - 1)).min(1).values


def _check_boost_step(m, cfg, bt, states, beta, out, slots, mask_ids, table, what, stats):
    """One step's outputs against the recomputation from that step's unmasked logits. A row that is not boosted is the masked row."""
    tok, score, ptok, pprob = (np.asarray(a)[slots] for a in out)
    V = cfg.decoder.vocab_size
    lg = m.last_logits()
    assert lg.shape == (len(slots), V) and lg.dtype == torch.float32
    S = _sets(bt, states, V)
    boosted = torch.tensor([st >= 0 for st in states], device=lg.device)
    allowed = _allowed_rows(table, [-1 if st >= 0 else mask_ids[r] for r, st in enumerate(states)], V)
    lb = torch.where(S, lg + torch.tensor(beta, dtype=torch.float32, device=lg.device), lg)              # the fp32 addition
    lb = lb.masked_fill(~allowed, float("-inf"))
    ref_tok = _first_argmax(lb)
    ref_ptok = _first_argmax(lg)
    idx = torch.arange(len(slots), device=lg.device)
    ref_score = torch.softmax(lb.double(), 1)[idx, ref_tok].cpu().numpy()
    ref_pprob = torch.softmax(lg.double(), 1)[idx, ref_tok].cpu().numpy()
    ref_tok, ref_ptok = ref_tok.cpu().numpy(), ref_ptok.cpu().numpy()
    assert np.array_equal(tok, ref_tok), (what, tok.tolist(), ref_tok.tolist())
    assert np.array_equal(ptok, ref_ptok), (what, ptok.tolist(), ref_ptok.tolist())
    live = ~np.isin(ref_tok, [cfg.eos_token_id, cfg.pad_token_id])
    rel = np.abs(score[live] - ref_score[live]) / ref_score[live]
    relp = np.abs(pprob - ref_pprob) / ref_pprob
    print(f"{what}: score rel {rel.max() if rel.size else 0.0:.3e}, plain_prob rel {relp.max():.3e}")
    assert (rel <= 2e-3).all() and (score[~live] == 0).all() and (relp <= 2e-3).all(), (what, rel.max(), relp.max())
    b = boosted.cpu().numpy()
    nonempty = S.any(1).cpu().numpy() & b
    stats["flipped"] += int((b & (tok != ptok)).sum())
    stats["kept"] += int((nonempty & (tok == ptok)).sum())
    stats["nonempty"] += int(nonempty.sum())


def _beta_between_gaps(m, cfg, bt, roots):
    """An unboosted prefill of the same lines: beta between two distinct step-0 gaps maxB - maxA of the rows that will be boosted."""
    tiles, seqs = make_prompts(cfg, GRIDS, seed=9)
    m.prefill(tiles.cuda(), GRIDS, seqs, SLOTS)
    lg = m.last_logits()
    S = _sets(bt, roots, cfg.decoder.vocab_size)
    rows = [r for r, st in enumerate(roots) if st >= 0]
    for r in rows:
        assert len({t for t in bt.preferred(roots[r])}) >= 4                 # the root's first letters cover at least four distinct units
    gaps = sorted({float(lg[r].max() - lg[r][S[r]].max()) for r in rows})
    assert len(gaps) >= 2 and gaps[0] >= 0
    k = len(gaps) // 2
    return (gaps[k - 1] + gaps[k]) / 2


def _stepwise(m, n_steps, what):
    cfg = _cfg_sd()[0]
    bt, table = _setup()
    beta = _beta_between_gaps(m, cfg, bt, _roots(bt))
    print(f"{what}: beta {beta:.4f}")
    states = _arm(m, bt, table, beta)
    roots = list(states)
    tiles, seqs = make_prompts(cfg, GRIDS, seed=9)
    m.prefill(tiles.cuda(), GRIDS, seqs, SLOTS)
    stats = {"flipped": 0, "kept": 0, "nonempty": 0}
    for step in range(n_steps + 1):
        if step:
            m.decode(1)
        (t, s, _), (pt, pp) = m.read_outputs(1), m.read_boost(1)
        _check_boost_step(m, cfg, bt, states, beta, (t[0], s[0], pt[0], pp[0]), SLOTS, MASK_IDS, table, f"{what} step {step}", stats)
        states = [bt.advance(st, int(t[0, sl]), rt) for st, sl, rt in zip(states, SLOTS, roots)]
        assert m.copy_boost_states()[SLOTS].tolist() == states, (what, step)
        if step == 0:
            m.set_active(SLOTS)
    print(f"{what}: {stats}")
    assert stats["flipped"] >= 1 and stats["kept"] >= 1, "no token differs from the plain one, or none with a non-empty set agrees: the test shows nothing"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_every_step_equals_the_boosted_recomputation(hip_lib, dtype):
    _stepwise(_model(dtype), 6, str(dtype))


def test_mxfp8_head_with_boosting(hip_lib):
    _stepwise(_model(torch.bfloat16, decode_fp8=True), 4, "mxfp8")


def test_beta_zero_is_the_run_without_boosting_and_a_large_beta_follows_the_list(hip_lib):
    bt, table = _setup()
    m = _model(torch.bfloat16)
    plain = _run(m, SLOTS, 8)
    every = [0, 1, 0, 1, 0, 1]
    _arm(m, bt, table, 0.0, line_list=every, mask_ids=[-1] * 6)
    zero = _brun(m, SLOTS, 8)
    for a, b in zip(plain, zero[:3]):                                    # tot = sumB * exp(0) + sumA * 0: the same bits, not only the same tokens
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert np.array_equal(zero[3], zero[0])                              # and the plain reading is the reading
    _start(m, bt, 1e4, line_list=every, mask_ids=[-1] * 6)
    big = _brun(m, SLOTS, 8)
    hits = 0
    for r, k in enumerate(every):
        stream = big[0][:, r].tolist()
        before, _ = _replay(bt, bt.roots[k], stream)
        for t, st in zip(stream, before):
            if bt.preferred(st):
                assert t in bt.preferred(st), (r, stream)
                hits += 1
            if t in (bt.eos, bt.pad):
                break
    assert hits >= 12
    ended = np.isin(big[0], [bt.eos, bt.pad])
    assert (big[1][~ended] > 0).all() and (big[1] <= 1.0001).all() and np.isfinite(big[1]).all() and np.isfinite(big[4]).all()      # beta = 1e4 overflows nothing


def test_mixed_batch_leaves_the_other_rows_bit_identical(hip_lib):
    """Boosted, allowlist and unconstrained slots together: the rows that are not boosted equal, bit for bit, a handle that never saw a boost
    table; switching off restores every row."""
    bt, table = _setup()
    never = _model(torch.bfloat16)
    never.set_token_masks(table)
    never.set_slot_masks(SLOTS, MASK_IDS)
    without = _run(never, SLOTS, 6)
    m = _model(torch.bfloat16)
    _arm(m, bt, table, 1e4)
    mixed = _brun(m, SLOTS, 6)
    for a, b in zip(without, mixed[:3]):
        assert np.array_equal(a[:, [4, 5]].view(np.int32), b[:, [4, 5]].view(np.int32))
    assert not np.array_equal(without[0][:, :4], mixed[0][:, :4]), "the boosted rows were not boosted at all"
    st = m.copy_boost_states()
    assert st[4] == -1 and st[5] == -1 and (st[:4] >= 0).all()
    m.set_boost(None)
    m.set_slot_masks(SLOTS, MASK_IDS)
    off = _run(m, SLOTS, 6)
    for a, b in zip(without, off):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.read_boost(1)                                                  # the set is off


def test_eight_steps_in_one_call_equal_eight_calls(hip_lib):
    bt, table = _setup()
    m = _model(torch.bfloat16)
    _arm(m, bt, table, 3.0)
    one = _brun(m, SLOTS, 8, single=True)
    s1 = m.copy_boost_states()[SLOTS].tolist()
    _start(m, bt, 3.0)
    eight = _brun(m, SLOTS, 8)
    for a, b in zip(one, eight):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert m.copy_boost_states()[SLOTS].tolist() == s1


def test_streams_do_not_depend_on_the_slot_count(hip_lib):
    bt, table = _setup()
    lists = [i % 2 for i in range(64)]
    m8 = _model(torch.bfloat16, max_slots=8)
    _arm(m8, bt, table, 3.0, slots=list(range(8)), line_list=lists[:8], mask_ids=[-1] * 8)
    few = _brun(m8, list(range(8)), 5)
    s_few = m8.copy_boost_states()[:8].tolist()
    m = _model(torch.bfloat16, max_slots=64)
    _arm(m, bt, table, 3.0, slots=list(range(64)), line_list=lists, mask_ids=[-1] * 64)
    many = _brun(m, list(range(64)), 5)
    for a, c in zip(few, many):
        assert np.array_equal(a.view(np.int32), c[:, :8].view(np.int32))
    got = m.copy_boost_states()
    assert got[:8].tolist() == s_few
    assert got.tolist() == [_replay(bt, bt.roots[lists[r]], many[0][:, r].tolist())[1] for r in range(64)]


def test_a_reused_slot_starts_anew_and_a_plain_mask_id_stops_it(hip_lib):
    bt, table = _setup()
    m = _model(torch.bfloat16)
    _arm(m, bt, table, 1e4, slots=[0, 1], line_list=[0, 1], mask_ids=[-1, -1])
    ref = _brun(m, [0, 1], 4, lines=[2, 3])
    _start(m, bt, 1e4, slots=[0, 1], line_list=[1, 0], mask_ids=[-1, -1])          # other lines, other lists: their bits are anywhere in the rows
    _brun(m, [0, 1], 3, lines=[0, 1])
    _start(m, bt, 1e4, slots=[0, 1], line_list=[0, 1], mask_ids=[-1, -1])
    again = _brun(m, [0, 1], 4, lines=[2, 3])
    for a, b in zip(ref, again):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    m.set_slot_masks([0], [0])                                          # a plain mask id: the slot is not boosted any more
    assert m.copy_boost_states()[0] == -1
    toks = _brun(m, [0, 1], 4, lines=[2, 3])[0]
    assert m.copy_boost_states()[0] == -1
    digits = set(np.flatnonzero(_allowed_rows(table, [0], _cfg_sd()[0].decoder.vocab_size)[0].cpu().numpy()).tolist())
    assert set(toks[:, 0].tolist()) <= digits


def test_captured_steps_follow_new_table_contents(hip_lib):
    """hipGraph replay on: tables of the same capacity live at the same addresses, so steps captured under one automaton obey the next
    one's contents; a larger automaton moves them and is followed just the same."""
    from surya_amd.recognition.boost import compile_boost
    tk, V = _tokenizer(), _cfg_sd()[0].decoder.vocab_size
    _, table = _setup()
    word_row = _setup()[0].word_row
    rng = random.Random(5)
    small = compile_boost(tk, [PLACES, WORDS5[:40]], V)
    other = compile_boost(tk, [WORDS5[40:80], PLACES], V)
    big = compile_boost(tk, [WORDS5, ["".join(rng.choice(string.ascii_lowercase) for _ in range(7)) for _ in range(400)]], V)
    for t in (small, other, big):
        t.word_row = word_row
    assert max(small.n_states, other.n_states, small.n_edges, other.n_edges) <= 1024 < big.n_edges      # (1024: the smallest capacity)
    m = _model(torch.bfloat16)
    m.set_token_masks(table)
    L.check(m.lib.surya_set_tuning(b"graph", C.c_int(1)), "surya_set_tuning(graph)")
    try:
        streams = []
        for tables in (small, small, small, other, big, big, big, small):      # eager, capture, replay, new contents; grown; ...; smaller again
            lists = [0, 1, 0, 1]
            m.set_boost(tables)
            m.set_slot_masks([0, 1, 2, 3], [-1] * 4)
            m.set_slot_boost([0, 1, 2, 3], [tables.roots[k] for k in lists], 1e4)
            toks = _brun(m, [0, 1, 2, 3], 4)[0]
            for r in range(4):
                before, _ = _replay(tables, tables.roots[lists[r]], toks[:, r].tolist())
                assert all(t in tables.preferred(st) for t, st in zip(toks[:, r].tolist(), before) if tables.preferred(st)), r
            streams.append(toks)
        assert np.array_equal(streams[0], streams[1]) and np.array_equal(streams[0], streams[2]) and np.array_equal(streams[0], streams[7])
        assert np.array_equal(streams[4], streams[5]) and np.array_equal(streams[4], streams[6])
        assert not np.array_equal(streams[0], streams[3])
    finally:
        L.check(m.lib.surya_set_tuning(b"graph", C.c_int(0)), "surya_set_tuning(graph)")


def test_entry_points_refuse_bad_tables_and_modes(hip_lib):
    bt, table = _setup()
    V = _cfg_sd()[0].decoder.vocab_size
    m = _model(torch.bfloat16)

    def variant(**kw):
        d = dict(edge_off=bt.edge_off.copy(), edge_tok=bt.edge_tok.copy(), edge_next=bt.edge_next.copy(), out_state=bt.out_state, word_row=bt.word_row)
        d.update(kw)
        return SimpleNamespace(**d)
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.set_boost(bt)                                                 # no mask table yet
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.set_slot_boost([0], [1], 1.0)                                 # boosting is off
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.copy_boost_states()                                           # ... and never was on
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.read_boost(1)
    m.set_token_masks(table)
    root = bt.roots[0]
    a, b = int(bt.edge_off[root]), int(bt.edge_off[root + 1])
    assert b - a >= 2
    i = int(np.flatnonzero(np.diff(bt.edge_off) > 0)[1])
    off = bt.edge_off.copy(); off[i + 1] = off[i] - 1                   # not monotone
    end = bt.edge_off.copy(); end[-1] -= 1                              # does not end at n_edges
    tok_hi = bt.edge_tok.copy(); tok_hi[b - 1] = V                      # outside the vocabulary
    tok_eq = bt.edge_tok.copy(); tok_eq[a + 1] = tok_eq[a]              # not strictly ascending
    tok_eos = bt.edge_tok.copy(); tok_eos[a] = bt.eos                   # eos is never preferred
    nxt = bt.edge_next.copy(); nxt[5] = bt.n_states                     # a target that is no state
    many = np.zeros(L.SA_MAX_LEXICON_STATES + 2, np.int32)
    bad = [variant(edge_off=off), variant(edge_off=end), variant(edge_tok=tok_hi), variant(edge_tok=tok_eq), variant(edge_tok=tok_eos),
           variant(edge_next=nxt), variant(out_state=root), variant(out_state=bt.n_states), variant(word_row=len(table)), variant(word_row=-1),
           variant(edge_off=many, edge_tok=many[:0], edge_next=many[:0])]
    for k, v in enumerate(bad):
        with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
            m.set_boost(v)
        assert m.n_boost_states == 0, k
    # a refused call changes nothing: the next run is the one of the good tables
    _arm(m, bt, table, 2.0)
    ref = _brun(m, SLOTS, 3)
    _start(m, bt, 2.0)
    for v in bad[:8]:
        with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
            m.set_boost(v)
    for slots, roots, betas in (([0, 0], [1, 1], 1.0), ([0], [bt.n_states], 1.0), ([8], [1], 1.0), ([0], [1], -1.0), ([0], [1], float("inf")),
                                ([0], [1], float("nan"))):
        with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
            m.set_slot_boost(slots, roots, betas)
    again = _brun(m, SLOTS, 3)
    for x, y in zip(ref, again):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    # every refused mode pair, both orders
    from surya_amd.recognition.lexicon import compile_lexicons
    from surya_amd.recognition.pattern import compile_patterns
    from surya_amd.recognition.tokenizer import MaskTable
    lt = compile_lexicons(_tokenizer(), [["ab", "cd"]], V)
    tb = MaskTable(_tokenizer(), V, L.SA_MAX_TOKEN_MASKS)
    tb.id_for(DIGITS, None)
    word_row = tb.add_row(bt.word_mask)
    pt = compile_patterns(_tokenizer(), [r"\d+"], V, extra_mask_rows=tb)
    assert word_row == bt.word_row
    for on in (lambda: m.set_alternatives(True), lambda: m.set_beam(2), lambda: m.set_forced(True), lambda: m.set_patterns(pt), lambda: m.set_lexicon(lt)):
        with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
            on()
    m.set_boost(None)
    m.set_token_masks(tb.array())
    for on, off in ((lambda: m.set_alternatives(True), lambda: m.set_alternatives(False)), (lambda: m.set_beam(2), lambda: m.set_beam(None)),
                    (lambda: m.set_patterns(pt), lambda: m.set_patterns(None)), (lambda: m.set_lexicon(lt), lambda: m.set_lexicon(None))):
        on()
        with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
            m.set_boost(bt)
        off()
    m.set_token_masks(None)
    m.set_forced(True)
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.set_boost(bt)                                                 # (forced decoding admits no mask table either)
    m.set_forced(False)
    # allowed beside it: the fp8 KV cache; and a new mask table switches boosting off
    m.set_kv_fp8(True)
    _arm(m, bt, table, 2.0)
    _brun(m, SLOTS, 2)
    m.set_token_masks(table)
    assert m.n_boost_states == 0
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.set_slot_boost([0], [1], 1.0)
    m.set_token_masks(None)
    m.set_kv_fp8(False)


# ------------------------------------------------------------------------------------------------------------------ the predictor
def _crops(n, seed=4):
    imgs = [Image.fromarray(c) for c in make_line_crops(n, seed=seed)]
    return imgs, [[[0, 0, im.size[0], im.size[1]]] for im in imgs]


def _first_matches(text, words):
    return [w for w in words if text.startswith(w)]


def test_two_hundred_words_end_to_end_and_not_vacuous(hip_lib, _max_tokens):
    """8 lines, 200 five-letter words, beta = 1e4, token budget 8: every line reads a listed word first. Without boosting no line holds one."""
    pred = _predictor(max_tokens=8)
    imgs, boxes = _crops(8)
    plain = pred(imgs, bboxes=boxes)
    for ln in _lines_of(plain):
        assert ln.boost_matches is None and "boost_matches" not in ln.model_dump() and all(c.plain is None for c in ln.chars)
    from surya_amd.recognition.boost import compile_boost
    bt = compile_boost(pred.processor.ocr_tokenizer, [WORDS5], pred.model.vocab)
    hits = [ln.text for ln in _lines_of(plain) if any(w in ln.text for w in WORDS5)]
    print("unboosted lines that hold a listed word:", hits)
    assert not hits
    try:
        pred.boost_words, pred.boost_weight = WORDS5, 1e4
        lines = _lines_of(pred(imgs, bboxes=boxes))
        assert pred.model.n_boost_states == 0 and pred.model.n_token_masks == 0      # switched off on the way out
    finally:
        pred.boost_words = pred.boost_weight = None
    print("read:", [(ln.boost_matches, ln.text) for ln in lines])
    assert len(lines) == 8
    for ln in lines:
        assert ln.boost_matches, (ln.boost_matches, ln.text)
        assert ln.text.startswith(WORDS5[ln.boost_matches[0]]), (ln.boost_matches, ln.text)
        assert all(c.plain is not None and 0 <= c.plain_confidence <= 1.0001 for c in ln.chars[:5])
        assert any(c.plain != c.text for c in ln.chars[:5])                          # the model alone would have read something else
        assert 0 <= (ln.confidence or 0) <= 1
    assert bt.n_states > 64
    # a call with boost_words = None dumps exactly what it dumped before
    assert [r.model_dump() for r in pred(imgs, bboxes=boxes)] == [r.model_dump() for r in plain]


def test_predictor_boost_word_forms(hip_lib, _max_tokens):
    pred = _predictor(max_tokens=8)
    crops = make_line_crops(8, seed=4)
    imgs = [Image.fromarray(c) for c in crops[:4]]
    boxes = [[[0, 0, im.size[0], im.size[1]], [0, 0, im.size[0] // 2, im.size[1]]] for im in imgs]        # two lines per image
    plain = pred(imgs, bboxes=boxes)
    try:
        pred.boost_words, pred.boost_weight = WORDS5, 1e4
        every = _lines_of(pred(imgs, bboxes=boxes))
        assert len(every) == 8 and all(ln.boost_matches for ln in every)
        # per image: none / words / per line (places, none) / none, beside an allowlist on the last image
        pred.boost_words = [None, WORDS5, [PLACES, None], None]
        out = pred(imgs, bboxes=boxes, allowlist=[None, None, None, DIGITS])
        assert [ln.model_dump() for ln in out[0].text_lines] == [ln.model_dump() for ln in plain[0].text_lines]
        assert [ln.model_dump() for ln in out[1].text_lines] == [ln.model_dump() for ln in every[2:4]]       # a line does not depend on its batch mates
        a, b = out[2].text_lines
        assert a.boost_matches and all(PLACES[k] in a.text for k in a.boost_matches)
        assert b.model_dump() == plain[2].text_lines[1].model_dump() and b.boost_matches is None
        assert all(ln.boost_matches is None and set(ln.text) <= set(DIGITS) for ln in out[3].text_lines)
        # beta = 0: the text of the plain call, with the plain reading equal to the reading
        pred.boost_words, pred.boost_weight = WORDS5, 0.0
        zero = _lines_of(pred(imgs, bboxes=boxes))
        assert [ln.text for ln in zero] == [ln.text for ln in _lines_of(plain)]
        assert [ln.confidence for ln in zero] == [ln.confidence for ln in _lines_of(plain)]
        # malformed arguments raise before any device work
        pred.boost_weight = 2.0
        for bad, err in (([WORDS5], ValueError), ([[WORDS5], None, None, None], ValueError), (7, TypeError), ("abc", TypeError), ([], ValueError),
                         (["ok", ""], ValueError), ([None, [], None, None], ValueError), ([None, [3], None, None], TypeError)):
            pred.boost_words = bad
            with pytest.raises(err):
                pred(imgs, bboxes=boxes)
        pred.boost_words = WORDS5
        with pytest.raises(ValueError, match="takes no allowlist"):
            pred(imgs, bboxes=boxes, allowlist=DIGITS)
        for name, value in (("top_k", 2), ("beam_width", 2), ("pattern", r"\d+"), ("lexicon", ["ab"])):
            setattr(pred, name, value)
            with pytest.raises(ValueError, match=name):
                pred(imgs, bboxes=boxes)
            setattr(pred, name, None)
        with pytest.raises(ValueError, match="align"):
            pred.align(imgs, [["1", "2"]] * 4, bboxes=boxes)
        pred.boost_weight = None
        with pytest.raises(ValueError, match="boost_weight"):
            pred(imgs, bboxes=boxes)
    finally:
        pred.boost_words = pred.boost_weight = pred.pattern = pred.lexicon = pred.top_k = pred.beam_width = None
    assert [r.model_dump() for r in pred(imgs, bboxes=boxes)] == [r.model_dump() for r in plain]


def test_streamed_call_with_boost_words_equals_the_serial_one(hip_lib, _max_tokens):
    from surya_amd.synth import make_pages_with_lines
    from test_gpu_predictors import _det_with_drawn_rows
    size = 256
    pages_np, rows = make_pages_with_lines(5, size, seed=99)
    pages = [Image.fromarray(p) for p in pages_np]
    det = _det_with_drawn_rows(pages, rows, size, 2)
    pred = _predictor(max_slots=8, max_tokens=8)
    try:
        pred.boost_weight = 1e4
        for words in (WORDS5, [WORDS5, None, PLACES, None, WORDS5]):
            pred.boost_words = words
            pred.stream_detection = False
            serial = pred(pages, det_predictor=det)
            pred.stream_detection = True
            streamed = pred(pages, det_predictor=det)
            assert pred.last_timing.get("streamed") == 1.0
            assert [r.model_dump() for r in serial] == [r.model_dump() for r in streamed] and len(streamed) == 5
            assert sum(len(r.text_lines) for r in streamed) > 8
            assert all(ln.boost_matches and ln.text.startswith(WORDS5[ln.boost_matches[0]]) for ln in streamed[0].text_lines)
            assert words is WORDS5 or all(ln.boost_matches is None for ln in streamed[1].text_lines)
        pred.boost_words = [[WORDS5], None, None, None, None]
        with pytest.raises(ValueError, match="not known yet"):
            pred(pages, det_predictor=det)
    finally:
        pred.boost_words = pred.boost_weight = None
