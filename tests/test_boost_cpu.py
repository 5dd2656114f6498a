"""Boosted decoding, host side (no GPU): the compiler (recognition/boost.py) against a brute-force "live matches" oracle, `matches`,
surrogates, limits and refusals; the device loop's contract with the model (on the fake of tests/test_scheduler_cpu.py); boost_matches /
plain / plain_confidence from assembly; the predictor's argument forms; roots through shard_lines and the page-sharded call; and
csrc/boost_core.h compiled for the host against float64 numpy."""
import random
import re
import string
import time
from types import SimpleNamespace

import numpy as np
import pytest

from surya_amd import _lib as L
from surya_amd.config import rec_config
from surya_amd.recognition.boost import BoostTables, compile_boost, word_unit_bits
from surya_amd.recognition.loader import RecognitionModelLoader
from surya_amd.recognition.predictor import LineConstraints
from surya_amd.recognition.tokenizer import OCRTokenizer
from surya_amd.settings import settings

import boost_ref as br
from test_lexicon_cpu import STATES, ids_of
from test_pattern_cpu import PatternFakeModel
from test_scheduler_cpu import expected, make

SMILE = "\U0001F600"
ALPHABET = "abN -é"                                     # two letters, a capital, two boundaries, one foreign letter
LISTS = {"mixed": ["ab", "a b", "b-a", "Nab", "ab ab"], "states": STATES, "prefixes": ["a", "ab", "ab a", "ab ab", "b", "ba", "b-", "b-a", "N", "Na b"]}


@pytest.fixture(scope="module")
def tok():
    return OCRTokenizer()


def is_word(ch):
    return re.match(r"\w", ch) is not None


# ------------------------------------------------------------------------------------------------------------------ the compiler
class Oracle:
    """The definition, by brute force: a match of an entry is live at position p of the string s if it began at a boundary position i
    (i == 0, or s[i - 1] is no word unit) and s[i:p] is a proper prefix of the entry; it completes at p if s[i:p] is the entry."""

    def __init__(self, entries):
        self.next_of, self.whole = {}, {}
        for k, e in enumerate(entries):
            self.whole.setdefault(e, k)
            for j in range(len(e)):
                self.next_of.setdefault(e[:j], set()).add(e[j])

    @staticmethod
    def starts(s):
        return [i for i in range(len(s) + 1) if i == 0 or not is_word(s[i - 1])]

    def preferred(self, s):
        out = set()
        for i in self.starts(s):
            out |= self.next_of.get(s[i:], set())
        return out

    def matches(self, s):
        out = []
        for p in range(1, len(s) + 1):
            done = sorted(self.whole[s[i:p]] for i in self.starts(s[:p]) if i < p and s[i:p] in self.whole)
            out += [k for k in done if k not in out]
        return out


@pytest.mark.parametrize("name", list(LISTS))
def test_the_automaton_against_the_live_match_oracle(tok, name):
    entries = LISTS[name]
    bt = compile_boost(tok, [entries], tok.vocab_size)
    root, sto = bt.roots[0], tok.special_token_offset
    assert bt.edge_off.dtype == bt.edge_tok.dtype == bt.edge_next.dtype == np.int32
    assert bt.n_states == len(bt.edge_off) - 1 and bt.n_edges == len(bt.edge_tok) == len(bt.edge_next) == bt.edge_off[-1]
    assert bt.edges(bt.out_state)[0].size == 0 and root != bt.out_state
    for st in range(bt.n_states):
        toks, nxt = bt.edges(st)
        assert (np.diff(toks) > 0).all() and (nxt >= 0).all() and (nxt < bt.n_states).all()
        assert bt.eos not in toks and bt.pad not in toks
        assert set(np.flatnonzero(np.unpackbits(bt.row(st).view(np.uint8), bitorder="little")).tolist()) == bt.preferred(st)
    orc = Oracle(entries)
    ids = {ch: sto + ord(ch) for ch in ALPHABET}
    nodes = leaves = 0
    stack = [("", root)]
    while stack:                                             # every string up to length 6, walked as a trie
        s, st = stack.pop()
        nodes += 1
        assert bt.preferred(st) == {sto + ord(c) for c in orc.preferred(s)}, (s, st)
        if len(s) == 6:
            leaves += 1
            if leaves % 7 == 0:                              # (a seventh of the leaves: matches replays the whole string)
                assert bt.matches(root, [ids[c] for c in s]) == orc.matches(s), s
            continue
        for ch in ALPHABET:
            stack.append((s + ch, bt.advance(st, ids[ch], root)))
    assert nodes == sum(6 ** k for k in range(7))
    # the fallback transitions, by name: a word unit without an edge -> OUT, a boundary without an edge -> the root; eos / pad / ids
    # outside the vocabulary / a slot that is not boosted keep the state
    z = sto + ord("z")
    assert bt.advance(root, z, root) == bt.out_state and bt.advance(bt.out_state, z, root) == bt.out_state
    assert bt.advance(bt.out_state, sto + ord("."), root) == root and bt.advance(bt.out_state, 3, root) == root      # (3: a math BPE id)
    for st in (root, bt.out_state):
        assert bt.advance(st, bt.eos, root) == st and bt.advance(st, bt.pad, root) == st and bt.advance(st, tok.vocab_size + 5, root) == st
    assert bt.advance(-1, z, root) == -1 and bt.preferred(-1) == set()


def test_matches_on_hand_made_token_lists(tok):
    lst = ["New York", "York", "New Jersey", "Co-op", "op", "New"]
    bt = compile_boost(tok, [lst, ["York"]], tok.vocab_size)
    r0, r1 = bt.roots
    m = lambda s, r=r0: bt.matches(r, ids_of(tok, s))
    assert m("New York") == [5, 0, 1]                        # "New" first, then "New York" and the "York" that began behind the space
    assert m("in New Jersey, at the Co-op.") == [5, 2, 3, 4]     # "op" begins behind the hyphen, a boundary
    assert m("NewYork") == [5] and m("aNew York") == [1] and m("Yorkshire") == [1] and m("New Yor") == [5]
    assert m("York York") == [1] and m("") == [] and m("zzz") == []
    assert m("New York", r1) == [0] and m("New", r1) == []
    assert bt.matches(r0, ids_of(tok, "Yo") + [bt.eos] + ids_of(tok, "rk")) == [1]      # eos / pad keep the state, as on the device
    assert bt.matches(-1, ids_of(tok, "York")) == []
    # after "New " both "York" and the J of "New Jersey" are preferred, and the N of a new "New ..."
    st = r0
    for t in ids_of(tok, "New "):
        st = bt.advance(st, t, r0)
    sto = tok.special_token_offset
    assert bt.preferred(st) == {sto + ord(c) for c in "YJNCo"}
    assert bt.list_of_root(r1) == 1 and len(set(bt.roots)) == 2 and bt.roots[0] != bt.out_state


def test_surrogates_and_verbatim_entries(tok):
    bt = compile_boost(tok, [[SMILE + "a", "Été", " x"]], tok.vocab_size)
    r, sto = bt.roots[0], tok.special_token_offset
    hi, lo = [sto + u for u in (0xD83D, 0xDE00)]
    assert ids_of(tok, SMILE) == [hi, lo] and bt.word_bits[hi] and bt.word_bits[lo]
    assert bt.preferred(r) == {hi, sto + 0xC9, sto + 0x20}
    st = bt.advance(r, hi, r)
    assert bt.preferred(st) == {lo}
    assert bt.matches(r, ids_of(tok, SMILE + "a " + SMILE + "a")) == [0]
    assert bt.matches(r, ids_of(tok, "été Été")) == [1]          # no case folding
    # " x" begins at the line start or behind a boundary: the space behind "a" is itself no boundary POSITION
    assert bt.matches(r, ids_of(tok, "a, x")) == [2] and bt.matches(r, ids_of(tok, "a x")) == [] and bt.matches(r, ids_of(tok, "ax")) == []
    assert bt.matches(r, ids_of(tok, " x")) == [2]
    # the word-unit set: \w and the surrogates among the code units, nothing among math BPE, tags and specials
    w = word_unit_bits(sto, tok.vocab_size)
    assert not w[:sto].any() and w[sto + ord("a")] and w[sto + ord("_")] and w[sto + ord("9")] and w[sto + 0x4E2D]
    assert not w[sto + ord(" ")] and not w[sto + ord("-")] and not w[sto + ord(".")] and w[sto + 0xD800] and w[sto + 0xDFFF]
    assert (np.flatnonzero(np.unpackbits(bt.word_mask.view(np.uint8), bitorder="little")) == np.flatnonzero(w)).all()
    assert not w[bt.eos] and not w[bt.pad]


def test_compiler_refusals_and_limits(tok):
    V = tok.vocab_size
    with pytest.raises(ValueError, match="at least one"):
        compile_boost(tok, [], V)
    with pytest.raises(ValueError, match="list 1 is empty"):
        compile_boost(tok, [["a"], []], V)
    with pytest.raises(ValueError, match="entry 2 is the empty string"):
        compile_boost(tok, [["a", "b", ""]], V)
    with pytest.raises(ValueError, match="not a str"):
        compile_boost(tok, [["a", 5]], V)
    with pytest.raises(ValueError, match=r"entry 1 \('中文'\)"):
        compile_boost(tok, [["ok", "中文"]], tok.special_token_offset + 1024)
    with pytest.raises(ValueError, match="more than 40 automaton states"):
        compile_boost(tok, [STATES], V, max_states=40)
    with pytest.raises(ValueError, match="more than 100 automaton edges"):
        compile_boost(tok, [STATES], V, max_edges=100)
    from surya_amd.recognition.lexicon import SA_MAX_LEXICON_EDGES, SA_MAX_LEXICON_STATES
    assert (SA_MAX_LEXICON_STATES, SA_MAX_LEXICON_EDGES) == (L.SA_MAX_LEXICON_STATES, L.SA_MAX_LEXICON_EDGES)


def test_fifty_thousand_entries_compile_inside_the_limits(tok):
    rng = random.Random(3)
    big = ["".join(rng.choice(string.ascii_lowercase) for _ in range(rng.randint(5, 12))) for _ in range(49000)]
    big += [rng.choice(big)[:5].capitalize() + " " + "".join(rng.choice(string.ascii_lowercase) for _ in range(6)) for _ in range(1000)]
    t0 = time.perf_counter()
    bt = compile_boost(tok, [big], tok.vocab_size)
    print(f"50 000 entries: {time.perf_counter() - t0:.2f} s, {bt.n_states} states, {bt.n_edges} edges")
    assert bt.n_states <= L.SA_MAX_LEXICON_STATES and bt.n_edges <= L.SA_MAX_LEXICON_EDGES
    first = {}
    for i, e in enumerate(big):
        first.setdefault(e, i)
    for i in rng.sample(range(50000), 100):
        assert first[big[i]] in bt.matches(bt.roots[0], ids_of(tok, "x, " + big[i] + "."))
    with pytest.raises(ValueError, match=f"more than {bt.n_states - 1} automaton states"):
        compile_boost(tok, [big], tok.vocab_size, max_states=bt.n_states - 1)
    with pytest.raises(ValueError, match=f"more than {bt.n_edges - 1} automaton edges"):
        compile_boost(tok, [big], tok.vocab_size, max_edges=bt.n_edges - 1)


# ------------------------------------------------------------------------------------------------------------------ boost_core.h
def test_the_core_compiled_for_the_host_against_float64():
    rng = np.random.default_rng(11)
    rec = br.edge_records(rng, 20000)
    maxA, idxA, sumA, maxB, idxB, sumB, beta = rec
    # every corner is in the set
    assert (maxA == -np.inf).sum() > 100 and all((beta == b).sum() > 100 for b in (0.0, 1.5, 80.0, np.inf))
    fin = np.isfinite(beta) & np.isfinite(maxA)
    tie = fin & (np.where(fin, maxA, 0) + np.where(fin, beta, 0) == maxB)
    assert (tie & (idxA < idxB)).sum() > 100 and (tie & (idxA > idxB)).sum() > 100 and (np.isfinite(maxA) & (idxA == idxB)).sum() > 100
    token, tot, ptok, pprob = br.native_combine(*rec)
    r_token, r_tot, r_ptok, r_pprob = br.ref_combine(*rec)
    assert (token == r_token).all() and (ptok == r_ptok).all()
    e_tot, e_pp = np.abs(tot / r_tot - 1).max(), np.abs(pprob / r_pprob - 1).max()
    print(f"boost_core.h against float64: tot rel {e_tot:.3g}, plain_prob rel {e_pp:.3g}")
    assert e_tot <= 2e-3 and e_pp <= 2e-3
    assert np.isfinite(tot).all() and (tot > 0).all() and np.isfinite(pprob).all()
    # the named rules: empty S is the unmasked row; +inf is record A alone; 0 gives the unmasked token; the tie goes to the lower id
    e = maxA == -np.inf
    assert (token[e] == idxB[e]).all() and (tot[e] == sumB[e]).all()
    i = (beta == np.inf) & ~e
    assert (token[i] == idxA[i]).all() and (tot[i] == sumA[i]).all()
    z = (beta == 0) & ~e
    assert (token[z] == np.where((maxA[z] == maxB[z]) & (idxA[z] < idxB[z]), idxA[z], idxB[z])).all()
    assert (token[tie] == np.minimum(idxA[tie], idxB[tie])).all()
    big = (beta == 80) & ~e & (maxA + 80 > maxB)
    assert (token[big] == idxA[big]).all() and big.sum() > 100


# ------------------------------------------------------------------------------------------------------------------ the device loop
class BoostFakeModel(PatternFakeModel):
    """The pattern fake plus the boost entry points, with their contracts: tables only behind a mask table that holds their word row;
    roots and beta only while boosting is on, for slots whose mask ids were set for this prefill, before the prefill; the boost outputs
    of exactly the steps whose outputs were read."""

    def __init__(self, max_slots):
        super().__init__(max_slots)
        self.boost_calls, self.slot_root, self.line_root_seen, self.pending_root, self.betas = [], {}, {}, {}, set()
        self.last = None

    def set_boost(self, tables):
        assert not self.inflight and self.prefill_out is None
        assert tables is None or (self.tables and self.tables[-1] is not None and tables.word_row < len(self.tables[-1])), \
            "SA_ERR_STATE: boost tables without a mask table that holds their word row"
        self.boost_calls.append(tables)
        self.events.append("boost" if tables is not None else "boost off")
        self.slot_root = {}

    def set_slot_masks(self, slots, ids):
        super().set_slot_masks(slots, ids)
        for s in slots:
            self.slot_root[s] = -1                                           # a slot given a mask id is not boosted any more

    def set_slot_boost(self, slots, roots, betas):
        assert self.boost_calls and self.boost_calls[-1] is not None, "SA_ERR_STATE: roots while boosting is off"
        assert not self.inflight and len(slots) == len(roots) == len(set(slots))
        self.betas.add(float(betas))
        for s, r in zip(slots, roots):
            assert s not in self.active and -1 <= r < self.boost_calls[-1].n_states
            assert self.pending.get(s), "roots go behind the slot's mask id"
            self.slot_root[s] = r
            self.pending_root[s] = True

    def prefill(self, tiles, grid_hw, input_ids, slot_ids):
        if self.boost_calls and self.boost_calls[-1] is not None:
            for s in slot_ids:
                assert self.pending_root.pop(s, False), "a slot was prefilled without its root being set first"
        super().prefill(tiles, grid_hw, input_ids, slot_ids)
        for ids, s in zip(input_ids, slot_ids):
            self.line_root_seen[ids[0] - 1000] = self.slot_root.get(s, -1)

    def read_outputs(self, n):
        self.last = super().read_outputs(n)
        return self.last

    def wait_outputs(self, n, ring):
        self.last = super().wait_outputs(n, ring)
        return self.last

    def _boost_of(self):
        assert self.boost_calls and self.boost_calls[-1] is not None and self.last is not None, "boost outputs without their step outputs"
        tok, sc, _ = self.last
        self.last = None
        return tok + 1, sc * 0.5                                             # plain token = token + 1, plain probability = score / 2

    def read_boost(self, n):
        assert n == 1
        return self._boost_of()

    def wait_boost(self, n, ring):
        return self._boost_of()


def _fake_boost(n_states=9):
    return SimpleNamespace(n_states=n_states, word_row=2)


@pytest.mark.parametrize("n_lines,max_tokens,slots,sps,ahead", [(23, 12, 4, 4, True), (40, 6, 7, 1, False)])
def test_roots_reach_the_prefilled_slots_and_boosting_is_switched_off(n_lines, max_tokens, slots, sps, ahead):
    old = (settings.RECOGNITION_STEPS_PER_SYNC, settings.RECOGNITION_ENCODE_AHEAD)
    settings.RECOGNITION_STEPS_PER_SYNC, settings.RECOGNITION_ENCODE_AHEAD = sps, ahead
    done = {}
    try:
        pred, prep = make(n_lines, max_tokens, slots)
        pred.model = BoostFakeModel(slots)
        tables = _fake_boost()
        want_root = [(i % 4) * 2 if i % 4 else -1 for i in range(n_lines)]                   # -1, 2, 4, 6: reused slots change kind
        want_mask = [0 if r < 0 and i % 8 == 0 else -1 for i, r in enumerate(want_root)]
        prep.update(token_masks=np.ones((3, 5), np.uint32), mask_ids=want_mask, boost_tables=tables, boost_weight=2.5, boost_roots=want_root)
        toks, _, scores = pred.generate(prep, slots, on_done=lambda k, t, s, b, *more: done.__setitem__(k, (list(t), list(s), more)))
    finally:
        settings.RECOGNITION_STEPS_PER_SYNC, settings.RECOGNITION_ENCODE_AHEAD = old
    m = pred.model
    assert m.events == ["masks", "boost", "boost off", "masks off"] and m.boost_calls[0] is tables and m.betas == {2.5}
    assert [m.line_root_seen[i] for i in range(n_lines)] == want_root
    assert [m.line_mask_seen[i] for i in range(n_lines)] == want_mask
    assert n_lines > slots and len(done) == n_lines
    for i in range(n_lines):
        assert toks[i] == expected(i, prep["max_tokens"][i])                                # scheduling is what it was
        t, s, more = done[i]
        assert len(more) == 2 and more[0].tolist() == [x + 1 for x in t] and more[1].tolist() == pytest.approx([x * 0.5 for x in s])
    ptok, pprob = pred.last_boost                                                           # the dense arrays, for the sharded gather
    assert ptok[3] == [x + 1 for x in toks[3]] and len(pprob) == n_lines


def test_fed_chunks_carry_their_roots():
    from surya_amd.recognition.loop import FEED_END
    from test_scheduler_cpu import _chunks
    pred, prep = make(20, 8, 4)
    pred.model = BoostFakeModel(4)
    want = [(i % 3) - 1 for i in range(20)]
    chunks = _chunks(prep, [0, 7, 12, 20])
    for ch in chunks:
        ch["boost_roots"] = [want[p.id] for p in ch["prompts"]]
    feed_items = chunks + [FEED_END]
    first = {"prompts": [], "max_tokens": {}, "overall_max_tokens": 8, "token_masks": np.ones((3, 4), np.uint32), "boost_tables": _fake_boost(2),
             "boost_weight": 1.0}
    pred.generate(first, 4, feed=lambda block: feed_items.pop(0))
    assert [pred.model.line_root_seen[i] for i in range(20)] == want
    assert pred.model.events == ["masks", "boost", "boost off", "masks off"]


def test_a_failed_loop_still_switches_boosting_off_and_a_plain_call_never_calls_it():
    pred, prep = make(6, 6, 4)
    pred.model = BoostFakeModel(4)

    def boom(n, ring):
        raise RuntimeError("device lost")
    pred.model.decode_async = boom
    prep.update(token_masks=np.ones((3, 4), np.uint32), mask_ids=[-1] * 6, boost_tables=_fake_boost(), boost_weight=1.0, boost_roots=[1] * 6)
    with pytest.raises(RuntimeError):
        pred.generate(prep, 4)
    assert pred.model.events == ["masks", "boost", "boost off", "masks off"]
    # masks without boosting, on a model object that has no boost entry points at all
    pred, prep = make(6, 6, 4)
    pred.model = PatternFakeModel(4)
    assert not hasattr(pred.model, "set_boost") and not hasattr(pred.model, "read_boost")
    prep.update(token_masks=np.ones((1, 4), np.uint32), mask_ids=[0] * 6)
    pred.generate(prep, 4)
    assert pred.model.events == ["masks", "masks off"]
    pred, prep = make(6, 6, 4)
    pred.model = BoostFakeModel(4)
    pred.generate(prep, 4)
    assert pred.model.events == [] and not pred.model.boost_calls
    # roots without tables are a caller's bug, and so is boosting beside a mode it excludes
    pred, prep = make(5, 6, 4)
    prep["boost_roots"] = [0, -1, 0, -1, 0]
    with pytest.raises(AssertionError):
        pred.generate(prep, 4)
    from test_pattern_cpu import _fake_tables
    pred, prep = make(5, 6, 4)
    pred.model = BoostFakeModel(4)
    prep.update(token_masks=np.ones((3, 4), np.uint32), boost_tables=_fake_boost(), boost_weight=1.0, pattern_tables=_fake_tables())
    with pytest.raises(AssertionError, match="excludes"):
        pred.generate(prep, 4)
    assert pred.model.events == []


# ------------------------------------------------------------------------------------------------------------------ assembly
def test_assembly_sets_boost_matches_and_the_plain_reading():
    """assemble_batch and assemble_line on hand-made streams: boost_matches from the host replay, plain / plain_confidence from the
    token every character takes its confidence from; None -- and absent from the serialised form -- on a line that was not boosted."""
    from surya_amd.recognition.predictor import RecognitionPredictor
    from surya_amd.recognition.processor import SuryaOCRProcessor
    tk = OCRTokenizer(None, None, reserve_special=64)
    proc = SuryaOCRProcessor(tk)
    pred = object.__new__(RecognitionPredictor)
    pred.processor = proc
    bt = compile_boost(tk, [["Boston", "Austin", "Bo"], ["Austin"]], tk.vocab_size)
    eos = proc.eos_token_id
    streams = [ids_of(tk, "in Austin") + [eos], ids_of(tk, "Boston Bo") + [eos], ids_of(tk, "Bost"), [proc.no_output_token],
               ids_of(tk, "Austin") + [eos], ids_of(tk, "Austin, Boston") + [eos]]
    roots = [bt.roots[0], bt.roots[0], bt.roots[0], bt.roots[0], -1, bt.roots[1]]
    want = [[1], [2, 0], [2], [], None, [0]]
    n = len(streams)
    flat = {"polygons": [[7, 9, 300, 52]] * n, "res_scales": [(1.0, 1.0)] * n, "slices": [np.zeros((40, 300, 3), np.uint8)] * n,
            "boost_tables": bt, "boost_roots": roots, "boost_weight": 3.0}
    items = []
    for i, toks in enumerate(streams):
        rows = np.sort(np.random.default_rng(i).integers(0, 1025, size=(len(toks), 6)), axis=0).astype(np.float32)
        plain = np.asarray(toks, np.int32).copy()
        if len(plain) > 2:
            plain[2] = ids_of(tk, "Q")[0]                                                    # the model alone would have read a Q there
        items.append((i, i, toks, [0.5] * len(toks), rows, (plain, np.linspace(0.1, 0.4, len(toks)).astype(np.float32))))
    got = pred._assemble_batch(flat, items, False, False, 1025)
    assert [g.boost_matches for g in got] == want
    assert [g.text for g in got] == ["in Austin", "Boston Bo", "Bost", "", "Austin", "Austin, Boston"]
    from surya_amd.recognition import assemble
    for it, g in zip(items, got):
        ref = assemble.assemble_line(proc, flat, *it[:5], False, False, 1025, alts=it[5])
        assert g.model_dump() == ref.model_dump() and g.model_fields_set == ref.model_fields_set
        assert [c.model_fields_set for c in g.chars] == [c.model_fields_set for c in ref.chars]
    a = got[0]
    assert [c.plain for c in a.chars] == list("inQAustin") and a.text == "in Austin"
    assert [c.plain_confidence for c in a.chars] == pytest.approx(np.linspace(0.1, 0.4, 10)[:9].tolist())
    assert all(c.alternatives is None and "alternatives" not in c.model_fields_set for g in got for c in g.chars)
    assert all(c.plain is None and c.plain_confidence is None for c in got[4].chars) and got[4].boost_matches is None
    d = got[4].model_dump()
    assert "boost_matches" not in d and all("plain" not in c and "plain_confidence" not in c for c in d["chars"])
    d = got[0].model_dump()
    assert d["boost_matches"] == [1] and d["chars"][2]["plain"] == "Q" and d["chars"][2]["plain_confidence"] == pytest.approx(0.1 + 0.3 * 2 / 9)
    assert got[3].boost_matches == [] and got[3].model_dump()["boost_matches"] == []
    bare = {k: v for k, v in flat.items() if not k.startswith("boost_")}
    plain = pred._assemble_batch(bare, [it[:5] for it in items], False, False, 1025)
    assert all(p.boost_matches is None and all(c.plain is None for c in p.chars) for p in plain)
    strip = lambda d: {**{k: v for k, v in d.items() if k != "boost_matches"},
                       "chars": [{k: v for k, v in c.items() if k not in ("plain", "plain_confidence")} for c in d["chars"]]}
    assert [p.model_dump() for p in plain] == [strip(g.model_dump()) for g in got]


def test_schema_leaves_absent_boost_fields_out():
    from surya_amd.recognition.schema import TextChar, TextLine
    ln = TextLine(text="x", polygon=[[0, 0], [1, 0], [1, 1], [0, 1]], confidence=0.5, chars=[])
    assert ln.boost_matches is None and "boost_matches" not in ln.model_dump()
    ln.boost_matches = []
    assert ln.model_dump()["boost_matches"] == []
    ch = TextChar(text="x", polygon=[[0, 0], [1, 0], [1, 1], [0, 1]], confidence=0.5)
    assert ch.plain is None and ch.plain_confidence is None and not {"plain", "plain_confidence"} & set(ch.model_dump())
    ch.plain, ch.plain_confidence = "y", 0.25
    assert ch.model_dump()["plain"] == "y" and ch.model_dump()["plain_confidence"] == 0.25
    assert "plain" in TextChar.model_json_schema()["properties"] and "boost_matches" in TextLine.model_json_schema()["properties"]


# ------------------------------------------------------------------------------------------------------------------ the predictor
DRUGS, NAMES = ["Paracetamol", "Ibuprofen"], ["Smith", "Jones", "Smith"]


def test_argument_forms_and_exclusions(tok):
    V = tok.vocab_size
    c = LineConstraints(tok, None, None, 3, [2, 0, 1], vocab_size=V, limit=64, boost_words=DRUGS)       # one list of str: every line
    r = c.boost.roots[0]
    assert c.line_boost_roots([2, 0, 1]) == [r, r, r] and c.line_ids([2, 0, 1]) == [-1, -1, -1] and c
    assert len(c.table) == 1 and c.boost.word_row == 0 and (c.table.array()[0] == c.boost.word_mask).all()     # the mask table holds the word row
    c = LineConstraints(tok, [None, "01", [None, "ab", None, None]], None, 3, [1, 2, 4], vocab_size=V, limit=64,
                        boost_words=[DRUGS, None, [NAMES, None, None, tuple(DRUGS)]])
    a, b = c.boost.roots
    assert c.line_boost_roots([1, 2, 4]) == [a, -1, -1, b, -1, -1, a] and c.line_ids([1, 2, 4]) == [-1, 0, 0, -1, 1, -1, -1]
    assert len(c.boost.roots) == 2 and c.boost.word_row == 2 and len(c.table) == 3                             # equal lists are compiled once
    assert LineConstraints(tok, "01", None, 2, None, vocab_size=V).boost is None                                # no list: nothing is compiled
    assert not LineConstraints(tok, None, None, 2, [1, 1], vocab_size=V, boost_words=[None, None])
    c = LineConstraints(tok, None, None, 2, None, vocab_size=V, boost_words=[DRUGS, None])                     # per image works without known lines
    assert c.line_boost_roots([4, 2]) == [c.boost.roots[0]] * 4 + [-1, -1]
    with pytest.raises(ValueError, match="not known yet"):
        LineConstraints(tok, None, None, 2, None, vocab_size=V, boost_words=[[DRUGS], None])
    for kw in (dict(allowlist="01"), dict(blocklist="01")):
        with pytest.raises(ValueError, match="takes no allowlist"):
            LineConstraints(tok, kw.get("allowlist"), kw.get("blocklist"), 1, [1], vocab_size=V, boost_words=DRUGS)
    with pytest.raises(ValueError, match="line 1: .*takes no allowlist"):
        LineConstraints(tok, [[None, "01"]], None, 1, [2], vocab_size=V, boost_words=[[DRUGS, DRUGS]])
    for kw in (dict(pattern=r"\d+"), dict(lexicon=NAMES)):
        with pytest.raises(ValueError, match="not available with pattern or lexicon"):
            LineConstraints(tok, None, None, 1, [1], vocab_size=V, boost_words=DRUGS, **kw)
    with pytest.raises(ValueError, match="has 3 lines"):
        LineConstraints(tok, None, None, 1, [3], vocab_size=V, boost_words=[[DRUGS, None]])
    with pytest.raises(ValueError, match="2 entries for 1 images"):
        LineConstraints(tok, None, None, 1, [1], vocab_size=V, boost_words=[None, DRUGS])
    for bad in (5, "Aspirin", [None, 5], [[DRUGS, "x"]]):
        with pytest.raises(TypeError, match="boost_words"):
            LineConstraints(tok, None, None, len(bad) if isinstance(bad, list) else 1, [2, 2][: len(bad) if isinstance(bad, list) else 1],
                            vocab_size=V, boost_words=bad)
    with pytest.raises(ValueError, match="empty"):
        LineConstraints(tok, None, None, 1, [1], vocab_size=V, boost_words=[])
    with pytest.raises(ValueError, match="empty string"):
        LineConstraints(tok, None, None, 1, [1], vocab_size=V, boost_words=["a", ""])


def test_predictor_validates_before_any_device_work():
    from PIL import Image
    from surya_amd.recognition.predictor import RecognitionPredictor
    pred = object.__new__(RecognitionPredictor)
    cfg = rec_config("REC-TINY")
    pred.processor = RecognitionModelLoader({"config": cfg, "state_dict": {}}).processor()
    pred.model = SimpleNamespace(vocab=cfg.decoder.vocab_size)
    pred.shard_lines = pred.shard_pages = False
    pred.process_group = None
    assert RecognitionPredictor.boost_words is None and RecognitionPredictor.boost_weight is None
    img, box = Image.new("RGB", (64, 32)), [[[0, 0, 10, 10]]]
    pred.boost_words = DRUGS
    with pytest.raises(ValueError, match="needs boost_weight"):                              # required, no default
        pred([img], bboxes=box)
    for bad in (-1.0, float("inf"), float("nan"), "3", True):
        pred.boost_weight = bad
        with pytest.raises(ValueError, match="finite float >= 0"):
            pred([img], bboxes=box)
    pred.boost_weight = 3.0
    for name, value in (("top_k", 2), ("beam_width", 2), ("pattern", r"\d+"), ("lexicon", NAMES)):
        setattr(pred, name, value)
        with pytest.raises(ValueError, match=f"not available with {name}"):
            pred([img], bboxes=box)
        setattr(pred, name, None)
    with pytest.raises(ValueError, match="align"):
        pred.align([img], [["1"]], bboxes=box)
    with pytest.raises(ValueError, match="takes no allowlist"):
        pred([img], bboxes=box, allowlist="01")
    with pytest.raises(ValueError, match="takes no allowlist"):
        pred([img], bboxes=box, blocklist="01")
    pred.boost_words = [[DRUGS]]
    with pytest.raises(ValueError, match="not known yet"):
        pred([img], det_predictor=object())
    pred.boost_words = []
    with pytest.raises(ValueError, match="empty"):
        pred([img], bboxes=box)
    pred.boost_words = ["ok", ""]
    with pytest.raises(ValueError, match="empty string"):
        pred([img], bboxes=box)
    pred.boost_words = ["ok", "中文"]
    with pytest.raises(ValueError, match="中文"):                                    # REC-TINY's 1024 ids cannot write it
        pred([img], bboxes=box)


@pytest.mark.parametrize("rank", [0, 1])
def test_shard_lines_deals_the_roots_with_the_lines_and_gathers_the_plain_reading(monkeypatch, rank):
    import torch
    from surya_amd import dist as sdist
    from surya_amd.recognition.predictor import RecognitionPredictor
    n, world = 7, 2
    monkeypatch.setattr(sdist, "collectives_on", lambda group=None: True)
    monkeypatch.setattr(sdist, "world_info", lambda group=None: (rank, world))
    monkeypatch.setattr(sdist, "collective_device", lambda dev, group=None: "cpu")
    monkeypatch.setattr(sdist, "assert_same_inputs", lambda *a, **k: None)
    sent = {}

    def gather(toks, scores, boxes, mine, n_total, max_tokens, alts=None, **k):
        sent["alts"] = alts
        return toks, scores, boxes, alts[0], alts[1]
    monkeypatch.setattr(sdist, "gather_line_outputs", gather)
    pred = object.__new__(RecognitionPredictor)
    pred.model = SimpleNamespace(device="cpu")
    pred.process_group = None
    seen = {}

    def loop(local, rbs, math_mode):
        seen.update(local)
        m = len(local["slices"])
        lens = np.full(m, 2, np.int64)
        pred.last_boost = (sdist.PackedLines(np.arange(m * 9, dtype=np.int32).reshape(m, 9), lens),
                           sdist.PackedLines(np.full((m, 9), 0.25, np.float32), lens))
        return [[5, 6]] * m, torch.zeros((m, 6, 6)), [[0.5, 0.5]] * m
    pred.prediction_loop = loop
    tables = _fake_boost()
    roots = [(i % 3) - 1 for i in range(n)]
    flat = {"slices": [np.zeros((4, 10 + i, 3), np.float32) for i in range(n)], "input_text": [None] * n, "task_names": ["ocr_with_boxes"] * n,
            "token_masks": np.ones((3, 3), np.uint32), "mask_ids": [-1] * n, "boost_tables": tables, "boost_weight": 2.0, "boost_roots": roots}
    pred.sharded_prediction_loop(flat, 4, True)
    mine = list(range(rank, n, world))
    assert seen["boost_roots"] == [roots[i] for i in mine] and seen["boost_tables"] is tables and seen["boost_weight"] == 2.0
    assert sent["alts"][0].data.shape == (len(mine), 9, 1) and sent["alts"][1].data.dtype == np.float32      # one "alternative" per token
    ptok, pprob = pred.last_boost
    assert ptok.data.shape == (len(mine), 9) and ptok[1] == [9, 10] and pprob[0] == [0.25, 0.25]
    seen.clear()
    for k in ("boost_tables", "boost_weight", "boost_roots"):
        del flat[k]
    monkeypatch.setattr(sdist, "gather_line_outputs", lambda toks, scores, boxes, mine, n_total, max_tokens, **k: (toks, scores, boxes))
    pred.sharded_prediction_loop(flat, 4, True)
    assert not any(k.startswith("boost_") for k in seen) and "mask_ids" in seen


def test_page_sharded_call_slices_per_image_boost_words(monkeypatch):
    from PIL import Image
    from surya_amd import dist as sdist
    from surya_amd.recognition.predictor import RecognitionPredictor
    from surya_amd.recognition.schema import OCRResult
    monkeypatch.setattr(sdist, "world_info", lambda group=None: (1, 2))
    monkeypatch.setattr(sdist, "collective_device", lambda dev, group=None: "cpu")
    monkeypatch.setattr(sdist, "assert_same_inputs", lambda *a, **k: None)
    monkeypatch.setattr(sdist, "gather_objects", lambda local, mine, n, group=None: list(local))
    pred = object.__new__(RecognitionPredictor)
    pred.model = SimpleNamespace(device="cpu")
    pred.process_group, pred.shard_pages, pred.shard_lines = None, True, False
    got = {}

    def rank_call(images, *a, **kw):
        got["n"], got["kw"] = len(images), kw
        return [OCRResult(text_lines=[], image_bbox=[0, 0, 1, 1]) for _ in images]
    pred._call = rank_call
    pages = [Image.new("RGB", (8 + i, 8)) for i in range(5)]
    args = (pages, ["ocr_with_boxes"] * 5, SimpleNamespace(), None, None, [None] * 5, False, True, False, False)
    pred._call_page_sharded(*args, boost_words=[DRUGS, None, ["c"], NAMES, None], boost_weight=4.0)
    assert got["n"] == 2 and got["kw"] == {"boost_words": [None, NAMES], "boost_weight": 4.0}
    pred._call_page_sharded(*args, allowlist=None, blocklist="xy", boost_words=DRUGS, boost_weight=1.0)
    assert got["kw"] == {"allowlist": [None, None], "blocklist": ["xy", "xy"], "boost_words": [DRUGS, DRUGS], "boost_weight": 1.0}
    pred._call_page_sharded(*args)
    assert got["kw"] == {}
