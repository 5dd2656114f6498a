"""Lexicon-guided decoding, host side (no GPU): the lexicon compiler (recognition/lexicon.py) -- the automaton accepts exactly the entries,
is minimal where it must be, its limits and refusals --; the device loop's contract with the model (on the fake of
tests/test_scheduler_cpu.py); lexicon_index from assembly; the predictor's argument forms; start states through shard_lines and the
page-sharded call."""
import random
import string
import time
from types import SimpleNamespace

import numpy as np
import pytest

from surya_amd import _lib as L
from surya_amd.config import rec_config
from surya_amd.recognition.lexicon import SA_MAX_LEXICON_EDGES, SA_MAX_LEXICON_STATES, compile_lexicons
from surya_amd.recognition.loader import RecognitionModelLoader
from surya_amd.recognition.predictor import LineConstraints
from surya_amd.recognition.tokenizer import OCRTokenizer
from surya_amd.settings import settings

from test_pattern_cpu import PatternFakeModel, _fake_tables
from test_scheduler_cpu import expected, make

STATES = ["Alabama", "Alaska", "Arizona", "Arkansas", "California", "Colorado", "Connecticut", "Delaware", "Florida", "Georgia", "Hawaii", "Idaho",
          "Illinois", "Indiana", "Iowa", "Kansas", "Kentucky", "Louisiana", "Maine", "Maryland", "Massachusetts", "Michigan", "Minnesota",
          "Mississippi", "Missouri", "Montana", "Nebraska", "Nevada", "New Hampshire", "New Jersey", "New Mexico", "New York", "North Carolina",
          "North Dakota", "Ohio", "Oklahoma", "Oregon", "Pennsylvania", "Rhode Island", "South Carolina", "South Dakota", "Tennessee", "Texas",
          "Utah", "Vermont", "Virginia", "Washington", "West Virginia", "Wisconsin", "Wyoming"]
_r1 = random.Random(1)
WORDS200 = ["".join(_r1.choice(string.ascii_lowercase) for _ in range(_r1.randint(4, 9))) for _ in range(200)]      # the pattern compiler refuses it
SHARED = ["tested", "rested", "nested", "testing", "resting", "nesting", "test", "rest", "nest", "tester", "Tested"]   # shared prefixes and tails
PREFIXES = ["a", "ab", "abc", "abcd", "b", "ba", "New", "New York", "New Yorker"]                                     # entries that are prefixes of entries
LISTS = {"states": STATES, "words200": WORDS200, "shared": SHARED, "prefixes": PREFIXES}
SMILE = "\U0001F600"


@pytest.fixture(scope="module")
def tok():
    return OCRTokenizer()


def units(s):
    raw = s.encode("utf-16le", "surrogatepass")
    return [raw[i] + (raw[i + 1] << 8) for i in range(0, len(raw), 2)]


def ids_of(tok, s):
    return [tok.special_token_offset + u for u in units(s)]


def walk(lt, start, ids):
    """The state after `ids` from `start`, or None where an id has no edge."""
    st = start
    for t in ids:
        ns = lt.advance(st, t)
        if ns == st:
            return None
        st = ns
    return st


def trie_nodes(entries):
    return 1 + len({e[:k] for e in entries for k in range(1, len(e) + 1)})


# ------------------------------------------------------------------------------------------------------------------ the compiler
@pytest.mark.parametrize("name", list(LISTS))
def test_the_automaton_accepts_exactly_the_entries(tok, name):
    entries = LISTS[name]
    lt = compile_lexicons(tok, [entries], tok.vocab_size)
    s0, eos = lt.starts[0], lt.eos
    assert lt.n_states == len(lt.state_flags) == len(lt.edge_off) - 1 and lt.n_edges == len(lt.edge_tok) == len(lt.edge_next) == lt.edge_off[-1]
    assert lt.edge_off.dtype == lt.edge_tok.dtype == lt.edge_next.dtype == np.int32 and lt.state_flags.dtype == np.uint8
    for i, e in enumerate(entries):                                          # every entry, with its first index
        assert lt.entry_of(0, ids_of(tok, e) + [eos]) == entries.index(e), e
        assert lt.entry_of(0, ids_of(tok, e)) == -1                          # cut by the token budget: no eos
        assert lt.accepts(walk(lt, s0, ids_of(tok, e)))
    have = set(entries)
    for e in entries:                                                        # every proper prefix that is no entry is not terminal
        for k in range(1, len(e)):
            st = walk(lt, s0, ids_of(tok, e[:k]))
            assert st is not None and lt.accepts(st) == (e[:k] in have), (e, k)
            assert lt.entry_of(0, ids_of(tok, e[:k]) + [eos]) == (entries.index(e[:k]) if e[:k] in have else -1)
    assert not lt.accepts(s0) and lt.entry_of(0, [eos]) == -1
    rng = random.Random(7)
    alphabet = sorted(set("".join(entries)))
    rejected = 0
    while rejected < 1000:                                                   # 1000 random non-entries over the same alphabet
        base = rng.choice(entries)
        w = list(base[: rng.randint(1, len(base))] if rng.random() < 0.5 else rng.choices(alphabet, k=rng.randint(1, 10)))
        if rng.random() < 0.7:
            w[rng.randrange(len(w))] = rng.choice(alphabet)
        if rng.random() < 0.3:
            w.append(rng.choice(alphabet))
        w = "".join(w)
        if w in have:
            continue
        st = walk(lt, s0, ids_of(tok, w))
        assert st is None or not lt.accepts(st), w
        assert lt.entry_of(0, ids_of(tok, w) + [eos]) == -1
        rejected += 1
    for st in range(lt.n_states):                                            # allowed(state) = the children's ids plus the flag ids
        toks, nxt = lt.edges(st)
        want = set(toks.tolist())
        assert (np.diff(toks) > 0).all() and (nxt >= 0).all() and (nxt < lt.n_states).all()
        f = int(lt.state_flags[st])
        if f & 1:
            want |= {lt.eos, lt.pad}
        if f & 2:
            want.add(lt.nop)
        assert lt.allowed(st) == want and want, st
        assert set(np.flatnonzero(np.unpackbits(lt.row(st).view(np.uint8), bitorder="little")).tolist()) == want
    assert [int(s) for s in np.flatnonzero(lt.state_flags & 2)] == [s0]     # the no-output token at the start state only
    assert lt.n_states <= trie_nodes(entries) + 1                            # (+ 1: the start state is the root's copy and is never shared)


def test_the_pattern_compiler_refuses_what_the_lexicon_compiler_takes(tok):
    import re
    from surya_amd.recognition.pattern import compile_patterns
    with pytest.raises(ValueError, match="more than 64 distinct"):
        compile_patterns(tok, ["|".join(map(re.escape, WORDS200))], tok.vocab_size)
    assert compile_lexicons(tok, [WORDS200], tok.vocab_size).n_states > 64


def test_equal_tails_and_equal_lexicons_share_states(tok):
    lt = compile_lexicons(tok, [["ab", "cb"]], tok.vocab_size)
    s0 = lt.starts[0]
    a, c = walk(lt, s0, ids_of(tok, "a")), walk(lt, s0, ids_of(tok, "c"))
    assert a == c and lt.n_states == 3                                       # leaf, the shared "b" state, the start
    shared = compile_lexicons(tok, [SHARED], tok.vocab_size)
    assert shared.n_states < trie_nodes(SHARED) - 10
    # two equal lexicons in one call share everything but the start-state copy; a third one shares its tails
    one = compile_lexicons(tok, [STATES], tok.vocab_size)
    two = compile_lexicons(tok, [STATES, list(STATES), ["Utah", "Idaho", "Ohio"]], tok.vocab_size)
    assert two.n_states <= one.n_states + 2 + 3 and two.starts[0] != two.starts[1]
    assert [t.tolist() for t in two.edges(two.starts[0])] == [t.tolist() for t in two.edges(two.starts[1])]
    for k, lex in enumerate([STATES, STATES, ["Utah", "Idaho", "Ohio"]]):
        for i, e in enumerate(lex):
            assert two.entry_of(k, ids_of(tok, e) + [two.eos]) == i
    assert two.entry_of(2, ids_of(tok, "Texas") + [two.eos]) == -1           # a start state of its own: its lexicon, no other


def test_duplicates_surrogates_and_verbatim_entries(tok):
    lt = compile_lexicons(tok, [["b", "a", "b", "a" + SMILE, " a", "A", "é", "é"]], tok.vocab_size)
    eos, pad = lt.eos, lt.pad
    assert lt.entry_of(0, ids_of(tok, "b") + [eos]) == 0 and lt.entry_of(0, ids_of(tok, "b") + [pad]) == 0      # first index; ended by pad
    ids = ids_of(tok, "a" + SMILE)
    assert len(ids) == 3 and ids[1] - tok.special_token_offset == 0xD83D      # a non-BMP entry: high surrogate, then low: two edges
    assert lt.entry_of(0, ids + [eos]) == 3 and lt.entry_of(0, ids[:2] + [eos]) == -1
    assert [lt.entry_of(0, ids_of(tok, e) + [eos]) for e in (" a", "A", "é", "é", "a ", "E")] == [4, 5, 6, 7, -1, -1]    # no folding, no NFC, no strip
    assert lt.entry_of(0, [lt.nop]) == -1 and lt.advance(lt.starts[0], lt.nop) == lt.starts[0]
    assert lt.advance(-1, ids[0]) == -1 and lt.advance(lt.starts[0], eos) == lt.starts[0] and not lt.accepts(-1)
    assert lt.advance(lt.starts[0], 0x7fffffff) == lt.starts[0]


def test_refusals_and_limits(tok):
    V = tok.vocab_size
    with pytest.raises(ValueError, match="at least one"):
        compile_lexicons(tok, [], V)
    with pytest.raises(ValueError, match="lexicon 1 is empty"):
        compile_lexicons(tok, [["a"], []], V)
    with pytest.raises(ValueError, match="entry 2 is the empty string"):
        compile_lexicons(tok, [["a", "b", ""]], V)
    with pytest.raises(ValueError, match="not a str"):
        compile_lexicons(tok, [["a", 7]], V)
    cfg = rec_config("REC-TINY")                                             # 1024 ids: most of the BMP has none
    tk = RecognitionModelLoader({"config": cfg, "state_dict": {}}).processor().ocr_tokenizer
    small = compile_lexicons(tk, [["abc", "12"]], cfg.decoder.vocab_size)
    assert small.vocab == cfg.decoder.vocab_size and int(small.edge_tok.max()) < small.vocab
    with pytest.raises(ValueError, match=r"entry 1 \('中文'\)"):
        compile_lexicons(tk, [["abc", "中文"]], cfg.decoder.vocab_size)
    with pytest.raises(ValueError, match="more than 40 automaton states"):
        compile_lexicons(tok, [WORDS200], V, max_states=40)
    with pytest.raises(ValueError, match="more than 100 automaton edges"):
        compile_lexicons(tok, [WORDS200], V, max_edges=100)
    assert (SA_MAX_LEXICON_STATES, SA_MAX_LEXICON_EDGES) == (L.SA_MAX_LEXICON_STATES, L.SA_MAX_LEXICON_EDGES) == (1 << 20, 1 << 21)


def test_fifty_thousand_entries_compile_with_room(tok):
    rng = random.Random(3)
    big = ["".join(rng.choice(string.ascii_lowercase) for _ in range(rng.randint(5, 12))) for _ in range(50000)]
    t0 = time.perf_counter()
    lt = compile_lexicons(tok, [big], tok.vocab_size)
    print(f"50 000 entries: {time.perf_counter() - t0:.2f} s, {lt.n_states} states, {lt.n_edges} edges")
    assert 4 * lt.n_states <= SA_MAX_LEXICON_STATES and 4 * lt.n_edges <= SA_MAX_LEXICON_EDGES
    for i in rng.sample(range(50000), 200):
        assert lt.entry_of(0, ids_of(tok, big[i]) + [lt.eos]) == big.index(big[i])


# ------------------------------------------------------------------------------------------------------------------ the device loop
class LexiconFakeModel(PatternFakeModel):
    """The pattern fake plus the lexicon entry points, with their contracts: tables only behind a mask table; start states only while
    the lexicon is on, for slots whose mask ids were set for this prefill, before the prefill; a new mask table switches the lexicon off."""

    def __init__(self, max_slots):
        super().__init__(max_slots)
        self.lexicon_calls, self.slot_lex, self.line_lex_seen, self.pending_lex = [], {}, {}, {}

    def set_token_masks(self, masks):
        super().set_token_masks(masks)
        assert not (self.lexicon_calls and self.lexicon_calls[-1] is not None), "the mask table was replaced under a live lexicon"

    def set_lexicon(self, tables):
        assert not self.inflight and self.prefill_out is None
        assert tables is None or (self.tables and self.tables[-1] is not None), "SA_ERR_STATE: a lexicon without a mask table"
        self.lexicon_calls.append(tables)
        self.events.append("lexicon" if tables is not None else "lexicon off")
        self.slot_lex = {}

    def set_slot_masks(self, slots, ids):
        super().set_slot_masks(slots, ids)
        for s in slots:
            self.slot_lex[s] = -1                                            # a slot given a mask id rewrites no row any more

    def set_slot_lexicon(self, slots, states):
        assert self.lexicon_calls and self.lexicon_calls[-1] is not None, "SA_ERR_STATE: start states while the lexicon is off"
        assert not self.inflight and len(slots) == len(states) == len(set(slots))
        for s, st in zip(slots, states):
            assert s not in self.active and -1 <= st < self.lexicon_calls[-1].n_states
            assert self.pending.get(s), "start states go behind the slot's mask id"
            self.slot_lex[s] = st
            self.pending_lex[s] = True

    def prefill(self, tiles, grid_hw, input_ids, slot_ids):
        if self.lexicon_calls and self.lexicon_calls[-1] is not None:
            for s in slot_ids:
                assert self.pending_lex.pop(s, False), "a slot was prefilled without its lexicon start state being set first"
        super().prefill(tiles, grid_hw, input_ids, slot_ids)
        for ids, s in zip(input_ids, slot_ids):
            self.line_lex_seen[ids[0] - 1000] = self.slot_lex.get(s, -1)


def _fake_lexicon(n_states=9):
    return SimpleNamespace(n_states=n_states)


@pytest.mark.parametrize("n_lines,max_tokens,slots,sps,ahead", [(23, 12, 4, 4, True), (40, 6, 7, 1, False)])
def test_start_states_reach_the_prefilled_slots_and_the_lexicon_is_switched_off(n_lines, max_tokens, slots, sps, ahead):
    old = (settings.RECOGNITION_STEPS_PER_SYNC, settings.RECOGNITION_ENCODE_AHEAD)
    settings.RECOGNITION_STEPS_PER_SYNC, settings.RECOGNITION_ENCODE_AHEAD = sps, ahead
    try:
        pred, prep = make(n_lines, max_tokens, slots)
        pred.model = LexiconFakeModel(slots)
        tables, ptables = _fake_lexicon(), _fake_tables()
        want_lex = [(i % 4) * 2 if i % 4 else -1 for i in range(n_lines)]                    # -1, 2, 4, 6: reused slots change kind
        want_state = [3 if s < 0 and i % 8 == 4 else -1 for i, s in enumerate(want_lex)]     # a pattern line here and there: never both
        want_mask = [0 if s < 0 and i % 8 == 0 else -1 for i, s in enumerate(want_lex)]
        prep.update(token_masks=np.ones((3, 5), np.uint32), mask_ids=want_mask, pattern_tables=ptables, start_states=want_state,
                    lexicon_tables=tables, lexicon_starts=want_lex)
        toks, _, _ = pred.generate(prep, slots)
    finally:
        settings.RECOGNITION_STEPS_PER_SYNC, settings.RECOGNITION_ENCODE_AHEAD = old
    m = pred.model
    assert m.events == ["masks", "patterns", "lexicon", "lexicon off", "patterns off", "masks off"]     # behind the masks; off in reverse
    assert m.lexicon_calls[0] is tables
    assert [m.line_lex_seen[i] for i in range(n_lines)] == want_lex
    assert [m.line_state_seen[i] for i in range(n_lines)] == want_state
    assert [m.line_mask_seen[i] for i in range(n_lines)] == want_mask
    assert n_lines > slots
    for i in range(n_lines):
        assert toks[i] == expected(i, prep["max_tokens"][i])                                # scheduling is what it was


def test_fed_chunks_carry_their_lexicon_starts():
    from surya_amd.recognition.loop import FEED_END
    from test_scheduler_cpu import _chunks
    pred, prep = make(20, 8, 4)
    pred.model = LexiconFakeModel(4)
    want = [(i % 3) - 1 for i in range(20)]
    chunks = _chunks(prep, [0, 7, 12, 20])
    for ch in chunks:
        ch["lexicon_starts"] = [want[p.id] for p in ch["prompts"]]
    feed_items = chunks + [FEED_END]
    first = {"prompts": [], "max_tokens": {}, "overall_max_tokens": 8, "token_masks": np.ones((1, 4), np.uint32), "lexicon_tables": _fake_lexicon(2)}
    pred.generate(first, 4, feed=lambda block: feed_items.pop(0))
    assert [pred.model.line_lex_seen[i] for i in range(20)] == want
    assert pred.model.events == ["masks", "lexicon", "lexicon off", "masks off"] and not pred.model.pattern_calls


def test_a_failed_loop_still_switches_the_lexicon_off_and_a_plain_call_never_calls_it():
    pred, prep = make(6, 6, 4)
    pred.model = LexiconFakeModel(4)

    def boom(n, ring):
        raise RuntimeError("device lost")
    pred.model.decode_async = boom
    prep.update(token_masks=np.ones((1, 4), np.uint32), mask_ids=[-1] * 6, lexicon_tables=_fake_lexicon(), lexicon_starts=[0] * 6)
    with pytest.raises(RuntimeError):
        pred.generate(prep, 4)
    assert pred.model.events == ["masks", "lexicon", "lexicon off", "masks off"]
    # masks and patterns without a lexicon, on a model object that has no lexicon entry points at all
    pred, prep = make(6, 6, 4)
    pred.model = PatternFakeModel(4)
    assert not hasattr(pred.model, "set_lexicon")
    prep.update(token_masks=np.ones((1, 4), np.uint32), mask_ids=[0] * 6, pattern_tables=_fake_tables(), start_states=[-1] * 6)
    pred.generate(prep, 4)
    assert pred.model.events == ["masks", "patterns", "patterns off", "masks off"]
    pred, prep = make(6, 6, 4)
    pred.model = LexiconFakeModel(4)
    pred.generate(prep, 4)
    assert pred.model.events == [] and not pred.model.lexicon_calls
    # start states without tables are a caller's bug
    pred, prep = make(5, 6, 4)
    prep["lexicon_starts"] = [0, -1, 0, -1, 0]
    with pytest.raises(AssertionError):
        pred.generate(prep, 4)


# ------------------------------------------------------------------------------------------------------------------ assembly
def test_assembly_sets_lexicon_index():
    """assemble_batch and assemble_line on hand-made streams: the entry's index for a whole entry ended by eos or by pad, the first index
    for a duplicate, -1 for a cut or blank line (which keeps its partial text), None -- and absent from the serialised form -- for a line
    without a lexicon."""
    from surya_amd.recognition.predictor import RecognitionPredictor
    from surya_amd.recognition.processor import SuryaOCRProcessor
    tk = OCRTokenizer(None, None, reserve_special=64)
    proc = SuryaOCRProcessor(tk)
    pred = object.__new__(RecognitionPredictor)
    pred.processor = proc
    lt = compile_lexicons(tk, [["Boston", "Austin", "Boston", "Bo"], ["Austin"]], tk.vocab_size)
    eos, pad = proc.eos_token_id, proc.pad_token_id
    boston, austin = ids_of(tk, "Boston"), ids_of(tk, "Austin")
    streams = [austin + [eos], boston + [eos], boston[:4], [proc.no_output_token], austin + [eos], boston + [pad], austin + [eos], boston[:2] + [eos]]
    starts = [lt.starts[0]] * 4 + [-1, lt.starts[0], lt.starts[1], lt.starts[0]]
    want = [1, 0, -1, -1, None, 0, 0, 3]
    n = len(streams)
    flat = {"polygons": [[7, 9, 300, 52]] * n, "res_scales": [(1.0, 1.0)] * n, "slices": [np.zeros((40, 300, 3), np.uint8)] * n,
            "lexicon_tables": lt, "lexicon_starts": starts}
    items = []
    for i, toks in enumerate(streams):
        rows = np.sort(np.random.default_rng(i).integers(0, 1025, size=(len(toks), 6)), axis=0).astype(np.float32)
        items.append((i, i, toks, [0.5] * len(toks), rows))
    got = pred._assemble_batch(flat, items, False, False, 1025)
    assert [g.lexicon_index for g in got] == want
    assert [g.text for g in got] == ["Austin", "Boston", "Bost", "", "Austin", "Boston", "Austin", "Bo"]
    for it, g in zip(items, got):
        ref = pred._assemble_line(flat, *it, False, False, 1025)
        assert g.model_dump() == ref.model_dump() and g.model_fields_set == ref.model_fields_set
    assert "lexicon_index" not in got[4].model_dump() and got[0].model_dump()["lexicon_index"] == 1 and got[2].model_dump()["lexicon_index"] == -1
    plain = pred._assemble_batch({k: v for k, v in flat.items() if k not in ("lexicon_tables", "lexicon_starts")}, items, False, False, 1025)
    assert all(p.lexicon_index is None for p in plain)
    assert [p.model_dump() for p in plain] == [{k: v for k, v in g.model_dump().items() if k != "lexicon_index"} for g in got]


# ------------------------------------------------------------------------------------------------------------------ the predictor
DATE = r"\d{2}/\d{2}/\d{4}"
CITY, CODE = ["Boston", "Austin"], ["02134", "73301", "02134"]


def test_argument_forms_and_exclusions(tok):
    V = tok.vocab_size
    c = LineConstraints(tok, None, None, 3, [2, 0, 1], vocab_size=V, limit=64, lexicon=CITY)             # one list of str: every line
    s = c.lexicons.starts[0]
    assert c.line_lexicon_starts([2, 0, 1]) == [s, s, s] and c.line_ids([2, 0, 1]) == [-1, -1, -1] and c
    assert len(c.table) == 1 and c.patterns is None                                                      # the engine wants a mask table: one row nobody names
    c = LineConstraints(tok, [None, "01", [None, "ab", None, None]], None, 3, [1, 2, 4], vocab_size=V, limit=64,
                        pattern=[None, None, [None, None, DATE, None]], lexicon=[CITY, None, [CODE, None, None, tuple(CITY)]])
    a, b = c.lexicons.starts
    assert c.line_lexicon_starts([1, 2, 4]) == [a, -1, -1, b, -1, -1, a]
    assert c.line_states([1, 2, 4]) == [-1, -1, -1, -1, -1, c.patterns.starts[0], -1] and c.line_ids([1, 2, 4]) == [-1, 0, 0, -1, 1, -1, -1]
    assert len(c.lexicons.starts) == 2                                                                   # equal lists are compiled once
    assert c.lexicons.entry_of(1, ids_of(tok, "02134") + [c.lexicons.eos]) == 0
    assert LineConstraints(tok, "01", None, 2, None, vocab_size=V).lexicons is None                      # no lexicon: nothing is compiled
    assert not LineConstraints(tok, None, None, 2, [1, 1], vocab_size=V, lexicon=[None, None])
    c = LineConstraints(tok, None, None, 2, None, vocab_size=V, lexicon=[CITY, None])                    # per image works without known lines
    assert c.line_lexicon_starts([4, 2]) == [c.lexicons.starts[0]] * 4 + [-1, -1]
    with pytest.raises(ValueError, match="not known yet"):
        LineConstraints(tok, None, None, 2, None, vocab_size=V, lexicon=[[CITY], None])
    for kw in (dict(allowlist="01"), dict(blocklist="01"), dict(pattern=DATE)):
        args = dict(allowlist=None, blocklist=None, pattern=None)
        args.update(kw)
        with pytest.raises(ValueError, match="never two"):
            LineConstraints(tok, args["allowlist"], args["blocklist"], 1, [1], vocab_size=V, pattern=args["pattern"], lexicon=CITY)
    with pytest.raises(ValueError, match="line 1: .*never two"):
        LineConstraints(tok, [[None, "01"]], None, 1, [2], vocab_size=V, lexicon=[[CITY, CITY]])
    with pytest.raises(ValueError, match="never two"):
        LineConstraints(tok, None, None, 1, [2], vocab_size=V, pattern=[[DATE, None]], lexicon=CITY)
    with pytest.raises(ValueError, match="has 3 lines"):
        LineConstraints(tok, None, None, 1, [3], vocab_size=V, lexicon=[[CITY, None]])
    with pytest.raises(ValueError, match="2 entries for 1 images"):
        LineConstraints(tok, None, None, 1, [1], vocab_size=V, lexicon=[None, CITY])
    for bad in (5, "Boston", [None, 5], [[CITY, "x"]]):
        with pytest.raises(TypeError):
            LineConstraints(tok, None, None, len(bad) if isinstance(bad, list) else 1, [2, 2][: len(bad) if isinstance(bad, list) else 1],
                            vocab_size=V, lexicon=bad)
    with pytest.raises(ValueError, match="empty"):
        LineConstraints(tok, None, None, 1, [1], vocab_size=V, lexicon=[])
    with pytest.raises(ValueError, match="empty string"):
        LineConstraints(tok, None, None, 1, [1], vocab_size=V, lexicon=["a", ""])


def test_predictor_validates_before_any_device_work():
    from PIL import Image
    from surya_amd.recognition.predictor import RecognitionPredictor
    pred = object.__new__(RecognitionPredictor)
    cfg = rec_config("REC-TINY")
    pred.processor = RecognitionModelLoader({"config": cfg, "state_dict": {}}).processor()
    pred.model = SimpleNamespace(vocab=cfg.decoder.vocab_size)
    assert RecognitionPredictor.lexicon is None
    img, box = Image.new("RGB", (64, 32)), [[[0, 0, 10, 10]]]
    pred.lexicon = [[CITY]]
    with pytest.raises(ValueError, match="not known yet"):
        pred([img], det_predictor=object())
    pred.lexicon = []
    with pytest.raises(ValueError, match="empty"):
        pred([img], bboxes=box)
    pred.lexicon = ["ok", ""]
    with pytest.raises(ValueError, match="empty string"):
        pred([img], bboxes=box)
    pred.lexicon = ["ok", "中文"]
    with pytest.raises(ValueError, match="中文"):                          # REC-TINY's 1024 ids cannot write it
        pred([img], bboxes=box)
    pred.lexicon = CITY
    with pytest.raises(ValueError, match="never two"):
        pred([img], bboxes=box, allowlist="01")
    pred.pattern = r"\d+"
    with pytest.raises(ValueError, match="never two"):
        pred([img], bboxes=box)
    pred.pattern = None
    pred.beam_width = 2
    pred.shard_lines = pred.shard_pages = False
    pred.process_group = None
    with pytest.raises(ValueError, match="beam_width"):
        pred([img], bboxes=box)
    pred.beam_width = None
    with pytest.raises(ValueError, match="align"):
        pred.align([img], [["1"]], bboxes=box)


def test_text_line_leaves_an_absent_lexicon_index_out():
    from surya_amd.recognition.schema import TextLine
    ln = TextLine(text="x", polygon=[[0, 0], [1, 0], [1, 1], [0, 1]], confidence=0.5, chars=[])
    assert ln.lexicon_index is None and "lexicon_index" not in ln.model_dump()
    ln.lexicon_index = -1
    assert ln.model_dump()["lexicon_index"] == -1


@pytest.mark.parametrize("rank", [0, 1])
def test_shard_lines_deals_the_lexicon_starts_with_the_lines(monkeypatch, rank):
    import torch
    from surya_amd import dist as sdist
    from surya_amd.recognition.predictor import RecognitionPredictor
    n, world = 7, 2
    monkeypatch.setattr(sdist, "collectives_on", lambda group=None: True)
    monkeypatch.setattr(sdist, "world_info", lambda group=None: (rank, world))
    monkeypatch.setattr(sdist, "collective_device", lambda dev, group=None: "cpu")
    monkeypatch.setattr(sdist, "assert_same_inputs", lambda *a, **k: None)
    monkeypatch.setattr(sdist, "gather_line_outputs", lambda toks, scores, boxes, mine, n_total, max_tokens, **k: (toks, scores, boxes))
    pred = object.__new__(RecognitionPredictor)
    pred.model = SimpleNamespace(device="cpu")
    pred.process_group = None
    seen = {}

    def loop(local, rbs, math_mode):
        seen.update(local)
        m = len(local["slices"])
        return [[5]] * m, torch.zeros((m, 6, 6)), [[0.5]] * m
    pred.prediction_loop = loop
    tables = _fake_lexicon()
    states = [(i % 3) - 1 for i in range(n)]
    flat = {"slices": [np.zeros((4, 10 + i, 3), np.float32) for i in range(n)], "input_text": [None] * n, "task_names": ["ocr_with_boxes"] * n,
            "token_masks": np.ones((2, 3), np.uint32), "mask_ids": [-1] * n, "lexicon_tables": tables, "lexicon_starts": states}
    pred.sharded_prediction_loop(flat, 4, True)
    mine = list(range(rank, n, world))
    assert seen["lexicon_starts"] == [states[i] for i in mine] and seen["lexicon_tables"] is tables
    seen.clear()
    del flat["lexicon_tables"], flat["lexicon_starts"]
    pred.sharded_prediction_loop(flat, 4, True)
    assert "lexicon_starts" not in seen and "lexicon_tables" not in seen and "mask_ids" in seen


def test_page_sharded_call_slices_a_per_image_lexicon(monkeypatch):
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
    pred._call_page_sharded(*args, lexicon=[CITY, None, ["c"], CODE, None])
    assert got["n"] == 2 and got["kw"] == {"lexicon": [None, CODE]}
    pred._call_page_sharded(*args, allowlist=None, blocklist="xy", lexicon=CITY)
    assert got["kw"] == {"allowlist": [None, None], "blocklist": ["xy", "xy"], "lexicon": [CITY, CITY]}
    pred._call_page_sharded(*args)
    assert got["kw"] == {}
