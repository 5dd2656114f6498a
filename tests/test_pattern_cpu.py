"""Pattern-guided decoding, host side (no GPU): the pattern compiler (recognition/pattern.py) against re.fullmatch, the properties of its
tables, its limits and refusals; the device loop's contract with the model (on the fake of tests/test_scheduler_cpu.py); pattern_matched
from assembly; start states through shard_lines and the page-sharded call."""
import re
from types import SimpleNamespace

import numpy as np
import pytest

from surya_amd import _lib as L
from surya_amd.config import rec_config
from surya_amd.recognition.loader import RecognitionModelLoader
from surya_amd.recognition.pattern import compile_patterns
from surya_amd.recognition.predictor import LineConstraints
from surya_amd.recognition.tokenizer import MaskTable, OCRTokenizer
from surya_amd.settings import settings

from test_allowlist_cpu import MaskFakeModel, bits_of
from test_scheduler_cpu import expected, make

DATE, AMOUNT, IBAN = r"\d{2}/\d{2}/\d{4}", r"-?\d{1,3}(,\d{3})*\.\d{2}", r"[A-Z]{2}\d{2}( ?[A-Z0-9]{4}){2,7}"
SMILE = "\U0001F600"
# (pattern, six symbols drawn from it, strings it must accept, strings it must refuse): every supported construct occurs somewhere
CASES = [
    (DATE, "0179/5", ["12/03/2024", "٣1/12/1999"], ["12/3/20245", "12/03/202", "12-03-2024", ""]),
    (AMOUNT, "-19,.0", ["-1.00", "12,345.67", "999.99", "1,000,000.00"], ["1234.00", "1,00.00", "-.50", "1.0"]),
    (IBAN, "AZ09 b", ["DE89 3704 0044", "GB82WEST12345698", "FR14 2004 1010 0505 0001 3M02 606A"], ["DE89", "de89 3704 0044", "DE89  3704 0044"]),
    (r"[^a-c\d]x?", "abdx1 ", ["d", "dx", " x", "\n"], ["a", "1x", "dxx", "dx "]),
    (r"cat|dog|cow", "catdgo", ["cat", "dog", "cow"], ["ca", "cog", "catdog"]),
    ("a" + SMILE + "b+", "ab" + SMILE + "xyz", ["a" + SMILE + "b", "a" + SMILE + "bbb"], ["ab", "a" + SMILE, SMILE + "b"]),
    (r"(ab)*c+", "abcxyz", ["c", "abc", "ababccc"], ["", "ab", "abac", "bc"]),
    (r".\w\s", "a_ \n-1", ["a_ ", "-é\t", " a\n"], ["\na ", "a- ", "a_"]),
    (r"\D\S\W", "a1 -_\t", ["a1 ", "-_-", " a\t"], ["1a ", "a a", "aaa"]),
    (r"a{2,}b{,2}c{3}", "abcxyz", ["aaccc", "aaabbccc"], ["accc", "aabbbccc", "aacc"]),
    (r"(?:x|yz){1,2}\.?", "xyz.ab", ["x", "yzx", "xx.", "yzyz"], ["", "xxx", "y", "zx"]),
    (r"[\d.\-+]+\x41é\t", "1.-+Aé", ["1Aé\t", "+-.9Aé\t"], ["Aé\t", "1Aé"]),
    (r"", "abcdef", [""], ["a"]),
]
PATTERNS = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def tok():
    return OCRTokenizer()


@pytest.fixture(scope="module")
def joint(tok):
    """All the patterns of the module compiled as ONE call's tables: one state space, one class map, one mask table."""
    return compile_patterns(tok, PATTERNS, tok.vocab_size)


def units(s):
    raw = s.encode("utf-16le", "surrogatepass")
    return [raw[i] + (raw[i + 1] << 8) for i in range(0, len(raw), 2)]


def dfa_accepts(pt, tok, pattern, s):
    st = pt.start_of(pattern)
    for u in units(s):
        t = tok.special_token_offset + u
        if not pt.allowed(st, t):
            return False
        st = pt.advance(st, t)
    return pt.accepts(st)


@pytest.mark.parametrize("case", CASES, ids=[repr(c[0]) for c in CASES])
def test_dfa_accepts_iff_fullmatch(tok, joint, case):
    """Every string up to length 6 over six symbols of the pattern and two foreign ones, walked as a trie so the automaton takes one step
    per string; then the hand-picked strings, which reach the lengths the longer patterns need."""
    pattern, symbols, yes, no = case
    rx = re.compile(pattern)
    alphabet = list(dict.fromkeys(list(symbols) + ["q", "€"]))
    assert len(alphabet) == 8                                           # (the non-BMP literal is ONE symbol, of two code units)
    sto = tok.special_token_offset
    steps = [[sto + u for u in units(ch)] for ch in alphabet]
    n = bad = 0
    stack = [("", joint.start_of(pattern), True)]
    while stack:
        s, st, alive = stack.pop()
        n += 1
        if (rx.fullmatch(s) is not None) != (alive and joint.accepts(st)):
            bad += 1
            assert bad < 5, (pattern, s)
        if len(s) >= 6:
            continue
        for ch, ids in zip(alphabet, steps):
            st2, ok = st, alive
            for t in ids:
                ok = ok and joint.allowed(st2, t)
                st2 = joint.advance(st2, t) if ok else st2
            stack.append((s + ch, st2, ok))
    assert bad == 0 and n == sum(len(alphabet) ** k for k in range(7))
    for s in yes:
        assert rx.fullmatch(s) and dfa_accepts(joint, tok, pattern, s), (pattern, s)
    for s in no:
        assert not rx.fullmatch(s) and not dfa_accepts(joint, tok, pattern, s), (pattern, s)


def test_a_non_bmp_literal_is_exact(tok):
    """High surrogate then low surrogate, in sequence: no other pairing of the two halves gets through (token_mask(allow=) permits both)."""
    pt = compile_patterns(tok, [SMILE + "|\U0001F431"], tok.vocab_size)
    hi1, lo1 = units(SMILE)
    hi2, lo2 = units("\U0001F431")
    sto, s0 = tok.special_token_offset, pt.starts[0]
    assert hi1 == hi2 and lo1 != lo2
    assert pt.allowed(s0, sto + hi1) and not pt.allowed(s0, sto + lo1)
    s1 = pt.advance(s0, sto + hi1)
    assert pt.allowed(s1, sto + lo1) and pt.allowed(s1, sto + lo2) and not pt.allowed(s1, sto + lo1 + 1) and not pt.allowed(s1, sto + hi1)
    assert pt.accepts(pt.advance(s1, sto + lo2)) and not pt.accepts(s1)
    # `.` and negated sets are the BMP without the surrogates: unlike re on str, they do not reach a character outside it
    neg = compile_patterns(tok, [r"[^a]", r"."], tok.vocab_size)
    for s in neg.starts:
        assert not neg.allowed(s, sto + hi1) and not neg.allowed(s, sto + lo1) and neg.allowed(s, sto + ord("b"))


def test_table_properties(tok, joint):
    pt = joint
    V = tok.vocab_size
    sp = tok.SPECIAL_TOKEN_MAPPING
    eos, pad, nop = sp["</S>"], sp["<PAD>"], sp["<NOP>"]
    assert (pt.eos, pt.pad, pt.nop) == (eos, pad, nop)
    assert pt.tok_class.shape == (V,) and pt.tok_class.dtype == np.uint8
    assert pt.next_state.shape == (pt.n_states, pt.n_classes) and pt.next_state.dtype == np.uint16 and int(pt.next_state.max()) < pt.n_states
    assert pt.state_mask.shape == (pt.n_states,) and int(pt.state_mask.max()) < len(pt.table) <= L.SA_MAX_TOKEN_MASKS
    assert pt.n_states <= L.SA_MAX_PATTERN_STATES and pt.n_classes <= L.SA_MAX_PATTERN_CLASSES
    # ids that are no code unit -- math BPE, tags, eos / pad / no-output -- share the dead class, which moves nowhere
    assert (pt.tok_class[: tok.special_token_offset] == 0).all()
    assert (pt.next_state[:, 0] == np.arange(pt.n_states)).all()
    starts = set(pt.starts)
    assert len(pt.starts) == len(PATTERNS)
    entered = {int(t) for s in range(pt.n_states) for c, t in enumerate(pt.next_state[s]) if c and int(t) != s}
    for s in range(pt.n_states):
        row = np.zeros(((V + 31) // 32) * 32, bool)
        row[bits_of(pt.table.rows[int(pt.state_mask[s])])] = True
        ids = np.flatnonzero(row[:V])
        text_ids = ids[ids >= tok.special_token_offset]
        assert len(text_ids) or pt.accepts(s), f"state {s} neither moves nor accepts"
        assert not len(ids[ids < tok.special_token_offset]) or set(ids[ids < tok.special_token_offset].tolist()) <= {eos, pad, nop}
        assert bool(row[eos]) == bool(row[pad]) == pt.accepts(s)          # a line may end exactly where the pattern accepts
        assert bool(row[nop]) == (s in starts)                             # "no output" is a first-token answer
        for t in text_ids[:50].tolist():                                   # an allowed id has a transition of its own
            assert pt.tok_class[t] != 0
        assert len(ids) > 0
    assert not (starts & entered), "a start state can be re-entered: the no-output id would be allowed inside a line"
    # the same set, however it is reached, is one row
    assert len(pt.table) == len({pt.table.rows[i].tobytes() for i in range(len(pt.table))})


def test_state_rows_merge_with_identical_allowlist_rows(tok):
    table = MaskTable(tok, tok.vocab_size, L.SA_MAX_TOKEN_MASKS)
    dig = table.id_for("0123456789", None)
    other = table.id_for("xyz", None)
    pt = compile_patterns(tok, [r"[0-9]*"], tok.vocab_size, extra_mask_rows=table)
    # the start state of [0-9]*: digits, and -- accepting, first token -- eos, pad and no-output: exactly the digits allowlist
    assert int(pt.state_mask[pt.starts[0]]) == dig and pt.table is table
    assert len(table) == 3 and other == 1                                  # one more row: the loop state (no no-output id)
    c = LineConstraints(tok, [None, "0123456789"], None, 2, [1, 1], vocab_size=tok.vocab_size, limit=L.SA_MAX_TOKEN_MASKS, pattern=[r"[0-9]*", None])
    assert c.line_ids([1, 1]) == [-1, 0] and c.line_states([1, 1]) == [c.patterns.starts[0], -1]
    assert int(c.patterns.state_mask[c.patterns.starts[0]]) == 0 and len(c.table) == 2


def test_limits_raise_with_the_count(tok):
    V = tok.vocab_size
    with pytest.raises(ValueError, match="5001 automaton states"):
        compile_patterns(tok, [r"a{5000}"], V)
    with pytest.raises(ValueError, match="automaton positions"):
        compile_patterns(tok, [r"(a{300}){300}"], V)
    with pytest.raises(ValueError, match=r"30\d symbol classes"):
        compile_patterns(tok, ["|".join(chr(0x4E00 + i) for i in range(300))], V)
    with pytest.raises(ValueError, match=f"more than {L.SA_MAX_TOKEN_MASKS} distinct"):
        compile_patterns(tok, ["".join(chr(0x4E00 + i) for i in range(70))], V)
    small = compile_patterns(tok, [r"a{40}"], V, max_states=64)
    assert small.n_states == 41
    with pytest.raises(ValueError, match="41 automaton states"):
        compile_patterns(tok, [r"a{40}"], V, max_states=40)
    iban = compile_patterns(tok, [IBAN], V)
    assert len(iban.table) <= L.SA_MAX_TOKEN_MASKS and iban.n_classes <= L.SA_MAX_PATTERN_CLASSES and iban.n_states <= L.SA_MAX_PATTERN_STATES
    with pytest.raises(ValueError, match="matches no text"):
        compile_patterns(tok, [r"a[^\x00-￿]"], V)


@pytest.mark.parametrize("pattern,what", [
    (r"^a", "anchor"), (r"a$", "anchor"), (r"\bx", "anchor"), (r"x\Z", "anchor"), (r"a*?", "lazy"), (r"a+?", "lazy"), (r"a{2}?", "lazy"),
    (r"a++", "possessive"), (r"a?+", "possessive"), (r"(?=a)b", "look-ahead"), (r"(?!a)b", "look-ahead"), (r"(?<=a)b", "look-behind"),
    (r"(a)\1", "back-reference"), (r"(?P<n>a)", "named group"), (r"(?i)a", "flag"), (r"(?#c)a", "comment"), (r"[[:alpha:]]", "POSIX"),
    (r"[\U0001F600]", "Basic Multilingual Plane"), (r"a{2,1}", "n < m"), (r"a{", "'{'"), (r"*a", "nothing to repeat"), (r"(a", "unclosed"),
    (r"a)", "unbalanced"), (r"[a", "unclosed"), (r"\q", "escape"), (r"a**", "quantifier on a quantifier"), ("a\\", "trailing backslash")])
def test_unsupported_constructs_raise_naming_the_construct(tok, pattern, what):
    with pytest.raises(ValueError, match=re.escape(what)):
        compile_patterns(tok, [pattern], tok.vocab_size)


def test_a_small_model_vocabulary_restricts_the_alphabet():
    """REC-TINY writes 704 code units: a pattern over them compiles, one that needs a unit beyond them matches nothing the model can write."""
    cfg = rec_config("REC-TINY")
    tk = RecognitionModelLoader({"config": cfg, "state_dict": {}}).processor().ocr_tokenizer
    V = cfg.decoder.vocab_size
    pt = compile_patterns(tk, [r"\d+", r"[^a]"], V)
    assert pt.tok_class.shape == (V,)
    for row in pt.table.rows:
        assert (bits_of(row) < V).all()
    with pytest.raises(ValueError, match="matches no text"):
        compile_patterns(tk, ["中"], V)


def test_matched_on_hand_made_token_lists(tok, joint):
    sto, sp = tok.special_token_offset, tok.SPECIAL_TOKEN_MAPPING
    eos, pad, nop = sp["</S>"], sp["<PAD>"], sp["<NOP>"]
    s0 = joint.start_of(DATE)
    ids = [sto + u for u in units("12/03/2024")]
    assert joint.matched(s0, ids + [eos])
    assert not joint.matched(s0, ids)                                      # cut by the token budget: no eos
    assert not joint.matched(s0, ids + [pad])                              # ended, but not with eos
    assert not joint.matched(s0, ids[:9] + [eos])                          # (the mask never allows this eos; a replay must still say no)
    assert not joint.matched(s0, [nop])                                    # a blank crop
    assert not joint.matched(s0, ids[:4] + [sto + ord("x")] + ids[5:] + [eos])
    assert not joint.matched(s0, ids + [eos, eos])
    assert joint.matched(joint.start_of(""), [eos]) and not joint.matched(joint.start_of(""), [])
    assert joint.advance(-1, ids[0]) == -1 and joint.advance(s0, eos) == s0 and joint.advance(s0, nop) == s0 and not joint.accepts(-1)


def test_assembly_sets_pattern_matched():
    """assemble_batch and assemble_line on hand-made streams: True for a completed match, False for a cut or blank line (which keeps its
    partial text), None -- and absent from the serialised form -- for a line without a pattern."""
    from surya_amd.recognition.predictor import RecognitionPredictor
    from surya_amd.recognition.processor import SuryaOCRProcessor
    tk = OCRTokenizer(None, None, reserve_special=64)
    proc = SuryaOCRProcessor(tk)
    pred = object.__new__(RecognitionPredictor)
    pred.processor = proc
    pt = compile_patterns(tk, [DATE], tk.vocab_size)
    sto = tk.special_token_offset
    date = [sto + u for u in units("12/03/2024")]
    streams = [date + [proc.eos_token_id], date[:6], [proc.no_output_token], date + [proc.eos_token_id], date + [proc.pad_token_id]]
    starts = [pt.starts[0], pt.starts[0], pt.starts[0], -1, pt.starts[0]]
    want = [True, False, False, None, False]
    flat = {"polygons": [[7, 9, 300, 52]] * 5, "res_scales": [(1.0, 1.0)] * 5, "slices": [np.zeros((40, 300, 3), np.uint8)] * 5,
            "pattern_tables": pt, "start_states": starts}
    items = []
    for i, toks in enumerate(streams):
        rows = np.sort(np.random.default_rng(i).integers(0, 1025, size=(len(toks), 6)), axis=0).astype(np.float32)
        items.append((i, i, toks, [0.5] * len(toks), rows))
    got = pred._assemble_batch(flat, items, False, False, 1025)
    assert [g.pattern_matched for g in got] == want
    assert [g.text for g in got] == ["12/03/2024", "12/03/", "", "12/03/2024", "12/03/2024"]
    for it, g in zip(items, got):
        ref = pred._assemble_line(flat, *it, False, False, 1025)
        assert g.model_dump() == ref.model_dump() and g.model_fields_set == ref.model_fields_set
    assert "pattern_matched" not in got[3].model_dump() and got[0].model_dump()["pattern_matched"] is True
    plain = pred._assemble_batch({k: v for k, v in flat.items() if k not in ("pattern_tables", "start_states")}, items, False, False, 1025)
    assert all(p.pattern_matched is None for p in plain)
    assert [p.model_dump() for p in plain] == [{k: v for k, v in g.model_dump().items() if k != "pattern_matched"} for g in got]


# ------------------------------------------------------------------------------------------------------------------ the device loop
class PatternFakeModel(MaskFakeModel):
    """The mask fake plus the pattern entry points, with their contracts: tables only behind a mask table; start states only while
    patterns are on, for slots whose mask ids were set for this prefill, before the prefill; a new mask table switches patterns off."""

    def __init__(self, max_slots):
        super().__init__(max_slots)
        self.pattern_calls, self.slot_state, self.line_state_seen, self.pending_state, self.events = [], {}, {}, {}, []

    def set_token_masks(self, masks):
        super().set_token_masks(masks)
        self.events.append("masks" if masks is not None else "masks off")
        assert not (self.pattern_calls and self.pattern_calls[-1] is not None), "the mask table was replaced under a live automaton"

    def set_patterns(self, tables):
        assert not self.inflight and self.prefill_out is None
        assert tables is None or (self.tables and self.tables[-1] is not None), "SA_ERR_STATE: patterns without a mask table"
        self.pattern_calls.append(tables)
        self.events.append("patterns" if tables is not None else "patterns off")
        self.slot_state = {}

    def set_slot_masks(self, slots, ids):
        super().set_slot_masks(slots, ids)
        for s in slots:
            self.slot_state[s] = -1                                         # a slot given a mask id follows no automaton any more

    def set_slot_patterns(self, slots, states):
        assert self.pattern_calls and self.pattern_calls[-1] is not None, "SA_ERR_STATE: start states while patterns are off"
        assert not self.inflight and len(slots) == len(states) == len(set(slots))
        for s, st in zip(slots, states):
            assert s not in self.active and -1 <= st < self.pattern_calls[-1].n_states
            assert self.pending.get(s), "start states go behind the slot's mask id"
            self.slot_state[s] = st
            self.pending_state[s] = True

    def prefill(self, tiles, grid_hw, input_ids, slot_ids):
        if self.pattern_calls and self.pattern_calls[-1] is not None:
            for s in slot_ids:
                assert self.pending_state.pop(s, False), "a slot was prefilled without its start state being set first"
        super().prefill(tiles, grid_hw, input_ids, slot_ids)
        for ids, s in zip(input_ids, slot_ids):
            self.line_state_seen[ids[0] - 1000] = self.slot_state.get(s, -1)


def _fake_tables(n_states=7):
    return SimpleNamespace(n_states=n_states, tok_class=None, next_state=None, state_mask=None)


@pytest.mark.parametrize("n_lines,max_tokens,slots,sps,ahead", [(23, 12, 4, 4, True), (40, 6, 7, 1, False)])
def test_start_states_reach_the_prefilled_slots_and_patterns_are_switched_off(n_lines, max_tokens, slots, sps, ahead):
    old = (settings.RECOGNITION_STEPS_PER_SYNC, settings.RECOGNITION_ENCODE_AHEAD)
    settings.RECOGNITION_STEPS_PER_SYNC, settings.RECOGNITION_ENCODE_AHEAD = sps, ahead
    try:
        pred, prep = make(n_lines, max_tokens, slots)
        pred.model = PatternFakeModel(slots)
        tables = _fake_tables()
        want_state = [(i % 4) * 2 - 1 if i % 4 else -1 for i in range(n_lines)]            # -1, 1, 3, 5: reused slots change kind
        want_mask = [0 if s < 0 and i % 8 == 0 else -1 for i, s in enumerate(want_state)]
        prep.update(token_masks=np.ones((3, 5), np.uint32), mask_ids=want_mask, pattern_tables=tables, start_states=want_state)
        toks, _, _ = pred.generate(prep, slots)
    finally:
        settings.RECOGNITION_STEPS_PER_SYNC, settings.RECOGNITION_ENCODE_AHEAD = old
    m = pred.model
    assert m.events == ["masks", "patterns", "patterns off", "masks off"]                    # uploaded once, behind the masks; off in reverse
    assert m.pattern_calls[0] is tables
    assert [m.line_state_seen[i] for i in range(n_lines)] == want_state
    assert [m.line_mask_seen[i] for i in range(n_lines)] == want_mask
    assert n_lines > slots
    for i in range(n_lines):
        assert toks[i] == expected(i, prep["max_tokens"][i])                                # scheduling is what it was


def test_fed_chunks_carry_their_start_states():
    from surya_amd.recognition.loop import FEED_END
    from test_scheduler_cpu import _chunks
    pred, prep = make(20, 8, 4)
    pred.model = PatternFakeModel(4)
    want = [(i % 3) - 1 for i in range(20)]
    chunks = _chunks(prep, [0, 7, 12, 20])
    for ch in chunks:
        ch["start_states"] = [want[p.id] for p in ch["prompts"]]
    feed_items = chunks + [FEED_END]
    first = {"prompts": [], "max_tokens": {}, "overall_max_tokens": 8, "token_masks": np.ones((2, 4), np.uint32), "pattern_tables": _fake_tables(2)}
    pred.generate(first, 4, feed=lambda block: feed_items.pop(0))
    assert [pred.model.line_state_seen[i] for i in range(20)] == want
    assert pred.model.events[-2:] == ["patterns off", "masks off"]


def test_a_failed_loop_still_switches_patterns_off_and_a_plain_call_never_calls_them():
    pred, prep = make(6, 6, 4)
    pred.model = PatternFakeModel(4)

    def boom(n, ring):
        raise RuntimeError("device lost")
    pred.model.decode_async = boom
    prep.update(token_masks=np.ones((1, 4), np.uint32), mask_ids=[-1] * 6, pattern_tables=_fake_tables(), start_states=[0] * 6)
    with pytest.raises(RuntimeError):
        pred.generate(prep, 4)
    assert pred.model.events == ["masks", "patterns", "patterns off", "masks off"]
    # masks without patterns: the pattern entry points are never touched
    pred, prep = make(6, 6, 4)
    pred.model = PatternFakeModel(4)
    prep.update(token_masks=np.ones((1, 4), np.uint32), mask_ids=[0] * 6)
    pred.generate(prep, 4)
    assert pred.model.events == ["masks", "masks off"] and not pred.model.pattern_calls
    # start states without tables are a caller's bug; so are patterns in a beam or forced loop
    pred, prep = make(5, 6, 4)
    prep["start_states"] = [0, -1, 0, -1, 0]
    with pytest.raises(AssertionError):
        pred.generate(prep, 4)


# ------------------------------------------------------------------------------------------------------------------ the predictor
def test_argument_forms_and_exclusions(tok):
    V = tok.vocab_size
    c = LineConstraints(tok, None, None, 3, [2, 0, 1], vocab_size=V, limit=64, pattern=DATE)
    s = c.patterns.starts[0]
    assert c.line_states([2, 0, 1]) == [s, s, s] and c.line_ids([2, 0, 1]) == [-1, -1, -1] and c
    c = LineConstraints(tok, [None, "01", [None, "ab", None]], None, 3, [1, 2, 3], vocab_size=V, limit=64, pattern=[DATE, None, [AMOUNT, None, DATE]])
    d, a = c.patterns.start_of(DATE), c.patterns.start_of(AMOUNT)
    assert c.line_states([1, 2, 3]) == [d, -1, -1, a, -1, d] and c.line_ids([1, 2, 3]) == [-1, 0, 0, -1, 1, -1]
    assert c.patterns.patterns == [DATE, AMOUNT] and c.patterns.table is c.table
    assert LineConstraints(tok, "01", None, 2, None, vocab_size=V).patterns is None                  # no pattern: nothing is compiled
    assert not LineConstraints(tok, None, None, 2, [1, 1], vocab_size=V, pattern=[None, None])
    c = LineConstraints(tok, None, None, 2, None, vocab_size=V, pattern=[DATE, None])
    assert c.line_states([4, 2]) == [c.patterns.starts[0]] * 4 + [-1, -1]
    with pytest.raises(ValueError, match="not known yet"):
        LineConstraints(tok, None, None, 2, None, vocab_size=V, pattern=[[DATE], None])
    with pytest.raises(ValueError, match="not both"):
        LineConstraints(tok, "01", None, 1, [1], vocab_size=V, pattern=DATE)
    with pytest.raises(ValueError, match="not both"):
        LineConstraints(tok, [["01", None]], None, 1, [2], vocab_size=V, pattern=[[DATE, DATE]])
    with pytest.raises(ValueError):
        LineConstraints(tok, None, None, 1, [3], vocab_size=V, pattern=[[DATE, None]])
    with pytest.raises(TypeError):
        LineConstraints(tok, None, None, 1, [1], vocab_size=V, pattern=5)
    with pytest.raises(ValueError, match="anchor"):
        LineConstraints(tok, None, None, 1, [1], vocab_size=V, pattern=r"^\d+$")


def test_predictor_validates_before_any_device_work():
    from PIL import Image
    from surya_amd.recognition.predictor import RecognitionPredictor
    pred = object.__new__(RecognitionPredictor)
    pred.processor = RecognitionModelLoader({"config": rec_config("REC-TINY"), "state_dict": {}}).processor()
    pred.model = None
    assert RecognitionPredictor.pattern is None
    img = Image.new("RGB", (64, 32))
    pred.pattern = [[r"\d+"]]
    with pytest.raises(ValueError, match="not known yet"):
        pred([img], det_predictor=object())
    pred.pattern = r"\d+$"
    with pytest.raises(ValueError, match="anchor"):
        pred([img], bboxes=[[[0, 0, 10, 10]]])
    pred.pattern = r"\d+"
    with pytest.raises(ValueError, match="not both"):
        pred([img], bboxes=[[[0, 0, 10, 10]]], allowlist="01")
    pred.beam_width = 2
    pred.shard_lines = pred.shard_pages = False
    pred.process_group = None
    with pytest.raises(ValueError, match="beam_width"):
        pred([img], bboxes=[[[0, 0, 10, 10]]])
    pred.beam_width = None
    with pytest.raises(ValueError, match="align"):
        pred.align([img], [["1"]], bboxes=[[[0, 0, 10, 10]]])


@pytest.mark.parametrize("rank", [0, 1])
def test_shard_lines_deals_the_start_states_with_the_lines(monkeypatch, rank):
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
    tables = _fake_tables()
    states = [(i % 3) - 1 for i in range(n)]
    flat = {"slices": [np.zeros((4, 10 + i, 3), np.float32) for i in range(n)], "input_text": [None] * n, "task_names": ["ocr_with_boxes"] * n,
            "token_masks": np.ones((2, 3), np.uint32), "mask_ids": [-1] * n, "pattern_tables": tables, "start_states": states}
    pred.sharded_prediction_loop(flat, 4, True)
    mine = list(range(rank, n, world))
    assert seen["start_states"] == [states[i] for i in mine] and seen["pattern_tables"] is tables
    seen.clear()
    del flat["pattern_tables"], flat["start_states"]
    pred.sharded_prediction_loop(flat, 4, True)
    assert "start_states" not in seen and "pattern_tables" not in seen and "mask_ids" in seen


def test_page_sharded_call_slices_a_per_image_pattern(monkeypatch):
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
    pred._call_page_sharded(*args, pattern=[DATE, None, "c", AMOUNT, None])
    assert got["n"] == 2 and got["kw"] == {"pattern": [None, AMOUNT]}
    pred._call_page_sharded(*args, allowlist=None, blocklist="xy", pattern=DATE)
    assert got["kw"] == {"allowlist": [None, None], "blocklist": ["xy", "xy"], "pattern": [DATE, DATE]}
    pred._call_page_sharded(*args)
    assert got["kw"] == {}
