"""Pattern-guided decoding: regular expressions compiled to the tables of surya_rec_set_patterns (include/surya_amd.h).

A token mask (OCRTokenizer.token_mask) is one allowed set per line. A pattern makes the set depend on what the line has emitted so far:
every line follows a deterministic finite automaton over its tokens, and a state's allowed set is a row of the call's token-mask table.
Ordinary text is one token per UTF-16 code unit (special_token_offset + unit), so an automaton over code units is one over tokens.

Syntax: a subset of Python's `re`, with the semantics of `re.fullmatch` on the line's text:
  literals and escapes (\\n \\t \\r \\f \\v \\a \\0 \\xhh \\uhhhh \\Uhhhhhhhh, \\ before punctuation); `.`; \\d \\w \\s \\D \\W \\S; classes
  [...] and [^...] with ranges and the escapes above; groups (...) and (?:...); alternation |; quantifiers ? * + {m} {m,} {m,n}.
Everything else raises ValueError naming the construct: anchors and \\b \\B \\A \\Z, look-around, back-references, named groups, flags,
lazy (`*?`) and possessive (`*+`) quantifiers, and a quantifier bound that needs more states than the limit.
Alphabet: UTF-16 code units. `.`, the negated escapes and negated classes mean code units of the Basic Multilingual Plane that are not
surrogates (`.` does not match a line feed, as in `re` without DOTALL); \\d \\w \\s are `re`'s Unicode sets. A literal outside the BMP is
its high surrogate followed by its low surrogate, in sequence -- exact, unlike token_mask(allow=), which permits each surrogate by itself;
inside a class such a character raises. Math-BPE ids and tags are never allowed: patterns speak about text.

Pipeline: parse -> Thompson NFA -> subset construction over symbol classes -> trim to the states from which acceptance is reachable ->
minimise (all patterns of a call in one state space) -> tables. A state's allowed set is the code units with a live transition; EOS
and pad are added in accepting states only, the no-output token only in a pattern's start state (a blank crop still reads as blank),
which is why a start state that the automaton would re-enter gets a copy of its own. After trimming every state has a live transition
or accepts, so every mask row has an allowed id."""
from __future__ import annotations

import re
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

SA_MAX_PATTERN_STATES = 4096       # include/surya_amd.h
SA_MAX_PATTERN_CLASSES = 256
_UNITS = 65536
_NFA_LIMIT = 16 * SA_MAX_PATTERN_STATES      # positions of one pattern's NFA: past this no DFA within the state limit is in reach

_BMP = np.ones(_UNITS, bool)
_BMP[0xD800:0xE000] = False                  # surrogates: never matched by `.`, a negated class or a negated escape
_ESC_SETS: Dict[str, np.ndarray] = {}


def _escape_set(ch: str) -> np.ndarray:
    """The code units \\d / \\w / \\s match in `re` (str patterns: the Unicode sets); upper case: the BMP complement."""
    if not _ESC_SETS:
        for c in "dws":
            rx = re.compile("\\" + c)
            s = np.zeros(_UNITS, bool)
            for u in range(_UNITS):
                if not 0xD800 <= u < 0xE000 and rx.match(chr(u)):
                    s[u] = True
            _ESC_SETS[c] = s
            _ESC_SETS[c.upper()] = _BMP & ~s
    return _ESC_SETS[ch]


def _single(u: int) -> np.ndarray:
    s = np.zeros(_UNITS, bool)
    s[u] = True
    return s


# AST: ("set", bool[65536]) | ("cat", [nodes]) | ("alt", [nodes]) | ("rep", node, lo, hi or None)
class _Parser:
    _SIMPLE = {"n": "\n", "t": "\t", "r": "\r", "f": "\f", "v": "\v", "a": "\a", "0": "\0"}

    def __init__(self, pattern: str):
        if not isinstance(pattern, str):
            raise TypeError("a pattern is a str")
        self.p, self.i = pattern, 0

    def fail(self, what: str):
        raise ValueError(f"pattern {self.p!r}: {what} at position {self.i} is not supported "
                         "(supported: literals, escapes, ., \\d \\w \\s, [...] classes, groups, |, ? * + {m} {m,n})")

    def peek(self) -> str:
        return self.p[self.i] if self.i < len(self.p) else ""

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            self.fail("unbalanced ')'")
        return node

    def alt(self):
        arms = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            arms.append(self.cat())
        return arms[0] if len(arms) == 1 else ("alt", arms)

    def cat(self):
        items = []
        while self.i < len(self.p) and self.peek() not in "|)":
            items.append(self.repeat())
        return ("cat", items)

    def repeat(self):
        if self.peek() in "*+?{":
            self.fail(f"a quantifier {self.peek()!r} with nothing to repeat")
        node = self.atom()
        while True:
            c = self.peek()
            if c == "*":
                lo, hi = 0, None
            elif c == "+":
                lo, hi = 1, None
            elif c == "?":
                lo, hi = 0, 1
            elif c == "{":
                m = re.compile(r"\{(\d*)(,?)(\d*)\}").match(self.p, self.i)
                if not m or (m.group(1) == "" and m.group(3) == ""):
                    self.fail("an unescaped '{' that is no {m} / {m,n} quantifier")
                lo = int(m.group(1) or 0)
                hi = lo if not m.group(2) else (int(m.group(3)) if m.group(3) else None)
                if hi is not None and hi < lo:
                    self.fail("a quantifier {m,n} with n < m")
                self.i = m.end() - 1
            else:
                return node
            self.i += 1
            if self.peek() == "?":
                self.fail("a lazy quantifier")
            if self.peek() == "+":
                self.fail("a possessive quantifier")
            if self.peek() in ("*", "{"):
                self.fail("a quantifier on a quantifier")
            node = ("rep", node, lo, hi)

    def atom(self):
        c = self.peek()
        if c == "(":
            self.i += 1
            if self.peek() == "?":
                nxt = self.p[self.i + 1: self.i + 2]
                if nxt == ":":
                    self.i += 2
                else:
                    self.fail({"=": "look-ahead", "!": "negative look-ahead", "<": "look-behind or a named group", "P": "a named group",
                               "#": "a comment group", "(": "a conditional group", ">": "an atomic group"}.get(nxt, "an inline flag group"))
            node = self.alt()
            if self.peek() != ")":
                self.fail("an unclosed '('")
            self.i += 1
            return node
        if c == "[":
            return ("set", self.char_class())
        if c == ".":
            self.i += 1
            s = _BMP.copy()
            s[0x0A] = False
            return ("set", s)
        if c in "^$":
            self.fail(f"the anchor {c!r}")
        if c == "\\":
            kind, val = self.escape(False)
            return ("set", val) if kind == "set" else self.literal(val)
        self.i += 1
        return self.literal(ord(c))

    def literal(self, cp: int):
        if cp <= 0xFFFF:
            return ("set", _single(cp))
        cp -= 0x10000                       # outside the BMP: the high surrogate, then the low one
        return ("cat", [("set", _single(0xD800 + (cp >> 10))), ("set", _single(0xDC00 + (cp & 0x3FF)))])

    def escape(self, in_class: bool) -> Tuple[str, object]:
        """At a backslash: ("set", units) for \\d \\w \\s and their negations, ("cp", code point) for a character."""
        self.i += 1
        c = self.peek()
        if c == "":
            self.fail("a trailing backslash")
        self.i += 1
        if c in "dwsDWS":
            return "set", _escape_set(c)
        if c in self._SIMPLE and not (c == "0" and self.peek().isdigit()):
            return "cp", ord(self._SIMPLE[c])
        if c in "xuU":
            n = {"x": 2, "u": 4, "U": 8}[c]
            h = self.p[self.i: self.i + n]
            if len(h) != n or any(ch not in "0123456789abcdefABCDEF" for ch in h) or int(h, 16) > 0x10FFFF:
                self.fail(f"a malformed \\{c} escape")
            self.i += n
            return "cp", int(h, 16)
        if c == "b" and in_class:
            return "cp", 8
        if c.isdigit():
            self.fail("a back-reference or octal escape")
        if c in "AZbB":
            self.fail(f"the anchor \\{c}")
        if c.isalnum() or ord(c) > 0x7F:
            self.fail(f"the escape \\{c}")
        return "cp", ord(c)                 # escaped punctuation

    def char_class(self) -> np.ndarray:
        self.i += 1                         # '['
        neg = self.peek() == "^"
        if neg:
            self.i += 1
        s = np.zeros(_UNITS, bool)
        first = True
        while True:
            c = self.peek()
            if c == "":
                self.fail("an unclosed '['")
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            if c == "[" and self.p[self.i + 1: self.i + 2] == ":":
                self.fail("a POSIX class")
            lo = self.class_atom()
            if isinstance(lo, np.ndarray):
                s |= lo
                continue
            if self.peek() == "-" and self.p[self.i + 1: self.i + 2] not in ("]", ""):
                self.i += 1
                hi = self.class_atom()
                if isinstance(hi, np.ndarray) or hi < lo:
                    self.fail("a bad character range")
                s[lo: hi + 1] = True
            else:
                s[lo] = True
        return (_BMP & ~s) if neg else s

    def class_atom(self):
        if self.peek() == "\\":
            kind, val = self.escape(True)
            if kind == "set":
                return val
        else:
            val = ord(self.peek())
            self.i += 1
        if val > 0xFFFF:
            self.fail("a character outside the Basic Multilingual Plane inside a class (write it as an alternative: it is two code units)")
        return val


class _NFA:
    """Thompson NFA over symbol sets: eps[s] = list of states, edges[s] = list of (set index, state)."""

    def __init__(self, pattern: str, sets: List[np.ndarray], set_ids: Dict[bytes, int], universe: np.ndarray):
        self.pattern, self.sets, self.set_ids, self.universe = pattern, sets, set_ids, universe
        self.eps: List[List[int]] = []
        self.edges: List[List[Tuple[int, int]]] = []

    def new(self) -> int:
        if len(self.eps) >= _NFA_LIMIT:
            raise ValueError(f"pattern {self.pattern!r}: its quantifier bounds need more than {_NFA_LIMIT} automaton positions, beyond any "
                             f"automaton of at most {SA_MAX_PATTERN_STATES} states")
        self.eps.append([]); self.edges.append([])
        return len(self.eps) - 1

    def set_id(self, s: np.ndarray) -> int:
        s = s & self.universe
        key = np.packbits(s).tobytes()
        if key not in self.set_ids:
            self.set_ids[key] = len(self.sets)
            self.sets.append(s)
        return self.set_ids[key]

    def build(self, node) -> Tuple[int, int]:
        """-> (entry, exit) of a fragment with fresh states."""
        kind = node[0]
        a, b = self.new(), self.new()
        if kind == "set":
            if (node[1] & self.universe).any():                   # a set with no representable unit: no edge, the fragment is dead
                self.edges[a].append((self.set_id(node[1]), b))
        elif kind == "cat":
            cur = a
            for sub in node[1]:
                x, y = self.build(sub)
                self.eps[cur].append(x)
                cur = y
            self.eps[cur].append(b)
        elif kind == "alt":
            for sub in node[1]:
                x, y = self.build(sub)
                self.eps[a].append(x); self.eps[y].append(b)
        else:
            _, sub, lo, hi = node
            cur = a
            for _ in range(lo):
                x, y = self.build(sub)
                self.eps[cur].append(x)
                cur = y
            if hi is None:
                x, y = self.build(sub)
                self.eps[cur].append(x); self.eps[y].append(x); self.eps[y].append(b); self.eps[cur].append(b)
            else:
                for _ in range(hi - lo):
                    x, y = self.build(sub)
                    self.eps[cur].append(x); self.eps[cur].append(b)
                    cur = y
                self.eps[cur].append(b)
        return a, b


def _closure(nfa: _NFA, states) -> frozenset:
    seen, stack = set(states), list(states)
    while stack:
        for t in nfa.eps[stack.pop()]:
            if t not in seen:
                seen.add(t); stack.append(t)
    return frozenset(seen)


class PatternTables:
    """The joint tables of a call's patterns and their host restatement.
      tok_class [vocab] uint8, next_state [n_states, n_classes] uint16, state_mask [n_states] uint8 (rows of `table`, the call's MaskTable),
      starts[i] = start state of patterns[i], accepting [n_states] bool.
    A transition the pattern does not have keeps the state (the mask never lets the device take one; the no-output token at a start state
    is the one id that gets there)."""

    def __init__(self, patterns, tok_class, next_state, state_mask, starts, accepting, table, eos, pad, nop):
        self.patterns, self.tok_class, self.next_state, self.state_mask = list(patterns), tok_class, next_state, state_mask
        self.starts, self.accepting, self.table = list(starts), accepting, table
        self.eos, self.pad, self.nop = eos, pad, nop
        self.n_states, self.n_classes = next_state.shape

    def start_of(self, pattern: str) -> int:
        return self.starts[self.patterns.index(pattern)]

    def allowed(self, state: int, token: int) -> bool:
        row = self.table.rows[int(self.state_mask[state])]
        return 0 <= token < len(self.tok_class) and bool((int(row[token >> 5]) >> (token & 31)) & 1)

    def advance(self, state: int, token: int) -> int:
        """What the greedy head does behind `token`: no pattern (-1) and a row that ended (eos / pad) keep the state."""
        if state < 0 or token == self.eos or token == self.pad or not 0 <= token < len(self.tok_class):
            return state
        return int(self.next_state[state, self.tok_class[token]])

    def accepts(self, state: int) -> bool:
        return state >= 0 and bool(self.accepting[state])

    def matched(self, start: int, tokens: Sequence[int]) -> bool:
        """A finished line: true iff it ended with EOS in an accepting state and every token before was allowed where it stood."""
        st = start
        for k, t in enumerate(tokens):
            t = int(t)
            if t == self.eos:
                return k == len(tokens) - 1 and self.accepts(st)
            if t == self.pad or t == self.nop or not self.allowed(st, t):
                return False
            st = self.advance(st, t)
        return False                            # cut by the token budget or the repeat rule: no EOS


def compile_patterns(tokenizer, patterns: Sequence[str], vocab_size: Optional[int] = None, extra_mask_rows=None,
                     max_states: int = SA_MAX_PATTERN_STATES) -> PatternTables:
    """One joint table set for the distinct `patterns` of a predictor call. extra_mask_rows: the call's MaskTable (tokenizer.py), which the
    states' allowed sets are merged into (identical sets once, also with the call's allowlist rows); None: a fresh one with the
    engine's row limit. ValueError with the count when states > max_states, classes > 256 or distinct rows > the table's limit."""
    from .tokenizer import MaskTable
    from .._lib import SA_MAX_TOKEN_MASKS
    V = tokenizer.vocab_size if vocab_size is None else int(vocab_size)
    sto = tokenizer.special_token_offset
    table = extra_mask_rows if extra_mask_rows is not None else MaskTable(tokenizer, V, SA_MAX_TOKEN_MASKS)
    sp = tokenizer.SPECIAL_TOKEN_MAPPING
    eos, pad, nop = sp.get("</S>", -1), sp.get("<PAD>", -1), sp.get("<NOP>", -1)
    universe = np.zeros(_UNITS, bool)
    universe[: max(0, min(_UNITS, V - sto))] = True               # code units that have an id inside the model's vocabulary
    patterns = list(dict.fromkeys(patterns))
    if not patterns:
        raise ValueError("compile_patterns needs at least one pattern")

    # 1. one NFA per pattern over a shared list of symbol sets
    sets: List[np.ndarray] = []
    set_ids: Dict[bytes, int] = {}
    nfas = []
    for pat in patterns:
        nfa = _NFA(pat, sets, set_ids, universe)
        a, b = nfa.build(_Parser(pat).parse())
        nfas.append((nfa, a, b))

    # 2. symbol classes: the joint refinement of every set; class 0 = the units in no set (and every id that is no code unit)
    if sets:
        member = np.stack(sets)                                    # [n_sets, 65536]
        sig = np.packbits(member, axis=0).T                        # one signature row per unit
        _, first, unit_class = np.unique(sig, axis=0, return_index=True, return_inverse=True)
        unit_class = unit_class.reshape(-1)
        dead = unit_class[np.flatnonzero(~member.any(axis=0))[:1]]
        n_classes = int(unit_class.max()) + 1
        if dead.size:                                              # swap so that the dead class is 0
            d = int(dead[0])
            unit_class = np.where(unit_class == d, 0, np.where(unit_class == 0, d, unit_class))
        else:
            unit_class = unit_class + 1
            n_classes += 1
        class_in_set = np.zeros((len(sets), n_classes), bool)
        for k, s in enumerate(sets):
            class_in_set[k, np.unique(unit_class[s])] = True
    else:
        unit_class, n_classes, class_in_set = np.zeros(_UNITS, np.int64), 1, np.zeros((0, 1), bool)
    if n_classes > SA_MAX_PATTERN_CLASSES:
        raise ValueError(f"the patterns split the alphabet into {n_classes} symbol classes, more than {SA_MAX_PATTERN_CLASSES}")

    # 3. subset construction per pattern into one disjoint union: trans [state][class] = state or -1
    trans: List[List[int]] = []
    accept: List[bool] = []
    starts: List[int] = []
    for nfa, a, b in nfas:
        ids: Dict[frozenset, int] = {}
        work = []

        def state_of(key):
            if key not in ids:
                if len(trans) >= 4 * max_states:
                    raise ValueError(f"pattern {nfa.pattern!r} needs more than {len(trans)} automaton states before minimisation, "
                                     f"far beyond the limit of {max_states}")
                ids[key] = len(trans)
                trans.append([-1] * n_classes); accept.append(b in key)
                work.append(key)
            return ids[key]
        starts.append(state_of(_closure(nfa, [a])))
        while work:
            key = work.pop()
            src = ids[key]
            by_class: Dict[int, set] = {}
            for s in key:
                for sid, dst in nfa.edges[s]:
                    for c in np.flatnonzero(class_in_set[sid]).tolist():
                        by_class.setdefault(c, set()).add(dst)
            for c, dsts in by_class.items():
                trans[src][c] = state_of(_closure(nfa, dsts))
    T = np.asarray(trans, np.int64).reshape(len(trans), n_classes)
    acc = np.asarray(accept, bool)

    # 4. trim: keep the states from which an accepting state is reachable
    live = acc.copy()
    layers = 1                                                     # distinct distances to acceptance: states that differ in it are not equivalent
    while True:
        reach = ((T >= 0) & live[np.maximum(T, 0)]).any(axis=1) | live
        if (reach == live).all():
            break
        live = reach
        layers += 1
    if layers > max_states:                                        # (known before the minimisation, which a long chain makes quadratic)
        raise ValueError(f"the patterns need at least {layers} automaton states, more than the limit of {max_states}")
    for pat, s in zip(patterns, starts):
        if not live[s]:
            raise ValueError(f"pattern {pat!r} matches no text this model can write")
    T = np.where((T >= 0) & live[np.maximum(T, 0)], T, -1)

    # 5. minimise (Moore): states of one block accept alike and move to the same blocks; only live states reachable from a start count
    seen = np.zeros(len(T), bool)
    stack = list(starts)
    seen[stack] = True
    while stack:
        for t in T[stack.pop()]:
            if t >= 0 and not seen[t]:
                seen[t] = True; stack.append(int(t))
    keep = np.flatnonzero(seen & live)
    remap = np.full(len(T), -1, np.int64)
    remap[keep] = np.arange(len(keep))
    T = np.where(T[keep] >= 0, remap[np.maximum(T[keep], 0)], -1)
    acc = acc[keep]
    starts = [int(remap[s]) for s in starts]
    block = acc.astype(np.int64)
    n_blocks = len(np.unique(block))
    while True:
        sig = np.concatenate([block[:, None], np.where(T >= 0, block[np.maximum(T, 0)], -1)], axis=1)
        _, block = np.unique(sig, axis=0, return_inverse=True)
        block = block.reshape(-1)
        nb = int(block.max()) + 1
        if nb == n_blocks:
            break
        n_blocks = nb
    rep = np.zeros(n_blocks, np.int64)
    rep[block[::-1]] = np.arange(len(block))[::-1]                 # a block's first state represents it
    T = np.where(T[rep] >= 0, block[np.maximum(T[rep], 0)], -1)
    acc = acc[rep]
    starts = [int(block[s]) for s in starts]

    # 6. a start state the automaton can re-enter gets a copy of its own: the no-output token is a first-token-only id
    entered = np.zeros(n_blocks, bool)
    entered[T[T >= 0]] = True
    copies: Dict[int, int] = {}
    for k, s in enumerate(starts):
        if entered[s]:
            if s not in copies:
                copies[s] = len(T)
                T = np.concatenate([T, T[s: s + 1]])
                acc = np.concatenate([acc, acc[s: s + 1]])
            starts[k] = copies[s]
    n_states = len(T)
    if n_states > max_states:
        raise ValueError(f"the patterns need {n_states} automaton states, more than the limit of {max_states}")

    # 7. tables: a missing transition keeps the state; the allowed set of a state is a row of the call's mask table
    words = (V + 31) // 32
    class_bits = np.zeros((n_classes, words * 32), bool)
    units = np.flatnonzero(universe)
    class_bits[unit_class[units], sto + units] = True
    class_bits[0] = False                                          # the dead class allows nothing
    is_start = np.zeros(n_states, bool)
    is_start[starts] = True
    state_mask = np.zeros(n_states, np.uint8)
    row_of: Dict[tuple, int] = {}
    for s in range(n_states):
        key = (tuple(np.flatnonzero(T[s] >= 0).tolist()), bool(acc[s]), bool(is_start[s]))
        if key not in row_of:
            bits = class_bits[list(key[0])].any(axis=0) if key[0] else np.zeros(words * 32, bool)
            if key[1]:
                bits[[t for t in (eos, pad) if 0 <= t < V]] = True
            if key[2] and 0 <= nop < V:
                bits[nop] = True
            assert bits.any(), "a trimmed state without an allowed id"
            row = np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1).astype(np.uint32)
            row_of[key] = table.add_row(row, what="allowed sets of pattern states and allowlists / blocklists")
        state_mask[s] = row_of[key]
    next_state = np.where(T >= 0, T, np.arange(n_states)[:, None]).astype(np.uint16)
    tok_class = np.zeros(V, np.uint8)
    ids = sto + units
    tok_class[ids] = unit_class[units]
    return PatternTables(patterns, tok_class, np.ascontiguousarray(next_state), state_mask, starts, acc.copy(), table, eos, pad, nop)
