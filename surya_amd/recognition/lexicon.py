"""Lexicon-guided decoding: read a line as exactly one entry of a word list (a city, a surname, a product code, a postal code).

A pattern (pattern.py) gives every automaton state a full vocabulary bit row of the call's 64-row mask table, which a word list outgrows
at about 150 entries: it has about as many distinct allowed sets as it has inner trie nodes. Here the automaton is sparse. All lexicons
of a call are compiled into ONE minimised acyclic automaton (a DAWG: equal tails and equal lexicons share states) in CSR form,

    edge_off   [n_states + 1] int32     edges of state s: edge_off[s] .. edge_off[s + 1]
    edge_tok   [n_edges]      int32     token ids, strictly ascending inside a state
    edge_next  [n_edges]      int32     target states
    state_flags[n_states]     uint8     bit 0: terminal (EOS and pad allowed), bit 1: the no-output token allowed (start states)

and every decoder slot owns one row of the mask table, which a small kernel rewrites behind each token (csrc/lexicon.h): clear the old
state's handful of bits, set the new state's. The masked lm_head then reads that row like any static allowlist.

Entries are taken verbatim (no case folding, no normalisation, no stripping), one token per UTF-16 code unit
(special_token_offset + unit; a character outside the BMP is its high surrogate, then its low one), with re.fullmatch semantics: a line
is exactly one entry. Duplicates are allowed, the first index wins. Every lexicon has a start state of its own -- a copy of its root that
additionally allows the no-output token, so a blank crop still reads as blank (the rule of pattern.py; the automaton is acyclic, so a
start state is never re-entered and the copy is all it takes).

Construction is the incremental minimisation of Daciuk et al. over the sorted entries: linear in the total length; the register of
finished states is shared by the call's lexicons. A state is numbered when it is finished, so children precede their parents and
every state has an allowed id by construction (a leaf is terminal).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np

SA_MAX_LEXICON_STATES = 1 << 20    # include/surya_amd.h
SA_MAX_LEXICON_EDGES = 1 << 21
TERMINAL, NO_OUTPUT = 1, 2         # state_flags bits


def entry_units(entry: str) -> List[int]:
    """The UTF-16 code units of `entry`, verbatim."""
    b = entry.encode("utf-16-le", "surrogatepass")
    return np.frombuffer(b, "<u2").tolist()


class CsrTables:
    """A sparse automaton in CSR form over a vocabulary with its eos and pad ids: what the lexicon's and the boost's tables
    (recognition/boost.py) share, and the host restatement of what both do with it on the device (csrc/lexicon.h)."""

    def __init__(self, edge_off, edge_tok, edge_next, vocab, eos, pad):
        self.edge_off, self.edge_tok, self.edge_next = edge_off, edge_tok, edge_next
        self.vocab, self.eos, self.pad = int(vocab), eos, pad
        self.n_states, self.n_edges = len(edge_off) - 1, len(edge_tok)

    def edges(self, state: int):
        a, b = int(self.edge_off[state]), int(self.edge_off[state + 1])
        return self.edge_tok[a:b], self.edge_next[a:b]

    def _edge(self, state: int, token: int) -> int:
        """Index of the edge of `state` for `token`, or -1."""
        a, b = int(self.edge_off[state]), int(self.edge_off[state + 1])
        k = a + int(np.searchsorted(self.edge_tok[a:b], token))
        return k if k < b and int(self.edge_tok[k]) == token else -1

    def _stays(self, state: int, token: int) -> bool:
        """The step kernel touches nothing: no automaton (-1), a row that ended (eos / pad), an id outside the vocabulary."""
        return state < 0 or token == self.eos or token == self.pad or not 0 <= token < self.vocab

    def _row(self, ids) -> np.ndarray:
        """The ids as a mask-table row, uint32 [cdiv(vocab, 32)]."""
        bits = np.zeros((self.vocab + 31) // 32 * 32, bool)
        bits[np.fromiter(ids, np.int64)] = True
        return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1).astype(np.uint32)


class LexiconTables(CsrTables):
    """The joint CSR automaton of a call's lexicons and its host restatement (what csrc/lexicon.h does on the device).
    starts[i] = start state of lexicons[i]; entries[i] maps an entry's token tuple to its first index in lexicons[i]."""

    def __init__(self, edge_off, edge_tok, edge_next, state_flags, starts, entries, vocab, eos, pad, nop):
        super().__init__(edge_off, edge_tok, edge_next, vocab, eos, pad)
        self.state_flags, self.nop = state_flags, nop
        self.starts, self.entries = list(starts), entries

    def advance(self, state: int, token: int) -> int:
        """What the step kernel does behind `token`: no lexicon (-1), a row that ended (eos / pad), an id outside the vocabulary and
        an id the state has no edge for (the mask never lets the device emit one; the no-output token at a start state is the one id
        that gets there) keep the state."""
        if self._stays(state, token):
            return state
        e = self._edge(state, token)
        return int(self.edge_next[e]) if e >= 0 else state

    def allowed(self, state: int) -> set:
        """The ids a slot in `state` may emit: its children, EOS and pad where it is terminal, the no-output token at a start state."""
        ids = set(self.edges(state)[0].tolist())
        f = int(self.state_flags[state])
        if f & TERMINAL:
            ids.update(t for t in (self.eos, self.pad) if 0 <= t < self.vocab)
        if f & NO_OUTPUT and 0 <= self.nop < self.vocab:
            ids.add(self.nop)
        return ids

    def accepts(self, state: int) -> bool:
        return state >= 0 and bool(int(self.state_flags[state]) & TERMINAL)

    def row(self, state: int) -> np.ndarray:
        """allowed(state) as a mask-table row, uint32 [cdiv(vocab, 32)]."""
        return self._row(self.allowed(state))

    def entry_of(self, lexicon: int, tokens: Sequence[int]) -> int:
        """A finished line of lexicons[lexicon]: the index of the entry read, the first one for a duplicate, iff the line ended (EOS or
        pad) in a terminal state and every token before had an edge where it stood; else -1 (a line cut by the token budget, the
        repeat rule or the no-output token)."""
        st, path = self.starts[lexicon], []
        for t in tokens:
            t = int(t)
            if t == self.eos or t == self.pad:
                return self.entries[lexicon].get(tuple(path), -1) if self.accepts(st) else -1
            ns = self.advance(st, t)
            if ns == st:                        # no edge (the automaton is acyclic: a taken edge always changes the state)
                return -1
            st = ns
            path.append(t)
        return -1

    def lexicon_of_start(self, start: int) -> int:
        return self.starts.index(start)


class _Node:
    __slots__ = ("edges", "term")

    def __init__(self):
        self.edges: Dict[int, object] = {}      # token -> _Node (open) or int (finished state id); ascending, as the entries are sorted
        self.term = False


def compile_lexicons(tokenizer, lexicons: Sequence[Sequence[str]], vocab_size: Optional[int] = None,
                     max_states: int = SA_MAX_LEXICON_STATES, max_edges: int = SA_MAX_LEXICON_EDGES) -> LexiconTables:
    """One joint automaton for the `lexicons` of a predictor call. ValueError, before any device work, for no lexicon, an empty
    lexicon, an empty entry, an entry that needs a code unit whose id lies past the model's vocabulary (naming entry and index),
    and with the count for more than max_states states or max_edges edges."""
    V = tokenizer.vocab_size if vocab_size is None else int(vocab_size)
    sto = tokenizer.special_token_offset
    sp = tokenizer.SPECIAL_TOKEN_MAPPING
    eos, pad, nop = sp.get("</S>", -1), sp.get("<PAD>", -1), sp.get("<NOP>", -1)
    lexicons = [list(lx) for lx in lexicons]
    if not lexicons:
        raise ValueError("compile_lexicons needs at least one lexicon")

    off: List[int] = [0]                        # CSR under construction: a finished state's edges are appended once
    tok: List[int] = []
    nxt: List[int] = []
    flags: List[int] = []
    register: Dict[tuple, int] = {}

    def new_state(key, f) -> int:
        term, edges = key
        if len(flags) >= max_states:
            raise ValueError(f"the lexicons need more than {max_states} automaton states (SA_MAX_LEXICON_STATES)")
        if len(tok) + len(edges) > max_edges:
            raise ValueError(f"the lexicons need more than {max_edges} automaton edges (SA_MAX_LEXICON_EDGES), {len(tok) + len(edges)} so far")
        for t, n in edges:
            tok.append(t); nxt.append(n)
        off.append(len(tok))
        flags.append(f)
        return len(flags) - 1

    def finish(node: _Node) -> int:
        """The id of the finished state equivalent to `node`, whose children are all finished."""
        key = (node.term, tuple(node.edges.items()))
        s = register.get(key)
        if s is None:
            s = register[key] = new_state(key, TERMINAL if node.term else 0)
        return s

    starts, entries = [], []
    for li, lex in enumerate(lexicons):
        if not lex:
            raise ValueError(f"lexicon {li} is empty")
        index: Dict[tuple, int] = {}
        for i, e in enumerate(lex):
            if not isinstance(e, str):
                raise ValueError(f"lexicon {li}, entry {i}: {e!r} is not a str")
            if e == "":
                raise ValueError(f"lexicon {li}, entry {i} is the empty string")
            units = entry_units(e)
            if sto + max(units) >= V:
                raise ValueError(f"lexicon {li}, entry {i} ({e!r}) needs a character the model's vocabulary of {V} ids does not hold")
            index.setdefault(tuple(sto + u for u in units), i)
        root = _Node()
        path: List[_Node] = [root]              # the open nodes: the path of the previous word
        prev: tuple = ()
        for word in sorted(index):
            k = 0
            while k < len(prev) and k < len(word) and prev[k] == word[k]:
                k += 1
            for d in range(len(prev), k, -1):   # the previous word's tail below the common prefix is final: finish it bottom-up
                path[d - 1].edges[prev[d - 1]] = finish(path[d])
            del path[k + 1:]
            for t in word[k:]:
                n = _Node()
                path[-1].edges[t] = n
                path.append(n)
            path[-1].term = True
            prev = word
        for d in range(len(prev), 0, -1):
            path[d - 1].edges[prev[d - 1]] = finish(path[d])
        # the start state: the root's copy, never shared, which also allows the no-output token
        starts.append(new_state((False, tuple(root.edges.items())), NO_OUTPUT if 0 <= nop < V else 0))
        entries.append(index)
    return LexiconTables(np.asarray(off, np.int32), np.asarray(tok, np.int32), np.asarray(nxt, np.int32), np.asarray(flags, np.uint8),
                         starts, entries, V, eos, pad, nop)
