"""Boosted decoding: prefer the words of a user list without forcing them ("hot words", Tesseract's user_words).

A lexicon (lexicon.py) reads a line as exactly one entry; here the line runs free, and wherever the tokens so far could be the beginning of
a listed entry that began at a word boundary, the entry's next unit gets `boost_weight` added to its logit. Nothing is forbidden. The
lists of a call are compiled into ONE deterministic automaton in the lexicon's CSR form,

    edge_off   [n_states + 1] int32     edges of state s: edge_off[s] .. edge_off[s + 1]
    edge_tok   [n_edges]      int32     token ids, strictly ascending inside a state
    edge_next  [n_edges]      int32     target states

whose state's edge tokens ARE the preferred set of the position; a small kernel keeps them in the slot's own mask-table row
(csrc/boost.h) and the boosted head decodes from v + beta * [in the set] (csrc/boost_core.h).

Entries are taken verbatim (no case folding, no normalisation, no stripping), one token per UTF-16 code unit (special_token_offset + unit;
a character outside the BMP is its high surrogate, then its low one); they may hold spaces and punctuation. A *word unit* is a code unit
whose character matches re's Unicode \\w, or a surrogate; every other token id -- punctuation, space, math BPE, tags, the no-output
token -- is a *boundary*. A match of an entry is live if it began at a boundary position (the line start, or behind a boundary token) and
every token since has followed the entry; the preferred set is the set of next units of all live matches. That is the subset construction
over a list's trie with a restart at every boundary: a state is a set of trie nodes. Every list has a root state of its own ({trie root});
one shared state OUT has no edges (inside a word that follows no entry). Edges are stored only where some live match continues; a token
without an edge takes the fallback transition the device evaluates: OUT for a word unit, the line's root for a boundary. EOS and pad are
never preferred and keep the state.
"""
from __future__ import annotations

import re
from functools import lru_cache
from typing import Dict, List, Optional, Sequence

import numpy as np

from .lexicon import SA_MAX_LEXICON_EDGES, SA_MAX_LEXICON_STATES, CsrTables, entry_units


@lru_cache(maxsize=4)
def word_unit_bits(special_token_offset: int, vocab: int) -> np.ndarray:
    """bool [vocab]: id is a word unit."""
    bits = np.zeros(vocab, bool)
    units = np.zeros(65536, bool)
    units[0xD800:0xE000] = True
    bmp = "".join(chr(u) for u in range(65536) if not 0xD800 <= u < 0xE000)
    units[[ord(ch) for ch in re.findall(r"\w", bmp)]] = True
    n = max(0, min(65536, vocab - special_token_offset))
    bits[special_token_offset:special_token_offset + n] = units[:n]
    return bits


class BoostTables(CsrTables):
    """The joint CSR automaton of a call's lists and its host restatement (what csrc/boost.h does on the device). roots[i] = root state of
    lists[i]; out_state = the shared state without edges; word_bits = the word-unit set (word_mask: the same as a mask-table row;
    word_row: that row's id in the call's table, set by whoever adds it); edge_done[e] = the entries of the root's list (indices, ascending)
    that a match completes by taking edge e."""

    def __init__(self, edge_off, edge_tok, edge_next, roots, out_state, word_bits, edge_done, vocab, eos, pad):
        super().__init__(edge_off, edge_tok, edge_next, vocab, eos, pad)
        self.roots, self.out_state, self.word_bits, self.edge_done = list(roots), int(out_state), word_bits, edge_done
        self.word_row: Optional[int] = None

    @property
    def word_mask(self) -> np.ndarray:
        return self._row(np.flatnonzero(self.word_bits))

    def advance(self, state: int, token: int, root: int) -> int:
        """What the step kernel does behind `token` for a slot whose list has root state `root`: not boosted (-1), a row that ended (eos /
        pad) and an id outside the vocabulary keep the state; else the edge's target, or OUT for a word unit, or the root."""
        if self._stays(state, token):
            return state
        e = self._edge(state, token)
        if e >= 0:
            return int(self.edge_next[e])
        return self.out_state if self.word_bits[token] else root

    def preferred(self, state: int) -> set:
        """The ids boosted for a slot in `state`: the next units of all live matches."""
        return set(self.edges(state)[0].tolist()) if state >= 0 else set()

    def row(self, state: int) -> np.ndarray:
        """preferred(state) as a mask-table row, uint32 [cdiv(vocab, 32)]."""
        return self._row(self.preferred(state))

    def matches(self, root: int, tokens: Sequence[int]) -> List[int]:
        """The entries (indices in the root's own list) that some live match completed while the line's `tokens` went by, in order of
        completion (entries completed by the same token: by index), each once."""
        st, out, seen = root, [], set()
        for t in tokens:
            t = int(t)
            if not self._stays(st, t):
                e = self._edge(st, t)
                for i in (self.edge_done.get(e, ()) if e >= 0 else ()):
                    if i not in seen:
                        seen.add(i)
                        out.append(i)
            st = self.advance(st, t, root)
        return out

    def list_of_root(self, root: int) -> int:
        return self.roots.index(root)


def compile_boost(tokenizer, lists: Sequence[Sequence[str]], vocab_size: Optional[int] = None, max_states: int = SA_MAX_LEXICON_STATES,
                  max_edges: int = SA_MAX_LEXICON_EDGES) -> BoostTables:
    """One joint automaton for the `lists` of a predictor call. ValueError, before any device work, for no list, an empty list, an empty
    entry, an entry that needs a code unit whose id lies past the model's vocabulary (naming entry and index), and with the count for more
    than max_states states or max_edges edges."""
    V = tokenizer.vocab_size if vocab_size is None else int(vocab_size)
    sto = tokenizer.special_token_offset
    sp = tokenizer.SPECIAL_TOKEN_MAPPING
    eos, pad = sp.get("</S>", -1), sp.get("<PAD>", -1)
    lists = [list(x) for x in lists]
    if not lists:
        raise ValueError("compile_boost needs at least one list")
    word = word_unit_bits(sto, V)

    edges_of: List[Optional[list]] = [[]]           # state -> [(token, target)], ascending; state 0 is OUT
    done_of: Dict[tuple, tuple] = {}                # (state, token) -> completed entries
    n_edges = 0
    roots = []
    for li, lst in enumerate(lists):
        if not lst:
            raise ValueError(f"boost_words list {li} is empty")
        # the list's trie: children[n] = {token: node}, term[n] = index of the first entry that ends at n
        children: List[dict] = [{}]
        term: Dict[int, int] = {}
        for i, e in enumerate(lst):
            if not isinstance(e, str):
                raise ValueError(f"boost_words list {li}, entry {i}: {e!r} is not a str")
            if e == "":
                raise ValueError(f"boost_words list {li}, entry {i} is the empty string")
            units = entry_units(e)
            if sto + max(units) >= V:
                raise ValueError(f"boost_words list {li}, entry {i} ({e!r}) needs a character the model's vocabulary of {V} ids does not hold")
            n = 0
            for u in units:
                nxt = children[n].get(sto + u)
                if nxt is None:
                    nxt = children[n][sto + u] = len(children)
                    children.append({})
                n = nxt
            term.setdefault(n, i)
        # subset construction with a restart at every boundary; a state is a frozenset of trie nodes that have children
        ids: Dict[frozenset, int] = {}
        work: List[frozenset] = []

        def state_of(key: frozenset) -> int:
            s = ids.get(key)
            if s is None:
                if len(edges_of) >= max_states:
                    raise ValueError(f"boost_words need more than {max_states} automaton states (SA_MAX_LEXICON_STATES)")
                s = ids[key] = len(edges_of)
                edges_of.append(None)
                work.append(key)
            return s

        roots.append(state_of(frozenset((0,))))
        while work:
            key = work.pop()
            s = ids[key]
            toks = sorted(set().union(*(children[n].keys() for n in key)))
            n_edges += len(toks)
            if n_edges > max_edges:
                raise ValueError(f"boost_words need more than {max_edges} automaton edges (SA_MAX_LEXICON_EDGES), {n_edges} so far")
            out = []
            for t in toks:
                hit = [children[n][t] for n in key if t in children[n]]
                done = tuple(sorted(term[n] for n in hit if n in term))
                nxt = set(n for n in hit if children[n])
                if not word[t]:
                    nxt.add(0)
                out.append((t, state_of(frozenset(nxt)) if nxt else 0))
                if done:
                    done_of[(s, t)] = done
            edges_of[s] = out
    off = np.zeros(len(edges_of) + 1, np.int32)
    np.cumsum([len(e) for e in edges_of], out=off[1:])
    tok = np.fromiter((t for e in edges_of for t, _ in e), np.int32, count=int(off[-1]))
    nxt = np.fromiter((n for e in edges_of for _, n in e), np.int32, count=int(off[-1]))
    edge_done = {}
    for (s, t), d in done_of.items():
        a, b = int(off[s]), int(off[s + 1])
        edge_done[a + int(np.searchsorted(tok[a:b], t))] = d
    return BoostTables(off, tok, nxt, roots, 0, word, edge_done, V, eos, pad)
