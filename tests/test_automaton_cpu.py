"""The table checks of lexicon-guided and boosted decoding, host side (no GPU): csrc/automaton_core.h compiled for the host
(tests/native/automaton_host.cpp). The kernels read the tables unchecked, so these checks are what stands between a bad table and a stray
read on the device.

Good tables -- compile_lexicons and compile_boost on a dozen words, the hand-made automata of tests/test_gpu_rec_lexicon_ops.py and
tests/test_gpu_rec_boost_ops.py, a star whose leaves are its first and last states -- get SA_OK. Every bad variant the two GPU tests
test_entry_points_refuse_bad_tables_and_modes build gets SA_ERR_ARG, with the bad value at the first, a middle and the last state or edge
it can sit at, so that an off-by-one in a walk shows."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from surya_amd import _lib as L
from surya_amd.recognition.boost import BoostTables, compile_boost
from surya_amd.recognition.lexicon import LexiconTables, compile_lexicons
from surya_amd.recognition.tokenizer import OCRTokenizer

import test_gpu_rec_boost_ops as bops
import test_gpu_rec_lexicon_ops as lops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = ["Ohio", "Oregon", "Oklahoma", "Iowa", "Idaho", "Indiana", "Illinois", "Utah", "Maine", "Maryland", "New York", "New Jersey"]
N_ROWS = 8                              # rows of the mask table a boost's word_row may name
_native = None


def native():
    global _native
    if _native is None:
        out = os.path.join(tempfile.mkdtemp(prefix="automaton_host_"), "libautomaton_host.so")
        subprocess.run(["g++", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-o", out, os.path.join(ROOT, "tests", "native", "automaton_host.cpp")],
                       check=True)
        _native = C.CDLL(out)
        for f in (_native.csr_check_host, _native.lexicon_tables_check_host, _native.boost_tables_check_host):
            f.restype = C.c_int
    return _native


def _star(V) -> LexiconTables:
    """Leaves 0, 1, 3, 4 (terminal, no edges) around the root 2: an edgeless state at the first and at the last index."""
    return LexiconTables(np.asarray([0, 0, 0, 4, 4, 4], np.int32), np.asarray([300, 301, 302, 303], np.int32), np.asarray([0, 1, 3, 4], np.int32),
                         np.asarray([1, 1, 2, 1, 1], np.uint8), [2], [{}], V, lops.EOS, lops.PAD, lops.NOP)


def lexicon_case(t, **kw):
    d = dict(edge_off=t.edge_off, edge_tok=t.edge_tok, edge_next=t.edge_next, flags=t.state_flags, vocab=t.vocab, eos=t.eos, pad=t.pad, nop=t.nop)
    d.update(kw)
    return ("lexicon", d)


def boost_case(t, **kw):
    d = dict(edge_off=t.edge_off, edge_tok=t.edge_tok, edge_next=t.edge_next, vocab=t.vocab, out_state=t.out_state, word_row=N_ROWS - 1,
             n_rows=N_ROWS, eos=t.eos, pad=t.pad)
    d.update(kw)
    return ("boost", d)


def run(case) -> int:
    kind, d = case
    off, tok, nxt = (np.ascontiguousarray(d[k], np.int32) for k in ("edge_off", "edge_tok", "edge_next"))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    n_states, n_edges = len(off) - 1, len(tok)
    if kind == "lexicon":
        fl = np.ascontiguousarray(d["flags"], np.uint8)
        return native().lexicon_tables_check_host(p(off), p(tok), p(nxt), p(fl), n_states, n_edges, d["vocab"], d["eos"], d["pad"], d["nop"])
    return native().boost_tables_check_host(p(off), p(tok), p(nxt), n_states, n_edges, d["vocab"], d["out_state"], d["word_row"], d["n_rows"],
                                            d["eos"], d["pad"])


def three(xs):
    """The first, a middle and the last of xs."""
    xs = list(xs)
    assert xs
    return sorted({xs[0], xs[len(xs) // 2], xs[-1]})


def put(a, i, v):
    a = np.array(a)
    a[i] = v
    return a


def good_tables():
    tok = OCRTokenizer()
    V = tok.vocab_size
    lex = [("compiled", compile_lexicons(tok, [WORDS, WORDS[:3]], V)), ("ops-1024", lops._automaton(1024)), ("ops-81920", lops._automaton(81920)),
           ("star", _star(1024))]
    bst = [("compiled", compile_boost(tok, [WORDS, WORDS[:3]], V)), ("ops-1024", bops._automaton(1024)), ("ops-81920", bops._automaton(81920))]
    return lex, bst


def structure_variants(t, make):
    """The variants of the structure both features share: (label, case)."""
    n, ne, off = t.n_states, t.n_edges, t.edge_off
    with_edges = np.flatnonzero(np.diff(off) > 0)
    with_two = np.flatnonzero(np.diff(off) > 1)
    out = []
    for s in three(range(n)):
        out.append((f"offsets step back at state {s}", make(t, edge_off=put(off, s + 1, off[s] - 1))))
    for s in three(with_edges):
        out.append((f"offsets step back behind the edges of state {s}", make(t, edge_off=put(off, s + 1, off[s] - 1))))
    out.append(("last offset below n_edges", make(t, edge_off=put(off, n, ne - 1))))
    out.append(("last offset above n_edges", make(t, edge_off=put(off, n, ne + 1))))
    out.append(("first offset not 0", make(t, edge_off=put(off, 0, 1))))
    for e in three(range(ne)):
        out.append((f"token at vocab, edge {e}", make(t, edge_tok=put(t.edge_tok, e, t.vocab))))
        out.append((f"token -1, edge {e}", make(t, edge_tok=put(t.edge_tok, e, -1))))
        out.append((f"target n_states, edge {e}", make(t, edge_next=put(t.edge_next, e, n))))
        out.append((f"target -1, edge {e}", make(t, edge_next=put(t.edge_next, e, -1))))
    for s in three(with_two):
        a, b = int(off[s]), int(off[s + 1])
        out.append((f"first two tokens of state {s} equal", make(t, edge_tok=put(t.edge_tok, a + 1, t.edge_tok[a]))))
        out.append((f"last two tokens of state {s} descend", make(t, edge_tok=put(t.edge_tok, b - 1, t.edge_tok[b - 2] - 1))))
    return out


def lexicon_variants(t):
    n = t.n_states
    leaves = np.flatnonzero(np.diff(t.edge_off) == 0)
    out = structure_variants(t, lexicon_case)
    for s in three(leaves):
        out.append((f"state {s} without an allowed id", lexicon_case(t, flags=put(t.state_flags, s, 0))))
    out.append(("a terminal state without edges, eos and pad outside the vocabulary", lexicon_case(t, eos=-1, pad=t.vocab)))
    for s in three(range(n)):
        out.append((f"flag bit 2 at state {s}", lexicon_case(t, flags=put(t.state_flags, s, t.state_flags[s] | 4))))
        for nop in (t.vocab, -1):
            out.append((f"no-output flag at state {s}, nop {nop}", lexicon_case(t, flags=put(t.state_flags, s, t.state_flags[s] | 2), nop=nop)))
    return out


def boost_variants(t):
    with_edges = np.flatnonzero(np.diff(t.edge_off) > 0)
    out = structure_variants(t, boost_case)
    for e in three(range(t.n_edges)):                       # (eos / pad move onto the edge, so the structure stays good)
        out.append((f"edge {e} on eos", boost_case(t, eos=int(t.edge_tok[e]))))
        out.append((f"edge {e} on pad", boost_case(t, pad=int(t.edge_tok[e]))))
    for s in three(with_edges):
        out.append((f"out_state {s} has edges", boost_case(t, out_state=int(s))))
    for o in (t.n_states, -1):
        out.append((f"out_state {o}", boost_case(t, out_state=o)))
    for w in (N_ROWS, -1):
        out.append((f"word_row {w}", boost_case(t, word_row=w)))
    return out


def all_cases():
    """(label, case, expected code) for every table of the module; also what the sanitizer run of the checks is fed."""
    lex, bst = good_tables()
    out = []
    for name, t in lex:
        out.append((f"lexicon {name}", lexicon_case(t), L.SA_OK))
        out += [(f"lexicon {name}: {label}", case, L.SA_ERR_ARG) for label, case in lexicon_variants(t)]
    for name, t in bst:
        out.append((f"boost {name}", boost_case(t), L.SA_OK))
        out.append((f"boost {name}, word_row 0", boost_case(t, word_row=0), L.SA_OK))
        out += [(f"boost {name}: {label}", case, L.SA_ERR_ARG) for label, case in boost_variants(t)]
    return out


def test_good_tables_pass_and_every_bad_variant_is_refused():
    cases = all_cases()
    assert sum(code == L.SA_OK for _, _, code in cases) == 10 and len(cases) > 200
    wrong = [(label, got) for label, case, code in cases for got in [run(case)] if got != code]
    assert not wrong, wrong[:10]


def test_the_variants_hold_the_cases():
    """What the docstring promises about the positions, checked on the tables themselves."""
    lex, bst = good_tables()
    for _, t in lex + bst:
        assert isinstance(t, (LexiconTables, BoostTables)) and t.n_edges >= 3 and t.n_states >= 5
        labels = [label for label, _ in structure_variants(t, lexicon_case if isinstance(t, LexiconTables) else boost_case)]
        assert "token at vocab, edge 0" in labels and f"token at vocab, edge {t.n_edges - 1}" in labels
        assert "offsets step back at state 0" in labels and f"offsets step back at state {t.n_states - 1}" in labels
    star = dict(lex)["star"]
    leaves = np.flatnonzero(np.diff(star.edge_off) == 0)
    assert leaves[0] == 0 and leaves[-1] == star.n_states - 1
    ops = dict(bst)["ops-1024"]
    assert ops.out_state == 0 and len(ops.edges(ops.n_states - 1)[0]) > 0      # states with edges up to the last one


def test_structure_alone_is_what_both_features_share():
    lex, bst = good_tables()
    for _, t in lex + bst:
        off, tok, nxt = (np.ascontiguousarray(a, np.int32) for a in (t.edge_off, t.edge_tok, t.edge_next))
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert native().csr_check_host(p(off), p(tok), p(nxt), t.n_states, t.n_edges, t.vocab) == L.SA_OK
        assert native().csr_check_host(p(off), p(tok), p(nxt), t.n_states, t.n_edges, int(tok.max())) == L.SA_ERR_ARG
