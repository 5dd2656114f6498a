"""The beam-search rules of surya_amd/csrc/beam_core.h restated in plain Python (tests/test_beam_cpu.py checks the header against this;
the GPU tests and the fake model of the device-loop test use it as their reference), and a g++ build of the header itself."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 4                       # alternatives per row
NEG = np.float32(-np.inf)


def log_prob(p):
    """float(log(double(p))) of a float32 probability."""
    return np.float32(np.log(np.float64(np.float32(p))))


def select_group(B, slot0, score, fin, ids, ps, eos, pad, nop, first):
    """-> dict of per-slot lists: token, parent, rank, finished, fork_src, prob, logp."""
    cands = []                                          # (score, parent, rank); rank -1 = a frozen beam
    for b in range(1 if first else B):
        if not first and fin[b]:
            if score[b] > NEG:
                cands.append((np.float32(score[b]), b, -1))
            continue
        cum = np.float32(0) if first else np.float32(score[b])
        for j in range(A):
            if ids[b][j] >= 0 and ps[b][j] > 0:
                cands.append((np.float32(cum + log_prob(ps[b][j])), b, j))
    chosen = sorted(cands, key=lambda c: (-float(c[0]), c[1], c[2]))[:B]
    at = [None] * B
    further = []
    for c in chosen:                                    # a parent's first chosen child stays in the parent's slot
        if at[c[1]] is None:
            at[c[1]] = c
        else:
            further.append(c)
    free = [b for b in range(B) if at[b] is None]       # beams that did not survive, ascending
    for c in sorted(further, key=lambda c: c[1]):       # (stable: parent by parent, each parent's children in selection order)
        at[free.pop(0)] = c
    out = {k: [] for k in ("token", "parent", "rank", "finished", "fork_src", "prob", "logp")}
    for b in range(B):
        c = at[b]
        if c is None:
            row = (pad, -1, 0, 1, -1, np.float32(0), NEG)
        elif c[2] < 0:
            row = (pad, c[1], 0, 1, -1, np.float32(0), c[0])
        else:
            t = int(ids[c[1]][c[2]])
            row = (t, c[1], c[2], int(t in (eos, pad) or (first and t == nop)), -1 if c[1] == b else slot0 + c[1], np.float32(ps[c[1]][c[2]]),
                   c[0])
        for k, v in zip(out, row):
            out[k].append(v)
    return out


_native = None


def native():
    """beam_core.h compiled for the host (tests/native/beam_host.cpp)."""
    global _native
    if _native is None:
        import tempfile
        out = os.path.join(tempfile.mkdtemp(prefix="beam_host_"), "libbeam_host.so")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", out, os.path.join(ROOT, "tests", "native", "beam_host.cpp")],
                       check=True)
        _native = C.CDLL(out)
        _native.beam_select_host.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p] * 7
        _native.beam_select_host.restype = None
    return _native


def native_select(n_groups, B, score, fin, ids, ps, eos, pad, nop, first):
    """The header on n_groups groups laid out back to back (group g at slots [g * B, g * B + B)) -> dict of [n_groups * B] arrays."""
    n = n_groups * B
    score, fin = np.ascontiguousarray(score, np.float32), np.ascontiguousarray(fin, np.int32)
    ids, ps = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(ps, np.float32)
    assert score.shape == (n,) and fin.shape == (n,) and ids.shape == (n, A) and ps.shape == (n, A)
    o = {k: np.zeros(n, np.int32) for k in ("token", "parent", "rank", "finished", "fork_src")}
    o["prob"], o["logp"] = np.zeros(n, np.float32), np.zeros(n, np.float32)
    native().beam_select_host(n_groups, B, score.ctypes.data, fin.ctypes.data, ids.ctypes.data, ps.ctypes.data, eos, pad, nop, int(first),
                              *[o[k].ctypes.data for k in ("token", "parent", "rank", "finished", "fork_src", "prob", "logp")])
    return o


def random_groups(rng, n_groups, B, eos, pad, nop, first):
    """Groups that hit the corners: exact score ties (probabilities and scores on a coarse power-of-two grid), frozen and empty beams,
    rows with fewer than four (or no) candidates, one parent far ahead of the others (all children of one parent), eos / pad / nop ids."""
    n = n_groups * B
    ids = rng.integers(4, 40, size=(n, A)).astype(np.int32)
    ps = np.sort(rng.choice([0.5, 0.25, 0.125, 0.0625, 0.03125], size=(n, A)), axis=1)[:, ::-1].astype(np.float32)
    smooth = rng.random(n) < 0.4                         # some rows with unrelated probabilities
    ps[smooth] = np.sort(rng.random((int(smooth.sum()), A)).astype(np.float32) * 0.5, axis=1)[:, ::-1]
    special = rng.random((n, A))
    ids[special < 0.08] = eos
    ids[(special >= 0.08) & (special < 0.11)] = pad
    ids[(special >= 0.11) & (special < 0.14)] = nop
    few = rng.integers(0, A + 1, size=n)                 # entries kept per row; the others are "no such entry"
    cut = rng.random(n) < 0.3
    for r in np.flatnonzero(cut):
        ids[r, few[r]:], ps[r, few[r]:] = -1, 0
    score = (-rng.integers(0, 6, size=n) * np.float32(np.log(2.0))).astype(np.float32)      # a coarse grid: ties between parents
    ahead = rng.random(n_groups) < 0.25
    for g in np.flatnonzero(ahead):
        score[g * B + int(rng.integers(0, B))] = np.float32(40.0)
    fin = (rng.random(n) < 0.25).astype(np.int32)
    empty = (rng.random(n) < 0.1) & (fin == 1)
    score[empty] = NEG
    if first:
        thin = rng.random(n_groups) < 0.4                # a lead row with one or two candidates only
        for g in np.flatnonzero(thin):
            k = int(rng.integers(1, 3))
            ids[g * B, k:], ps[g * B, k:] = -1, 0
    return score, fin, ids, ps
