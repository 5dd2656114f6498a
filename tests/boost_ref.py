"""Boosted decoding for the tests: csrc/boost_core.h compiled for the host (tests/native/boost_host.cpp), the float64 statement of its
rules on per-row records, and the record sets both boost test files use (tests/test_boost_cpu.py checks the header against the float64
rules; tests/test_gpu_rec_boost_ops.py checks the kernel against the header)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0x7fffffff                       # the index of a record without a column
_native = None


def native():
    global _native
    if _native is None:
        import tempfile
        out = os.path.join(tempfile.mkdtemp(prefix="boost_host_"), "libboost_host.so")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", out, os.path.join(ROOT, "tests", "native", "boost_host.cpp")],
                       check=True)
        _native = C.CDLL(out)
        _native.boost_combine_host.argtypes = [C.c_int] + [C.c_void_p] * 11
        _native.boost_combine_host.restype = None
    return _native


def native_combine(maxA, idxA, sumA, maxB, idxB, sumB, beta):
    """The header on n rows -> (token, tot, plain_token, plain_prob)."""
    f = [np.ascontiguousarray(a, np.float32) for a in (maxA, sumA, maxB, sumB, beta)]
    i = [np.ascontiguousarray(a, np.int32) for a in (idxA, idxB)]
    n = len(f[0])
    token, ptok = np.zeros(n, np.int32), np.zeros(n, np.int32)
    tot, pprob = np.zeros(n, np.float32), np.zeros(n, np.float32)
    native().boost_combine_host(n, f[0].ctypes.data, i[0].ctypes.data, f[1].ctypes.data, f[2].ctypes.data, i[1].ctypes.data, f[3].ctypes.data,
                                f[4].ctypes.data, token.ctypes.data, tot.ctypes.data, ptok.ctypes.data, pprob.ctypes.data)
    return token, tot, ptok, pprob


def ref_combine(maxA, idxA, sumA, maxB, idxB, sumB, beta):
    """The rules of the issue in float64 (only a = fl32(maxA + beta) is an fp32 operation: it decides the winner) -> the same four."""
    n = len(maxA)
    token, ptok = np.zeros(n, np.int64), np.asarray(idxB, np.int64).copy()
    tot, pprob = np.zeros(n, np.float64), np.zeros(n, np.float64)
    for k in range(n):
        mA, mB, sA, sB = (np.float64(v[k]) for v in (maxA, maxB, sumA, sumB))
        if mA == -np.inf:
            token[k], tot[k], pprob[k] = idxB[k], sB, 1.0 / sB
        elif beta[k] == np.inf:
            token[k], tot[k], pprob[k] = idxA[k], sA, np.exp(mA - mB) / sB
        else:
            a = np.float64(np.float32(maxA[k]) + np.float32(beta[k]))
            win_a = a > mB or (a == mB and idxA[k] < idxB[k])
            m = max(a, mB)
            token[k] = idxA[k] if win_a else idxB[k]
            tot[k] = sB * np.exp(mB - m) + sA * (np.exp(a - m) - np.exp(mA - m))
            pprob[k] = np.exp((mA if win_a else mB) - mB) / sB
    return token, tot, ptok, pprob


def edge_records(rng, n):
    """n rows of consistent records (A over a subset of B's columns: maxA <= maxB, sumA * exp(maxA - maxB) <= sumB) that hit the corners:
    an empty set, beta in {0, 1.5, 80, +inf}, exact ties fl32(maxA + beta) == maxB with idxA below and above idxB, idxA == idxB."""
    maxB = rng.normal(3.0, 4.0, n).astype(np.float32)
    idxB = rng.integers(0, 5000, n).astype(np.int32)
    sumB = (1.0 + rng.random(n) * 50).astype(np.float32)
    gap = np.where(rng.random(n) < 0.3, 0.0, rng.random(n) * 12).astype(np.float32)
    maxA = (maxB - gap).astype(np.float32)
    idxA = rng.integers(0, 5000, n).astype(np.int32)
    same = maxA == maxB                                     # S holds the row's maximum: the same column (or a later equal one)
    idxA = np.where(same & (rng.random(n) < 0.7), idxB, np.where(same, idxB + 1 + rng.integers(0, 9, n), idxA)).astype(np.int32)
    share = rng.random(n).astype(np.float32)                # A's part of B's mass
    sumA = np.maximum(1.0, share * sumB * np.exp((maxB - maxA).astype(np.float64))).astype(np.float32)
    sumB = np.maximum(sumB, (sumA.astype(np.float64) * np.exp((maxA - maxB).astype(np.float64))).astype(np.float32) * np.float32(1.0001)).astype(np.float32)
    beta = rng.choice(np.asarray([0.0, 1.5, 80.0, np.inf], np.float32), n).astype(np.float32)
    kind = rng.integers(0, 8, n)
    empty = kind == 0
    maxA[empty], idxA[empty], sumA[empty] = -np.inf, NONE, 0.0
    tie = (kind == 1) | (kind == 2)                         # beta such that fl32(maxA + beta) == maxB exactly: a power-of-two grid
    maxB[tie] = np.round(maxB[tie] * 4) / 4
    beta[tie] = rng.integers(0, 24, int(tie.sum())).astype(np.float32) / 4
    maxA[tie] = maxB[tie] - beta[tie]
    sumB[tie] = np.maximum(sumB[tie], (sumA[tie].astype(np.float64) * np.exp((maxA[tie] - maxB[tie]).astype(np.float64))).astype(np.float32)
                           * np.float32(1.0001))
    zero = tie & (beta == 0)
    idxA[tie & (kind == 1)] = idxB[tie & (kind == 1)] - 1 - rng.integers(0, 3, int((tie & (kind == 1)).sum()))
    idxA[tie & (kind == 2)] = idxB[tie & (kind == 2)] + 1 + rng.integers(0, 3, int((tie & (kind == 2)).sum()))
    idxA[zero & (kind == 1)] = idxB[zero & (kind == 1)]     # (beta 0 on a tie: A's maximum IS the row's first maximum, or a later equal one)
    idxA = np.maximum(idxA, 0).astype(np.int32)
    assert (maxA[tie] + beta[tie] == maxB[tie]).all()
    return maxA, idxA, sumA, maxB, idxB, sumB, beta
