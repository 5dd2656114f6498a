"""GPU: the MXFP8 GEMMs above 256 rows (csrc/gemm_mx.h, sa::Tuning mx_big_m_split / mx_big_m_gateup) through surya_op_gemm_mx.

What is pinned to what:
  * plain (mode 0) and split-K (mode 1) launches at M in {257, 384, 640} -- one row into the third 128-row tile (clamped rows), whole
    128-row tiles, a partial 256-row block -- on a partial column tile with two K-tiles (fewer than the ring depth: the ring's tail
    logic), on REC-SMALL's qkv and down shapes and on one real-size gate|up shape == the float64 product of the DEQUANTISED
    operands within 3e-4 x sum_k |x_k w_k| (test_gpu_mx.py's bound for the scaled MFMA), outputs pre-filled with NaN, under every
    value of mx_big_m_split;
  * row-block invariance, exact: the slice count is a function of (N, K) and every tile walks K in the same order, so rows of an
    M = 384 launch carry the bits of the <= 256-row launches of the same rows, whatever the tile;
  * SwiGLU -> MXFP8 (mode 2) under every value of mx_big_m_gateup: e4m3 and scale bytes of every row bit-identical to the <= 256-row
    launches of the same rows, dequantised values within one e4m3 step of the block of the float64 + oracle-quantiser result.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import mx_oracle as mo
from test_gpu_mx import _operands, _gemm, _row_major

pytestmark = pytest.mark.gpu

SPLIT_ARMS = (-1, 0, 2, 3)
GATEUP_ARMS = (-1, 0, 1, 2)


def _set(hip_lib, key, value):
    rc = hip_lib.surya_set_tuning(key.encode(), C.c_int(value))
    assert rc == 0, (key, value, rc)


@functools.lru_cache(maxsize=4)
def _case(M, N, K):
    """Operands, float64 reference and bound of one shape: computed once, shared by the arms (read-only)."""
    ops, xd, wd = _operands(M, N, K, 1000 + M + N)
    return ops, xd @ wd.T, np.abs(xd) @ np.abs(wd).T


def _rows(ops, a, b):
    return (ops[0][a:b], ops[1][a:b], ops[2], ops[3])


def _bits(t):
    return t.contiguous().view(torch.int32)


CASES = [(M, N, K) for (N, K) in [(192, 256), (1792, 1280), (1280, 768)] for M in (257, 384, 640)] + [(1024, 10240, 1280)]


@pytest.mark.parametrize("M,N,K", CASES)
def test_gemm_mx_above_256_rows_against_float64(hip_lib, M, N, K):
    ops, ref, bound = _case(M, N, K)
    ref_d, bound_d = torch.from_numpy(ref).cuda(), torch.from_numpy(bound).cuda()
    out = torch.full((M, N), float("nan"), device="cuda")
    _gemm(hip_lib, 0, ops, M, N, K, out)
    err = ((out.double() - ref_d).abs() / bound_d).max().item()          # NaN (an unwritten element) fails the comparison
    print(f"gemm_mx {M}x{N}x{K} plain: max err / sum|x w| = {err:.2e}")
    assert err <= 3e-4, err
    try:
        for arm in SPLIT_ARMS:
            _set(hip_lib, "mx_big_m_split", arm)
            slabs = torch.full((8, M, N), float("nan"), device="cuda")
            S = _gemm(hip_lib, 1, ops, M, N, K, slabs)
            assert 1 <= S <= 8
            got = torch.zeros((M, N), dtype=torch.float64, device="cuda")
            for i in range(S):
                got += slabs[i].double()
            err = ((got - ref_d).abs() / bound_d).max().item()
            print(f"gemm_mx {M}x{N}x{K} split-K {S}, mx_big_m_split = {arm}: max err / sum|x w| = {err:.2e}")
            assert err <= 3e-4, (arm, S, err)
            del slabs, got
    finally:
        _set(hip_lib, "mx_big_m_split", -1)


@pytest.mark.parametrize("N,K", [(192, 256), (1792, 1280)])
def test_rows_carry_the_bits_of_the_small_launches(hip_lib, N, K):
    M = 384
    ops, _, _ = _case(M, N, K)
    lo, hi = _rows(ops, 0, 256), _rows(ops, 256, 384)
    # mode 0: 128 x 128 tiles at 384 rows, 64 x 64 tiles at 256 / 128 rows
    out = torch.full((M, N), float("nan"), device="cuda")
    a = torch.full((256, N), float("nan"), device="cuda")
    b = torch.full((128, N), float("nan"), device="cuda")
    _gemm(hip_lib, 0, ops, M, N, K, out)
    _gemm(hip_lib, 0, lo, 256, N, K, a)
    _gemm(hip_lib, 0, hi, 128, N, K, b)
    assert not torch.isnan(out).any()
    assert torch.equal(_bits(out[:256]), _bits(a)) and torch.equal(_bits(out[256:]), _bits(b))
    sa = torch.full((8, 256, N), float("nan"), device="cuda")
    sb = torch.full((8, 128, N), float("nan"), device="cuda")
    Sa = _gemm(hip_lib, 1, lo, 256, N, K, sa)
    Sb = _gemm(hip_lib, 1, hi, 128, N, K, sb)
    assert Sa == Sb
    try:
        for arm in SPLIT_ARMS:
            _set(hip_lib, "mx_big_m_split", arm)
            slabs = torch.full((8, M, N), float("nan"), device="cuda")
            S = _gemm(hip_lib, 1, ops, M, N, K, slabs)
            assert S == Sa, (arm, S, Sa)
            assert not torch.isnan(slabs[:S]).any(), arm
            assert torch.equal(_bits(slabs[:S, :256]), _bits(sa[:S])), arm
            assert torch.equal(_bits(slabs[:S, 256:]), _bits(sb[:S])), arm
    finally:
        _set(hip_lib, "mx_big_m_split", -1)


@pytest.mark.parametrize("M,N,K", [(320, 512, 256), (1024, 10240, 1280)])
def test_swiglu_mx_above_256_rows(hip_lib, M, N, K):
    ops, acc, _ = _case(M, N, K)
    g, u = acc[:, 0::2], acc[:, 1::2]                      # weight rows interleaved (gate_j, up_j)
    y = (g / (1.0 + np.exp(-g))) * u
    q_ref, s_ref = mo.quantize(y.astype(np.float32))
    # the <= 256-row launches (64 x 64 tiles) of the same rows
    q_small = torch.zeros((M, N // 2), dtype=torch.uint8, device="cuda")
    s_small = np.zeros((M, N // 64), np.uint8)
    for r0 in range(0, M, 256):
        r1 = min(M, r0 + 256)
        s = torch.zeros((N // 256, r1 - r0, 4), dtype=torch.uint8, device="cuda")
        _gemm(hip_lib, 2, _rows(ops, r0, r1), r1 - r0, N, K, None, q_small[r0:r1], s)
        s_small[r0:r1] = _row_major(s.cpu().numpy())
    want = mo.dequantize(q_ref, s_ref)
    try:
        for arm in GATEUP_ARMS:
            _set(hip_lib, "mx_big_m_gateup", arm)
            q = torch.full((M, N // 2), 0xFF, dtype=torch.uint8, device="cuda")          # 0xFF = NaN in e4m3, and no scale byte of these blocks
            s = torch.full((N // 256, M, 4), 0xFF, dtype=torch.uint8, device="cuda")
            _gemm(hip_lib, 2, ops, M, N, K, None, q, s)
            sc = _row_major(s.cpu().numpy())
            assert torch.equal(q, q_small), arm
            assert np.array_equal(sc, s_small), arm
            got = mo.dequantize(q.cpu().numpy(), sc)
            step = np.ldexp(1.0, np.maximum(sc, s_ref).astype(np.int64) - 127)[..., None] * 32.0     # one step at the top binade
            diff = np.abs(got - want).reshape(M, N // 64, 32)
            assert (diff <= step).all(), (arm, diff.max())
    finally:
        _set(hip_lib, "mx_big_m_gateup", -1)
