"""GPU: the prompt fan-out kernel alone (kv_fanout_kernel, csrc/kv_fanout.h), through the launcher the engine uses
(surya_op_rec_kv_fanout), in the three cache dtypes.

The reference is a numpy copy of the same rows; the WHOLE cache afterwards equals the expectation byte for byte, so rows at and past the
length, slots in no fan and the sources themselves did not move."""
import ctypes as C

import numpy as np
import pytest
import torch

from surya_amd import _lib as L

pytestmark = pytest.mark.gpu
DT = {torch.float32: L.DTYPE_F32, torch.bfloat16: L.DTYPE_BF16, torch.float16: L.DTYPE_F16}
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.int32))).cuda()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _as_bytes(t):
    return t.cpu().contiguous().view(torch.uint8).numpy().copy()


def _cache(shape, dtype, seed):
    """Random finite values everywhere (the kernel moves bytes): a row copied from the wrong place, or not at all, shows."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype).cuda()


def _fan(k, v, dtype, src, off, dst, ln, dims):
    layers, S, nkv, Tmax, D = dims
    d_src, d_off, d_dst, d_ln = _dev(src), _dev(off), _dev(dst), _dev(ln)     # (named: a temporary's memory would be handed to the next one)
    rc = L.lib().surya_op_rec_kv_fanout(DT[dtype], L.ptr(k), L.ptr(v), L.ptr(d_src), L.ptr(d_off), L.ptr(d_dst), L.ptr(d_ln), len(src), len(dst),
                                        layers, S, nkv, Tmax, D, _stream())
    torch.cuda.synchronize()
    return rc


def _expect(t, src, off, dst, ln, dims):
    layers, S, nkv, Tmax, D = dims
    want = _as_bytes(t)
    w = want.reshape(layers, S, nkv, Tmax, -1)
    orig = w.copy()
    for n, s in enumerate(src):
        rows = min(max(int(ln[n]), 0), Tmax)
        for d in dst[off[n]:off[n + 1]]:
            if 0 <= d < S and d != s:
                w[:, d, :, :rows] = orig[:, s, :, :rows]
    return want


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("length", [0, 1, 23, 24, 40])
def test_fanout_copies_exactly_the_rows(hip_lib, dtype, length):
    """Case A: 2 layers x 6 slots x 2 kv heads x 24 rows x 16; fans {0 -> 2, 5} and {3 -> 1}, slot 4 in no fan; the list also names a
    destination equal to its source and one out of range, both skipped. Lengths 0 (nothing), 1, 23, 24 (the run) and 40 (clamped)."""
    dims = (2, 6, 2, 24, 16)
    k, v = _cache(dims, dtype, 1), _cache(dims, dtype, 2)
    src, off, dst = [0, 3], [0, 4, 6], [2, 0, 5, 6, 1, -1]                     # 0 -> 2, (0), 5, (6: out of range); 3 -> 1, (-1)
    ln = [length, length]
    before_k, before_v = _as_bytes(k), _as_bytes(v)
    want_k, want_v = _expect(k, src, off, dst, ln, dims), _expect(v, src, off, dst, ln, dims)
    assert _fan(k, v, dtype, src, off, dst, ln, dims) == 0
    got_k, got_v = _as_bytes(k), _as_bytes(v)
    assert got_k.tobytes() == want_k.tobytes() and got_v.tobytes() == want_v.tobytes()
    # said once more in the open: sources and slot 4 as they were, every row at and past the length as it was
    rows = min(length, 24)
    for got, before in ((got_k, before_k), (got_v, before_v)):
        g, b = got.reshape(2, 6, 2, 24, -1), before.reshape(2, 6, 2, 24, -1)
        assert np.array_equal(g[:, [0, 3, 4]], b[:, [0, 3, 4]]) and np.array_equal(g[:, :, :, rows:], b[:, :, :, rows:])
        if rows:
            assert np.array_equal(g[:, 2, :, :rows], b[:, 0, :, :rows]) and np.array_equal(g[:, 5, :, :rows], b[:, 0, :, :rows])
            assert np.array_equal(g[:, 1, :, :rows], b[:, 3, :, :rows]) and not np.array_equal(g[:, 1], b[:, 1])
        else:
            assert np.array_equal(g, b)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fanout_reaches_the_unrolled_loop_and_its_tail(hip_lib, dtype):
    """Case B: 1 layer x 3 slots x 1 kv head x 256 rows x 64, length 200: 12800 elements per run are 1600 (16-bit) or 3200 (fp32) 16-byte
    units, against the 1024 units of one unrolled pass: the 16-bit dtypes take one pass, fp32 three, and both a tail whose last round
    only some threads take part in."""
    dims = (1, 3, 1, 256, 64)
    k, v = _cache(dims, dtype, 3), _cache(dims, dtype, 4)
    src, off, dst, ln = [1], [0, 2], [0, 2], [200]
    want_k, want_v = _expect(k, src, off, dst, ln, dims), _expect(v, src, off, dst, ln, dims)
    assert _fan(k, v, dtype, src, off, dst, ln, dims) == 0
    assert _as_bytes(k).tobytes() == want_k.tobytes() and _as_bytes(v).tobytes() == want_v.tobytes()
    g = _as_bytes(k).reshape(3, 256, -1)
    assert np.array_equal(g[0, :200], g[1, :200]) and np.array_equal(g[2, :200], g[1, :200]) and not np.array_equal(g[0, 200:], g[1, 200:])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_fanout_long_runs_in_the_unrolled_loop(hip_lib, dtype):
    """The engine's own shape class: 128-wide heads, 2 layers x 4 slots x 2 kv heads x 96 rows, a fan of three at length 77 (1232 / 2464
    units: whole unrolled passes and a tail) beside a sequence without destinations, which leaves at once."""
    dims = (2, 4, 2, 96, 128)
    k, v = _cache(dims, dtype, 5), _cache(dims, dtype, 6)
    src, off, dst, ln = [2, 2], [0, 3, 3], [0, 1, 3], [77, 50]                 # 2 -> 0, 1, 3; then a sequence that names no destination
    want_k, want_v = _expect(k, src, off, dst, ln, dims), _expect(v, src, off, dst, ln, dims)
    assert _fan(k, v, dtype, src, off, dst, ln, dims) == 0
    assert _as_bytes(k).tobytes() == want_k.tobytes() and _as_bytes(v).tobytes() == want_v.tobytes()


def test_fanout_refusals(hip_lib):
    k = torch.zeros(2 * 4 * 2 * 8 * 32 + 8, dtype=torch.float16, device="cuda")
    src, off, dst, ln = _dev([0]), _dev([0, 1]), _dev([1]), _dev([8])
    lib = L.lib()

    def call(dt, D, kp=None, n_seqs=1, n_dst=1, layers=2):
        p = L.ptr(k) if kp is None else kp
        return lib.surya_op_rec_kv_fanout(dt, p, p, L.ptr(src), L.ptr(off), L.ptr(dst), L.ptr(ln), n_seqs, n_dst, layers, 4, 2, 8, D, _stream())
    assert call(7, 32) == L.SA_ERR_UNSUPPORTED                          # an unknown dtype
    assert call(L.DTYPE_F16, 4) == L.SA_ERR_SHAPE                       # rows of 8 bytes: no 16-byte units
    assert call(L.DTYPE_F16, 32, kp=C.c_void_p(k.data_ptr() + 2)) == L.SA_ERR_SHAPE      # a cache that is not 16-byte aligned
    assert call(L.DTYPE_F16, 32, layers=40000) == L.SA_ERR_SHAPE        # layers x kv heads beyond the grid
    assert call(L.DTYPE_F16, 32, kp=C.c_void_p(0)) == L.SA_ERR_ARG
    assert call(L.DTYPE_F16, 32, n_seqs=-1) == L.SA_ERR_ARG
    assert call(L.DTYPE_F16, 32, n_dst=0) == 0 and call(L.DTYPE_F16, 32, n_seqs=0) == 0      # nothing to do
    assert call(L.DTYPE_F16, 32) == 0
    torch.cuda.synchronize()
    assert not k.any()
