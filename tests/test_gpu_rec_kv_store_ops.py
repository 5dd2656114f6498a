"""GPU: the two kernels of the prompt store alone (kv_keep_kernel / kv_restore_kernel, csrc/kv_store.h), through the launchers the engine
uses (surya_op_rec_kv_keep / surya_op_rec_kv_restore), in the three cache dtypes.

The reference is a numpy copy of the same rows; the WHOLE cache, the WHOLE store and the WHOLE hidden-row array afterwards equal the
expectation byte for byte, so nothing outside the named runs moved. Shape: 2 layers x 8 slots x 2 kv heads x 80 rows x 128, the engine's
head width: 64 rows x 16 units are exactly one pass of the four-deep loop in the 16-bit dtypes (two in fp32), so the lengths 0, 1, 63, 64,
65 and 80 are nothing, tail only, a tail whose last round is partial, loop only, loop + tail and a full run."""
import ctypes as C

import numpy as np
import pytest
import torch

from surya_amd import _lib as L

pytestmark = pytest.mark.gpu
DT = {torch.float32: L.DTYPE_F32, torch.bfloat16: L.DTYPE_BF16, torch.float16: L.DTYPE_F16}
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
LAYERS, SLOTS, NKV, TMAX, D, CAP, H, XROWS = 2, 8, 2, 80, 128, 250, 64, 12
DIMS = (LAYERS, SLOTS, NKV, TMAX, D)
SDIMS = (LAYERS, NKV, CAP, D)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.int32))).cuda()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _as_bytes(t):
    return t.cpu().contiguous().view(torch.uint8).numpy().copy()


def _rand(shape, dtype, seed):
    """Random finite values everywhere (the kernels move bytes): a row copied from the wrong place, or not at all, shows."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype).cuda()


def _run_of(first, ln):
    """(first row, rows) the kernels move for an entry: the clamps of csrc/kv_store.h, written out once more."""
    if first < 0 or first >= CAP:
        return 0, 0
    return first, min(min(max(int(ln), 0), TMAX), CAP - first)


def _keep(dtype, k, v, sk, sv, slot, first, ln, x=None, last_row=None, hid=None):
    d_slot, d_first, d_ln = _dev(slot), _dev(first), _dev(ln)                  # (named: a temporary's memory would be handed to the next one)
    d_last = _dev(last_row) if last_row is not None else None
    rc = L.lib().surya_op_rec_kv_keep(DT[dtype], L.ptr(k), L.ptr(v), L.ptr(sk), L.ptr(sv), L.ptr(d_slot), L.ptr(d_first), L.ptr(d_ln), len(slot),
                                      LAYERS, SLOTS, NKV, TMAX, D, CAP, L.ptr(x), L.ptr(d_last), L.ptr(hid), H, XROWS, _stream())
    torch.cuda.synchronize()
    return rc


def _restore(dtype, k, v, sk, sv, first, ln, off, dst):
    d_first, d_ln, d_off, d_dst = _dev(first), _dev(ln), _dev(off), _dev(dst)
    rc = L.lib().surya_op_rec_kv_restore(DT[dtype], L.ptr(k), L.ptr(v), L.ptr(sk), L.ptr(sv), L.ptr(d_first), L.ptr(d_ln), L.ptr(d_off), L.ptr(d_dst),
                                         len(first), len(dst), LAYERS, SLOTS, NKV, TMAX, D, CAP, _stream())
    torch.cuda.synchronize()
    return rc


def _expect_keep(cache, store, slot, first, ln):
    """The store's bytes after keeping `slot` -> (first, ln) out of `cache`."""
    want = _as_bytes(store)
    w, c = want.reshape(LAYERS, NKV, CAP, -1), _as_bytes(cache).reshape(LAYERS, SLOTS, NKV, TMAX, -1)
    for s, f, n in zip(slot, first, ln):
        f0, rows = _run_of(f, n)
        if 0 <= s < SLOTS and rows:
            w[:, :, f0:f0 + rows] = c[:, s, :, :rows]
    return want


def _expect_restore(cache, store, first, ln, off, dst):
    """The cache's bytes after landing the entries (first, ln) of `store` in their fans."""
    want = _as_bytes(cache)
    w, st = want.reshape(LAYERS, SLOTS, NKV, TMAX, -1), _as_bytes(store).reshape(LAYERS, NKV, CAP, -1)
    for n, (f, m) in enumerate(zip(first, ln)):
        f0, rows = _run_of(f, m)
        for d in dst[max(off[n], 0):max(off[n + 1], 0)]:
            if 0 <= d < SLOTS and rows:
                w[:, d, :, :rows] = st[:, :, f0:f0 + rows]
    return want


def _same(t, want):
    return _as_bytes(t).tobytes() == want.tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("length", [0, 1, 63, 64, 65, 80])
def test_keep_then_restore_is_the_identity_on_the_rows(hip_lib, dtype, length):
    """Three entries of one length out of slots 5, 0 and 2 of one cache into store rows 3.., 90.. and 170.., with their hidden rows; then
    the entries into ANOTHER cache's slots in fans of 1, 2 and 5. Store, hidden rows and both caches equal the numpy expectation whole;
    the fan slots' rows [0, length) are the kept slots' rows and every row at and past the length is what it was."""
    k, v = _rand(DIMS, dtype, 1), _rand(DIMS, dtype, 2)
    sk, sv = _rand(SDIMS, dtype, 3), _rand(SDIMS, dtype, 4)
    x, hid = _rand((XROWS, H), dtype, 5), _rand((CAP, H), dtype, 6)
    slot, first, ln, last = [5, 0, 2], [3, 90, 170], [length] * 3, [11, 0, 4]
    want_sk, want_sv = _expect_keep(k, sk, slot, first, ln), _expect_keep(v, sv, slot, first, ln)
    want_hid = _as_bytes(hid)
    if length:
        for f, r in zip(first, last):
            want_hid.reshape(CAP, -1)[f] = _as_bytes(x).reshape(XROWS, -1)[r]
    before_k, before_v, before_x = _as_bytes(k), _as_bytes(v), _as_bytes(x)
    assert _keep(dtype, k, v, sk, sv, slot, first, ln, x, last, hid) == 0
    assert _same(sk, want_sk) and _same(sv, want_sv) and _same(hid, want_hid)
    assert _same(k, before_k) and _same(v, before_v) and _same(x, before_x)       # keeping reads the cache and the hidden rows, no more
    k2, v2 = _rand(DIMS, dtype, 7), _rand(DIMS, dtype, 8)
    off, dst = [0, 1, 3, 8], [6, 0, 3, 1, 2, 4, 5, 7]
    want_k2, want_v2 = _expect_restore(k2, sk, first, ln, off, dst), _expect_restore(v2, sv, first, ln, off, dst)
    before_k2 = _as_bytes(k2).reshape(LAYERS, SLOTS, NKV, TMAX, -1)
    assert _restore(dtype, k2, v2, sk, sv, first, ln, off, dst) == 0
    assert _same(k2, want_k2) and _same(v2, want_v2)
    assert _same(sk, want_sk) and _same(sv, want_sv)                             # restoring reads the store, no more
    # said once more in the open: the identity, and the rows behind the length
    g, src = _as_bytes(k2).reshape(LAYERS, SLOTS, NKV, TMAX, -1), before_k.reshape(LAYERS, SLOTS, NKV, TMAX, -1)
    assert np.array_equal(g[:, :, :, length:], before_k2[:, :, :, length:])
    for s, fan in zip(slot, ([6], [0, 3], [1, 2, 4, 5, 7])):
        for d_ in fan:
            assert np.array_equal(g[:, d_, :, :length], src[:, s, :, :length])
    if length:
        assert not np.array_equal(g[:, :, :, :length], before_k2[:, :, :, :length])


@pytest.mark.parametrize("dtype", DTYPES)
def test_out_of_range_ids_are_skipped_and_entries_are_clamped_to_the_capacity(hip_lib, dtype):
    """keep: a slot out of range, a first row below 0 and one at the capacity are skipped whole, hidden row included; an entry that
    reaches past the capacity keeps the rows that fit; a length above max_kv_len is clamped; a last_row out of range copies no hidden
    row. restore: destinations -1 and 8 are skipped, an entry past the capacity lands the rows that fit, slot 7 is in no fan."""
    k, v = _rand(DIMS, dtype, 11), _rand(DIMS, dtype, 12)
    sk, sv = _rand(SDIMS, dtype, 13), _rand(SDIMS, dtype, 14)
    x, hid = _rand((XROWS, H), dtype, 15), _rand((CAP, H), dtype, 16)
    slot, first, ln = [8, 1, 2, 3, 4, 6], [0, -1, CAP, CAP - 30, 100, 20], [10, 10, 10, 65, 200, 7]
    last = [0, 1, 2, 3, XROWS, 5]
    want_sk, want_sv = _expect_keep(k, sk, slot, first, ln), _expect_keep(v, sv, slot, first, ln)
    want_hid = _as_bytes(hid)
    want_hid.reshape(CAP, -1)[CAP - 30] = _as_bytes(x).reshape(XROWS, -1)[3]
    want_hid.reshape(CAP, -1)[20] = _as_bytes(x).reshape(XROWS, -1)[5]
    before_sk = _as_bytes(sk).reshape(LAYERS, NKV, CAP, -1)
    assert _keep(dtype, k, v, sk, sv, slot, first, ln, x, last, hid) == 0
    assert _same(sk, want_sk) and _same(sv, want_sv) and _same(hid, want_hid)
    g, c = _as_bytes(sk).reshape(LAYERS, NKV, CAP, -1), _as_bytes(k).reshape(LAYERS, SLOTS, NKV, TMAX, -1)
    assert np.array_equal(g[:, :, CAP - 30:], c[:, 3, :, :30]) and np.array_equal(g[:, :, 100:180], c[:, 4, :, :80])
    assert np.array_equal(g[:, :, :20], before_sk[:, :, :20]) and np.array_equal(g[:, :, 27:100], before_sk[:, :, 27:100])
    # without hidden rows: the KV rows only
    hid2 = _as_bytes(hid)
    assert _keep(dtype, k, v, sk, sv, [7], [40], [33]) == 0
    assert _same(hid, hid2) and np.array_equal(_as_bytes(sk).reshape(LAYERS, NKV, CAP, -1)[:, :, 40:73], c[:, 7, :, :33])
    k2, v2 = _rand(DIMS, dtype, 17), _rand(DIMS, dtype, 18)
    rfirst, rln, off, dst = [CAP - 30, 100, -5, CAP], [65, 80, 10, 10], [0, 3, 5, 6, 7], [0, -1, 8, 1, 2, 3, 4]
    want_k2, want_v2 = _expect_restore(k2, sk, rfirst, rln, off, dst), _expect_restore(v2, sv, rfirst, rln, off, dst)
    before_k2 = _as_bytes(k2).reshape(LAYERS, SLOTS, NKV, TMAX, -1)
    assert _restore(dtype, k2, v2, sk, sv, rfirst, rln, off, dst) == 0
    assert _same(k2, want_k2) and _same(v2, want_v2)
    g2, st = _as_bytes(k2).reshape(LAYERS, SLOTS, NKV, TMAX, -1), _as_bytes(sk).reshape(LAYERS, NKV, CAP, -1)
    assert np.array_equal(g2[:, 0, :, :30], st[:, :, CAP - 30:]) and np.array_equal(g2[:, 0, :, 30:], before_k2[:, 0, :, 30:])
    assert np.array_equal(g2[:, 1, :, :80], st[:, :, 100:180]) and np.array_equal(g2[:, 2], g2[:, 1])
    assert np.array_equal(g2[:, 3:], before_k2[:, 3:])                           # entries outside the store, and slots in no fan


def test_store_refusals(hip_lib):
    k = torch.zeros(2 * 4 * 2 * 8 * 32 + 8, dtype=torch.float16, device="cuda")
    s = torch.zeros(2 * 2 * 16 * 32 + 8, dtype=torch.float16, device="cuda")
    one, off, dst, ln = _dev([0]), _dev([0, 1]), _dev([1]), _dev([8])
    lib = L.lib()

    def keep(dt, D_, kp=None, n=1, layers=2, cap=16, x=None, Hd=32):
        p = L.ptr(k) if kp is None else kp
        return lib.surya_op_rec_kv_keep(dt, p, p, L.ptr(s), L.ptr(s), L.ptr(one), L.ptr(one), L.ptr(ln), n, layers, 4, 2, 8, D_, cap,
                                        x, None if x is None else L.ptr(one), None if x is None else L.ptr(s), Hd, 1, _stream())

    def restore(dt, D_, sp=None, n=1, n_dst=1, layers=2, cap=16):
        p = L.ptr(s) if sp is None else sp
        return lib.surya_op_rec_kv_restore(dt, L.ptr(k), L.ptr(k), p, p, L.ptr(one), L.ptr(ln), L.ptr(off), L.ptr(dst), n, n_dst, layers, 4, 2, 8,
                                           D_, cap, _stream())
    for call in (keep, restore):
        assert call(7, 32) == L.SA_ERR_UNSUPPORTED                      # an unknown dtype
        assert call(L.DTYPE_F16, 4) == L.SA_ERR_SHAPE                   # rows of 8 bytes: no 16-byte units
        assert call(L.DTYPE_F16, 32, layers=40000) == L.SA_ERR_SHAPE    # layers x kv heads beyond the grid
        assert call(L.DTYPE_F16, 32, n=-1) == L.SA_ERR_ARG
        assert call(L.DTYPE_F16, 32, cap=0) == L.SA_ERR_ARG
        assert call(L.DTYPE_F16, 32, n=0) == 0                          # nothing to do
        assert call(L.DTYPE_F16, 32) == 0
    assert keep(L.DTYPE_F16, 32, kp=C.c_void_p(k.data_ptr() + 2)) == L.SA_ERR_SHAPE        # a cache that is not 16-byte aligned
    assert restore(L.DTYPE_F16, 32, sp=C.c_void_p(s.data_ptr() + 2)) == L.SA_ERR_SHAPE     # a store that is not
    assert keep(L.DTYPE_F16, 32, kp=C.c_void_p(0)) == L.SA_ERR_ARG and restore(L.DTYPE_F16, 32, sp=C.c_void_p(0)) == L.SA_ERR_ARG
    assert keep(L.DTYPE_F16, 32, x=L.ptr(k), Hd=4) == L.SA_ERR_SHAPE    # hidden rows of 8 bytes
    assert keep(L.DTYPE_F16, 32, x=L.ptr(k), Hd=0) == L.SA_ERR_ARG
    assert restore(L.DTYPE_F16, 32, n_dst=0) == 0
    torch.cuda.synchronize()
    assert not k.any() and not s.any()
