"""GPU: the *_FORCED epilogues of the lm_head, alone, through surya_op_lm_head_forced (the launchers RecModel::heads uses).

Case grid and operands: those of test_gpu_rec_allowlist_ops.py (N = 69 632, K = 256, M in {1, 64, 320}, bf16 / fp16 / fp32 / MXFP8, plus the
bf16 128 x 128 and 4 160-column 64 x 64 variants), shared with it through its cache of operands.

What must hold: `amax` has the bits of the unmasked surya_op_lm_head_partials launch whatever the forced columns are; flogit[m] is the tile's
own fp32 number of column forced_col[m] -- the bits of the fp32-output logits of the same launcher (`Head.logits`, the numbers the epilogue
reduced), of the partial's max where the column is the tile's argmax, and of a *_TOPK candidate where it is one -- and rows with -1 keep
what flogit held. Against the float64 product of the same operands a logit meets 2e-3 absolute: the recognition tests' rtol = 2e-3 on a
probability, taken through the logarithm (p = exp(logit - lse)).
"""
import ctypes as C

import pytest
import torch

from surya_amd import _lib as L
from surya_amd.mx import dequantize_mx
from test_gpu_rec_allowlist_ops import CASES, K, LIB_DT, _head, _stream, _tune
from test_gpu_rec_topk_ops import topk_launch

pytestmark = pytest.mark.gpu
SENTINEL = -12345.5
TOL = 2e-3


@pytest.fixture(autouse=True)
def _restore_tuning(hip_lib):
    yield
    _tune(hip_lib, 1)


def forced_launch(h, cols):
    """cols: int [M] (-1 = none) -> (amax [M, tiles, 4], flogit [M] with SENTINEL where nothing was written, tile width)."""
    M, N = h.M, h.N
    _tune(h.lib, h.lmhead)
    amax = torch.full((M, (N + 63) // 64, 4), float("nan"), dtype=torch.float32, device="cuda")
    fl = torch.full((M,), SENTINEL, dtype=torch.float32, device="cuda")
    dc = torch.as_tensor(cols, dtype=torch.int32).cuda()
    assert dc.shape == (M,)
    bn = C.c_int(0)
    L.check(h.lib.surya_op_lm_head_forced(LIB_DT[h.kind], L.ptr(h.x), L.ptr(h.sx), L.ptr(h.w), L.ptr(h.sw), L.ptr(h.bias), M, N, K, L.ptr(dc),
                                          L.ptr(amax), L.ptr(fl), C.byref(bn), _stream()), "surya_op_lm_head_forced")
    torch.cuda.synchronize()
    assert bn.value >= 64
    tiles = (N + bn.value - 1) // bn.value
    return amax.view(-1)[: M * tiles * 4].view(M, tiles, 4).clone(), fl, bn.value


def bits(t):
    return t.contiguous().view(torch.int32)


def check(h, cols, what):
    """One launch: amax bits, flogit bits against the launcher's own logits, sentinels on the rows without a column."""
    cols = torch.as_tensor(cols, dtype=torch.int64)
    amax, fl, bn = forced_launch(h, cols)
    plain, bn2 = h.partials()
    assert bn == bn2, "the tile width must not depend on the epilogue"
    assert torch.equal(bits(amax), bits(plain)), f"{what}: amax differs from the *_ARGMAX epilogue's bits"
    on = ((cols >= 0) & (cols < h.N)).cuda()
    want = torch.where(on, h.logits[torch.arange(h.M, device="cuda"), cols.clamp(0, h.N - 1).cuda()], torch.full_like(fl, SENTINEL))
    bad = (bits(fl) != bits(want)).nonzero().flatten().tolist()
    assert not bad, f"{what}: rows {bad[:5]} cols {cols[bad[:5]].tolist()} got {fl[bad[:5]].tolist()} want {want[bad[:5]].tolist()}"
    return amax, fl, bn


@pytest.mark.parametrize("variant,M", CASES)
def test_every_position_of_three_tiles_and_the_tile_borders(hip_lib, variant, M):
    """Row m forced to column t0 + m % bn of the tile at 0, one in the middle and the last (partial) one, whose columns past N are -1: with
    M = 320 on the 256 x 320 tile every wave, lane half and (j, g, r) once. Then the columns around 64 / 128 / 320 and N - 1."""
    h = _head(variant, M, False)
    bn, N = forced_launch(h, [-1] * M)[2], h.N
    tiles = (N + bn - 1) // bn
    m = torch.arange(M)
    for t in (0, tiles // 2, tiles - 1):
        cols = t * bn + m % bn
        cols = torch.where(cols < N, cols, torch.full_like(cols, -1))
        _, fl, _ = check(h, cols, f"tile {t}")
        assert ((fl == SENTINEL).cpu() == (cols < 0)).all()
        if M == 320 and bn == 320 and t == tiles - 1:
            assert (cols[192:] == -1).all() and (cols[:192] >= 0).all()          # 69 632 = 217 x 320 + 192
    borders = torch.tensor([63, 64, 127, 128, 319, 320, N - 1, bn - 1, bn, (tiles - 1) * bn - 1, (tiles - 1) * bn, 0])
    for shift in range(0, len(borders), 5):
        check(h, borders[(m + shift) % len(borders)], f"borders {shift}")


@pytest.mark.parametrize("variant,M", CASES)
def test_the_value_is_the_tiles_own_number(hip_lib, variant, M):
    """Forced to the row's argmax: the bits of the partial's max. Forced to entries 1..3 of a tile's *_TOPK candidates: that candidate's
    bits. Random columns: within 2e-3 of the float64 product of the same operands."""
    h = _head(variant, M, False)
    rows = torch.arange(M, device="cuda")
    arg = h.logits.argmax(1)
    amax, fl, bn = check(h, arg.cpu(), "argmax")
    assert torch.equal(bits(fl), bits(amax[rows, arg // bn, 0])), "flogit of the argmax column is not the partial's max, bit for bit"
    assert torch.equal(bits(amax[rows, arg // bn, 1]), arg.to(torch.int32))
    top = topk_launch(h, combine=False)
    assert top["bn"] == bn
    tiles = top["tiles"]
    t = (rows * 7 + 3) % tiles
    j = 1 + rows % 3
    cols, vals = top["alt_c"][rows, t, j].long(), top["alt_v"][rows, t, j]
    _, fl, _ = check(h, cols.cpu(), "candidates")
    assert torch.equal(bits(fl), bits(vals)), "flogit of a *_TOPK candidate is not the candidate's value, bit for bit"
    g = torch.Generator().manual_seed(M + 23)
    cols = torch.randint(0, h.N, (M,), generator=g)
    _, fl, _ = check(h, cols, "random")
    if h.kind == "mx":
        un = lambda q, s: dequantize_mx(q, s.permute(1, 0, 2).reshape(q.shape[0], -1)).double()
        x, w = un(h.x, h.sx), un(h.w[cols.cuda()], h.sw[:, cols.cuda()])
    else:
        x, w = h.x.double().cpu(), h.w[cols.cuda()].double().cpu()
    ref = (x * w).sum(1) + h.bias[cols.cuda()].double().cpu()
    err = (fl.double().cpu() - ref).abs().max().item()
    print(f"{variant} M={M}: max |flogit - float64 product| {err:.3e}")
    assert err <= TOL, (variant, M, err)


@pytest.mark.parametrize("variant,M", CASES)
def test_free_rows_keep_the_sentinel_and_ties_do_not_disturb_amax(hip_lib, variant, M):
    """No forced column at all, a column past N, and a mix: untouched rows. Integer operands (every value at c, c + 1, c + N / 2,
    c + N / 2 + 1): forcing the argmax's equal neighbour, or its copy in the other half, changes no partial and yields the same value."""
    h = _head(variant, M, False)
    _, fl, _ = check(h, [-1] * M, "all free")
    assert (fl == SENTINEL).all()
    _, fl, _ = check(h, [h.N + 3] * M, "past N")
    assert (fl == SENTINEL).all()
    m = torch.arange(M)
    _, fl, _ = check(h, torch.where(m % 2 == 0, m * 5 + 1, torch.full_like(m, -1)), "every other row")
    assert ((fl == SENTINEL).cpu() == (m % 2 == 1)).all()
    hi = _head(variant, M, True)
    arg = hi.logits.argmax(1).cpu()
    best = hi.logits.max(1).values
    for what, cols in (("neighbour", arg + 1), ("other half", arg + hi.N // 2)):
        _, fl, _ = check(hi, cols, f"ties: {what}")
        assert torch.equal(bits(fl), bits(best)), what


def test_op_hook_refusals(hip_lib):
    x = torch.zeros(64, 64, dtype=torch.bfloat16, device="cuda")
    out = torch.zeros(64 * 4, dtype=torch.float32, device="cuda")
    cols = torch.zeros(64, dtype=torch.int32, device="cuda")
    bn = C.c_int(0)
    args = (L.ptr(x), None, L.ptr(x), None, None, 64, 64, 64)
    f = hip_lib.surya_op_lm_head_forced
    assert f(L.DTYPE_BF16, *args, None, L.ptr(out), L.ptr(out), C.byref(bn), _stream()) == L.SA_ERR_ARG           # no forced columns
    assert f(L.DTYPE_BF16, *args, L.ptr(cols), L.ptr(out), None, C.byref(bn), _stream()) == L.SA_ERR_ARG          # nowhere to write
    assert f(L.DTYPE_BF16, *args, L.ptr(cols), None, L.ptr(out), C.byref(bn), _stream()) == L.SA_ERR_ARG          # no partials
    assert f(7, *args, L.ptr(cols), L.ptr(out), L.ptr(out), C.byref(bn), _stream()) == L.SA_ERR_UNSUPPORTED
    assert f(L.OP_MXFP8, *args, L.ptr(cols), L.ptr(out), L.ptr(out), C.byref(bn), _stream()) == L.SA_ERR_ARG          # MXFP8 without scales
