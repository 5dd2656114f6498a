"""GPU: the *_TOPK epilogues of the lm_head and the combine kernel, alone, through surya_op_lm_head_topk (the launchers RecModel::heads uses).

Case grid and operands: those of test_gpu_rec_allowlist_ops.py (N = 69 632, K = 256, M in {1, 64, 320}, bf16 / fp16 / fp32 / MXFP8, plus the
bf16 128 x 128 and 4 160-column 64 x 64 variants), shared with it through its cache of operands.

Reference: the fp32-output logits of the same operands from the same launcher (`Head._logits` there: the numbers the epilogue reduced, bit
for bit), masked in torch and ordered by a STABLE sort on (-value, column) -- never torch.topk, whose tie order is unspecified. Values and
columns must be equal exactly; probabilities meet rtol = 2e-3 against float64.
"""
import copy
import ctypes as C

import pytest
import torch

from surya_amd import _lib as L
from test_gpu_rec_allowlist_ops import CASES, INT_MAX, K, LIB_DT, _head, _stream, _tune, pack_masks, reference

pytestmark = pytest.mark.gpu
A = L.SA_MAX_ALTERNATIVES
NEG_INF = float("-inf")


@pytest.fixture(autouse=True)
def _restore_tuning(hip_lib):
    yield
    _tune(hip_lib, 1)


def topk_launch(h, masks=None, slot_mask=None, row_slot=None, combine=True):
    """-> dict(amax [M, tiles, 4], alt_v [M, tiles, 4] fp32, alt_c [M, tiles, 4] int32, bn, and with `combine` top_tok [M, 4], top_p [M, 4],
    head_tok [M], head_score [M]). masks: bool [n, N] or None (the unconstrained launch through the same kernel)."""
    M, N = h.M, h.N
    _tune(h.lib, h.lmhead)
    t64 = (N + 63) // 64
    amax = torch.full((M, t64, 4), float("nan"), dtype=torch.float32, device="cuda")
    alt = torch.full((M, t64, A, 2), float("nan"), dtype=torch.float32, device="cuda")
    bn = C.c_int(0)
    dm = None if masks is None else pack_masks(masks).cuda()
    if masks is not None and slot_mask is None:
        slot_mask = torch.arange(M, dtype=torch.int32) % masks.shape[0]
    ds = None if slot_mask is None else slot_mask.to(torch.int32).cuda()
    dr = None if row_slot is None else row_slot.to(torch.int32).cuda()
    tt = torch.full((M, A), -7, dtype=torch.int32, device="cuda") if combine else None
    tp = torch.full((M, A), float("nan"), dtype=torch.float32, device="cuda") if combine else None
    ht = torch.full((M,), -7, dtype=torch.int32, device="cuda") if combine else None
    hs = torch.full((M,), float("nan"), dtype=torch.float32, device="cuda") if combine else None
    scratch = torch.empty(16 * M + 16, dtype=torch.float32, device="cuda") if combine else None
    L.check(h.lib.surya_op_lm_head_topk(LIB_DT[h.kind], L.ptr(h.x), L.ptr(h.sx), L.ptr(h.w), L.ptr(h.sw), L.ptr(h.bias), M, N, K, L.ptr(dm),
                                        L.ptr(ds), L.ptr(dr), L.ptr(amax), L.ptr(alt), C.byref(bn), L.ptr(tt), L.ptr(tp), L.ptr(ht), L.ptr(hs),
                                        L.ptr(scratch), _stream()), "surya_op_lm_head_topk")
    torch.cuda.synchronize()
    assert bn.value >= 64
    tiles = (N + bn.value - 1) // bn.value
    am = amax.view(-1)[: M * tiles * 4].view(M, tiles, 4).clone()
    al = alt.view(-1)[: M * tiles * A * 2].view(M, tiles, A, 2).clone()
    return {"amax": am, "alt_v": al[..., 0].contiguous(), "alt_c": al[..., 1].contiguous().view(torch.int32), "bn": bn.value, "tiles": tiles,
            "top_tok": tt, "top_p": tp, "head_tok": ht, "head_score": hs}


def stable_top(ml, k, col0=0):
    """The k first entries of `ml` [R, C] (fp32, -inf = not a candidate) by a stable sort on (-value, column): (values [R, k] with -inf
    for missing entries, columns [R, k] int32 with 0x7fffffff there)."""
    order = torch.sort(-ml, dim=1, stable=True).indices[:, :k]
    v = torch.gather(ml, 1, order)
    c = (order + col0).to(torch.int32)
    if v.shape[1] < k:
        pad = k - v.shape[1]
        v = torch.cat([v, torch.full((v.shape[0], pad), NEG_INF, device=v.device)], 1)
        c = torch.cat([c, torch.zeros((c.shape[0], pad), dtype=torch.int32, device=c.device)], 1)
    c = torch.where(v == NEG_INF, torch.full_like(c, INT_MAX), c)
    return v, c


def check(h, out, allowed, what, masks_for_partials=None):
    """Everything the issue states for one launch: amax bits, per-tile candidates, combine output."""
    M, N, bn, tiles = h.M, h.N, out["bn"], out["tiles"]
    ml = h.logits.masked_fill(~allowed, NEG_INF)
    # per tile: the stable top four of the tile's allowed columns inside N
    pad = tiles * bn - N
    mlp = torch.cat([ml, torch.full((M, pad), NEG_INF, device=ml.device)], 1).view(M * tiles, bn)
    rv, rc = stable_top(mlp, A)
    rc = torch.where(rc == INT_MAX, rc, rc + (torch.arange(M * tiles, device=rc.device, dtype=torch.int32) % tiles)[:, None] * bn)
    rv, rc = rv.view(M, tiles, A), rc.view(M, tiles, A)
    bad = ((out["alt_v"] != rv) | (out["alt_c"] != rc)).any(-1).nonzero().tolist()
    assert not bad, (f"{what}: (row, tile) {bad[:3]} got {out['alt_v'][bad[0][0], bad[0][1]].tolist()} {out['alt_c'][bad[0][0], bad[0][1]].tolist()} "
                     f"want {rv[bad[0][0], bad[0][1]].tolist()} {rc[bad[0][0], bad[0][1]].tolist()}")
    # entry 0 is (max, argmax) of the partial
    assert torch.equal(out["alt_v"][..., 0].view(torch.int32), out["amax"][..., 0].contiguous().view(torch.int32))
    assert torch.equal(out["alt_c"][..., 0], out["amax"][..., 1].contiguous().view(torch.int32))
    # the row's four best, their probabilities against float64, and the head's own token and score
    gv, gc = stable_top(ml, A)
    want_tok = torch.where(gc == INT_MAX, torch.full_like(gc, -1), gc)
    assert torch.equal(out["top_tok"], want_tok), (what, out["top_tok"][:3].tolist(), want_tok[:3].tolist())
    ref_tok, ref_score = reference(h.logits, allowed)
    assert torch.equal(out["top_tok"][:, 0].long(), ref_tok) and torch.equal(out["head_tok"], out["top_tok"][:, 0])
    assert torch.equal(out["top_p"][:, 0].view(torch.int32), out["head_score"].view(torch.int32)), f"{what}: entry 0 is not the greedy score's bits"
    ref_p = torch.exp(gv.double() - gv[:, :1].double()) * ref_score[:, None]
    ref_p = torch.where(gc == INT_MAX, torch.zeros_like(ref_p), ref_p)
    p = out["top_p"].double()
    assert (p[gc == INT_MAX] == 0).all()
    rel = ((p - ref_p).abs() / ref_p.clamp_min(1e-300))[gc != INT_MAX].max().item()
    print(f"{what}: max relative probability error {rel:.3e}")
    assert rel <= 2e-3, (what, rel)
    assert (out["top_p"][:, 1:] <= out["top_p"][:, :-1]).all(), f"{what}: probabilities increase along the entries"
    assert (p.sum(1) <= 1 + 1e-6).all()


def amax_equals_partials(h, out, masks=None, slot_mask=None, row_slot=None):
    plain, bn = h.partials(masks, slot_mask, row_slot)
    assert bn == out["bn"], "the tile width must not depend on the epilogue"
    assert torch.equal(out["amax"].view(torch.int32), plain.view(torch.int32)), "amax differs from the *_ARGMAX(_MASK) epilogue's bits"


@pytest.mark.parametrize("variant,M", CASES)
def test_unconstrained_and_random_masks(hip_lib, variant, M):
    """No table (bits of *_ARGMAX), slot id -1 through a table, and eight random masks over permuted slots (bits of *_ARGMAX_MASK)."""
    h = _head(variant, M, False)
    ones = torch.ones(M, h.N, dtype=torch.bool, device="cuda")
    out = topk_launch(h)
    amax_equals_partials(h, out)
    check(h, out, ones, "no table")
    free = topk_launch(h, torch.zeros(1, h.N, dtype=torch.bool), slot_mask=torch.full((M,), -1))
    for k in ("amax", "alt_v", "alt_c", "top_tok", "top_p"):
        assert torch.equal(free[k].view(torch.int32), out[k].view(torch.int32)), k
    g = torch.Generator().manual_seed(M + 11)
    masks = torch.rand(8, h.N, generator=g) < 0.5
    row_slot = torch.randperm(M, generator=g)                     # (the hook's outputs are indexed by slot: slots stay below M)
    slot_mask = torch.arange(M) % 9 - 1
    out = topk_launch(h, masks, slot_mask, row_slot)
    amax_equals_partials(h, out, masks, slot_mask, row_slot)
    ids = slot_mask[row_slot]
    allowed = torch.where((ids >= 0)[:, None], masks[ids.clamp_min(0)], torch.ones(M, h.N, dtype=torch.bool)).cuda()
    for k in ("top_tok", "top_p", "head_tok", "head_score"):
        out[k] = out[k][row_slot.cuda()]                          # slot order -> row order
    check(h, out, allowed, "random masks")


@pytest.mark.parametrize("variant,M", CASES)
def test_exact_ties_inside_chunks_and_across_tiles(hip_lib, variant, M):
    """Integer operands: every value occurs at c, c + 1, c + N / 2, c + N / 2 + 1. Unmasked, and with the unmasked winner (and, on every
    third row, its neighbour too) disallowed."""
    h = _head(variant, M, True)
    N = h.N
    ones = torch.ones(M, N, dtype=torch.bool, device="cuda")
    out = topk_launch(h)
    amax_equals_partials(h, out)
    check(h, out, ones, "ties")
    tt = out["top_tok"].cpu()
    # the maximum occurs at least four times: all four entries tie, in ascending column order, the first two adjacent, and the four
    # spread over more than one tile
    lg = h.logits.cpu()
    assert (torch.gather(lg, 1, tt.long()) == lg.max(1, keepdim=True).values).all() and (tt[:, 1:] > tt[:, :-1]).all()
    assert (tt[:, 1] == tt[:, 0] + 1).all() and (tt[:, 3] // out["bn"] != tt[:, 0] // out["bn"]).any()
    a0 = tt[:, 0].long()
    r = torch.arange(M)
    allowed = torch.ones(M, N, dtype=torch.bool)
    allowed[r, a0] = False
    allowed[r, a0 + 1] = r % 3 != 1
    out = topk_launch(h, allowed)
    amax_equals_partials(h, out, allowed)
    check(h, out, allowed.cuda(), "ties, winner disallowed")
    assert (out["top_tok"][:, 0].cpu() != a0).all()


@pytest.mark.parametrize("variant,M", CASES)
def test_planted_winners(hip_lib, variant, M):
    """The four best columns of every row planted through the bias (+64 on four columns of a copy of the shared operands, which stay as
    they are): in one tile, in four tiles, at the borders of a tile, in the partial last tile."""
    h = _head(variant, M, False)
    bn, N = topk_launch(h, combine=False)["bn"], h.N
    tiles = (N + bn - 1) // bn
    t, last = tiles // 2, tiles - 1
    plants = {"one tile": [t * bn + 5, t * bn + 6, t * bn + 40, t * bn + 41],
              "four tiles": [1 * bn + 7, (t - 1) * bn + 9, t * bn + 11, (t + 1) * bn + 13],
              "tile borders": [t * bn - 1, t * bn, (t + 1) * bn - 1, (t + 1) * bn],
              "last tile": [last * bn, last * bn + 1, N - 2, N - 1]}
    ones = torch.ones(M, N, dtype=torch.bool, device="cuda")
    for what, cols in plants.items():
        h2 = copy.copy(h)
        h2.bias = h.bias.clone()
        h2.bias[cols] += 64
        h2.logits = h2._logits()
        out = topk_launch(h2)
        amax_equals_partials(h2, out)
        check(h2, out, ones, what)
        assert torch.equal(out["top_tok"].cpu().sort(1).values, torch.tensor(sorted(cols), dtype=torch.int32).expand(M, A)), what


@pytest.mark.parametrize("variant,M", CASES)
def test_few_allowed_columns(hip_lib, variant, M):
    """Masks that leave 0, 1 and 3 allowed columns in a tile (others full), and 1 and 3 allowed columns in the whole row: missing entries are
    (-inf, 0x7fffffff) per tile and (-1, 0) per row, nothing is NaN."""
    h = _head(variant, M, False)
    bn, N = topk_launch(h, combine=False)["bn"], h.N
    tiles = (N + bn - 1) // bn
    masks = torch.ones(4, N, dtype=torch.bool)
    masks[:2, 0:bn] = False                                        # tile 0: nothing
    masks[:2, bn:2 * bn] = False
    masks[:2, bn + 17] = True                                      # tile 1: one column
    masks[:2, 2 * bn:3 * bn] = False
    masks[0, [2 * bn, 2 * bn + 31, 3 * bn - 1]] = True             # tile 2: three columns
    masks[1, [2 * bn + 1, 2 * bn + 32, 3 * bn - 2]] = True
    masks[2] = False
    masks[2, (tiles - 1) * bn + 3] = True                          # the whole row: one column, in the partial last tile
    masks[3] = False
    masks[3, [5, bn + 5, N - 1]] = True                            # the whole row: three columns in three tiles
    out = topk_launch(h, masks)
    assert not torch.isnan(out["alt_v"]).any() and not torch.isnan(out["top_p"]).any() and not torch.isnan(out["amax"][..., [0, 2]]).any()
    amax_equals_partials(h, out, masks)
    ids = torch.arange(M) % 4
    check(h, out, masks[ids].cuda(), "few allowed")
    tt, tp = out["top_tok"].cpu(), out["top_p"].cpu()
    one, three = ids == 2, ids == 3
    if one.any():
        assert (tt[one, 0] == (tiles - 1) * bn + 3).all() and (tt[one, 1:] == -1).all() and (tp[one, 0] == 1.0).all() and (tp[one, 1:] == 0).all()
    if three.any():
        assert (tt[three, 3] == -1).all() and (tt[three, :3] >= 0).all() and (tp[three, 3] == 0).all()
    empty = out["alt_c"][ids == 0][:, 0]                          # tile 0 of a mask-0 row: no candidate at all
    assert (empty == INT_MAX).all() and (out["alt_v"][ids == 0][:, 0] == NEG_INF).all()


def test_op_hook_refusals(hip_lib):
    x = torch.zeros(64, 64, dtype=torch.bfloat16, device="cuda")
    out = torch.zeros(64 * 64, dtype=torch.float32, device="cuda")
    bn = C.c_int(0)
    tt = torch.zeros(64 * 4, dtype=torch.int32, device="cuda")
    args = (L.DTYPE_BF16, L.ptr(x), None, L.ptr(x), None, None, 64, 64, 64, None, None, None, L.ptr(out))
    assert hip_lib.surya_op_lm_head_topk(*args, None, C.byref(bn), None, None, None, None, None, _stream()) == L.SA_ERR_ARG      # no alt array
    assert hip_lib.surya_op_lm_head_topk(*args, L.ptr(out), C.byref(bn), L.ptr(tt), None, None, None, None, _stream()) == L.SA_ERR_ARG   # half a combine
