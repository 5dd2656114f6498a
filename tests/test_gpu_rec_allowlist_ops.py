"""GPU: the masked greedy-partial epilogues of the lm_head, alone, through surya_op_lm_head_partials (the launchers RecModel::heads uses).

Shapes: N = 69 632 (REC-SMALL's vocabulary: no multiple of 320, last tile partial), K = 256, M in {1, 64, 320} (320 rows take the grouped
256 x 320 launch), operands bf16 / fp16 / fp32 / MXFP8. Those run the from-the-accumulators epilogue of gemm.h (256 x 320) and the staged one
of gemm_mx.h (128 x 128); two more bf16 variants run gemm.h's staged epilogue: Tuning lmhead = 0 (128 x 128 tiles) and a 4 160-column head
(64 x 64 tiles). The tile width is always read back from the launch (`bn_used`).

Reference: the fp32-output logits of the same operands from the same launcher (every tile walks K in the same order with the same MFMA, so
they are the numbers the epilogue reduced), masked in torch. Tokens must be equal; scores meet the rtol = 2e-3 of
test_full_vocab_fused_argmax_equals_recomputed_logits.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from surya_amd import _lib as L

pytestmark = pytest.mark.gpu
N_SMALL, K = 4096 + 65536, 256
INT_MAX = 0x7FFFFFFF
# (operand kind, N, Tuning lmhead)
VARIANTS = {"bf16": ("bf16", N_SMALL, 1), "fp16": ("fp16", N_SMALL, 1), "fp32": ("fp32", N_SMALL, 1), "mxfp8": ("mx", N_SMALL, 1),
            "bf16-128x128": ("bf16", N_SMALL, 0), "bf16-64x64": ("bf16", 4160, 1)}
CASES = [(v, M) for v in ("bf16", "fp16", "fp32", "mxfp8") for M in (1, 64, 320)] + [("bf16-128x128", 64), ("bf16-128x128", 320),
                                                                                     ("bf16-64x64", 64)]
TORCH_DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
LIB_DT = {"bf16": L.DTYPE_BF16, "fp16": L.DTYPE_F16, "fp32": L.DTYPE_F32, "mx": L.OP_MXFP8}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tune(hip_lib, lmhead):
    L.check(hip_lib.surya_set_tuning(b"lmhead", C.c_int(lmhead)), "surya_set_tuning(lmhead)")


@pytest.fixture(autouse=True)
def _restore_tuning(hip_lib):
    yield
    _tune(hip_lib, 1)


def _mx_quant(lib, x):
    rows, k = x.shape
    q = torch.empty((rows, k), dtype=torch.uint8, device="cuda")
    s = torch.empty((k // 128, rows, 4), dtype=torch.uint8, device="cuda")
    L.check(lib.surya_op_mx_quantize(L.ptr(x.float().contiguous()), C.c_int(rows), C.c_int(k), L.ptr(q), L.ptr(s), _stream()), "mx_quantize")
    return q, s


class Head:
    """Operands of one (variant, M, integer data or not) and the fp32 logits the same launcher computes from them."""

    def __init__(self, lib, variant, M, ints):
        self.lib, self.M = lib, M
        self.kind, self.N, self.lmhead = VARIANTS[variant]
        g = torch.Generator().manual_seed(1000 * M + len(variant) + (7 if ints else 0))
        N = self.N
        if ints:
            # integer operands: every logit is an exact integer in any summation order. Rows of W repeat -- (c, c + 1) for even c of the
            # first half, and the second half repeats the first -- so every logit value occurs at c, c + 1, c + N / 2, c + N / 2 + 1:
            # ties inside a thread's chunk, and across tiles
            x = torch.randint(-2, 3, (M, K), generator=g).float()
            w = torch.randint(-2, 3, (N, K), generator=g).float()
            w[1:N // 2:2] = w[0:N // 2:2]
            w[N // 2:] = w[:N // 2].clone()
            bias = torch.randint(-3, 4, (N,), generator=g).float()
            bias[1:N // 2:2] = bias[0:N // 2:2]
            bias[N // 2:] = bias[:N // 2].clone()
        else:
            x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.25
            bias = torch.randn(N, generator=g)
        if self.kind == "mx":
            self.x, self.sx = _mx_quant(lib, x.cuda())
            self.w, self.sw = _mx_quant(lib, w.cuda())
            self.bias = bias.to(torch.bfloat16).cuda()
        else:
            dt = TORCH_DT[self.kind]
            self.x, self.w, self.bias, self.sx, self.sw = x.to(dt).cuda(), w.to(dt).cuda(), bias.to(dt).cuda(), None, None
        self.logits = self._logits()
        assert torch.isfinite(self.logits).all()

    def _logits(self):
        lib, M, N = self.lib, self.M, self.N
        c = torch.full((M, N), float("nan"), dtype=torch.float32, device="cuda")
        if self.kind == "mx":
            S = C.c_int(0)
            L.check(lib.surya_op_gemm_mx(C.c_int(0), L.ptr(self.x), L.ptr(self.sx), L.ptr(self.w), L.ptr(self.sw), C.c_int(M), C.c_int(N), C.c_int(K),
                                         L.ptr(c), C.byref(S), None, None, _stream()), "gemm_mx")
            c += self.bias.float()                      # the epilogue's own fp32 add of the bf16 bias
        elif self.kind == "fp16":
            bn = C.c_int(0)
            L.check(lib.surya_op_rec_gemm_f16(1, L.EPI_BIAS, L.ptr(self.x), K, L.ptr(self.w), K, L.ptr(c), N, L.ptr(self.bias), None, 0, M, N, K, None,
                                              C.byref(bn), _stream()), "rec_gemm_f16")
        else:
            L.check(lib.surya_op_gemm(LIB_DT[self.kind], int(self.kind == "bf16"), L.EPI_BIAS, L.ptr(self.x), C.c_long(K), L.ptr(self.w), C.c_long(K),
                                      L.ptr(c), C.c_long(N), L.ptr(self.bias), None, C.c_long(0), M, N, K, _stream()), "op_gemm")
        torch.cuda.synchronize()
        return c

    def partials(self, masks=None, slot_mask=None, row_slot=None):
        """-> (partials [M, tiles, 4] fp32, tile width). masks: bool [n, N] (or None: the unmasked launch)."""
        M, N = self.M, self.N
        _tune(self.lib, self.lmhead)
        out = torch.full((M, (N + 63) // 64, 4), float("nan"), dtype=torch.float32, device="cuda")
        bn = C.c_int(0)
        dm = None if masks is None else pack_masks(masks).cuda()
        if masks is not None and slot_mask is None:
            slot_mask = torch.arange(M, dtype=torch.int32) % masks.shape[0]
        ds = None if slot_mask is None else slot_mask.to(torch.int32).cuda()
        dr = None if row_slot is None else row_slot.to(torch.int32).cuda()
        L.check(self.lib.surya_op_lm_head_partials(LIB_DT[self.kind], L.ptr(self.x), L.ptr(self.sx), L.ptr(self.w), L.ptr(self.sw), L.ptr(self.bias),
                                                   M, N, K, L.ptr(dm), L.ptr(ds), L.ptr(dr), L.ptr(out), C.byref(bn), _stream()),
                "surya_op_lm_head_partials")
        torch.cuda.synchronize()
        assert bn.value >= 64
        tiles = (N + bn.value - 1) // bn.value
        return out.view(-1)[: M * tiles * 4].view(M, tiles, 4).clone(), bn.value


@functools.lru_cache(maxsize=None)
def _head(variant, M, ints):
    return Head(L.lib(), variant, M, ints)


def pack_masks(allowed):
    """bool [n, N] -> uint32 [n, ceil(N / 32)]: bit (c & 31) of word (c >> 5)."""
    a = allowed.cpu().numpy().astype(bool)
    n, N = a.shape
    pad = np.zeros((n, (N + 31) // 32 * 32), bool)
    pad[:, :N] = a
    words = np.packbits(pad.reshape(n, -1, 32), axis=2, bitorder="little").view("<u4").reshape(n, -1)
    return torch.from_numpy(np.ascontiguousarray(words.astype(np.uint32)).view(np.int32).copy())


def combine(part):
    """The greedy head's reduction of the per-tile partials: (token, 1 / sum exp) per row."""
    mx, idx, se = part[..., 0], part[..., 1].contiguous().view(torch.int32), part[..., 2]
    assert not torch.isnan(mx).any() and not torch.isnan(se).any()
    best = mx.max(1, keepdim=True).values
    tok = torch.where(mx == best, idx, torch.full_like(idx, INT_MAX)).min(1).values
    w = torch.where(se > 0, se.double() * torch.exp(mx.double() - best.double()), torch.zeros_like(se, dtype=torch.float64))
    return tok.long(), 1.0 / w.sum(1)


def reference(logits, allowed):
    """First argmax and max softmax of logits.masked_fill(~allowed, -inf) (process_outputs on masked logits), in float64."""
    ml = logits.double().masked_fill(~allowed, float("-inf"))
    best = ml.max(1, keepdim=True).values
    cols = torch.arange(ml.shape[1], device=ml.device).expand_as(ml)
    tok = torch.where(ml == best, cols, torch.full_like(cols, INT_MAX)).min(1).values
    return tok, 1.0 / torch.exp(ml - best).sum(1)


def check(h, part, allowed, what):
    tok, score = combine(part)
    ref_tok, ref_score = reference(h.logits, allowed)
    bad = (tok != ref_tok).nonzero().flatten().tolist()
    assert not bad, f"{what}: rows {bad[:5]} got {tok[bad[:5]].tolist()} want {ref_tok[bad[:5]].tolist()}"
    assert allowed[torch.arange(h.M, device=tok.device), tok].all(), f"{what}: a disallowed column won"
    rel = ((score - ref_score).abs() / ref_score).max().item()
    print(f"{what}: max relative score error {rel:.3e}")
    assert rel <= 2e-3, (what, rel)
    return tok


@pytest.mark.parametrize("variant,M", CASES)
def test_all_ones_mask_is_bit_identical_to_the_unmasked_launch(hip_lib, variant, M):
    """(a) every column allowed, through a mask row and through slot id -1: the partials of the unmasked kernel, bit for bit."""
    h = _head(variant, M, False)
    plain, bn = h.partials()
    ones = torch.ones(1, h.N, dtype=torch.bool)
    masked, bn2 = h.partials(ones)
    assert bn2 == bn, "the tile width must not depend on the mask"
    assert torch.equal(masked.view(torch.int32), plain.view(torch.int32))
    free, _ = h.partials(torch.zeros(1, h.N, dtype=torch.bool), slot_mask=torch.full((M,), -1))
    assert torch.equal(free.view(torch.int32), plain.view(torch.int32))
    check(h, plain, torch.ones(M, h.N, dtype=torch.bool, device="cuda"), "unmasked")


@pytest.mark.parametrize("variant,M", CASES)
def test_random_masks_per_row(hip_lib, variant, M):
    """(b) eight random 50 % masks, rows mapped to slots through a permutation, a different id per slot, some slots unconstrained."""
    h = _head(variant, M, False)
    g = torch.Generator().manual_seed(M + 11)
    masks = torch.rand(8, h.N, generator=g) < 0.5
    n_slots = M + 5
    row_slot = torch.randperm(n_slots, generator=g)[:M]
    slot_mask = torch.arange(n_slots) % 9 - 1                     # -1, 0 .. 7
    part, _ = h.partials(masks, slot_mask, row_slot)
    ids = slot_mask[row_slot]
    allowed = torch.where((ids >= 0)[:, None], masks[ids.clamp_min(0)], torch.ones(M, h.N, dtype=torch.bool)).cuda()
    check(h, part, allowed, "random masks")


@pytest.mark.parametrize("variant,M", CASES)
def test_single_allowed_column_at_tile_borders(hip_lib, variant, M):
    """(c) + (d) one allowed column: first, around the first tile border (by bn_used and by 319 / 320), last; every other tile reports
    (-inf, 0x7fffffff, 0), nothing is NaN, the token is that column and the score exactly 1."""
    h = _head(variant, M, False)
    _, bn = h.partials()
    cols = sorted({0, 319, 320, bn - 1, bn, h.N - 1, ((h.N - 1) // bn) * bn})
    for c in cols:
        one = torch.zeros(1, h.N, dtype=torch.bool)
        one[0, c] = True
        part, _ = h.partials(one)
        assert not torch.isnan(part[..., [0, 2]]).any()              # (field 1 holds index bits: 0x7fffffff reads as a NaN)
        tok, score = combine(part)
        assert (tok == c).all(), (c, tok[:4].tolist())
        assert (score == 1.0).all(), (c, score[:4].tolist())
        others = torch.ones(part.shape[1], dtype=torch.bool)
        others[c // bn] = False
        o = part[:, others]
        assert (o[..., 0] == float("-inf")).all() and (o[..., 1].contiguous().view(torch.int32) == INT_MAX).all() and (o[..., 2] == 0).all()


@pytest.mark.parametrize("variant,M", CASES)
def test_allowed_columns_confined_to_one_tile(hip_lib, variant, M):
    """(d) a handful of allowed columns inside one middle tile, and inside the last (partial) tile: all-(-inf) tiles in the majority."""
    h = _head(variant, M, False)
    _, bn = h.partials()
    tiles = (h.N + bn - 1) // bn
    masks = torch.zeros(2, h.N, dtype=torch.bool)
    t = tiles // 2
    masks[0, t * bn + 3: t * bn + 41] = True
    masks[1, (tiles - 1) * bn + 1: h.N: 3] = True
    part, _ = h.partials(masks)
    assert not torch.isnan(part[..., [0, 2]]).any()
    allowed = masks[torch.arange(M) % 2].cuda()
    check(h, part, allowed, "one tile")


@pytest.mark.parametrize("variant,M", CASES)
def test_exact_ties_take_the_lowest_allowed_index(hip_lib, variant, M):
    """(e) integer data where every value occurs at c, c + 1, c + N / 2, c + N / 2 + 1. Row r % 3 == 0 disallows the unmasked winner c:
    c + 1 wins (a tie with a disallowed lower index does not); r % 3 == 1 disallows c and c + 1: the next column of that value wins, c + N / 2 at the latest (a tie across tiles);
    r % 3 == 2 keeps c inside a random mask: c wins."""
    h = _head(variant, M, True)
    N = h.N
    a0, _ = reference(h.logits, torch.ones(M, N, dtype=torch.bool, device="cuda"))
    a0 = a0.cpu()
    assert (a0 % 2 == 0).all() and (a0 < N // 2).all()
    g = torch.Generator().manual_seed(M + 5)
    allowed = torch.ones(M, N, dtype=torch.bool)
    r = torch.arange(M)
    allowed[r[r % 3 == 2]] = torch.rand(int((r % 3 == 2).sum()), N, generator=g) < 0.5
    allowed[r, a0] = r % 3 == 2
    allowed[r, a0 + 1] = r % 3 != 1
    allowed[r, a0 + N // 2] = True
    part, _ = h.partials(allowed)                                  # one mask row per GEMM row
    tok = check(h, part, allowed.cuda(), "ties")
    tok = tok.cpu()
    lg = h.logits.cpu()
    assert torch.equal(lg[r, tok], lg[r, a0])                      # every winner ties with the unmasked one ...
    assert torch.equal(tok[r % 3 == 0], a0[r % 3 == 0] + 1) and torch.equal(tok[r % 3 == 2], a0[r % 3 == 2])
    one = r % 3 == 1                                               # ... here with two disallowed lower indices: the next column of that value,
    assert ((tok[one] > a0[one] + 1) & (tok[one] <= a0[one] + N // 2)).all()      # the copy in the second half at the latest
    if M >= 64:
        _, bn = h.partials()
        assert (tok[one] // bn != a0[one] // bn).any()             # (a tie decided across tiles, by the head's combine)


@pytest.mark.parametrize("variant,M", CASES)
def test_unmasked_argmax_of_every_row_is_disallowed(hip_lib, variant, M):
    """(f) every row's own winner is the one column it may not emit."""
    h = _head(variant, M, False)
    a0, _ = reference(h.logits, torch.ones(M, h.N, dtype=torch.bool, device="cuda"))
    allowed = torch.ones(M, h.N, dtype=torch.bool)
    allowed[torch.arange(M), a0.cpu()] = False
    part, _ = h.partials(allowed)
    tok = check(h, part, allowed.cuda(), "winner disallowed")
    assert (tok.cpu() != a0.cpu()).all()


def test_op_hook_refuses_half_a_mask(hip_lib):
    x = torch.zeros(64, 64, dtype=torch.bfloat16, device="cuda")
    out = torch.zeros(64 * 4, dtype=torch.float32, device="cuda")
    bn = C.c_int(0)
    m = torch.zeros(2, dtype=torch.int32, device="cuda")
    rc = hip_lib.surya_op_lm_head_partials(L.DTYPE_BF16, L.ptr(x), None, L.ptr(x), None, None, 64, 64, 64, L.ptr(m), None, None, L.ptr(out), C.byref(bn),
                                           _stream())
    assert rc == L.SA_ERR_ARG                                        # a mask table without the slot ids
    rc = hip_lib.surya_op_lm_head_partials(7, L.ptr(x), None, L.ptr(x), None, None, 64, 64, 64, None, None, None, L.ptr(out), C.byref(bn), _stream())
    assert rc == L.SA_ERR_UNSUPPORTED
