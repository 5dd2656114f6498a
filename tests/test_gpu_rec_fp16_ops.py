"""GPU: the kernels the float16 recogniser adds, each alone through its op hook (the launchers RecModel<fp16_t> uses).

- surya_op_rec_gemm_f16 / surya_op_gemm_splitk_f16 on exact small-integer data over every tile launch_gemm / launch_gemm_splitk picks up to
  320 rows, and on random data against float64 with a derived bound;
- the greedy partials of the fp16 lm_head against the fp32-output logits of the same operands;
- the loader / consumer ring (Tuning dring) in fp16, bit for bit against the gemm_nt_kernel tiles it replaces;
- fp16 decode attention at the recogniser's head shape (d = 128, 10 / 2 heads) and at d = 32, against float64 PyTorch.
"""
import ctypes as C
import math

import pytest
import torch

from surya_amd import _lib as L

pytestmark = pytest.mark.gpu
EPI_ARGMAX = 6
DEFAULTS = dict(dring=1, dring_min_kt=0, big_m_split=-1, dattn_db=0)


def tune(**kw):
    for k, v in kw.items():
        L.check(L.lib().surya_set_tuning(k.encode(), C.c_int(int(v))), f"surya_set_tuning({k})")


@pytest.fixture(autouse=True)
def _restore_tuning(hip_lib):
    assert hip_lib.surya_gemm_ring_status(1) == 0
    yield
    tune(**DEFAULTS)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _gemm(lib, mode, epi, x, w, bias=None, res=None):
    """mode 0: fp16 output, 1: fp32 output, 2: greedy partials (returns (partials [M, tiles, 4], tile width))."""
    M, K = x.shape
    N = w.shape[0]
    n_out = N // 2 if epi == L.EPI_SWIGLU else N
    bn = C.c_int(0)
    if mode == 2:
        c = torch.full((M, (N + 63) // 64, 4), float("nan"), dtype=torch.float32, device=x.device)
        rc = lib.surya_op_rec_gemm_f16(2, epi, L.ptr(x), K, L.ptr(w), K, None, 0, L.ptr(bias), None, 0, M, N, K, L.ptr(c), C.byref(bn), _stream())
    else:
        c = torch.full((M, n_out), float("nan"), dtype=torch.float32 if mode else torch.float16, device=x.device)
        rc = lib.surya_op_rec_gemm_f16(mode, epi, L.ptr(x), K, L.ptr(w), K, L.ptr(c), n_out, L.ptr(bias), L.ptr(res), N if res is not None else 0,
                                       M, N, K, None, C.byref(bn), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    if mode == 2:
        tiles = (N + bn.value - 1) // bn.value
        return c.view(-1)[: M * tiles * 4].view(M, tiles, 4), bn.value
    return c


def _splitk(lib, x, w):
    M, K = x.shape
    N = w.shape[0]
    part = torch.full((8, M, N), float("nan"), dtype=torch.float32, device=x.device)
    s = C.c_int(0)
    rc = lib.surya_op_gemm_splitk_f16(L.ptr(x), K, L.ptr(w), K, L.ptr(part), M, N, K, C.byref(s), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return part[: s.value], s.value


def _ints(shape, g, lo=-4, hi=4):
    return torch.randint(lo, hi + 1, shape, generator=g).to(torch.float16).cuda()


def _fp16_ulp(ref):
    a = ref.abs().float()
    return torch.where(a < 6.1e-5, torch.full_like(a, 2.0 ** -24), torch.pow(2.0, torch.floor(torch.log2(a.clamp_min(6.1e-5)))) * 2.0 ** -10)


# M in {1, 8, 64, 200, 256, 320} (+ 100: the 64 < M <= 128 tiles) x N in {320, 1024} x K in {256, 768}; N = 8192 adds the N >= 8192 tiles
# only: one K, one M per row class
EXACT_CASES = [(M, N, K) for M in (1, 8, 64, 100, 200, 256, 320) for N in (320, 1024) for K in (256, 768)] + [(M, 8192, 256) for M in (8, 100, 256)]


@pytest.mark.parametrize("M,N,K", EXACT_CASES)
def test_rec_gemm_f16_exact_integer_data(hip_lib, M, N, K):
    """fp16 operands with integer values in [-4, 4] (bias / residual in [-64, 64]): every partial sum is an integer far below 2^24 and every
    result an integer below 2048 + 64 < 2^11 x 2, so fp32 accumulation is exact in any order and bias / residual / fp32-output results are
    representable: the kernels must return the integers. SwiGLU and GELU take exact accumulators through an exp: within one fp16 step of
    float64. The sweep's tiles (launch_gemm, 2-byte elements):
      M <= 64:        64x32 (N < 8192), 64x64 register-staged (N >= 8192)
      64 < M <= 128:  128x32 (N < 8192), 128x64 (N >= 8192)                       [M = 100]
      128 < M <= 256: 64x64 direct-to-LDS 2-stage; SwiGLU without bias: the loader / consumer ring 64x160 (dring = 1, the default)
      M = 320:        64x64 register-staged (fewer than 256 tiles of 128x128)
    and of launch_gemm_splitk: 64x64 4-stage ring of stages (M <= 256); at 320 rows 128x128 (big_m_split 2), 128x64 (3), 64x64 (0).
    The 256x320 and 128x128 lm_head tiles: test_lm_head_f16_* below."""
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    x, w = _ints((M, K), g), _ints((N, K), g)
    bias, res = _ints((N,), g, -64, 64), _ints((M, N), g, -64, 64)
    acc = x.double() @ w.double().t()
    exact = acc + bias.double()
    assert float(exact.abs().max()) + 64 < 2048                                  # + residual: still an integer fp16 holds
    got = _gemm(hip_lib, 0, L.EPI_BIAS, x, w, bias)
    assert torch.equal(got, exact.half()), f"bias: max diff {(got.double() - exact).abs().max():.3e}"
    got = _gemm(hip_lib, 0, L.EPI_BIAS, x, w, None)
    assert torch.equal(got, acc.half()), "no bias"
    got = _gemm(hip_lib, 0, L.EPI_RESIDUAL, x, w, bias, res)
    assert torch.equal(got.double(), exact + res.double()), "residual"
    got = _gemm(hip_lib, 1, L.EPI_BIAS, x, w, bias)
    assert got.dtype == torch.float32 and torch.equal(got.double(), exact), "fp32 output"
    # SwiGLU: weight rows interleaved (gate_j, up_j); with bias (the encoder) and without (the decoder; the ring at 128 < M <= 256).
    # Smaller integers (x in [-1, 1], w in [-2, 2]): gate x up stays below fp16's 65504
    x, w = _ints((M, K), g, -1, 1), _ints((N, K), g, -2, 2)
    acc = x.double() @ w.double().t()
    exact = acc + bias.double()
    assert float(exact.abs().max()) < 250
    for b in (bias, None):
        y = exact if b is not None else acc
        ref = (torch.nn.functional.silu(y[:, 0::2]) * y[:, 1::2])
        got = _gemm(hip_lib, 0, L.EPI_SWIGLU, x, w, b)
        assert ((got.double() - ref).abs() <= _fp16_ulp(ref.half())).all(), f"SwiGLU (bias: {b is not None}) beyond one fp16 step"
    ref = torch.nn.functional.gelu(exact)
    got = _gemm(hip_lib, 0, L.EPI_GELU, x, w, bias)
    assert ((got.double() - ref).abs() <= _fp16_ulp(ref.half())).all(), "GELU beyond one fp16 step"
    assert hip_lib.surya_gemm_ring_status(1) == 0
    # split-K: the slabs sum to the integers (slab sums are integers too: exact in fp32)
    if N != 8192:
        for mode in ((2, 3, 0) if M > 256 else (-1,)):
            tune(big_m_split=mode)
            part, s = _splitk(hip_lib, x, w)
            assert 1 <= s <= 8 and torch.equal(part.double().sum(0), acc), f"split-K (big_m_split {mode}, {s} slabs)"


@pytest.mark.parametrize("M,N,K", [(1, 320, 256), (64, 1024, 768), (200, 1024, 768), (256, 320, 768), (320, 1024, 768), (320, 8192, 256)])
def test_rec_gemm_f16_random_data_vs_float64(hip_lib, M, N, K):
    """Random fp16 operands against float64 on the same (rounded) operands. Per element the bound is one output rounding,
    2^-11 |y|, plus fp32 accumulation, K 2^-24 sum |x||w| -- doubled; fp32 output and split-K slabs: the accumulation term alone."""
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    x = torch.randn(M, K, device="cuda", generator=g).half()
    w = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).half()
    bias = torch.randn(N, device="cuda", generator=g).half()
    y = x.double() @ w.double().t() + bias.double()
    mag = x.double().abs() @ w.double().abs().t() + bias.double().abs()
    acc_b = K * 2.0 ** -24 * mag
    got = _gemm(hip_lib, 0, L.EPI_BIAS, x, w, bias)
    err = (got.double() - y).abs()
    print(f"fp16 GEMM {M}x{N}x{K}: worst err / bound {float((err / (2 * (2.0 ** -11 * y.abs() + acc_b))).max()):.3f}")
    assert (err <= 2 * (2.0 ** -11 * y.abs() + acc_b)).all()
    got = _gemm(hip_lib, 1, L.EPI_BIAS, x, w, bias)
    assert ((got.double() - y).abs() <= 2 * acc_b + 2.0 ** -23 * y.abs()).all()
    part, s = _splitk(hip_lib, x, w)
    yk = x.double() @ w.double().t()
    assert ((part.double().sum(0) - yk).abs() <= 2 * acc_b).all()


def _head_from_partials(part, bn, N):
    """greedy_head's combine: (token, softmax max) from per-tile {max, argmax bits, sum exp(v - max)}."""
    mx, col, se = part[..., 0], part[..., 1].contiguous().view(torch.int32), part[..., 2]
    best = mx.max(-1).values
    first = torch.where(mx == best[:, None], torch.arange(mx.shape[1], device=mx.device)[None], mx.shape[1]).min(-1).values
    token = col.gather(1, first[:, None])[:, 0]
    denom = (se.double() * torch.exp(mx.double() - best.double()[:, None])).sum(-1)
    return token.long(), (1.0 / denom)


@pytest.mark.parametrize("M,K", [(1, 256), (64, 256), (64, 768), (200, 256), (256, 256), (320, 256), (320, 768)])
def test_lm_head_f16_partials_exact_integer_data(hip_lib, M, K):
    """EPI_ARGMAX on the 256x320 tile (N >= 32768; 103 column tiles: not a multiple of 8, the mgroup mapping above 256 rows must still cover
    them) with integer data: the tile maxima are exact integers, the argmax column is the first maximum of the tile."""
    N = 320 * 103
    g = torch.Generator().manual_seed(M + K)
    x, w, bias = _ints((M, K), g), _ints((N, K), g), _ints((N,), g, -64, 64)
    exact = (x.double() @ w.double().t() + bias.double())
    part, bn = _gemm(hip_lib, 2, EPI_ARGMAX, x, w, bias)
    assert bn == 320 and part.shape[1] == 103 and not torch.isnan(part[..., :3]).any()
    tiles = exact.view(M, 103, 320)
    assert torch.equal(part[..., 0].double(), tiles.max(-1).values)
    first = torch.where(tiles == tiles.max(-1, keepdim=True).values, torch.arange(320, device="cuda")[None, None], 320).min(-1).values
    assert torch.equal(part[..., 1].contiguous().view(torch.int32).long(), first + 320 * torch.arange(103, device="cuda")[None])
    # the 128x128 direct-to-LDS tile of the fp32-output logits at lm_head width (surya_rec_copy_last_logits)
    assert torch.equal(_gemm(hip_lib, 1, L.EPI_BIAS, x, w, bias).double(), exact)


@pytest.mark.parametrize("M", [64, 320])
def test_lm_head_f16_greedy_partials_match_fp32_logits(hip_lib, M):
    """Token and score combined from the fp16 EPI_ARGMAX partials equal the argmax / softmax maximum of the fp32-output logits of the same
    operands (the same K order: the same accumulators), at 64 rows and at 320 (mgroup: the row blocks of a column tile on one XCD)."""
    N, K = 320 * 103, 768
    g = torch.Generator(device="cuda").manual_seed(M)
    x = torch.randn(M, K, device="cuda", generator=g).half()
    w = (torch.randn(N, K, device="cuda", generator=g) * (4.0 / K ** 0.5)).half()
    bias = torch.randn(N, device="cuda", generator=g).half()
    logits = _gemm(hip_lib, 1, L.EPI_BIAS, x, w, bias)
    part, bn = _gemm(hip_lib, 2, EPI_ARGMAX, x, w, bias)
    token, score = _head_from_partials(part, bn, N)
    assert torch.equal(token, logits.argmax(-1))
    ref = torch.softmax(logits.double(), -1).max(-1).values
    assert torch.allclose(score, ref, rtol=1e-4, atol=0), float((score / ref - 1).abs().max())


@pytest.mark.parametrize("M", [1, 64, 200, 256])
def test_ring_f16_bit_identical(hip_lib, M):
    """The loader / consumer ring in fp16 (gemm_ring.h is one template over the 16-bit type): gate|up outputs and split-K slabs bit for bit
    equal to the gemm_nt_kernel tiles at the recogniser's decode shapes, and no wait timed out."""
    g = torch.Generator(device="cuda").manual_seed(M)
    x = torch.randn(M, 1280, device="cuda", generator=g).half()
    w = (torch.randn(10240, 1280, device="cuda", generator=g) / 1280 ** 0.5).half()
    tune(dring=0)
    ref = _gemm(hip_lib, 0, L.EPI_SWIGLU, x, w)
    tune(dring=4 | 1)
    got = _gemm(hip_lib, 0, L.EPI_SWIGLU, x, w)
    assert hip_lib.surya_gemm_ring_status(1) == 0
    assert not torch.isnan(got.float()).any() and torch.equal(got.view(torch.int16), ref.view(torch.int16))
    xd = torch.randn(M, 5120, device="cuda", generator=g).half()
    wd = (torch.randn(1280, 5120, device="cuda", generator=g) / 5120 ** 0.5).half()
    tune(dring=0)
    ref, s_ref = _splitk(hip_lib, xd, wd)
    tune(dring=4 | 1, dring_min_kt=16)
    got, s_got = _splitk(hip_lib, xd, wd)
    assert hip_lib.surya_gemm_ring_status(1) == 0
    assert s_ref == s_got and s_ref > 1 and not torch.isnan(got).any()
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------- decode attention
LENS = [0, 7, 64, 127, 128, 130, 257]


def _rope_table(Tmax, d, theta=10000.0):
    inv = 1.0 / (theta ** (torch.arange(0, d, 2, dtype=torch.float32) / d))
    ang = torch.arange(Tmax, dtype=torch.float32)[:, None] * inv[None, :]
    return torch.stack([ang.cos().half().float(), ang.sin().half().float()], dim=-1).contiguous()


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("db", [-1, 1])
@pytest.mark.parametrize("d,nq,nkv", [(128, 10, 2), (32, 4, 2)])
def test_decode_attn_f16_vs_float64(hip_lib, d, nq, nkv, db, S):
    """decode_attn_flash2_kernel<d, MAXG, DB, fp16_t> through surya_op_decode_attn: d = 128 with 10 / 2 heads (the recogniser's rung, G <= 5)
    and d = 32 with 4 / 2, both dattn_db arms, 1 and 3 split-K slabs, contexts around the 128-key tile edges. Against float64 PyTorch on the
    rounded inputs: error <= 2.5e-3 x max|ref| (the bf16 test's 2e-2 / 8). The appended K / V rows equal the fp16 rounding of the roped keys /
    values: x = fp16(bias + slabs in order, fp32), k = fp16(fma(x1, cos, -(x2 sin)_fp32)), (x2 cos + (x1 sin)_fp32) likewise, v = x."""
    Tmax, M, G = 512, len(LENS), nq // nkv
    n_slots = M + 3
    g = torch.Generator(device="cuda").manual_seed(d + S)
    qkv_d = (nq + 2 * nkv) * d
    slots = torch.randperm(n_slots, generator=torch.Generator().manual_seed(d))[:M].to(torch.int32)
    part = torch.randn(S, M, qkv_d, device="cuda", generator=g) / math.sqrt(S)
    bias = (0.5 * torch.randn(qkv_d, device="cuda", generator=g)).half()
    kc = torch.randn(n_slots, nkv, Tmax, d, device="cuda", generator=g).half()
    vc = torch.randn(n_slots, nkv, Tmax, d, device="cuda", generator=g).half()
    kc0, vc0 = kc.clone(), vc.clone()
    cs = _rope_table(Tmax, d).cuda()
    out = torch.full((M, nq * d), float("nan"), device="cuda", dtype=torch.float16)
    act, rl = slots.cuda(), torch.tensor(LENS, dtype=torch.int32, device="cuda")
    scale = 1.0 / math.sqrt(d)
    tune(dattn_db=db)
    rc = hip_lib.surya_op_decode_attn(L.DTYPE_F16, d, L.ptr(part), S, L.ptr(bias), L.ptr(out), L.ptr(kc), L.ptr(vc), L.ptr(act), L.ptr(rl), L.ptr(cs),
                                      M, nq, nkv, Tmax, C.c_float(scale), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    v = bias.float()
    for s in range(S):
        v = v + part[s]                                                          # the kernel's order, fp32
    x = v.half()
    xq, xk, xv = x[:, :nq * d].view(M, nq, d), x[:, nq * d:(nq + nkv) * d].view(M, nkv, d), x[:, (nq + nkv) * d:].view(M, nkv, d)
    half = d // 2
    worst, ref_max = 0.0, 1.0
    for r in range(M):
        ln, s = LENS[r], int(slots[r])
        c, sn = cs[ln, :, 0], cs[ln, :, 1]

        def rope(t):                                                            # one rounded fp32 product, one fused multiply-add, then fp16
            t1, t2 = t[..., :half].float(), t[..., half:].float()
            lo = (t1.double() * c.double() - (t2 * sn).double()).float()
            hi = (t2.double() * c.double() + (t1 * sn).double()).float()
            return torch.cat([lo, hi], -1).half()

        kr = rope(xk[r])
        assert torch.equal(kc[s, :, ln], kr), f"row {r}: appended K != fp16 rounding of the roped key (max {float((kc[s, :, ln].float() - kr.float()).abs().max()):.3e})"
        assert torch.equal(vc[s, :, ln], xv[r]), f"row {r}: appended V"
        assert torch.equal(kc[s, :, :ln], kc0[s, :, :ln]) and torch.equal(kc[s, :, ln + 1:], kc0[s, :, ln + 1:])
        assert torch.equal(vc[s, :, :ln], vc0[s, :, :ln]) and torch.equal(vc[s, :, ln + 1:], vc0[s, :, ln + 1:])
        qr = (rope(xq[r]).float() * scale).half().double()                      # the kernel stores q x scale in fp16
        K = torch.cat([kc0[s, :, :ln].double(), kr.double()[:, None, :]], dim=1)
        V = torch.cat([vc0[s, :, :ln].double(), xv[r].double()[:, None, :]], dim=1)
        p = torch.softmax(torch.einsum("hd,hkd->hk", qr, K.repeat_interleave(G, dim=0)), dim=-1)
        ref = torch.einsum("hk,hkd->hd", p, V.repeat_interleave(G, dim=0))
        worst = max(worst, float((out[r].double().view(nq, d) - ref).abs().max()))
        ref_max = max(ref_max, float(ref.abs().max()))
    assert not torch.isnan(out.float()).any()
    print(f"fp16 decode attention d={d} db={db} S={S}: worst {worst:.3e}, bound {2.5e-3 * ref_max:.3e}")
    assert worst <= 2.5e-3 * ref_max, (worst, ref_max)
