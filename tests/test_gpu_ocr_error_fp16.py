"""GPU: the OCR-error classifier in float16 (SA_DTYPE_F16), the reference's GPU dtype (surya settings.MODEL_DTYPE).

- the two kernels fp16 adds, alone: segment attention on the matrix cores (attn_mfma_kernel<fp16_t, D> through surya_op_attn) against
  fp32 PyTorch on the fp16-rounded inputs, the tile and chunk edges and two "spike" rows whose other P entries are fp16 subnormals or
  zero; the GELU epilogue of every GEMM tile the model's shapes take (surya_op_gemm code 2) against float64;
- the engine against the reference's recorded fp32 logits (tests/golden/ocr_error_*.pt), against the plain-PyTorch restatement in
  float16 (tests/ocr_error_util.py) and against a bf16 engine on the same texts: fp16 must be at least twice as close;
- batch independence, the [CLS]-only last layer against the full one, one forward that takes every GEMM tile class, and
  OCRErrorPredictor(dtype=torch.float16) end to end.
"""
import ctypes as C
import functools
import math
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from surya_amd import _lib as L  # noqa: E402
from surya_amd.ocr_error.config import ocr_error_config  # noqa: E402
from surya_amd.ocr_error.model import HipOCRErrorModel, pack_ids  # noqa: E402
from surya_amd.synth import make_ocr_error_weights, make_wordpiece_vocab, write_ocr_error_checkpoint  # noqa: E402
from ocr_error_util import TorchOCRError  # noqa: E402

FIXTURES = ("tiny", "default")
F16 = torch.float16


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def golden(name):
    return torch.load(os.path.join(HERE, "golden", f"ocr_error_{name}.pt"))


@functools.lru_cache(maxsize=None)
def _weights(n_layers, dim):
    cfg = [c for c in (ocr_error_config("OCRERR-TINY"), ocr_error_config("OCRERR-DEFAULT")) if (c.n_layers, c.dim) == (n_layers, dim)][0]
    return make_ocr_error_weights(cfg, 0, "conditioned")


def weights(cfg):
    return _weights(cfg.n_layers, cfg.dim)


def model(cfg, dtype, max_texts=64, max_tokens=None):
    return HipOCRErrorModel(cfg, weights(cfg), dtype=dtype, device="cuda:0", max_texts=max_texts, max_tokens=max_tokens or max_texts * 512)


def run(m, seqs):
    ids, lens = pack_ids(seqs)
    return m.forward(ids, lens)


def cls_only(v):
    L.check(L.lib().surya_set_tuning(b"ocrerr_cls_only", int(v)), "surya_set_tuning")


@pytest.fixture(autouse=True)
def _restore_tuning():
    yield
    cls_only(1)


def _mixed_batch(cfg, n, seed, lo=1, hi=512):
    rng = random.Random(seed)
    return [[101] + [rng.randrange(104, cfg.vocab_size) for _ in range(rng.randint(lo, hi) - 1)] for _ in range(n)]


# ------------------------------------------------------------------------------------------------ 1. the engine takes the dtype
def test_engine_accepts_float16():
    cfg = ocr_error_config("OCRERR-TINY")
    m = model(cfg, F16, max_texts=4)
    lg, lb = run(m, [[101, 200, 102], [101, 102]])
    assert lg.shape == (2, cfg.num_labels) and lg.dtype == torch.float32 and torch.isfinite(lg).all()
    assert torch.equal(lg, lg.half().float())                       # logits are rounded to the compute dtype
    assert lb.long().tolist() == lg.argmax(-1).tolist()
    with pytest.raises(ValueError, match="float32.*bfloat16.*float16"):
        HipOCRErrorModel(cfg, weights(cfg), dtype=torch.float64)


# ------------------------------------------------------------------------------------------------ 2. attention alone
def _i64(a):
    a = np.ascontiguousarray(a, dtype=np.int64)
    return a, a.ctypes.data_as(C.POINTER(C.c_int64))


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(C.POINTER(C.c_int32))


def _ref_segment(q, k, v, scale, causal, group):
    """q [L, H, D], k / v [Lk, Hkv, D] (fp32) -> ([L, H, D], scores [H, L, Lk]); plain softmax attention."""
    kk = k.repeat_interleave(group, dim=1)
    vv = v.repeat_interleave(group, dim=1)
    s = torch.einsum("qhd,khd->hqk", q, kk) * scale
    if causal:
        m = torch.ones(q.shape[0], kk.shape[0], dtype=torch.bool, device=q.device).tril()
        s = s.masked_fill(~m, float("-inf"))
    return torch.einsum("hqk,khd->qhd", torch.softmax(s, dim=-1), vv), s


# the 64-query tile and 64-key chunk edges, then two spike segments of 512 keys (key SPIKE_KEY's score above every other by `gap`):
#   gap 24: every other P entry is below 2^-25 and rounds to zero in fp16;
#   gap 11: every other P entry lies in (2^-24, 2^-14): fp16 SUBNORMALS, 511 of them with 1.4e-2 of the row's weight between them --
#           a kernel (or matrix core) that flushed them would miss by ~2e-2, eight times the tolerance (their V is positive, the spike's -1).
EDGE_LENS = [1, 2, 63, 64, 65, 127, 128, 129, 512]
SPIKES = [(512, 24.0), (512, 11.0)]
SPIKE_KEY = 100
ATTN_TOL = 2.5e-3            # the bf16 rule of tests/test_gpu_attn_ops.py (2e-2: one rounding of P and of the output) / 8: three more significand bits


@pytest.mark.parametrize("D", [32, 64, 80, 128])
def test_attn_fp16_segments_vs_fp32(hip_lib, D):
    heads = 2
    He = heads * D
    g = torch.Generator(device="cuda").manual_seed(1000 + D)
    seg_lens = EDGE_LENS + [s[0] for s in SPIKES]
    P = sum(seg_lens)
    starts = np.cumsum([0] + seg_lens)[:-1]
    qkv = torch.randn(P, 3 * He, device="cuda", generator=g)
    for (Ls, gap), a in zip(SPIKES, starts[len(EDGE_LENS):]):
        a = int(a)
        qkv[a:a + Ls, :He] = 1.0 + 0.01 * torch.randn(Ls, He, device="cuda", generator=g)
        qkv[a:a + Ls, He:2 * He] = 0.02 * torch.randn(Ls, He, device="cuda", generator=g)
        qkv[a + SPIKE_KEY, He:2 * He] = gap / math.sqrt(D)          # score = scale * D * (gap / sqrt D) * ~1 = ~gap
        qkv[a:a + Ls, 2 * He:] = 1.0 + torch.randn(Ls, He, device="cuda", generator=g).abs()
        qkv[a + SPIKE_KEY, 2 * He:] = -1.0
    qkv = qkv.to(F16)
    out = torch.full((P, He), float("nan"), device="cuda", dtype=F16)
    sl, slp = _i32(seg_lens)
    qo, qop = _i64(starts * 3 * He)
    ko, kop = _i64(starts * 3 * He + He)
    vo, vop = _i64(starts * 3 * He + 2 * He)
    oo, oop = _i64(starts * He)
    scale = 1.0 / math.sqrt(D)
    rc = hip_lib.surya_op_attn(L.DTYPE_F16, D, L.ptr(qkv), L.ptr(qkv), L.ptr(qkv), L.ptr(out), slp, qop, kop, vop, oop, len(seg_lens), heads, 1,
                               0, C.c_float(scale), C.c_long(3 * He), C.c_long(D), C.c_long(3 * He), C.c_long(D), C.c_long(He), C.c_long(D),
                               _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    f = qkv.float().view(P, 3, heads, D)
    got = out.float().view(P, heads, D)
    assert not torch.isnan(got).any()
    for i, (Ls, a) in enumerate(zip(seg_lens, starts)):
        a = int(a)
        ref, s = _ref_segment(f[a:a + Ls, 0], f[a:a + Ls, 1], f[a:a + Ls, 2], scale, False, 1)
        if i >= len(EDGE_LENS):
            gap = SPIKES[i - len(EDGE_LENS)][1]
            others = torch.cat([s[..., :SPIKE_KEY], s[..., SPIKE_KEY + 1:]], -1)
            d = s[..., SPIKE_KEY:SPIKE_KEY + 1] - others
            if gap >= 20:
                assert float(d.min()) >= 20.0                       # the plain spike: everything else rounds to zero
            else:
                p = torch.exp(-d)
                assert float(p.max()) < 2.0 ** -14 and float(p.min()) > 2.0 ** -24, "the other entries must be fp16 subnormals"
        err = float((got[a:a + Ls] - ref).abs().max())
        tol = ATTN_TOL * max(1.0, float(ref.abs().max()))
        print(f"attn fp16 D={D} L={Ls}{' spike' if i >= len(EDGE_LENS) else ''}: err {err:.3e} tol {tol:.3e}")
        assert err <= tol, f"D={D} segment {i} (L={Ls}): max err {err} > {tol}"


def test_attn_fp16_causal_gqa_vs_fp32(hip_lib):
    """The decoder-prefill form: q rows packed per sequence, K / V from a slot cache [slot][kv_head][Tmax][d], causal, 4 query heads on 2
    kv heads; lengths around the 64-key chunk edge."""
    nq, nkv, d, Tmax, n_slots = 4, 2, 64, 192, 4
    lens, slots = [63, 65, 130], [2, 0, 3]
    g = torch.Generator(device="cuda").manual_seed(77)
    qkv_d = (nq + 2 * nkv) * d
    Ttot = sum(lens)
    q = torch.randn(Ttot, qkv_d, device="cuda", generator=g).to(F16)
    kc = torch.randn(n_slots, nkv, Tmax, d, device="cuda", generator=g).to(F16)
    vc = torch.randn(n_slots, nkv, Tmax, d, device="cuda", generator=g).to(F16)
    out = torch.full((Ttot, nq * d), float("nan"), device="cuda", dtype=F16)
    starts = np.cumsum([0] + lens)[:-1]
    sl, slp = _i32(lens)
    qo, qop = _i64(starts * qkv_d)
    ko, kop = _i64(np.array(slots) * nkv * Tmax * d)
    oo, oop = _i64(starts * nq * d)
    scale = 1.0 / math.sqrt(d)
    rc = hip_lib.surya_op_attn(L.DTYPE_F16, d, L.ptr(q), L.ptr(kc), L.ptr(vc), L.ptr(out), slp, qop, kop, kop, oop, len(lens), nq, nq // nkv, 1,
                               C.c_float(scale), C.c_long(qkv_d), C.c_long(d), C.c_long(d), C.c_long(Tmax * d), C.c_long(nq * d), C.c_long(d),
                               _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert not torch.isnan(out.float()).any()
    a = 0
    for Ls, s in zip(lens, slots):
        qs = q[a:a + Ls, :nq * d].float().view(Ls, nq, d)
        ref, _ = _ref_segment(qs, kc[s, :, :Ls].float().permute(1, 0, 2), vc[s, :, :Ls].float().permute(1, 0, 2), scale, True, nq // nkv)
        err = float((out[a:a + Ls].float().view(Ls, nq, d) - ref).abs().max())
        tol = ATTN_TOL * max(1.0, float(ref.abs().max()))
        print(f"attn fp16 causal GQA L={Ls}: err {err:.3e} tol {tol:.3e}")
        assert err <= tol
        a += Ls


# ------------------------------------------------------------------------------------------------ 3. the GELU epilogue alone
# Operands on a binary grid (x in 2^-4 steps within [-2, 2], W in 2^-6 steps within [-1/4, 1/4], bias in 2^-6 steps within [-1, 1]): every
# product is a multiple of 2^-10 and every partial sum stays below 2^9, so the fp32 accumulation is exact in ANY order and x W^T + b is the
# same number in the kernel and in float64. What is left to differ is what this test is about: the rounding of the projection to fp16,
# the GELU of that value, the rounding of the result. The projection's spread (sigma ~1.4 at K = 64, ~4.7 at K = 768) covers the GELU's
# negative tail down to the fp16 subnormals and zero.
#
# launch_gemm (gemm.h) for 2-byte outputs at N < 8192:   M <= 64: 64x32;   64 < M <= 128: 128x32;   128 < M <= 256: 64x64 direct-to-LDS;
# M > 256: the persistent 8-phase 256x256 loop once cdiv(M, 256) * cdiv(N, 256) >= 256 and the round cost model agrees (>= 4 even K-tiles),
# else 128x128 direct-to-LDS once cdiv(M, 128) * cdiv(N, 128) >= 256, else 64x64 (also the engine's pinned [CLS]-row tile).
# lin1 of OCRERR-DEFAULT (N = 3072, K = 768) is the model's only GELU GEMM: 12 column tiles of 256 -> the persistent loop from 22 row
# tiles = M 5377 up (a.M enters through cdiv, so the last row tile may hold one row), 128x128 from 11 row tiles of 128 = M 1281 up.
GELU_SMALL = [(M, N, K) for M in (1, 64, 65, 300) for N in (64, 192) for K in (64, 768)]
GELU_TILES = [(200, 3072, 768, "64x64 direct-to-LDS"), (1281, 3072, 768, "128x128 direct-to-LDS"), (5377, 3072, 768, "persistent 8-phase 256x256")]


def _grid(shape, g, lim, den):
    return (torch.randint(-lim, lim + 1, shape, generator=g).float() / den).to(F16).cuda()


def _gemm_gelu_f16(lib, x, w, bias):
    M, K = x.shape
    N = w.shape[0]
    c = torch.full((M, N), float("nan"), dtype=F16, device=x.device)
    rc = lib.surya_op_gemm(L.DTYPE_F16, 0, L.EPI_GELU, L.ptr(x), C.c_long(K), L.ptr(w), C.c_long(K), L.ptr(c), C.c_long(N), L.ptr(bias), None,
                           C.c_long(0), M, N, K, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return c


def _half64(t):
    """float64 -> fp16 in ONE correctly rounded step (numpy converts directly; torch goes through fp32 and can round twice), as float64."""
    with np.errstate(over="ignore"):
        return torch.from_numpy(t.cpu().numpy().astype(np.float16).astype(np.float64))


def _f16_step(e):
    """The fp16 spacing at |e| (float64 tensor): 2^-24 in the subnormal range, 2^(floor(log2 |e|) - 10) above."""
    a = e.abs().clamp_min(2.0 ** -14)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - 10)


def _check_gelu(lib, M, N, K, what):
    g = torch.Generator().manual_seed(M * 131 + N * 7 + K)
    x, w, b = _grid((M, K), g, 32, 16), _grid((N, K), g, 16, 64), _grid((N,), g, 64, 64)
    got = _gemm_gelu_f16(lib, x, w, b).cpu().double()
    pre = _half64(x.double() @ w.double().t() + b.double())         # half(x W^T + b): exact sum, one rounding
    want = _half64(0.5 * pre * (1.0 + torch.erf(pre * math.sqrt(0.5))))
    steps = ((got - want).abs() / _f16_step(want))
    assert torch.isfinite(got).all()
    print(f"fp16 GELU GEMM {M}x{N}x{K} ({what}): pre in [{float(pre.min()):.2f}, {float(pre.max()):.2f}], worst {float(steps.max()):.2f} fp16 steps, "
          f"{float((steps > 0).double().mean()):.2e} of the outputs off by one")
    assert float(steps.max()) <= 1.0, f"{what}: {float(steps.max())} fp16 steps from half(gelu(half(x W^T + b)))"


@pytest.mark.parametrize("M,N,K", GELU_SMALL)
def test_gemm_gelu_fp16_small_shapes(hip_lib, M, N, K):
    _check_gelu(hip_lib, M, N, K, "64x32" if M <= 64 else "128x32" if M <= 128 else "64x64")


@pytest.mark.parametrize("M,N,K,tile", GELU_TILES, ids=[t[3] for t in GELU_TILES])
def test_gemm_gelu_fp16_model_tiles(hip_lib, M, N, K, tile):
    _check_gelu(hip_lib, M, N, K, tile)


def test_gemm_gelu_fp16_every_input(hip_lib):
    """Every finite fp16 value as the projection (x_i times a weight of 1, K - 1 zeros): the epilogue's GELU over its whole domain, the
    negative tail through the fp16 subnormals to zero included. 63488 rows x 64 columns."""
    vals = torch.arange(0, 0x7C00, dtype=torch.int32).to(torch.int16).view(F16)
    vals = torch.cat([vals, -vals])
    M, N, K = vals.numel(), 64, 64
    x = torch.zeros(M, K, dtype=F16)
    x[:, 0] = vals
    w = torch.zeros(N, K, dtype=F16)
    w[:, 0] = 1.0
    got = _gemm_gelu_f16(hip_lib, x.cuda(), w.cuda(), torch.zeros(N, dtype=F16).cuda()).cpu().double()
    pre = vals.double()
    want = _half64(0.5 * pre * torch.erfc(-pre * math.sqrt(0.5)))[:, None].expand(M, N)       # erfc: no cancellation in the tail
    steps = (got - want).abs() / _f16_step(want)
    print(f"fp16 GELU over all {M} inputs: worst {float(steps.max()):.2f} fp16 steps, {float((steps > 0).double().mean()):.2e} off by one")
    assert torch.isfinite(got).all()
    assert float(steps.max()) <= 1.0
    assert torch.equal(got, got[:, :1].expand(M, N))                # the same value in every column of the tile


def test_gemm_gelu_fp16_overflow(hip_lib):
    """A projection above 65504 rounds to +inf before the GELU, as torch's .half() does, and gelu(+inf) = +inf; its neighbours stay finite."""
    M, N, K = 65, 64, 64
    g = torch.Generator().manual_seed(9)
    x, w, b = _grid((M, K), g, 32, 16), _grid((N, K), g, 16, 64), _grid((N,), g, 64, 64)
    x[3], w[5] = 32.0, 32.0                                         # 64 * 32 * 32 = 65536
    got = _gemm_gelu_f16(hip_lib, x, w, b).cpu().double()
    pre = _half64(x.double() @ w.double().t() + b.double())
    assert torch.isinf(pre[3, 5]) and pre[3, 5] > 0
    assert torch.isinf(got[3, 5]) and got[3, 5] > 0
    fin = torch.isfinite(pre)
    fin[3, 5] = False
    want = _half64(0.5 * pre * (1.0 + torch.erf(pre * math.sqrt(0.5))))
    assert (((got - want).abs() / _f16_step(want))[fin] <= 1.0).all()
    assert torch.isfinite(got[fin]).all()


def test_op_gemm_fp16_still_refuses_what_it_lacks(hip_lib):
    x = torch.zeros(64, 64, dtype=F16, device="cuda")
    args = (L.ptr(x), C.c_long(64), L.ptr(x), C.c_long(64), L.ptr(x), C.c_long(64))
    assert hip_lib.surya_op_gemm(L.DTYPE_F16, 1, L.EPI_GELU, *args, None, None, C.c_long(0), 64, 64, 64, _stream()) == -3      # fp32 output
    assert hip_lib.surya_op_gemm(L.DTYPE_F16, 0, L.EPI_GELU, *args, None, L.ptr(x), C.c_long(64), 64, 64, 64, _stream()) == -3  # gelu + residual
    assert hip_lib.surya_op_gemm(L.DTYPE_F16, 0, L.EPI_SWIGLU, *args, None, None, C.c_long(0), 64, 64, 64, _stream()) == -3


# ------------------------------------------------------------------------------------------------ 4. the fixtures
@functools.lru_cache(maxsize=None)
def _fixture_bound(name):
    """4(a): max(3.75e-3 x max|ref|, 1.5 x e_ref). 3.75e-3 = the bf16 test's 3e-2 floor / 8 (three more significand bits), 1.5 that test's
    own factor, e_ref = the error of the plain-PyTorch restatement in float16 on the same ids."""
    g = golden(name)
    cfg = ocr_error_config(g["config"])
    ref = g["logits_fp32"]
    e_ref = float((TorchOCRError(cfg, weights(cfg), F16, "cuda:0").logits(g["ids"], batch=16) - ref).abs().max())
    return max(3.75e-3 * float(ref.abs().max()), 1.5 * e_ref), e_ref


@pytest.mark.parametrize("name", FIXTURES)
def test_fp16_against_reference_and_bf16(name):
    """Measured on an MI355X, in units of max |reference logit| (7.07 tiny, 3.84 default): fp16 engine 1.67e-3 / 2.82e-3, bf16 engine
    9.91e-3 / 2.32e-2 (ratio 0.168 / 0.122), the fp16 restatement 1.24e-3 / 4.31e-3; clear-margin texts 100 % / 96.9 %."""
    g = golden(name)
    cfg = ocr_error_config(g["config"])
    ref = g["logits_fp32"]
    amax = float(ref.abs().max())
    lg, lb = run(model(cfg, F16), g["ids"])
    lg_bf, _ = run(model(cfg, torch.bfloat16), g["ids"])
    bound, e_ref = _fixture_bound(name)
    err, err_bf = float((lg - ref).abs().max()), float((lg_bf - ref).abs().max())
    top2 = torch.sort(ref, -1, descending=True).values
    clear = (top2[:, 0] - top2[:, 1]) > 2 * bound
    print(f"ocr-error {name}: max|ref| {amax:.4f}  fp16 engine {err:.3e} ({err / amax:.2e} x)  bf16 engine {err_bf:.3e} ({err_bf / amax:.2e} x)  "
          f"fp16 restatement {e_ref:.3e} ({e_ref / amax:.2e} x)  bound {bound:.3e}  ratio fp16/bf16 {err / err_bf:.3f}  clear {float(clear.float().mean()):.3f}")
    assert torch.isfinite(lg).all()                                                     # (d)
    assert err <= bound, (err, bound)                                                   # (a)
    assert err <= 0.5 * err_bf, (err, err_bf)                                           # (b) the feature's point
    assert float(clear.float().mean()) >= 0.8                                           # (c)
    assert lb.long()[clear].tolist() == ref.argmax(-1)[clear].tolist()


# ------------------------------------------------------------------------------------------------ 5. batch independence
def test_batch_independence_fp16():
    cfg = ocr_error_config("OCRERR-DEFAULT")
    seqs = _mixed_batch(cfg, 24, 5)
    m_small, m_big = model(cfg, F16, max_texts=24), model(cfg, F16, max_texts=64)
    alone = torch.cat([run(m_small, [s])[0] for s in seqs])
    together, _ = run(m_small, seqs)
    order = list(range(len(seqs)))
    random.Random(7).shuffle(order)
    filler = _mixed_batch(cfg, 40, 9)
    mixed, _ = run(m_big, [seqs[i] for i in order] + filler)
    shuffled = torch.empty_like(together)
    shuffled[order] = mixed[: len(seqs)]
    assert torch.isfinite(alone).all()
    assert torch.equal(alone, together)
    assert torch.equal(alone, shuffled)


# ------------------------------------------------------------------------------------------------ 6. the [CLS]-only last layer
def test_cls_only_last_layer_matches_full_layer_fp16():
    cfg = ocr_error_config("OCRERR-DEFAULT")
    seqs = _mixed_batch(cfg, 32, 11)
    m = model(cfg, F16)
    cls_only(1)
    a, _ = run(m, seqs)
    cls_only(0)
    b, _ = run(m, seqs)
    # the bound of the bf16 arm. fp16 meets it by equality: its [CLS] path runs the full layer's attention kernel over each text's first
    # query tile, as fp32 does (the one-query kernel cannot meet it, see the next test)
    d = float((a - b).abs().max())
    print(f"[CLS]-only vs full last layer, fp16: {d:.3e} = {d / float(b.abs().max()):.2e} x max|b|")
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    assert d <= 1e-3 * float(b.abs().max()) or torch.equal(a, b)


def test_one_query_cls_kernel_fp16():
    """ocrerr_cls_only = 2: cls_attn_kernel<fp16_t>. Its fp32 sums associate differently from attn_mfma_kernel's, so ~0.4 of a text's 768
    attention outputs land on the other side of an fp16 rounding boundary, and ONE such step moves a logit of this model by up to 1.2e-3 x
    max|logit| through the rest of the layer (plain PyTorch on the CPU; bf16: up to 6e-3, but its 8x coarser steps flip 8x more rarely).
    Measured on an MI355X: 1.38e-3 x max|b| from the full layer, about a tenth of fp16's distance from fp32 -- beyond the 1e-3 that the
    default path meets by equality, which is why it is not the default. As a forward of its own it is held to the fixtures' bound 4(a)."""
    g = golden("default")
    cfg = ocr_error_config(g["config"])
    ref = g["logits_fp32"]
    m = model(cfg, F16)
    cls_only(0)
    full, _ = run(m, g["ids"])
    cls_only(2)
    one, lb = run(m, g["ids"])
    bound, _ = _fixture_bound("default")
    err, d = float((one - ref).abs().max()), float((one - full).abs().max())
    same = float((one == full).all(-1).float().mean())
    print(f"one-query [CLS] kernel fp16: err vs fp32 reference {err:.3e} (bound {bound:.3e}); vs the full layer {d:.3e} = "
          f"{d / float(full.abs().max()):.2e} x max|b|, {same:.2f} of the texts bit-equal")
    assert torch.isfinite(one).all()
    assert err <= bound, (err, bound)
    top2 = torch.sort(ref, -1, descending=True).values
    clear = (top2[:, 0] - top2[:, 1]) > 2 * bound
    assert lb.long()[clear].tolist() == ref.argmax(-1)[clear].tolist()


# ------------------------------------------------------------------------------------------------ 7. every tile class in one forward
def test_every_tile_class_in_one_forward():
    """16 texts x 512 tokens = 8192 packed rows of OCRERR-DEFAULT: q | k | v (N = 2304: 32 x 9 tiles) and lin1 + GELU (N = 3072: 32 x 12)
    take the persistent 8-phase loop, out_lin and lin2 + residual (N = 768) the 128x128 tile, the [CLS] rows the pinned 64x64 tile."""
    cfg = ocr_error_config("OCRERR-DEFAULT")
    rng = random.Random(31)
    seqs = [[101] + [rng.randrange(104, cfg.vocab_size) for _ in range(510)] + [102] for _ in range(16)]
    got, _ = run(model(cfg, F16, max_texts=16), seqs)
    ref32 = TorchOCRError(cfg, weights(cfg), torch.float32, "cuda:0").logits(seqs, batch=16)
    e_ref = float((TorchOCRError(cfg, weights(cfg), F16, "cuda:0").logits(seqs, batch=16) - ref32).abs().max())
    amax = float(ref32.abs().max())
    bound = max(3.75e-3 * amax, 1.5 * e_ref)
    err = float((got - ref32).abs().max())
    print(f"16 x 512 tokens fp16: err {err:.3e} ({err / amax:.2e} x max|ref| {amax:.3f}), restatement {e_ref:.3e}, bound {bound:.3e}")
    assert torch.isfinite(got).all()
    assert err <= bound, (err, bound)


# ------------------------------------------------------------------------------------------------ 8. end to end
@pytest.fixture(scope="module")
def ckpt_dir(tmp_path_factory):
    cfg = ocr_error_config("OCRERR-TINY")
    return write_ocr_error_checkpoint(str(tmp_path_factory.mktemp("ocrerr_fp16_ckpt")), cfg, weights(cfg), make_wordpiece_vocab(0))


def test_predictor_end_to_end_fp16(ckpt_dir):
    from surya_amd.ocr_error import OCRErrorPredictor
    g = golden("tiny")
    ref = g["logits_fp32"]
    bound, _ = _fixture_bound("tiny")
    top2 = torch.sort(ref, -1, descending=True).values
    clear = ((top2[:, 0] - top2[:, 1]) > 2 * bound).tolist()
    assert sum(clear) >= 0.8 * len(clear)
    want = [{0: "good", 1: "bad"}[i] for i in ref.argmax(-1).tolist()]
    p = OCRErrorPredictor(checkpoint=ckpt_dir, dtype=F16)
    assert p.model.dtype == F16
    r = p(g["texts"])
    assert r.texts == g["texts"]
    assert [l for l, c in zip(r.labels, clear) if c] == [w for w, c in zip(want, clear) if c]
    assert p(g["texts"], batch_size=1).labels == r.labels
    assert p([]).labels == []
