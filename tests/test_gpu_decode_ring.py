"""GPU: the loader / consumer LDS ring of the decode GEMMs (csrc/gemm_ring.h, sa::Tuning dring) against the gemm_nt_kernel tiles it
replaces. Same K order and MFMA on both sides, so everything is compared bit for bit:
  * gate|up (EPI_SWIGLU, full K) and the split-K down projection's fp32 slabs at the decode shapes, M in {1, 64, 200, 256};
  * decode steps of REC-SMALL bf16 at 64 and 256 slots, ring on vs off: tokens, scores and boxes identical.
After every ring run the give-up word must be clear (no wait timed out).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from surya_amd import _lib as L
from surya_amd.config import rec_config
from surya_amd.synth import make_rec_weights
from util import make_prompts

pytestmark = pytest.mark.gpu

DEFAULTS = dict(dring=1, dring_min_kt=0)


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


def _gateup(lib, x, w):
    M, K = x.shape
    N = w.shape[0]
    c = torch.full((M, N // 2), float("nan"), dtype=torch.bfloat16, device=x.device)
    rc = lib.surya_op_gemm(L.DTYPE_BF16, 0, L.EPI_SWIGLU, L.ptr(x), C.c_long(K), L.ptr(w), C.c_long(K), L.ptr(c), C.c_long(N // 2),
                           None, None, C.c_long(0), M, N, K, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return c


def _splitk(lib, x, w):
    M, K = x.shape
    N = w.shape[0]
    part = torch.full((8, M, N), float("nan"), dtype=torch.float32, device=x.device)
    s = C.c_int(0)
    rc = lib.surya_op_gemm_splitk_bf16(L.ptr(x), C.c_long(K), L.ptr(w), C.c_long(K), L.ptr(part), M, N, K, C.byref(s), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return part[: s.value], s.value


def _operands(M, N, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).to(torch.bfloat16)
    return x, w


@pytest.mark.parametrize("M", [1, 64, 200, 256])
@pytest.mark.parametrize("nt", [0, 1])
def test_gateup_ring_is_bit_identical(hip_lib, M, nt):
    """REC-FULL decode gate|up: 256 x 10240 x 1280 (rows interleaved gate / up), ring forced at every M."""
    x, w = _operands(M, 10240, 1280, M)
    tune(dring=0)
    ref = _gateup(hip_lib, x, w)
    tune(dring=4 | (2 if nt else 1))
    got = _gateup(hip_lib, x, w)
    assert hip_lib.surya_gemm_ring_status(1) == 0
    assert not torch.isnan(got.float()).any()
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), (got.float() - ref.float()).abs().max().item()


@pytest.mark.parametrize("M", [1, 64, 200, 256])
@pytest.mark.parametrize("nt", [0, 1])
def test_down_ring_slabs_are_bit_identical(hip_lib, M, nt):
    """REC-FULL decode down projection: 256 x 1280 x 5120, split-K (same slice count in both arms), every fp32 slab bit for bit."""
    x, w = _operands(M, 1280, 5120, 1000 + M)
    tune(dring=0)
    ref, s_ref = _splitk(hip_lib, x, w)
    tune(dring=4 | (2 if nt else 1), dring_min_kt=16)
    got, s_got = _splitk(hip_lib, x, w)
    assert hip_lib.surya_gemm_ring_status(1) == 0
    assert s_ref == s_got and s_ref > 1
    assert not torch.isnan(got).any()
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), (got - ref).abs().max().item()
    assert torch.allclose(got.sum(0), (x.float() @ w.float().t()), rtol=2e-3, atol=2e-3)


def test_gateup_ring_ragged_last_column_tile(hip_lib):
    """Ragged N (not a multiple of 160: a last column tile of 16 weight rows) on the ring against the old tile, bit for bit."""
    x, w = _operands(256, 10256, 1280, 3)
    tune(dring=0)
    ref = _gateup(hip_lib, x, w)
    tune(dring=1)
    got = _gateup(hip_lib, x, w)
    assert hip_lib.surya_gemm_ring_status(1) == 0
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))


def _run_decode(m, cfg, n_lines, calls):
    from util import crop_grid
    rng = np.random.default_rng(n_lines)
    grids = [crop_grid(64, int(w)) for w in rng.integers(64, 257, size=n_lines)]
    tiles, seqs = make_prompts(cfg, grids, seed=n_lines)
    slots = list(range(n_lines))
    m.prefill(tiles.cuda(), grids, seqs, slots)
    t0, s0, b0 = m.read_outputs(1)
    m.set_active(slots)
    toks, scs, bbs = [t0[0][slots].copy()], [s0[0][slots].copy()], [b0[0][slots].copy()]
    for n in calls:
        m.decode(n)
        t, s, b = m.read_outputs(n)
        for k in range(n):
            toks.append(t[k][slots].copy()); scs.append(s[k][slots].copy()); bbs.append(b[k][slots].copy())
    return np.stack(toks), np.stack(scs), np.stack(bbs)


@pytest.mark.parametrize("n_lines", [64, 256])
def test_decode_steps_equal_with_ring_on_and_off(hip_lib, n_lines):
    from surya_amd.recognition.model import HipRecModel
    cfg = rec_config("REC-SMALL")
    sd = make_rec_weights(cfg, 0)
    m = HipRecModel(cfg, sd, image_token_id=cfg.image_token_id, pad_token_id=cfg.pad_token_id, eos_token_id=cfg.eos_token_id,
                    dtype=torch.bfloat16, max_slots=256, max_kv_len=512, max_patches=65536, max_prefill_tokens=256 * 80)
    calls = [4, 4]
    tune(dring=0)
    ref = _run_decode(m, cfg, n_lines, calls)
    tune(dring=1, dring_min_kt=1)          # every split-K projection of the step on the ring too
    got = _run_decode(m, cfg, n_lines, calls)
    assert hip_lib.surya_gemm_ring_status(1) == 0
    for a, b in zip(ref, got):
        assert np.array_equal(a, b)
