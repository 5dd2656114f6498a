"""GPU: the text detector in float16 (SA_DTYPE_F16), the reference's GPU default dtype (surya settings.MODEL_DTYPE).

- the fp16 GEMM (v_mfma_f32_32x32x16_f16) on exact integer data over every tile launch_gemm picks for the detector's epilogues, its
  epilogues against torch rounded once by .half(), and fp16 overflow;
- DET-DEFAULT fp16 against the reference module's fp32 output (tests/golden/det_fp16.pt, tools/make_golden_det_fp16.py), and against a
  bf16 engine on the same page: fp16 must be measurably closer;
- the fused forms (det_fuse bits) against the fp16 op list, the uint8 input path, and the predictors on an fp16 detector.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from oracle import det_oracle as do
from surya_amd import _lib as L
from surya_amd.config import det_config
from surya_amd.synth import make_det_weights, make_pages

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _tune(lib, key, v):
    L.check(lib.surya_set_tuning(key.encode(), C.c_int(v)), f"surya_set_tuning({key})")


def _gemm_f16(lib, x, w, bias, epi, res=None):
    M, K = x.shape
    N = w.shape[0]
    c = torch.full((M, N), float("nan"), dtype=torch.float16, device=x.device)
    rc = lib.surya_op_gemm(L.DTYPE_F16, 0, epi, L.ptr(x), C.c_long(K), L.ptr(w), C.c_long(K), L.ptr(c), C.c_long(N), L.ptr(bias),
                           L.ptr(res), C.c_long(N if res is not None else 0), M, N, K,
                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return c


def _ints(shape, g, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, shape, generator=g).to(torch.float16).cuda()


# (M, N, K, tuning, tile) -- the branches of launch_gemm (gemm.h) for 2-byte outputs:
#   M <= 256: 64x64 direct-to-LDS (M > 128), 128x64 / 128x32 (M > 64, N >= / < 8192), 64x64 / 64x32 (M <= 64);
#   M > 256: 128x64 for N <= 64 at M >= 32768; 256x256 when t256 = row x column tiles of 256 >= 256 and the round cost model picks it
#   (persistent 8-phase loop for >= 4 even K-tiles of 64, the 8-phase tile with persist = 0, the 2-stage tile for odd K-tile counts);
#   128x128 when the 128-tile count >= 256; else 64x64.
GEMM_SHAPES = [
    (200, 256, 128, {}, "64x64 direct-to-LDS (128 < M <= 256)"),
    (100, 256, 192, {}, "128x32"),
    (100, 8192, 64, {}, "128x64 (N >= 8192)"),
    (50, 8192, 128, {}, "64x64 (M <= 64)"),
    (50, 256, 64, {}, "64x32"),
    (32768, 64, 64, {}, "128x64 narrow"),
    (512, 256, 2048, {}, "64x64"),
    (2048, 2048, 320, {}, "128x128 direct-to-LDS"),
    (4096, 4096, 256, {}, "256x256 persistent 8-phase loop"),
    (4096, 4096, 384, {"persist": 0}, "256x256 8-phase tile"),
    (4096, 4096, 192, {}, "256x256 2-stage (odd K-tiles)"),
]


@pytest.mark.parametrize("M,N,K,tune,tile", GEMM_SHAPES, ids=[s[4] for s in GEMM_SHAPES])
def test_gemm_f16_lane_map_exact(hip_lib, M, N, K, tune, tile):
    """fp16 operands, integer values in [-8, 8]: every partial sum is an integer below 2^24, so the fp32 accumulation is exact in any
    order and the kernel's output must equal the exact product rounded once to fp16. A wrong fragment / lane map cannot pass."""
    assert K % 64 == 0 and K <= 2048
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    x, w = _ints((M, K), g), _ints((N, K), g)
    bias = _ints((N,), g, -64, 64)
    res = _ints((M, N), g, -64, 64)
    exact = x.double() @ w.double().t() + bias.double()
    try:
        for k, v in tune.items():
            _tune(hip_lib, k, v)
        got = _gemm_f16(hip_lib, x, w, bias, L.EPI_BIAS)
        assert torch.equal(got, exact.half()), f"{tile}: fp16 GEMM != exact product (max diff {(got.float() - exact.float()).abs().max():.3e})"
        # residual: the product + bias rounded to fp16, then + the residual and rounded again (the reference's conv(x) + x in the model dtype)
        got = _gemm_f16(hip_lib, x, w, bias, L.EPI_RESIDUAL, res)
        assert torch.equal(got, (exact.half().double() + res.double()).half()), f"{tile}: residual epilogue"
        got = _gemm_f16(hip_lib, x, w, bias, L.EPI_RELU)
        assert torch.equal(got, exact.clamp_min(0).half()), f"{tile}: ReLU epilogue"
        # Hardswish: x * clamp(x / 6 + 0.5, 0, 1) in two fp32 roundings (common.h hardswish_f): within one fp16 step of torch's
        got = _gemm_f16(hip_lib, x, w, bias, L.EPI_HARDSWISH).float()
        ref = F.hardswish(exact.float()).half().float()
        ulp = torch.where(ref.abs() < 6.1e-5, torch.full_like(ref, 2.0 ** -24),
                          torch.pow(2.0, torch.floor(torch.log2(ref.abs().clamp_min(6.1e-5)))) * 2.0 ** -10)
        assert ((got - ref).abs() <= ulp).all(), f"{tile}: Hardswish epilogue beyond 1 fp16 ulp"
    finally:
        _tune(hip_lib, "persist", 1)
    print(f"fp16 GEMM {M}x{N}x{K} ({tile}): exact")


def test_gemm_f16_real_data_and_overflow(hip_lib):
    """Random fp16 data (bias epilogue) against fp32 torch rounded once, and an output above 65504: +inf, as torch's .half() gives."""
    g = torch.Generator().manual_seed(5)
    M, N, K = 4096, 4096, 512
    x = torch.randn((M, K), generator=g).half().cuda()
    w = (torch.randn((N, K), generator=g) * 0.05).half().cuda()
    bias = torch.randn((N,), generator=g).half().cuda()
    x[3] = 8.0
    w[5] = 8.0 * 2.0                              # row 3 . w row 5 = 512 * 128 = 65536 > 65504 -> inf
    w[6] = -16.0
    got = _gemm_f16(hip_lib, x, w, bias, L.EPI_BIAS)
    ref = x.float() @ w.float().t() + bias.float()
    assert got[3, 5].item() == float("inf") and got[3, 6].item() == float("-inf")
    assert torch.isinf(ref[3, 5:7].half()).all()
    fin = torch.isfinite(ref.half())
    d = (got.float() - ref.half().float()).abs()[fin]
    scale = ref.half().float().abs()[fin].clamp_min(1.0)
    assert (d / scale).max().item() <= 2 ** -9, (d / scale).max().item()


def _det(name, size, dtype, max_batch):
    from surya_amd.detection.model import HipDetModel
    cfg = det_config(name)
    sd = make_det_weights(cfg, 0)
    return cfg, sd, HipDetModel(cfg, sd, height=size, width=size, dtype=dtype, max_batch=max_batch)


@pytest.mark.parametrize("key", ["p1024", "p256"])
def test_det_fp16_vs_reference(hip_lib, key):
    """DET-DEFAULT fp16 against the reference module's fp32 output: within twice the reference's own fp16 deviation (low-res logits
    and the x4 up-sampled maps), and at most a quarter of a bf16 engine's error on the same pages."""
    g = torch.load(os.path.join(GOLD, "det_fp16.pt"))[key]
    size = g["size"]
    pages = make_pages(g["pages"], size, seed=g["page_seed"])[g["page"]:g["page"] + g["n_pages"]]
    x = do.normalise_pages(pages).cuda().contiguous()
    ref = g["logits"]
    ref_up = F.interpolate(ref, size=(size, size), mode="bilinear", align_corners=False)
    errs = {}
    for dt in (torch.float16, torch.bfloat16):
        _, _, m = _det("DET-DEFAULT", size, dt, 2)
        heat, low = m.forward(x, want_lowres=True)
        assert torch.isfinite(heat).all() and torch.isfinite(low).all()
        el, eu = (low.cpu() - ref).abs(), (heat.cpu() - ref_up).abs()
        errs[dt] = (el.max().item(), el.mean().item(), eu.max().item(), eu.mean().item())
        del m
    f, b = errs[torch.float16], errs[torch.bfloat16]
    tmax, tmean = max(4e-3, 2 * g["fp16_dev"]), max(8e-4, 2 * g["fp16_dev_mean"])
    print(f"DET-DEFAULT {size}^2 x {g['n_pages']} vs reference fp32: fp16 low-res max {f[0]:.3e} mean {f[1]:.3e}, x4 max {f[2]:.3e} mean {f[3]:.3e} | "
          f"bf16 low-res max {b[0]:.3e} mean {b[1]:.3e}, x4 max {b[2]:.3e} mean {b[3]:.3e} | reference fp16 dev {g['fp16_dev']:.3e} / "
          f"{g['fp16_dev_mean']:.3e}, bf16 dev {g['bf16_dev']:.3e} / {g['bf16_dev_mean']:.3e}")
    assert f[0] <= tmax and f[2] <= tmax, (f, tmax)
    assert f[1] <= tmean and f[3] <= tmean, (f, tmean)
    assert f[0] <= 0.25 * b[0] and f[1] <= 0.25 * b[1], "fp16 must be measurably closer to fp32 than bf16"


@pytest.mark.parametrize("pages_n,size", [(16, 1024), (3, 672), (1, 256)])
def test_fused_forms_vs_op_list_fp16(hip_lib, pages_n, size):
    """test_gpu_det_fused.py's bf16 check in fp16: each det_fuse bit alone and all together against the fp16 op list (det_fuse = 0)."""
    cfg, sd, m = _det("DET-DEFAULT", size, torch.float16, pages_n)
    x = do.normalise_pages(list(make_pages(pages_n, size, seed=99))).cuda().contiguous()
    try:
        _tune(hip_lib, "det_fuse", 0)
        base = m.forward(x).clone()
        assert torch.equal(base, m.forward(x))
        assert torch.isfinite(base).all() and base.std().item() > 0.02
        for bit in (1, 2, 4, 8, 16, 32, 64, 72, 128, 288, 512, 800, 1023):
            _tune(hip_lib, "det_fuse", bit)
            h = m.forward(x).clone()
            assert torch.equal(h, m.forward(x)), f"det_fuse={bit}: not run-to-run identical"
            assert torch.isfinite(h).all()
            d = (h - base).abs()
            print(f"fp16 {size}^2 x {pages_n}: det_fuse={bit:4d} vs op list: max abs diff {d.max().item():.3e}, mean {d.mean().item():.3e}, "
                  f"identical {torch.equal(h, base)}")
            if bit in (4, 8, 16, 32, 64, 72, 288, 512, 800):
                assert torch.equal(h.view(torch.int32), base.view(torch.int32)), f"det_fuse={bit} must repeat the op list's bits"
            else:
                assert d.max().item() <= 4e-3 and d.mean().item() <= 4e-4, (bit, d.max().item(), d.mean().item())
    finally:
        _tune(hip_lib, "det_fuse", 1023)


def test_det_fp16_forward_u8_is_bit_identical(hip_lib):
    """surya_det_forward_u8 in fp16 (rescale + normalise in the first kernel; with det_fuse bit 8 in the stem convolution's patch loader)
    == normalise on the host + surya_det_forward, for RGB (pixel stride 3) and RGBX (4) pages."""
    from surya_amd.detection.predictor import SegformerImageProcessor
    for name, size in (("DET-TINY", 128), ("DET-DEFAULT", 256)):
        cfg, sd, m = _det(name, size, torch.float16, 3)
        pages = make_pages(3, size, seed=11)
        proc = SegformerImageProcessor({"height": size, "width": size})
        x = torch.from_numpy(np.stack([proc(p)["pixel_values"][0] for p in pages])).cuda().contiguous()
        ref = m.forward(x)
        assert torch.isfinite(ref).all()
        u8 = torch.from_numpy(np.stack(pages)).cuda().contiguous()
        assert torch.equal(m.forward_u8(u8, proc.image_mean, proc.image_std), ref)
        x4 = np.concatenate([np.stack(pages), np.random.default_rng(0).integers(0, 256, size=(3, size, size, 1), dtype=np.uint8)], 3)
        assert torch.equal(m.forward_u8(torch.from_numpy(x4).cuda().contiguous(), proc.image_mean, proc.image_std), ref)


def _predictor(cfg, sd, size, dtype):
    from surya_amd.detection.predictor import DetectionPredictor
    return DetectionPredictor(checkpoint={"config": cfg, "state_dict": sd, "size": size}, dtype=dtype)


def test_detection_predictor_fp16(hip_lib):
    """DetectionPredictor(dtype=torch.float16) reaches the fp16 engine: results have the bf16 predictor's schema, and its heat maps are
    within the fp16 tolerance of an fp32 predictor's."""
    cfg = det_config("DET-DEFAULT")
    sd = make_det_weights(cfg, 0)
    pages = [Image.fromarray(p) for p in make_pages(3, 256, seed=11)]
    p16, pbf, p32 = (_predictor(cfg, sd, 256, dt) for dt in (torch.float16, torch.bfloat16, torch.float32))
    assert p16.model.dtype == torch.float16
    r16, rbf = p16(pages, batch_size=2, include_maps=True), pbf(pages, batch_size=2, include_maps=True)
    assert len(r16) == len(rbf) == 3
    for a, b in zip(r16, rbf):
        assert type(a) is type(b) and a.model_dump().keys() == b.model_dump().keys()
        assert type(a.heatmap) is type(b.heatmap) and a.heatmap is not None and a.image_bbox == b.image_bbox
        assert all(type(x) is type(y) for x, y in zip(a.bboxes, b.bboxes))
    h16 = torch.cat([h for h, *_ in p16.batch_heatmaps(pages, 2)])
    h32 = torch.cat([h for h, *_ in p32.batch_heatmaps(pages, 2)])
    d = (h16 - h32).abs()
    print(f"predictor fp16 vs fp32 heat maps: max {d.max().item():.3e} mean {d.mean().item():.3e}")
    assert d.max().item() <= 4e-3 and d.mean().item() <= 8e-4


@pytest.mark.parametrize("stream", [False, True])
def test_recognition_with_fp16_detector(hip_lib, stream):
    """RecognitionPredictor(images, det_predictor=<fp16 detector>): the streamed detect -> recognise path (_iter_detect_device) gives
    the serial detect-then-recognise call's results with the same detector."""
    from test_gpu_predictors import make_rec_predictor
    cfg_d = det_config("DET-TINY")
    det = _predictor(cfg_d, make_det_weights(cfg_d, 0), 256, torch.float16)
    cfg, sd, rec = make_rec_predictor(max_slots=8, max_tokens=6)
    pages = [Image.fromarray(p) for p in make_pages(3, 256, seed=21)]
    det_res = det(pages)
    rec.stream_detection = False
    serial = rec(pages, det_predictor=det)
    rec.stream_detection = stream
    out = rec(pages, det_predictor=det)
    assert len(out) == 3
    assert [len(r.text_lines) for r in out] == [len(r.bboxes) for r in det_res]
    assert [r.model_dump() for r in out] == [r.model_dump() for r in serial]
