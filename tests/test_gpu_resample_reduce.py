"""GPU: pages whose thumbnail shrinks an axis by 4x or more. Pillow's integer box reduction on the device (surya_reduce_u8,
csrc/resample.h) vs `Image.reduce`, the device chain reduce -> boxed LANCZOS -> LANCZOS vs Pillow's `thumbnail` + `resize`, and
DetectionPredictor with the device resize vs the host (Pillow) resize on such pages: everything bit for bit."""
from functools import lru_cache

import numpy as np
import pytest
import torch
from PIL import Image

from surya_amd.common import pil_resample as pr
from reduce_cases import CHAIN_64, RAGGED, exhaustive_sum_image

pytestmark = pytest.mark.gpu

STRIDES = [(3, 4), (4, 3), (4, 4)]
# random images (w, h, fx, fy): the ragged ones of the CPU test, widths that are no multiple of any vector width, and one per load
# width of the span kernels (row pitch a multiple of 16 / 8 / 4 bytes at 4 and at 3 bytes per pixel) with ragged right / bottom edges
RANDOM = RAGGED + [(1031, 1, 2, 1), (1029, 5, 4, 4),
                   (70, 9, 2, 2), (68, 9, 2, 3), (80, 5, 2, 2), (66, 7, 3, 2), (100, 7, 3, 3), (70, 9, 4, 2), (100, 9, 4, 4), (112, 9, 4, 1),
                   (1300, 3, 2, 2)]                                                    # more than one block of lanes per row


@lru_cache(maxsize=None)
def reduce_case(kind, w, h, fx, fy):
    """(RGBX source with junk in X, Pillow's reduce of its RGB)."""
    rng = np.random.default_rng(w * 31 + h + fx * 7 + fy)
    a = exhaustive_sum_image(fx, fy) if kind == "sums" else rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    ref = np.asarray(Image.fromarray(a).reduce((fx, fy)))
    ax = np.concatenate([a, rng.integers(0, 256, a.shape[:2] + (1,), dtype=np.uint8)], 2)
    return ax, ref


@lru_cache(maxsize=None)
def chain_case(w, h, size):
    rng = np.random.default_rng(w * 7 + h)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    im = Image.fromarray(a)
    im.thumbnail(size, Image.Resampling.LANCZOS)
    ref = np.asarray(im.resize(size, Image.Resampling.LANCZOS))
    return np.concatenate([a, rng.integers(0, 256, (h, w, 1), dtype=np.uint8)], 2), ref


@pytest.mark.parametrize("spix,dpix", STRIDES)
@pytest.mark.parametrize("kind,w,h,fx,fy", [("sums", 0, 0, 3, 3), ("sums", 0, 0, 5, 2), ("sums", 0, 0, 6, 6)]
                         + [("random",) + c for c in RANDOM])
def test_device_reduce_equals_pillow(hip_lib, kind, w, h, fx, fy, spix, dpix):
    from surya_amd.detection.model import DeviceResampler
    ax, ref = reduce_case(kind, w, h, fx, fy)
    src = torch.from_numpy(np.ascontiguousarray(ax[..., :spix])).cuda()
    out = torch.full(ref.shape[:2] + (dpix,), 0xEE, dtype=torch.uint8, device="cuda")
    got = DeviceResampler("cuda:0").reduce(src, fx, fy, out=out).cpu().numpy()
    assert got.shape[:2] == (-(-ax.shape[0] // fy), -(-ax.shape[1] // fx))
    assert np.array_equal(got[..., :3], ref)
    if dpix == 4:
        assert (got[..., 3] == 0).all()


def test_reduce_rejects_bad_arguments(hip_lib):
    import ctypes as C
    from surya_amd import _lib as L
    src = torch.zeros((8, 8, 4), dtype=torch.uint8, device="cuda")
    dst = torch.zeros((8, 8, 4), dtype=torch.uint8, device="cuda")

    def call(w=8, h=8, sp=4, dp=4, fx=2, fy=2, s=src, d=dst):
        return hip_lib.surya_reduce_u8(L.ptr(s), C.c_int(w), C.c_int(h), C.c_int(sp), L.ptr(d), C.c_int(dp), C.c_int(fx), C.c_int(fy),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert call() == L.SA_OK
    for bad in [dict(fx=1, fy=1), dict(fx=0), dict(fy=256), dict(sp=2), dict(dp=5), dict(w=0), dict(h=-1), dict(s=None), dict(d=None)]:
        assert call(**bad) == L.SA_ERR_ARG, bad
    torch.cuda.synchronize()


@pytest.mark.parametrize("spix,dpix", STRIDES)
@pytest.mark.parametrize("w,h,size", [(w, h, (64, 64)) for w, h in CHAIN_64] + [(5000, 1100, (1024, 1024)), (4100, 300, (1024, 1024))])
def test_device_chain_with_reduce_equals_pillow(hip_lib, w, h, size, spix, dpix):
    from surya_amd.detection.model import DeviceResampler
    ax, ref = chain_case(w, h, size)
    rs = DeviceResampler("cuda:0")
    cur = torch.from_numpy(np.ascontiguousarray(ax[..., :spix])).cuda()
    steps = pr.plan_chain(w, h, size)
    assert steps[0][0] == "reduce" or (w, h) in [(256, 64), (255, 64)]
    for i, st in enumerate(steps):
        if st[0] == "reduce":
            cur = rs.reduce(cur, st[1], st[2])
        else:
            out = torch.empty((st[1][1], st[1][0], dpix), dtype=torch.uint8, device="cuda") if i == len(steps) - 1 else None
            cur = rs.resize(cur, st[1], out=out, box=st[2])
    got = cur.cpu().numpy()
    assert got.shape == (size[1], size[0], dpix)
    assert np.array_equal(got[..., :3], ref)
    if dpix == 4:
        assert (got[..., 3] == 0).all()


def test_predictor_device_resize_equals_host_resize_on_pages_that_reduce(hip_lib):
    from surya_amd.config import det_config
    from surya_amd.detection.predictor import DetectionPredictor
    from surya_amd.synth import make_det_weights, make_pages
    cfg = det_config("DET-TINY")
    pred = DetectionPredictor(checkpoint={"config": cfg, "state_dict": make_det_weights(cfg, 0), "size": 256})
    rng = np.random.default_rng(9)
    pages = []
    # (1200, 1500): a tall page, cut into 1200 x 256 strips that reduce by (2, 2); (300, 420): no reduction (the control)
    for (w, h) in [(1100, 300), (2100, 260), (1200, 1500), (300, 420)]:
        base = make_pages(1, 256, seed=int(rng.integers(1 << 30)))[0]
        pages.append(Image.fromarray(base).resize((w, h), Image.Resampling.BILINEAR))
    assert [pr.plan_chain(w, h, (256, 256))[0][:3] for w, h in [(1100, 300), (2100, 260), (1200, 256)]] == \
        [("reduce", 2, 2), ("reduce", 4, 4), ("reduce", 2, 2)]
    pred.device_resize = True
    dev = pred(pages)
    assert pred.last_resize_paths == {"device": 9, "host": 0, "ready": 0}            # 3 whole pages + 6 strips
    dev_heat = [h.clone() for h, _, _, _ in pred.batch_heatmaps(pages)]
    pred.device_resize = False
    host = pred(pages)
    assert pred.last_resize_paths == {"device": 0, "host": 9, "ready": 0}
    host_heat = [h.clone() for h, _, _, _ in pred.batch_heatmaps(pages)]
    assert len(dev_heat) == len(host_heat) and all(torch.equal(a, b) for a, b in zip(dev_heat, host_heat))   # same pixels went in
    assert len(dev) == len(host) == len(pages)
    for d, h_ in zip(dev, host):
        assert d.image_bbox == h_.image_bbox and len(d.bboxes) == len(h_.bboxes)
        for b1, b2 in zip(d.bboxes, h_.bboxes):
            assert b1.polygon == b2.polygon and b1.confidence == b2.confidence
