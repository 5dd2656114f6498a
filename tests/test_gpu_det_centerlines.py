"""GPU: DetectionPredictor.centerlines end to end on DET-TINY at processor size 256, fp32.

Synthetic weights give maps without line-shaped text, so the `Planted` predictor overwrites plane 0 of every page map with drawn bent
bands (tests/det_centerline_ref.bent_page) AFTER the forward -- the mechanism of tests/test_gpu_det_skew.py: overrides of `batch_heatmaps`,
`batch_detection` (the host checker arm) and `_tiled_batches` (both arms under `tiling`). The same drawn map reaches the device arm
(surya_det_centerlines behind surya_det_boxes) and the numpy statement of the checker arm, so the two must agree EXACTLY: centerline,
thickness and last_centerlines. The plain predictor shows that `centerlines` only adds."""
import numpy as np
import pytest
import torch
from PIL import Image

import det_centerline_ref as R
from surya_amd.config import det_config
from surya_amd.detection import centerline as cl
from surya_amd.detection import skew as sk
from surya_amd.synth import make_det_weights, make_pages

pytestmark = pytest.mark.gpu
P = 256


def _predictor(planted, max_batch=8):
    from surya_amd.detection.predictor import DetectionModelLoader, DetectionPredictor
    cfg = det_config("DET-TINY")

    class Loader(DetectionModelLoader):
        def model(self, device=None, dtype=None, max_batch_=None):
            return super().model(device, dtype, max_batch=max_batch)

    class Plain(DetectionPredictor):
        model_loader_cls = Loader

    class Planted(Plain):
        def batch_heatmaps(self, images, batch_size=None):
            for heat, split_index, split_heights, sizes in super().batch_heatmaps(images, batch_size):
                for pg in range(len(sizes)):
                    tiles = [t for t, k in enumerate(split_index) if k == pg]
                    rows = [split_heights[t] for t in tiles] if len(tiles) > 1 else [heat.shape[2]]
                    m = torch.from_numpy(R.bent_page(sum(rows), heat.shape[3])).to(heat.device)
                    r0 = 0
                    for t, r in zip(tiles, rows):
                        heat[t, 0, :r] = m[r0: r0 + r]
                        r0 += r
                yield heat, split_index, split_heights, sizes

        def batch_detection(self, images, batch_size=None):
            for preds, sizes in super().batch_detection(images, batch_size):
                yield [[R.bent_page(*p[0].shape), *p[1:]] for p in preds], sizes

        def _tiled_batches(self, images, batch_size, planes):
            for groups, sizes in super()._tiled_batches(images, batch_size, planes):
                for ks, maps, (mw, mh) in groups:
                    for i in range(len(ks)):
                        maps[i, 0, :, :mw] = torch.from_numpy(R.bent_page(mh, mw)).to(maps.device)
                yield groups, sizes

    return (Planted if planted else Plain)(checkpoint={"config": cfg, "state_dict": make_det_weights(cfg, 0), "size": P}, dtype=torch.float32)


@pytest.fixture(scope="module")
def plain(hip_lib):
    return _predictor(False)


@pytest.fixture(scope="module")
def planted(hip_lib):
    return _predictor(True)


@pytest.fixture(scope="module")
def pages():
    a, b = make_pages(2, 720, seed=7)
    tall = np.vstack([a[:700, :300], b[:700, :300], a[:100, :300]])
    return {(300, 256): Image.fromarray(a[:256, :300]), (256, 256): Image.fromarray(b[40:296, 30:286]), (200, 180): Image.fromarray(a[100:280, 50:250]),
            (260, 240): Image.fromarray(b[300:540, 10:270]), (300, 1500): Image.fromarray(tall), (400, 300): Image.fromarray(b[:300, :400])}


SMALL = [(300, 256), (256, 256), (200, 180), (260, 240)]


def _both_arms(pred, ims, **kw):
    dev = pred(ims, **kw)
    dev_info = list(pred.last_centerlines)
    pred.device_postprocess = False
    try:
        host = pred(ims, **kw)
        host_info = list(pred.last_centerlines)
    finally:
        pred.device_postprocess = True
    return dev, dev_info, host, host_info


def _equal(dev, dev_info, host, host_info, n):
    assert len(dev) == len(host) == len(dev_info) == len(host_info) == n
    assert dev_info == host_info
    for d, h in zip(dev, host):
        assert [b.polygon for b in d.bboxes] == [b.polygon for b in h.bboxes]
        assert [b.centerline for b in d.bboxes] == [b.centerline for b in h.bboxes]
        assert [b.thickness for b in d.bboxes] == [b.thickness for b in h.bboxes]
        assert d.model_dump() == h.model_dump()


def test_centerlines_only_add(plain, pages):
    ims = [pages[k] for k in SMALL + [(300, 1500)]]
    assert plain.centerlines is None
    before = plain(ims)
    plain.centerlines = cl.Centerlines()
    try:
        with_cl = plain(ims)
        info = list(plain.last_centerlines)
    finally:
        plain.centerlines = None
    assert len(info) == len(ims) and all(set(i) == {"n_boxes", "n_curved"} and 0 <= i["n_curved"] <= i["n_boxes"] for i in info)
    for a, b in zip(before, with_cl):
        assert a.image_bbox == b.image_bbox and [x.polygon for x in a.bboxes] == [x.polygon for x in b.bboxes]
        assert [x.confidence for x in a.bboxes] == [x.confidence for x in b.bboxes]
        stripped = b.model_dump()
        for x in stripped["bboxes"]:
            x.pop("centerline", None)
            x.pop("thickness", None)
        assert stripped == a.model_dump()
    after = plain(ims)
    assert [r.model_dump() for r in after] == [r.model_dump() for r in before]
    assert all("centerline" not in r.model_dump_json() and "thickness" not in r.model_dump_json() for r in after)


def test_device_equals_host_checker_on_small_pages(planted, pages):
    ims = [pages[k] for k in SMALL]
    planted.centerlines = cl.Centerlines()
    try:
        dev, dev_info, host, host_info = _both_arms(planted, ims)
    finally:
        planted.centerlines = None
    _equal(dev, dev_info, host, host_info, 4)
    for size, r, info in zip(SMALL, dev, dev_info):
        curved = [b for b in r.bboxes if b.centerline is not None]
        print(f"page {size}: {info}, {len(curved)} boxes with a centre line after clean_boxes")
        assert info["n_boxes"] >= 4 and 2 <= info["n_curved"] < info["n_boxes"]          # every third band is straight
        assert curved and all(b.thickness is not None and len(b.centerline) == 18 for b in curved)
        # ... and it IS the numpy statement on the drawn map, in page pixels
        prof = cl.profile_page(R.bent_page(P, P), R.TEXT_T, R.LOW_T, 16)
        assert info["n_boxes"] == len(prof["axis"])
        sx, sy = size[0] / P, size[1] / P
        first = next(i for i in range(len(prof["axis"])) if cl.finish(*[prof[k][i] for k in ("cnt", "sum", "lo", "hi", "axis", "box")], cl.Centerlines()))
        pts, _ = cl.finish(*[prof[k][first] for k in ("cnt", "sum", "lo", "hi", "axis", "box")], cl.Centerlines())
        assert any(np.allclose(np.asarray(b.centerline), pts * [sx, sy], rtol=0, atol=1e-9) for b in curved)
        for b in curved:                                                # the centre line runs inside its box's polygon
            x0, y0, x1, y1 = b.bbox
            c = np.asarray(b.centerline)
            assert (c[:, 0] >= x0 - 1).all() and (c[:, 0] <= x1 + 1).all() and (c[:, 1] >= y0 - 1).all() and (c[:, 1] <= y1 + 1).all()


def test_device_equals_host_checker_on_a_tall_page(planted, pages):
    ims = [pages[(300, 1500)], pages[(256, 256)]]
    planted.centerlines = cl.Centerlines(knots=8)
    try:
        dev, dev_info, host, host_info = _both_arms(planted, ims)
    finally:
        planted.centerlines = None
    _equal(dev, dev_info, host, host_info, 2)
    assert dev_info[0]["n_boxes"] > dev_info[1]["n_boxes"] and dev_info[0]["n_curved"] >= 10
    assert all(len(b.centerline) == 10 for b in dev[0].bboxes if b.centerline is not None)


def test_device_equals_host_checker_under_tiling(planted, pages):
    from surya_amd.detection.predictor import DetTiling
    ims = [pages[(400, 300)], pages[(200, 180)], pages[(260, 240)]]
    planted.tiling, planted.centerlines = DetTiling(scale=1.0, overlap=32), cl.Centerlines()
    try:
        dev, dev_info, host, host_info = _both_arms(planted, ims)
    finally:
        planted.tiling = planted.centerlines = None
    _equal(dev, dev_info, host, host_info, 3)
    assert all(i["n_curved"] >= 2 for i in dev_info)


def test_together_with_skew(planted, pages):
    ims = [pages[k] for k in SMALL[:2]] + [pages[(300, 1500)]]
    planted.centerlines, planted.skew = cl.Centerlines(), sk.SkewEstimate()
    try:
        dev, dev_info, host, host_info = _both_arms(planted, ims)
        both_skew = [(r.skew, r.skew_confidence) for r in dev]
        planted.centerlines = None
        only_skew = [(r.skew, r.skew_confidence) for r in planted(ims)]
    finally:
        planted.centerlines = planted.skew = None
    _equal(dev, dev_info, host, host_info, 3)
    assert both_skew == only_skew and [(r.skew, r.skew_confidence) for r in host] == both_skew
    assert all(i["n_curved"] >= 2 for i in dev_info)


@pytest.mark.parametrize("tiled", [False, True])
def test_every_option_in_one_call_device_equals_host_checker(planted, pages, tiled):
    """`skew`, `centerlines` and include_maps in one call, without and with `tiling`: four small pages of two sizes around a tall one, two
    tiles to a batch, so that a batch holds two groups under `tiling` and the tall page runs alone in several forwards."""
    from surya_amd.detection.predictor import DetTiling
    from test_gpu_det_tiling import _same
    sizes = [(256, 256), (200, 180), (300, 1500), (200, 180), (256, 256)]
    ims = [pages[k] for k in sizes]
    planted.skew, planted.centerlines = sk.SkewEstimate(), cl.Centerlines()
    planted.tiling = DetTiling(scale=1.0, overlap=32) if tiled else None
    try:
        dev = planted(ims, batch_size=2, include_maps=True)
        dev_info, dev_skew = list(planted.last_centerlines), list(planted.last_skew)
        planted.device_postprocess = False
        host = planted(ims, batch_size=2, include_maps=True)
        host_info, host_skew = list(planted.last_centerlines), list(planted.last_skew)
    finally:
        planted.device_postprocess = True
        planted.tiling = planted.skew = planted.centerlines = None
    assert len(dev) == len(host) == len(dev_info) == len(dev_skew) == 5
    _same(dev, host, atol=1e-6)
    assert dev_skew == host_skew and dev_info == host_info
    assert [i["map_size"] for i in dev_skew] == (sizes if tiled else [(P, P), (P, P), (P, 1500), (P, P), (P, P)])
    for d, h, s, size in zip(dev, host, dev_skew, sizes):
        assert (d.skew, d.skew_confidence) == (h.skew, h.skew_confidence) == (s["angle"], s["confidence"]) and d.skew is not None
        assert [b.centerline for b in d.bboxes] == [b.centerline for b in h.bboxes]
        assert [b.thickness for b in d.bboxes] == [b.thickness for b in h.bboxes]
        for a, b in ((d.heatmap, h.heatmap), (d.affinity_map, h.affinity_map)):
            assert a.size == b.size == (size if tiled else (P, 1500 if size[1] > P else P)) and np.array_equal(np.asarray(a), np.asarray(b))
    assert sum(len(r.bboxes) for r in dev) >= 1 and all(i["n_curved"] >= 2 for i in dev_info)


def test_iter_detect_and_the_streamed_call_carry_the_same_centre_lines(planted, pages):
    from test_gpu_predictors import make_rec_predictor
    ims = [pages[k] for k in SMALL + [(300, 1500)]]
    planted.centerlines = cl.Centerlines()
    try:
        whole = planted(ims, batch_size=4)
        info = list(planted.last_centerlines)
        parts = [r for part in planted.iter_detect(ims, batch_size=4) for r in part]
        assert planted.last_centerlines == info
        assert [r.model_dump() for r in whole] == [r.model_dump() for r in parts]
        assert all(any(b.centerline is not None for b in r.bboxes) for r in whole)
        cfg, sd, rec = make_rec_predictor(max_slots=8, max_tokens=4)
        rec.stream_detection = True
        planted.last_centerlines = []
        rec(ims[:2], det_predictor=planted, detection_batch_size=4)
        assert rec.last_timing.get("streamed") == 1.0
        assert planted.last_centerlines == info[:2]
    finally:
        planted.centerlines = None


def test_a_page_with_more_lines_than_travel_with_the_launch(planted, pages):
    """HipDetCenterlines.HEAD rows travel with the launch; a page with more components fetches its rows when collected."""
    from surya_amd.detection.model import HipDetCenterlines
    ims = [pages[(300, 1500)], pages[(256, 256)]]
    planted.centerlines = cl.Centerlines()
    old = HipDetCenterlines.HEAD
    try:
        want = [r.model_dump() for r in planted(ims)]
        HipDetCenterlines.HEAD = 3
        got = [r.model_dump() for r in planted(ims)]
    finally:
        HipDetCenterlines.HEAD = old
        planted.centerlines = None
    assert got == want
