"""GPU: DetectionPredictor.skew end to end on DET-TINY at processor size 256, fp32, and `straighten` on the device.

Where the estimate comes from: synthetic weights give maps without line-shaped text, so the `Planted` predictor below overwrites plane 0 of
every page map with drawn, rotated text bands (tests/det_skew_ref.band_map) AFTER the forward -- the mechanism of bench.py's e2e leg, an
override of `batch_heatmaps`, and its counterparts for the two other sources of a page map: `batch_detection` (the host checker arm) and
`_tiled_batches` (both arms under `tiling`). The same drawn map reaches the device estimator (surya_det_skew behind surya_det_boxes) and
the numpy reference of the checker arm, so the two arms must agree EXACTLY: skew, skew_confidence and last_skew. The plain predictor
(nothing planted) shows that `skew` only adds: boxes and dumps are those of `skew = None`."""
import numpy as np
import pytest
import torch
from PIL import Image

import det_skew_ref as R
from surya_amd.config import det_config
from surya_amd.detection import skew as sk
from surya_amd.synth import make_det_weights, make_pages

pytestmark = pytest.mark.gpu
P = 256
# page size -> planted angle of its MAP (the pages of a call have distinct sizes)
PLANT = {(300, 256): 3.0, (256, 256): -7.5, (200, 180): 0.75, (260, 240): -2.0, (300, 1500): 2.0, (400, 300): 5.0}


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
                for pg, size in enumerate(sizes):
                    tiles = [t for t, k in enumerate(split_index) if k == pg]
                    rows = [split_heights[t] for t in tiles] if len(tiles) > 1 else [heat.shape[2]]
                    m = torch.from_numpy(R.band_map(PLANT[size], (sum(rows), heat.shape[3]))).to(heat.device)
                    r0 = 0
                    for t, r in zip(tiles, rows):
                        heat[t, 0, :r] = m[r0: r0 + r]
                        r0 += r
                yield heat, split_index, split_heights, sizes

        def batch_detection(self, images, batch_size=None):
            for preds, sizes in super().batch_detection(images, batch_size):
                yield [[R.band_map(PLANT[s], p[0].shape), *p[1:]] for p, s in zip(preds, sizes)], sizes

        def _tiled_batches(self, images, batch_size, planes):
            for groups, sizes in super()._tiled_batches(images, batch_size, planes):
                for ks, maps, (mw, mh) in groups:
                    for i, k in enumerate(ks):
                        maps[i, 0, :, :mw] = torch.from_numpy(R.band_map(PLANT[sizes[k]], (mh, mw))).to(maps.device)
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


def _both_arms(pred, ims):
    """(device results, its last_skew, host-checker results, its last_skew) of one predictor with `skew` set by the caller."""
    dev = pred(ims)
    dev_info = list(pred.last_skew)
    pred.device_postprocess = False
    try:
        host = pred(ims)
        host_info = list(pred.last_skew)
    finally:
        pred.device_postprocess = True
    return dev, dev_info, host, host_info


def _equal_skew(dev, dev_info, host, host_info, n):
    assert len(dev) == len(host) == len(dev_info) == len(host_info) == n
    assert dev_info == host_info
    for d, h, info in zip(dev, host, dev_info):
        assert d.skew == h.skew and d.skew_confidence == h.skew_confidence
        assert info["angle"] == d.skew and info["confidence"] == d.skew_confidence


def test_skew_only_adds(plain, pages):
    ims = [pages[k] for k in SMALL + [(300, 1500)]]
    assert plain.skew is None
    before = plain(ims)
    plain.skew = sk.SkewEstimate()
    try:
        with_skew = plain(ims)
        info = list(plain.last_skew)
    finally:
        plain.skew = None
    assert len(info) == len(ims) and [i["map_size"] for i in info] == [(P, P)] * 4 + [(P, 1500)]
    for a, b, i in zip(before, with_skew, info):
        assert a.image_bbox == b.image_bbox and [x.polygon for x in a.bboxes] == [x.polygon for x in b.bboxes]
        assert [x.confidence for x in a.bboxes] == [x.confidence for x in b.bboxes]
        assert (b.skew, b.skew_confidence) == (i["angle"], i["confidence"]) and i["n_text"] >= 0
        assert {k: v for k, v in b.model_dump().items() if k not in ("skew", "skew_confidence")} == a.model_dump()
    # after `skew = None` the call is a fresh predictor's again
    after = plain(ims)
    fresh = _predictor(False)(ims)
    assert [r.model_dump() for r in after] == [r.model_dump() for r in fresh] == [r.model_dump() for r in before]
    assert all("skew" not in r.model_dump() for r in after)


def test_device_equals_host_checker_on_small_pages(planted, pages):
    ims = [pages[k] for k in SMALL]
    planted.skew = sk.SkewEstimate()
    try:
        dev, dev_info, host, host_info = _both_arms(planted, ims)
    finally:
        planted.skew = None
    _equal_skew(dev, dev_info, host, host_info, 4)
    for size, r, info in zip(SMALL, dev, dev_info):
        want = sk.page_angle(PLANT[size], size, (P, P))                 # the plant is the MAP's angle; the result speaks of the page
        print(f"page {size}: planted {PLANT[size]} in the map = {want:.3f} in the page, estimate {r.skew}, confidence {r.skew_confidence}, "
              f"{info['n_text']} text pixels")
        assert r.skew is not None and info["map_size"] == (P, P) and info["n_text"] > 256
        assert abs(r.skew - want) <= 0.5                                # the issue's bound on 256 x 256 maps: two steps of the grid
        # ... and it IS the numpy statement on the drawn map
        a, c, n = sk.estimate(R.band_map(PLANT[size], (P, P)), sk.SkewEstimate(), size, 0.35)
        assert (a, c, n) == (r.skew, r.skew_confidence, info["n_text"])


def test_device_equals_host_checker_on_a_tall_page(planted, pages):
    ims = [pages[(300, 1500)], pages[(256, 256)]]
    planted.skew = sk.SkewEstimate()
    try:
        dev, dev_info, host, host_info = _both_arms(planted, ims)
    finally:
        planted.skew = None
    _equal_skew(dev, dev_info, host, host_info, 2)
    assert dev_info[0]["map_size"] == (P, 1500) and dev[0].skew is not None
    a, c, n = sk.estimate(R.band_map(2.0, (1500, P)), sk.SkewEstimate(), (300, 1500), 0.35)
    assert (a, c, n) == (dev[0].skew, dev[0].skew_confidence, dev_info[0]["n_text"])


def test_device_equals_host_checker_under_tiling(planted, pages):
    from surya_amd.detection.predictor import DetTiling
    ims = [pages[(400, 300)], pages[(200, 180)], pages[(260, 240)]]
    planted.tiling, planted.skew = DetTiling(scale=1.0, overlap=32), sk.SkewEstimate()
    try:
        dev, dev_info, host, host_info = _both_arms(planted, ims)
    finally:
        planted.tiling = planted.skew = None
    _equal_skew(dev, dev_info, host, host_info, 3)
    assert [i["map_size"] for i in dev_info] == [(400, 300), (200, 180), (260, 240)]
    for size, r, info in zip([(400, 300), (200, 180), (260, 240)], dev, dev_info):
        # scale 1: the map is the page (pad columns behind its width), and the estimate IS the numpy statement on the drawn map
        m = np.zeros((size[1], (size[0] + 3) & ~3), np.float32)
        m[:, : size[0]] = R.band_map(PLANT[size], (size[1], size[0]))
        a, c, n = sk.estimate(m, sk.SkewEstimate(), size, 0.35, map_size=size)
        print(f"page {size}: planted {PLANT[size]}, estimate {r.skew}")
        assert r.skew is not None and (a, c, n) == (r.skew, r.skew_confidence, info["n_text"])


def test_iter_detect_and_the_streamed_call_carry_the_same_angles(planted, pages):
    from test_gpu_predictors import make_rec_predictor
    ims = [pages[k] for k in SMALL + [(300, 1500)]]
    planted.skew = sk.SkewEstimate()
    try:
        whole = planted(ims, batch_size=4)
        info = list(planted.last_skew)
        parts = [r for part in planted.iter_detect(ims, batch_size=4) for r in part]
        assert planted.last_skew == info
        assert [r.model_dump() for r in whole] == [r.model_dump() for r in parts] and all(r.skew is not None for r in whole)
        cfg, sd, rec = make_rec_predictor(max_slots=8, max_tokens=4)
        rec.stream_detection = True
        planted.last_skew = []
        rec(ims[:2], det_predictor=planted, detection_batch_size=4)
        assert rec.last_timing.get("streamed") == 1.0
        assert planted.last_skew == info[:2]
    finally:
        planted.skew = None


@pytest.mark.parametrize("shape", [(60, 80, 3), (96, 128, 4)])
def test_straighten_on_the_device_equals_the_host_path(hip_lib, shape):
    page = np.random.default_rng(shape[0]).integers(0, 256, shape, dtype=np.uint8)
    if shape[2] == 4:
        page[..., 3] = 255                                              # the X byte is ignored
    angles = [3.0, -3.0, 15.0, None, 0.05]
    host = sk.straighten([page] * 5, angles)
    dev = sk.straighten([page] * 5, angles, device="cuda:0")
    for a, h, d in zip(angles, host, dev):
        assert h.angle == d.angle and np.array_equal(h.matrix, d.matrix) and h.image.size == d.image.size
        assert np.array_equal(np.asarray(h.image), np.asarray(d.image)), a
    assert host[0].image.size == sk.straighten_size(shape[1], shape[0], 3.0) and host[3].image.size == (shape[1], shape[0])
