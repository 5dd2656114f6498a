"""GPU: DetectionPredictor.tiling end to end on DET-TINY at processor size 128, fp32, overlap 32 (the smallest shapes of test_gpu_det.py).
Every stage of a tiled call is held to an independent statement of it: the model's input batch to tiles Pillow built on the host, the
tiles' heat maps to forward_u8 of those, the stitched page map to the numpy stitch (tests/det_tile_ref.py) of them -- all bit for bit --
and the results to the host post-processing arm on the same call. Then batching, include_maps, iter_detect, the streamed recognise call,
and the default path before and after."""
import math

import numpy as np
import pytest
import torch
from PIL import Image

import det_tile_ref as tr
from surya_amd.config import det_config
from surya_amd.synth import make_det_weights, make_pages

pytestmark = pytest.mark.gpu
P, OVERLAP = 128, 32


def _predictor(max_batch=8):
    from surya_amd.detection.predictor import DetectionModelLoader, DetectionPredictor
    cfg = det_config("DET-TINY")

    class Loader(DetectionModelLoader):
        def model(self, device=None, dtype=None, max_batch_=None):
            return super().model(device, dtype, max_batch=max_batch)

    class Pred(DetectionPredictor):
        model_loader_cls = Loader
    return Pred(checkpoint={"config": cfg, "state_dict": make_det_weights(cfg, 0), "size": P}, dtype=torch.float32)


@pytest.fixture(scope="module")
def pred(hip_lib):
    return _predictor()


@pytest.fixture(scope="module")
def pages():
    a, b = make_pages(2, 720, seed=5)
    stacked = np.vstack([a[:200, :131], b[:130, :131]])
    return {"300x200": Image.fromarray(a[:200, :300]), "128x128": Image.fromarray(b[40:168, 30:158]), "100x90": Image.fromarray(a[100:190, 50:150]),
            "131x330": Image.fromarray(stacked), "520x700": Image.fromarray(b[:700, :520])}


def _host_tiles(im, scale):
    """The tiles as Pillow makes them: the double resize to (mw, mh), pasted on a white canvas, cropped at the grid's offsets (row-major)."""
    W, H = im.size
    mw, mh = max(1, math.ceil(W * scale)), max(1, math.ceil(H * scale))
    s = im
    if (mw, mh) != (W, H):
        s = im.copy()
        s.thumbnail((mw, mh), Image.Resampling.LANCZOS)
        s = s.resize((mw, mh), Image.Resampling.LANCZOS)
    canvas = Image.new("RGB", (max(mw, P), max(mh, P)), (255, 255, 255))
    canvas.paste(s, (0, 0))
    tiles = [np.asarray(canvas.crop((x0, y0, x0 + P, y0 + P))) for y0 in tr.offsets(mh, P, OVERLAP) for x0 in tr.offsets(mw, P, OVERLAP)]
    return (mw, mh), np.stack(tiles)


class _Probe:
    """Records what a call hands to the model and to the post-processing, by wrapping the two bound methods of ONE predictor."""

    def __init__(self, pred):
        from surya_amd.detection.model import HipDetPost
        self.pred, self.tiles, self.heat, self.maps = pred, [], [], []
        if getattr(pred, "_post", None) is None:
            pred._post = HipDetPost(pred.model.device)
        self.fwd, self.launch = pred.model.forward_u8, pred._post.launch

    def __enter__(self):
        def fwd(t, *a, **k):
            h = self.fwd(t, *a, **k)
            self.tiles.append(t.cpu().numpy())
            self.heat.append(h.cpu().numpy())
            return h

        def launch(m, *a, **k):
            self.maps.extend(m.cpu().numpy())
            return self.launch(m, *a, **k)
        self.pred.model.forward_u8, self.pred._post.launch = fwd, launch
        return self

    def __exit__(self, *exc):
        del self.pred.model.forward_u8, self.pred._post.launch


def _same(a, b, atol=0.0):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.image_bbox == y.image_bbox
        assert [bx.polygon for bx in x.bboxes] == [bx.polygon for bx in y.bboxes]
        assert np.allclose([bx.confidence for bx in x.bboxes], [bx.confidence for bx in y.bboxes], rtol=0, atol=atol)


@pytest.mark.parametrize("names,scale", [(("300x200", "128x128", "100x90", "131x330"), 1.0), (("520x700",), 0.5)])
def test_every_stage_of_a_tiled_call(pred, pages, names, scale):
    from surya_amd.detection.predictor import DetTiling
    ims = [pages[n] for n in names]
    pred.tiling = DetTiling(scale=scale, overlap=OVERLAP)
    try:
        with _Probe(pred) as probe:
            res = pred(ims)
        pred.device_postprocess = False
        host = pred(ims)
    finally:
        pred.device_postprocess, pred.tiling = True, None
    assert all(len(t) <= pred.model.max_batch for t in probe.tiles)
    got_tiles, got_heat = np.concatenate(probe.tiles), np.concatenate(probe.heat)
    maps = {m.shape: m for m in probe.maps}
    assert len(maps) == len(ims)
    mean, std = pred.processor.image_mean, pred.processor.image_std
    t0 = 0
    for im, info, r in zip(ims, pred.last_tiling, res):
        (mw, mh), want = _host_tiles(im, scale)
        n = len(want)
        assert info == {"size": (mw, mh), "grid": (len(tr.offsets(mw, P, OVERLAP)), len(tr.offsets(mh, P, OVERLAP))), "tiles": n}
        mine = got_tiles[t0: t0 + n]
        assert np.array_equal(mine[..., :3], want) and not mine[..., 3].any()                        # the model's input batch
        ref_heat = np.concatenate([pred.model.forward_u8(torch.from_numpy(want[s: s + 8]).cuda().contiguous(), mean, std).cpu().numpy()
                                   for s in range(0, n, 8)])
        assert np.array_equal(got_heat[t0: t0 + n].view(np.int32), ref_heat.view(np.int32))          # the tiles' heat maps
        pitch = (mw + 3) & ~3
        st = tr.stitch(ref_heat, mw, mh, P, OVERLAP, planes=1)
        assert np.array_equal(maps[(1, mh, pitch)].view(np.int32), st.view(np.int32))                # the stitched page map
        assert r.image_bbox == [0, 0, im.size[0], im.size[1]] and r.heatmap is None
        t0 += n
    assert t0 == len(got_tiles)
    if scale == 1.0:
        assert [i["tiles"] for i in pred.last_tiling] == [6, 1, 1, 8]
    else:
        assert pred.last_tiling[0]["size"] == (260, 350) and pred.last_resize_paths == {"device": 1, "host": 0, "ready": 0}
    _same(res, host, atol=1e-6)                                                                    # the checker arm on the same call
    assert sum(len(r.bboxes) for r in res) >= 1


def test_scaled_page_resized_by_pillow_on_the_host_gives_the_same_call(pred, pages):
    """DETECTOR_RESIZE_HOST under tiling: the scaled page comes from Pillow instead of the device resampler -- the same bytes, so the same results."""
    from surya_amd.detection.predictor import DetTiling
    pred.tiling = DetTiling(scale=0.5, overlap=OVERLAP)
    try:
        dev = pred([pages["520x700"]])
        pred.device_resize = False
        host = pred([pages["520x700"]])
        assert pred.last_resize_paths == {"device": 0, "host": 1, "ready": 0}
    finally:
        pred.device_resize, pred.tiling = True, None
    assert [r.model_dump() for r in dev] == [r.model_dump() for r in host]


def test_batching_does_not_change_a_page(pred, pages):
    """max_batch = 3: a page of six tiles runs alone in two forwards and is stitched incrementally; three one-tile pages share a forward
    (two of them of one map size: one post-processing call); a batch of one tile of each. Every page's result is that of the page alone."""
    from surya_amd.detection.predictor import DetTiling
    small = _predictor(max_batch=3)
    til = DetTiling(scale=1.0, overlap=OVERLAP)
    names = ["128x128", "300x200", "100x90", "128x128", "100x90"]
    ims = [pages[n] for n in names]
    small.tiling = pred.tiling = til
    try:
        with _Probe(small) as probe:
            together = small(ims)
        assert [len(t) for t in probe.tiles] == [1, 3, 3, 3]
        assert [m.shape for m in probe.maps] == [(1, 128, 128), (1, 200, 300), (1, 90, 100), (1, 90, 100), (1, 128, 128)]
        alone = [small([im])[0] for im in ims]
        wide = pred(ims)                                               # max_batch = 8: [1 + 6 + 1], [1 + 1]
        two = small(ims, batch_size=2)
    finally:
        pred.tiling = None
    for other in (alone, wide, two):
        assert [r.model_dump() for r in together] == [r.model_dump() for r in other]
    assert sum(len(r.bboxes) for r in together) >= 1


def test_include_maps_returns_the_stitched_valid_region(pred, pages):
    from surya_amd.detection.predictor import DetTiling
    ims = [pages["131x330"], pages["100x90"]]
    pred.tiling = DetTiling(scale=1.0, overlap=OVERLAP)
    try:
        plain = pred(ims)
        with _Probe(pred) as probe:
            res = pred(ims, include_maps=True)
    finally:
        pred.tiling = None
    heat = np.concatenate(probe.heat)
    _same(res, plain)
    t0 = 0
    for im, r, info in zip(ims, res, pred.last_tiling):
        (mw, mh), n = im.size, info["tiles"]
        st = tr.stitch(heat[t0: t0 + n], mw, mh, P, OVERLAP, planes=2)
        assert r.heatmap.size == (mw, mh) and r.affinity_map.size == (mw, mh)
        assert np.array_equal(np.asarray(r.heatmap), (st[0, :, :mw] * 255).astype(np.uint8))
        assert np.array_equal(np.asarray(r.affinity_map), (st[1, :, :mw] * 255).astype(np.uint8))
        t0 += n


def test_iter_detect_under_tiling_equals_the_call(pred, pages):
    from surya_amd.detection.predictor import DetTiling
    ims = [pages[n] for n in ("100x90", "300x200", "128x128", "131x330", "100x90")]
    pred.tiling = DetTiling(scale=1.0, overlap=OVERLAP)
    try:
        whole = pred(ims)
        parts = list(pred.iter_detect(ims))
    finally:
        pred.tiling = None
    assert [len(p) for p in parts] == [3, 1, 1]                          # tiles 1 + 6 + 1 | 8 | 1 at max_batch = 8
    assert [r.model_dump() for r in whole] == [r.model_dump() for p in parts for r in p]


def test_streamed_recognition_equals_serial_under_tiling(pred, pages):
    from test_gpu_predictors import make_rec_predictor
    from surya_amd.detection.predictor import DetTiling
    cfg, sd, rec = make_rec_predictor(max_slots=8, max_tokens=6)
    ims = [pages["300x200"], pages["131x330"]]
    pred.tiling = DetTiling(scale=1.0, overlap=OVERLAP)
    try:
        det_res = pred(ims)
        rec.stream_detection = False
        serial = rec(ims, det_predictor=pred)
        rec.stream_detection = True
        streamed = rec(ims, det_predictor=pred)
        assert rec.last_timing.get("streamed") == 1.0
    finally:
        pred.tiling = None
    assert [r.model_dump() for r in serial] == [r.model_dump() for r in streamed]
    assert [len(r.text_lines) for r in serial] == [len(d.bboxes) for d in det_res] and sum(len(d.bboxes) for d in det_res) >= 1


def test_default_path_is_untouched_by_a_tiled_call(pred, pages):
    from surya_amd.detection.predictor import DetTiling
    ims = [pages[n] for n in ("300x200", "128x128", "131x330", "520x700")]
    fresh = _predictor()
    assert fresh.tiling is None
    want = [r.model_dump() for r in fresh(ims)]
    want_paths = dict(fresh.last_resize_paths)
    assert pred.tiling is None
    before = [r.model_dump() for r in pred(ims)]
    assert pred.last_resize_paths == want_paths
    pred.tiling = DetTiling(scale=0.5, overlap=OVERLAP)
    try:
        pred(ims)
        with pytest.raises(ValueError):
            pred.tiling = DetTiling(scale=1.0, overlap=P // 2 + 1)
            pred(ims)
    finally:
        pred.tiling = None
    after = [r.model_dump() for r in pred(ims)]
    assert before == want and after == want and pred.last_resize_paths == want_paths
