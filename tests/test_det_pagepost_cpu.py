"""CPU: the page-map post stage of the detector (surya_amd/detection/pagepost.py) and the helpers the predictor's sources share: the greedy
packing, the groups of a batch of strips, the host arm's per-page function against heatmap.parallel_get_boxes, and the whole untiled
checker arm on a stand-in model with both extras on, through the thread pool and serially."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

from surya_amd.common.geometry import TextBox
from surya_amd.detection import heatmap as hm
from surya_amd.detection import pagepost as pp
from surya_amd.settings import settings

TEXT, BLANK = np.float32(0.9), np.float32(0.02)


def _plain_packing(counts, batch_size):
    """The reference's loop (surya/detection/__init__.py:77-90) said a second way: fill a batch until the next page would overflow it."""
    batches, i = [], 0
    while i < len(counts):
        batch, n = [i], counts[i]
        i += 1
        while i < len(counts) and n + counts[i] <= batch_size:
            batch.append(i)
            n += counts[i]
            i += 1
        batches.append(batch)
    return batches


@pytest.mark.parametrize("counts", [[1, 1, 3, 1, 4, 1, 1], [1, 20, 1, 1], [17], []])
@pytest.mark.parametrize("batch_size", [1, 3, 4, 16])
def test_pack_greedy(counts, batch_size):
    from surya_amd.detection.predictor import pack_greedy
    got = pack_greedy(counts, batch_size)
    assert got == _plain_packing(counts, batch_size)
    assert [i for b in got for i in b] == list(range(len(counts))) and all(got)
    for b in got:
        assert sum(counts[i] for i in b) <= batch_size or len(b) == 1


def test_strip_groups():
    rng = np.random.default_rng(0)
    split_index = [0, 1, 1, 1, 2, 3, 3, 3, 4, 4]
    split_heights = [8, 8, 8, 3, 8, 8, 8, 3, 8, 5]
    heat = torch.from_numpy(rng.random((10, 2, 8, 8), dtype=np.float32))
    before = heat.clone()
    groups = pp.strip_groups(heat, split_index, split_heights)
    assert [(list(ks), tuple(m.shape), size) for ks, m, size in groups] == [([0, 2], (2, 2, 8, 8), (8, 8)), ([1, 3], (2, 19, 8), (8, 19)),
                                                                            ([4], (1, 13, 8), (8, 13))]
    assert all(m.is_contiguous() and m.dtype == torch.float32 for _, m, _ in groups)
    assert torch.equal(groups[0].maps, heat[[0, 4]])
    for ks, maps, (mw, mh) in groups[1:]:
        for i, page in enumerate(ks):
            strips = [t for t, k in enumerate(split_index) if k == page]
            want = np.vstack([heat[t, 0, : split_heights[t]].numpy() for t in strips])
            assert want.shape == (mh, mw) and np.array_equal(maps[i].numpy(), want)
    assert torch.equal(heat, before)
    # only whole pages: the group's tensor IS the batch's, no copy on the default path
    (ks, maps, size), = pp.strip_groups(heat[:3], [0, 1, 2], [8, 5, 8])
    assert list(ks) == [0, 1, 2] and size == (8, 8) and maps.data_ptr() == heat.data_ptr() and maps.shape == (3, 2, 8, 8)


def _drawn_maps():
    empty = np.full((48, 48), BLANK)
    nested = np.full((96, 128), BLANK)                       # a frame and a bar in its hole: the bar's box lies inside the frame's
    nested[10:80, 10:110] = TEXT
    nested[16:74, 16:104] = BLANK
    nested[40:48, 30:90] = TEXT
    wide = np.full((40, 100), BLANK)
    wide[8:15, 5:90] = TEXT
    wide[24:31, 20:70] = TEXT
    square = np.full((64, 64), BLANK)                        # a near-square component (the upright box) beside a line
    square[10:30, 12:33] = TEXT
    square[44:50, 4:60] = TEXT
    tilted = np.full((80, 120), BLANK)
    yy, xx = np.mgrid[0:80, 0:120]
    tilted[np.abs(yy - (20 + 0.3 * xx)) < 4] = TEXT
    return {"empty": empty, "nested": nested, "wide": wide, "square": square, "tilted": tilted}


@pytest.mark.parametrize("name", ["empty", "nested", "wide", "square", "tilted"])
@pytest.mark.parametrize("include_maps", [False, True])
def test_host_page_is_parallel_get_boxes(name, include_maps):
    text = _drawn_maps()[name]
    H, W = text.shape
    aff = np.random.default_rng(1).random((H, W), dtype=np.float32)
    page_size = (3 * W + 1, 2 * H + 5)
    want = hm.parallel_get_boxes([text, aff], page_size, include_maps)
    got, infos = pp.host_page([], text, aff if include_maps else None, (W, H), page_size)
    assert infos == []
    a, b = got.model_dump(), want.model_dump()
    for key in ("heatmap", "affinity_map"):
        x, y = a.pop(key), b.pop(key)
        assert (x is None) == (y is None) == (not include_maps)
        if include_maps:
            assert x.size == y.size == (W, H) and x.mode == y.mode and np.array_equal(np.asarray(x), np.asarray(y))
    assert a == b
    n_found = len(hm.detect_boxes(text, settings.DETECTOR_TEXT_THRESHOLD, settings.DETECTOR_BLANK_THRESHOLD)[0])
    assert (n_found, len(got.bboxes)) == {"empty": (0, 0), "nested": (2, 1), "wide": (2, 2), "square": (2, 2), "tilted": (1, 1)}[name]


def test_host_page_crops_the_images_of_a_padded_map():
    """A stitched map is wider than its valid region by the pad columns: the boxes come from the whole array, the images from the region."""
    text = np.full((40, 52), BLANK)
    text[8:15, 5:45] = TEXT
    aff = np.random.default_rng(2).random((40, 52), dtype=np.float32)
    got, _ = pp.host_page([], text, aff, (50, 40), (100, 80))
    assert got.heatmap.size == got.affinity_map.size == (50, 40)
    assert np.array_equal(np.asarray(got.affinity_map), (aff[:, :50] * 255).astype(np.uint8))
    assert got.model_dump()["bboxes"] == pp.host_page([], text, None, (50, 40), (100, 80))[0].model_dump()["bboxes"]


def test_untiled_checker_arm_with_both_extras_pool_and_serial():
    """`_detect` with device_postprocess off on the stand-in model of tests/test_oracle_vs_reference.py (logits = a fixed function of the pixels,
    on the CPU): five pages in batches of two strips' worth, one of them cut into strips, skew and centre lines on."""
    from surya_amd.detection.predictor import Centerlines, DetectionPredictor, SegformerImageProcessor, SkewEstimate
    size = 64

    def fake_logits(x):
        x = x.float()
        return torch.stack([x.mean(1) * 0.5 + x[:, 0] * 0.25, x[:, 2] - x[:, 1]], 1)

    pred = object.__new__(DetectionPredictor)
    pred.processor = SegformerImageProcessor({"height": size, "width": size})
    pred.model = SimpleNamespace(max_batch=64, cfg=SimpleNamespace(num_labels=2), device="cpu", forward=fake_logits)
    pred.device_postprocess, pred.skew, pred.centerlines = False, SkewEstimate(), Centerlines(knots=8)

    def page(w, h, lines):                                    # white lines on black: the stand-in's text map is high where the page is white
        a = np.zeros((h, w, 3), np.uint8)
        for y0, x0, x1, slope in lines:
            for x in range(x0, x1):
                y = y0 + int(round(slope * (x - x0)))
                a[y: y + 6, x] = 255
        return Image.fromarray(a)
    pages = [page(64, 64, [(10, 4, 60, 0.0), (40, 4, 60, 0.1)]), page(128, 96, [(20, 8, 120, 0.05)]), page(60, 150, [(12, 4, 56, 0.0), (100, 4, 56, 0.0)]),
             page(64, 64, []), page(80, 64, [(30, 6, 74, -0.1)])]
    old = (settings.DETECTOR_IMAGE_CHUNK_HEIGHT, settings.DETECTOR_MIN_PARALLEL_THRESH)
    settings.DETECTOR_IMAGE_CHUNK_HEIGHT = 100
    runs = []
    try:
        for thresh in (3, 6):                                 # five pages: the thread pool, then the serial branch
            settings.DETECTOR_MIN_PARALLEL_THRESH = thresh
            res = pred._detect([p.copy() for p in pages], batch_size=2)
            runs.append(([r.model_dump() for r in res], list(pred.last_skew), list(pred.last_centerlines)))
            assert len(res) == len(pred.last_skew) == len(pred.last_centerlines) == 5
            assert [r.image_bbox for r in res] == [[0, 0, *p.size] for p in pages]
            assert [i["map_size"] for i in pred.last_skew] == [(64, 64), (64, 64), (64, 150), (64, 64), (64, 64)]
            for r, s, c in zip(res, pred.last_skew, pred.last_centerlines):
                assert r.skew == s["angle"] and r.skew_confidence == s["confidence"] and r.heatmap is None
                assert set(c) == {"n_boxes", "n_curved"} and c["n_boxes"] >= len(r.bboxes)
            assert sum(len(r.bboxes) for r in res) >= 4 and len(res[3].bboxes) == 0
        maps = [(p[0], s) for preds, sizes in pred.batch_detection([p.copy() for p in pages], batch_size=2) for p, s in zip(preds, sizes)]
    finally:
        settings.DETECTOR_IMAGE_CHUNK_HEIGHT, settings.DETECTOR_MIN_PARALLEL_THRESH = old
    assert runs[0] == runs[1]
    # ... and every entry IS the rule's own statement on that page's map, asked directly
    from surya_amd.detection import centerline as cl
    from surya_amd.detection import skew as sk
    tt, lt = settings.DETECTOR_TEXT_THRESHOLD, settings.DETECTOR_BLANK_THRESHOLD
    assert len(maps) == 5
    for (heat, size), r, s, c in zip(maps, res, runs[0][1], runs[0][2]):
        angle, conf, n_text = sk.estimate(heat, SkewEstimate(), size, lt)
        assert s == {"angle": angle, "confidence": conf, "n_text": n_text, "map_size": (heat.shape[1], heat.shape[0])}
        boxes = [TextBox(polygon=b, confidence=float(cf)) for b, cf in zip(*hm.detect_boxes(heat, tt, lt))]
        n_curved = cl.attach(boxes, cl.profile_page(heat, tt, lt, 8), Centerlines(knots=8))
        assert c == {"n_boxes": len(boxes), "n_curved": n_curved}
        assert sum(b.centerline is not None for b in r.bboxes) <= n_curved
    assert any(s["angle"] is not None for s in runs[0][1])


def test_groups_may_be_plain_tuples_and_refusals_keep_their_order():
    """The currency is (pages, maps, (mw, mh)): a source may yield it as a plain tuple. The skew is checked before the centre lines, and its
    `last_skew` is emptied as its own check passes."""
    from surya_amd.detection.predictor import Centerlines, DetectionPredictor, SegformerImageProcessor, SkewEstimate
    maps = torch.arange(2 * 2 * 6 * 8, dtype=torch.float32).reshape(2, 2, 6, 8) / 255
    images = pp.stitched_map_images([([1], maps[:1], (5, 6)), ([0, 2], maps, (7, 4))])
    heat, aff = images(2)
    assert heat.size == aff.size == (7, 4)
    assert np.array_equal(np.asarray(aff), (maps[1, 1, :4, :7].numpy() * 255).astype(np.uint8))
    assert images(1)[0].size == (5, 6)
    pred = object.__new__(DetectionPredictor)
    pred.processor = SegformerImageProcessor({"height": 64, "width": 64})
    pred.skew, pred.centerlines, pred.last_skew, pred.last_centerlines = SkewEstimate(max_angle=50), Centerlines(knots=1), ["old"], ["old"]
    with pytest.raises(ValueError, match="max_angle"):
        pp.PagePost(pred, [])
    assert pred.last_skew == ["old"] and pred.last_centerlines == ["old"]
    pred.skew = SkewEstimate()
    with pytest.raises(ValueError, match="knots"):
        pp.PagePost(pred, [])
    assert pred.last_skew == [] and pred.last_centerlines == ["old"]
    pred.centerlines = Centerlines()
    assert [type(e) for e in pp.PagePost(pred, []).extras] == [pp.CenterlineExtra, pp.SkewExtra] and pred.last_centerlines == []
