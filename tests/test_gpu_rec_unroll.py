"""GPU: RecognitionPredictor.unroll on REC-TINY, fp32 (tiny synthetic weights: what is compared is the route of the pixels, not the text).

  * a line with a straight, horizontal centre line at integer coordinates reads as the same line passed as `bboxes=`: tokens, scores and
    character boxes, and the prepared crops' tiles are byte-identical;
  * a bent line's prepared tiles on the device equal the host slicing arm (warp_columns, then the host chain) within
    test_gpu_prep.py's 2e-5, and the two predictor arms agree;
  * `TextLine.unrolled` per line; character quads lie inside the band around the centre line;
  * `unroll = None` returns and dumps what it always did; a bad curve raises ValueError before any launch;
  * end to end behind a detector whose `centerlines` is set, streamed == serial."""
import numpy as np
import pytest
import torch
from PIL import Image

from surya_amd.common.imageops import Curve, curve_size, curve_table, warp_columns
from surya_amd.config import rec_config
from surya_amd.synth import make_pages

pytestmark = pytest.mark.gpu


def _dump(results):
    return [r.model_dump() for r in results]


def _bent(x0, x1, y0, sag, n=9):
    xs = np.linspace(x0, x1, n)
    return [(float(x), float(y0 + sag * np.sin(np.pi * (x - x0) / (x1 - x0)))) for x in xs]


def _lines():
    """Two 256^2 pages; per page polygons (bounding rectangles) and centre lines: a straight integer one, two bent ones, and lines
    without a centre line."""
    pages = [Image.fromarray(p) for p in make_pages(2, 256, seed=8)]
    rect = lambda x0, y0, x1, y1: [[x0, y0], [x1, y0], [x1, y1], [x0, y1]]
    polys = [[rect(20, 30, 230, 58), rect(10, 80, 246, 140), rect(30, 170, 220, 200)], [rect(16, 20, 240, 90), rect(10, 200, 240, 240)]]
    curves = [[([(20, 44), (230, 44)], 28), (_bent(12.0, 244.0, 96.0, 24.0), 26.0), None], [(_bent(18.0, 238.0, 70.0, -30.0, n=13), 30.0), None]]
    return pages, polys, curves


def _processor():
    from surya_amd.recognition.predictor import RecognitionModelLoader
    return RecognitionModelLoader({"config": rec_config("REC-TINY"), "state_dict": {}}).processor()


@pytest.mark.parametrize("pix", [3, 4])
def test_device_preprocessor_unrolls_in_front_of_the_ordinary_chain(hip_lib, pix):
    from test_gpu_rectify import CountingLib
    from surya_amd.recognition.preprocess_gpu import DevicePreprocessor, bbox_ref, curve_ref, poly_ref, quad_ref
    proc = _processor()
    pages = [make_pages(1, 256, seed=5)[0], np.random.default_rng(4).integers(0, 256, size=(90, 131, 3), dtype=np.uint8)]
    if pix == 4:
        pages = [np.concatenate([p, np.full(p.shape[:2] + (1,), 77, np.uint8)], axis=2) for p in pages]
    pre = DevicePreprocessor("cuda:0")
    pre.lib = CountingLib(pre.lib, "surya_rec_unroll")
    sizes = lambda n: [(1024, 256)] * n
    plain = [bbox_ref(0, 256, 256, [10, 20, 240, 60]), poly_ref(0, 256, 256, [[20, 120], [230, 128], [228, 170], [18, 160]]),
             bbox_ref(1, 131, 90, [3, 5, 120, 47])]
    t0, o0, g0 = pre(pages, plain, sizes(3))
    assert pre.lib.calls == 0                                           # a call without a curve never reaches the new entry point
    # straight integer centre lines: bbox_ref's tiles, bit for bit (one of a size that takes both resampling stages)
    forced = curve_ref(0, 256, 256, [[10, 20], [240, 20], [240, 60], [10, 60]], Curve([(10, 40), (240, 40)], 40))
    odd = curve_ref(1, 131, 90, [[3, 5], [120, 5], [120, 47], [3, 47]], Curve([(3, 26), (60, 26), (120, 26)], 42))
    bent = [(0, Curve(_bent(12.0, 244.0, 96.0, 24.0), 26.0)), (0, Curve(_bent(30.0, 200.0, 200.0, -18.0, n=5), 17.0)),
            (1, Curve(_bent(-10.0, 140.0, 40.0, 12.0), 20.0))]         # the last one hangs over both sides of page 1
    tilt = quad_ref(0, 256, 256, [(40.0, 30.0), (200.0, 50.0), (197.0, 74.0), (37.0, 54.0)])
    lines = [forced, plain[1], odd] + [curve_ref(pi, pages[pi].shape[1], pages[pi].shape[0], [[0, 0], [9, 0], [9, 9], [0, 9]], c) for pi, c in bent] + [tilt, plain[0]]
    t1, o1, g1 = pre(pages, lines, sizes(len(lines)))
    assert pre.lib.calls == 1
    rows = lambda t, o, i: t[int(o[i]):int(o[i + 1])]
    assert g1[0] == g0[0] and torch.equal(rows(t1, o1, 0), rows(t0, o0, 0))
    assert g1[2] == g0[2] and torch.equal(rows(t1, o1, 2), rows(t0, o0, 2))
    assert torch.equal(rows(t1, o1, 1), rows(t0, o0, 1)) and torch.equal(rows(t1, o1, 7), rows(t0, o0, 0))      # neighbours do not notice
    worst = 0.0
    for k, (pi, c) in enumerate(bent):
        W, H, _ = curve_size(*c)
        assert lines[3 + k].shape == (H, W, 3)
        table, _, _ = curve_table(*c)
        crop = warp_columns(pages[pi], table, H)[..., :3].astype(np.float32)
        ref, grid = proc.process_and_tile(proc.scale_to_fit(crop, (1024, 256)))
        got = rows(t1, o1, 3 + k).cpu().numpy()
        assert g1[3 + k] == grid and got.shape == ref.shape
        worst = max(worst, float(np.abs(got - ref).max()))
    print("unrolled tiles vs host chain: worst |diff| =", worst)
    assert worst <= 2e-5, worst
    t2, o2, g2 = pre(pages, plain, sizes(3))                            # the plain call again: what it returned before
    assert pre.lib.calls == 1 and g2 == g0 and np.array_equal(o2, o0) and torch.equal(t2, t0)


def test_predictor_unrolls_on_both_paths_and_switches_off_cleanly(hip_lib):
    from test_gpu_predictors import make_rec_predictor
    pages, polys, curves = _lines()
    cfg, sd, fresh = make_rec_predictor(max_slots=8, max_tokens=8)
    baseline = fresh(pages, polygons=polys)
    as_bbox = fresh([pages[0]], bboxes=[[[20, 30, 230, 58]]])
    cfg, sd, pred = make_rec_predictor(max_slots=8, max_tokens=8)
    out = {}
    try:
        # `centerlines` without `unroll`: nothing changes
        pred.centerlines = curves
        assert _dump(pred(pages, polygons=polys)) == _dump(baseline)
        pred.unroll = True
        for dev in (True, False):
            pred.device_preprocess = dev
            out[dev] = pred(pages, polygons=polys)
        for a, b in zip(out[True], out[False]):
            assert [l.text for l in a.text_lines] == [l.text for l in b.text_lines]
            for la, lb in zip(a.text_lines, b.text_lines):
                assert [c.polygon for c in la.chars] == [c.polygon for c in lb.chars] and la.unrolled is lb.unrolled
        lines = [l for r in out[True] for l in r.text_lines]
        assert [l.unrolled for l in lines] == [True, True, False, True, False]
        assert [l.polygon for l in lines] == [[[float(x), float(y)] for x, y in p] for pg in polys for p in pg]     # the polygon that came in
        # the straight integer centre line: the line read as bboxes=[20, 30, 230, 58] -- text, confidence, characters
        a, b = lines[0], as_bbox[0].text_lines[0]
        assert a.text == b.text and a.confidence == b.confidence and len(a.chars) == len(b.chars)
        assert [(c.text, c.confidence, c.polygon) for c in a.chars] == [(c.text, c.confidence, c.polygon) for c in b.chars]
        # the lines without a centre line are the parent's, field for field
        strip = lambda d: {k: v for k, v in d.items() if k != "unrolled"}
        assert strip(lines[2].model_dump()) == baseline[0].text_lines[2].model_dump()
        assert strip(lines[4].model_dump()) == baseline[1].text_lines[1].model_dump()
        # character quads of the bent lines lie inside the band around the centre line (+ 1 px for the truncation)
        seen = 0
        for l, (pts, th) in ((lines[1], curves[0][1]), (lines[3], curves[1][0])):
            table, _, H = curve_table(pts, th)
            for ch in l.chars:
                for x, y in ch.polygon:
                    d = float(np.hypot(table[:, 0] - x, table[:, 1] - y).min())
                    assert d <= th / 2 + 1.0 + 0.75, (ch.polygon, d)          # (0.75: half a column between two table entries, and H's rounding)
                    seen += 1
        assert seen > 0
        # together with rectify and a pattern: an unrolled line is not rectified, every field is reported
        pred.device_preprocess, pred.rectify, pred.pattern = True, True, r"\d+"
        both = [l for r in pred(pages, polygons=polys) for l in r.text_lines]
        assert [l.unrolled for l in both] == [True, True, False, True, False] and [l.rectified for l in both] == [False] * 5
        assert all(l.pattern_matched is not None and set(l.text) <= set("0123456789") for l in both)
        # a bad curve: ValueError naming the line, before any launch
        pred.rectify = pred.pattern = None
        bad = [[None, ([(0, 0), (0, 0)], 5), None], [None, None]]
        pred.centerlines = bad
        with pytest.raises(ValueError, match="image 0, line 1"):
            pred(pages, polygons=polys)
        pred.centerlines = None
        pred.unroll = "yes"
        with pytest.raises(ValueError, match="unroll"):
            pred(pages, polygons=polys)
    finally:
        pred.unroll = pred.rectify = pred.pattern = pred.centerlines = None
        pred.device_preprocess = True
    again = pred(pages, polygons=polys)
    assert _dump(again) == _dump(baseline) and all(l.unrolled is None and "unrolled" not in l.model_dump() for r in again for l in r.text_lines)


def test_detect_with_centerlines_then_unroll_streamed_equals_serial(hip_lib):
    """A detector with `centerlines` set, its maps planted with bent bands: the bent lines arrive with their centre lines and are unrolled,
    on the streamed path as on the serial one."""
    import det_centerline_ref as R
    from test_gpu_det_centerlines import _predictor
    from test_gpu_predictors import make_rec_predictor
    from surya_amd.detection import centerline as cl
    det = _predictor(True)
    pages = [Image.fromarray(p) for p in make_pages(3, 256, seed=11)]
    cfg, sd, pred = make_rec_predictor(max_slots=8, max_tokens=6)
    try:
        det.centerlines = cl.Centerlines()
        pred.unroll = True
        pred.stream_detection = False
        serial = pred(pages, det_predictor=det, detection_batch_size=2)
        pred.stream_detection = True
        streamed = pred(pages, det_predictor=det, detection_batch_size=2)
        assert pred.last_timing.get("streamed") == 1.0
        assert _dump(serial) == _dump(streamed) and len(streamed) == 3
        flags = [l.unrolled for r in streamed for l in r.text_lines]
        assert len(flags) == 15 and sum(flags) == 12                    # per page five bands, one of them straight
        # without centre lines from the detector nothing is unrolled
        det.centerlines = None
        assert [l.unrolled for r in pred(pages, det_predictor=det, detection_batch_size=2) for l in r.text_lines] == [False] * 15
    finally:
        det.centerlines = None
        pred.unroll = None
    assert R.bent_page(256, 256).shape == (256, 256)
