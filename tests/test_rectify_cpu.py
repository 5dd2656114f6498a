"""CPU: rectification of rotated line quadrilaterals (RecognitionPredictor.rectify) -- the rule of common/imageops.py against an
independent scalar restatement, its exact cases, the gate, the geometry of assembly and the transport of a line's quad."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
from PIL import Image

from surya_amd.common.imageops import quad_homography, quad_ok, quad_size, rectify_threshold, should_rectify, warp_quad
from surya_amd.config import rec_config
from surya_amd.recognition.loader import RecognitionModelLoader
from surya_amd.recognition.tokenizer import OCRTokenizer

from test_lexicon_cpu import ids_of


# ---------------------------------------------------------------------------------------------- the restatement (no imageops)
def ref_size(quad):
    d = lambda a, b: math.sqrt((quad[a][0] - quad[b][0]) ** 2 + (quad[a][1] - quad[b][1]) ** 2)
    return max(1, int(max(d(1, 0), d(2, 3)) + 0.5)), max(1, int(max(d(3, 0), d(2, 1)) + 0.5))


def ref_homography(quad, W, H):
    A, b = [], []
    for (u, v), (x, y) in zip(((0.0, 0.0), (float(W), 0.0), (float(W), float(H)), (0.0, float(H))), quad):
        A.append([u, v, 1.0, 0.0, 0.0, 0.0, -u * x, -v * x])
        A.append([0.0, 0.0, 0.0, u, v, 1.0, -u * y, -v * y])
        b += [float(x), float(y)]
    return [float(t) for t in np.linalg.solve(np.array(A, np.float64), np.array(b, np.float64))] + [1.0]


def ref_weights(t, a=-0.75):
    w0 = ((a * (t + 1) - 5 * a) * (t + 1) + 8 * a) * (t + 1) - 4 * a
    w1 = ((a + 2) * t - (a + 3)) * t * t + 1
    w2 = ((a + 2) * (1 - t) - (a + 3)) * (1 - t) * (1 - t) + 1
    return [w0, w1, w2, 1.0 - w0 - w1 - w2]


def ref_warp(page, quad, W, H):
    """Section 1 of the rule in scalar Python floats (IEEE float64, one operation at a time: no contraction)."""
    h = ref_homography(quad, W, H)
    ph, pw, C = page.shape
    out = np.zeros((H, W, C), np.uint8)
    px = page.tolist()
    for v in range(H):
        for u in range(W):
            U, V = u + 0.5, v + 0.5
            w = h[6] * U + h[7] * V + h[8]
            sx = (h[0] * U + h[1] * V + h[2]) / w - 0.5
            sy = (h[3] * U + h[4] * V + h[5]) / w - 0.5
            ix, iy = math.floor(sx), math.floor(sy)
            wx, wy = ref_weights(sx - ix), ref_weights(sy - iy)
            for c in range(3):
                acc = None
                for j in range(4):
                    y = min(max(iy - 1 + j, 0), ph - 1)
                    row = None
                    for k in range(4):
                        x = min(max(ix - 1 + k, 0), pw - 1)
                        p = float(px[y][x][c]) * wx[k]
                        row = p if row is None else row + p
                    p = row * wy[j]
                    acc = p if acc is None else acc + p
                out[v, u, c] = int(min(max(round(acc), 0), 255))        # Python's round: half to even, like rint
    return out


def tilted(cx, cy, w, h, deg):
    """The w x h rectangle around (cx, cy), turned by `deg` (clockwise on the screen for deg > 0): clockwise from its top-left corner."""
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return [(cx + c * x - s * y, cy + s * x + c * y) for x, y in ((-w / 2, -h / 2), (w / 2, -h / 2), (w / 2, h / 2), (-w / 2, h / 2))]


QUADS = {
    "tilt17": tilted(31.0, 24.0, 30.0, 9.0, 17.0),
    "tilt-33": tilted(30.5, 23.0, 26.0, 8.0, -33.0),
    "trapezoid": [(8.0, 10.0), (50.0, 14.0), (47.0, 30.0), (12.0, 24.0)],
    "over_two_edges": tilted(58.0, 42.0, 24.0, 10.0, 25.0),              # hangs over the right and the bottom edge of a 64 x 48 page
    "one_pixel": [(10.2, 7.1), (11.1, 7.3), (10.9, 8.2), (10.0, 8.0)],
}


@pytest.fixture(scope="module")
def page():
    return np.random.default_rng(5).integers(0, 256, size=(48, 64, 3), dtype=np.uint8)


@pytest.mark.parametrize("name", list(QUADS))
def test_warp_quad_equals_the_scalar_restatement(page, name):
    quad = QUADS[name]
    assert quad_ok(quad)
    W, H = quad_size(quad)
    assert (W, H) == ref_size(quad)
    if name == "one_pixel":
        assert (W, H) == (1, 1)
    if name == "over_two_edges":
        assert max(p[0] for p in quad) > 64 and max(p[1] for p in quad) > 48
    h = quad_homography(quad, W, H)
    assert h.dtype == np.float64 and h.shape == (9,) and h[8] == 1.0 and h.tolist() == ref_homography(quad, W, H)
    got = warp_quad(page, h, W, H)
    assert got.dtype == np.uint8 and got.shape == (H, W, 3)
    assert np.array_equal(got, ref_warp(page, quad, W, H))


def test_a_stride_4_page_with_junk_in_x_writes_x_as_zero(page):
    rgbx = np.concatenate([page, np.random.default_rng(6).integers(1, 256, size=(48, 64, 1), dtype=np.uint8)], axis=2)
    quad = QUADS["tilt17"]
    W, H = quad_size(quad)
    got = warp_quad(rgbx, quad_homography(quad, W, H), W, H)
    assert got.shape == (H, W, 4) and not got[..., 3].any()
    assert np.array_equal(got[..., :3], ref_warp(page, quad, W, H))


def test_the_homography_maps_the_rectangle_corners_to_the_vertices():
    quad = QUADS["trapezoid"]
    W, H = quad_size(quad)
    h = quad_homography(quad, W, H).reshape(3, 3)
    for (u, v), p in zip(((0, 0), (W, 0), (W, H), (0, H)), quad):
        x, y, w = h @ np.array([u, v, 1.0])
        assert abs(x / w - p[0]) < 1e-9 and abs(y / w - p[1]) < 1e-9


# ------------------------------------------------------------------------------------------------------------- exact cases
def test_an_integer_rectangle_reproduces_the_crop_and_its_rolls_the_rotations(page):
    rect = [(10, 5), (40, 5), (40, 20), (10, 20)]
    crop = page[5:20, 10:40]
    W, H = quad_size(rect)
    assert (W, H) == (30, 15)
    assert np.array_equal(warp_quad(page, quad_homography(rect, W, H), W, H), crop)
    for roll, k in ((1, -1), (2, 2), (3, 1)):
        q = [tuple(p) for p in np.roll(np.array(rect), roll, axis=0).tolist()]
        assert quad_ok(q)
        W, H = quad_size(q)
        assert np.array_equal(warp_quad(page, quad_homography(q, W, H), W, H), np.rot90(crop, k)), roll


# ------------------------------------------------------------------------------------------------------------- small rules
def test_quad_size_rounds_half_up_and_never_below_one():
    assert quad_size([(0, 0), (10.5, 0), (10.5, 3.5), (0, 3.5)]) == (11, 4)
    assert quad_size([(0, 0), (10.25, 0), (10.25, 3.25), (0, 3.25)]) == (10, 3)
    assert quad_size([(0, 0), (12, 0), (11, 0.25), (1, 0.25)]) == (12, 1)                 # the LONGER of two opposite edges; at least 1
    assert quad_size([(0, 0), (3, 4), (3, 4.3), (0, 0.3)]) == (5, 1)                      # norms, not coordinate differences


def test_quad_ok_refuses_what_cannot_be_rectified():
    assert quad_ok([(0, 0), (10, 0), (10, 5), (0, 5)]) and quad_ok(QUADS["tilt-33"]) and quad_ok(QUADS["trapezoid"])
    assert not quad_ok([(0, 0), (10, 5), (10, 0), (0, 5)])                    # a bow-tie
    assert not quad_ok([(0, 0), (0, 5), (10, 5), (10, 0)])                    # counter-clockwise
    assert not quad_ok([(0, 0), (10, 0), (20, 0), (30, 0)])                   # zero area
    assert not quad_ok([(0, 0), (10, 0), (10, 0), (0, 5)])                    # a repeated vertex: not strictly convex
    assert not quad_ok([(0, 0), (10, 0), (5, 5)])                             # three points
    assert not quad_ok([(0, 0), (10, 0), (4, 1), (0, 5)])                     # concave


# ---------------------------------------------------------------------------------------------------------------- the gate
def test_the_gate():
    q5, q20 = tilted(100, 50, 80, 12, 5.0), tilted(100, 50, 80, 12, -20.0)
    rect = [(10, 5), (40, 5), (40, 20), (10, 20)]
    assert rectify_threshold(None) is None and rectify_threshold(True) == 0.0 and rectify_threshold(2.5) == 2.5 and rectify_threshold(0) == 0.0
    for thr, want5, want20 in ((None, False, False), (0.0, True, True), (4.9, True, True), (5.1, False, True), (20.1, False, False)):
        assert should_rectify(q5, thr) is want5 and should_rectify(q20, thr) is want20, thr
    assert not should_rectify(rect, 0.0)                                      # the axis-aligned rectangle in canonical order: today's crop
    assert should_rectify(np.roll(np.array(rect), 1, axis=0).tolist(), 0.0)   # ... but a caller's vertex order is a reading direction
    assert should_rectify(np.roll(np.array(rect), 2, axis=0).tolist(), 0.0)
    assert not should_rectify(rect[:3], 0.0) and not should_rectify(rect + [(5, 12)], 0.0)
    assert not should_rectify([(0, 0), (10, 5), (10, 0), (0, 5)], 0.0) and not should_rectify(q5[::-1], 0.0)
    for bad in (False, -1, -0.5, float("nan"), float("inf"), "10", [3.0], (1,)):
        with pytest.raises(ValueError, match="rectify"):
            rectify_threshold(bad)


def _predictor(device_preprocess=True):
    from surya_amd.recognition.predictor import RecognitionPredictor
    pred = object.__new__(RecognitionPredictor)
    cfg = rec_config("REC-TINY")
    pred.processor = RecognitionModelLoader({"config": cfg, "state_dict": {}}).processor()
    pred.model = SimpleNamespace(vocab=cfg.decoder.vocab_size, device="cpu")
    pred.device_preprocess = device_preprocess
    pred.shard_lines = pred.shard_pages = False
    pred.process_group = None
    return pred


def _page_image():
    return Image.fromarray(np.random.default_rng(9).integers(0, 256, size=(96, 200, 3), dtype=np.uint8), "RGB")


def test_the_predictor_refuses_a_bad_value_before_any_device_work():
    from surya_amd.recognition.predictor import RecognitionPredictor
    assert RecognitionPredictor.rectify is None
    pred, img, box = _predictor(), _page_image(), [[[0, 0, 10, 10]]]
    for bad in (False, -1.0, float("nan"), float("inf"), "on", [1]):
        pred.rectify = bad
        with pytest.raises(ValueError, match="rectify"):
            pred([img], bboxes=box)
        with pytest.raises(ValueError, match="rectify"):
            pred.align([img], [["1"]], bboxes=box)


@pytest.mark.parametrize("dev", [True, False])
def test_slicing_asks_the_gate_for_polygons_and_never_for_bboxes(dev):
    from surya_amd.recognition.predictor import slice_and_pad_poly
    from surya_amd.recognition.preprocess_gpu import LineRef, page_pixels
    pred, img = _predictor(dev), _page_image()
    q5, q20 = tilted(100, 50, 80, 12, 5.0), tilted(100, 40, 80, 12, -20.0)
    rect = [(10, 5), (40, 5), (40, 20), (10, 20)]
    polys = [[q5, rect, q20]]
    tasks = ["ocr_with_boxes"]
    arr = pred.processor.image_processor(img)

    def same(a, b):
        return a == b if dev else np.array_equal(a, b)
    pred.rectify = None
    off = pred.slice_bboxes([img], tasks, polygons=polys)
    assert "quads" not in off and (not dev or all(s.quad is None for s in off["slices"]))
    for value, want in ((True, [True, False, True]), (0.0, [True, False, True]), (10.0, [False, False, True]), (30, [False, False, False])):
        pred.rectify = value
        flat = pred.slice_bboxes([img], tasks, polygons=polys)
        assert [q is not None for q in flat["quads"]] == want and flat["polygons"] == polys[0]
        for s, s_off, pl, w in zip(flat["slices"], off["slices"], polys[0], want):
            if not w:                                                          # today's slice, today's bits
                assert same(s, s_off) and (not dev or s.quad is None)
                continue
            W, H = quad_size(pl)
            assert tuple(s.shape) == (H, W, 3)
            if dev:
                assert isinstance(s, LineRef) and s.quad == tuple((float(x), float(y)) for x, y in pl)
            else:
                assert s.dtype == np.float32
                assert np.array_equal(s, warp_quad(page_pixels(img), quad_homography(pl, W, H), W, H)[..., :3].astype(np.float32))
    if not dev:
        assert np.array_equal(off["slices"][0], slice_and_pad_poly(arr, q5))
    pred.rectify = True
    flat = pred.slice_bboxes([img], tasks, bboxes=[[[10, 5, 40, 20], [3, 3, 90, 30]]])
    assert flat["quads"] == [None, None] and (not dev or all(s.quad is None for s in flat["slices"]))


def test_detected_lines_use_the_scaled_polygon_the_slices_are_cut_from():
    pred, img = _predictor(True), _page_image()
    hi = img.resize((400, 192))
    q = [[int(x), int(y)] for x, y in tilted(100, 50, 80, 12, 8.0)]
    det = lambda images, batch_size=None: [SimpleNamespace(bboxes=[SimpleNamespace(polygon=q)]) for _ in images]
    pred.rectify = 2.0
    flat = pred.detect_and_slice_bboxes([img], ["ocr_with_boxes"], det, None, [hi])
    scaled = tuple((float(int(x * 2.0)), float(int(y * 2.0))) for x, y in q)
    assert flat["quads"] == [scaled] and flat["slices"][0].quad == scaled and flat["polygons"] == [q] and flat["res_scales"] == [(2.0, 2.0)]
    pred.rectify = None
    flat = pred.detect_and_slice_bboxes([img], ["ocr_with_boxes"], det, None, [hi])
    assert "quads" not in flat and flat["slices"][0].quad is None


# ---------------------------------------------------------------------------------------------------------------- assembly
def _assembly_case(quads, polygons, res_scales=None):
    from surya_amd.recognition.processor import SuryaOCRProcessor
    tk = OCRTokenizer(None, None, reserve_special=64)
    proc = SuryaOCRProcessor(tk)
    pred = _predictor()
    pred.processor = proc
    n = len(polygons)
    shapes = []
    for q, pl in zip(quads or [None] * n, polygons):
        if q is not None:
            W, H = quad_size(q)
        else:
            xs, ys = [p[0] for p in pl], [p[1] for p in pl]
            W, H = max(xs) - min(xs), max(ys) - min(ys)
        shapes.append(np.zeros((H, W, 3), np.uint8))
    flat = {"polygons": polygons, "res_scales": res_scales or [(1.0, 1.0)] * n, "slices": shapes}
    if quads is not None:
        flat["quads"] = quads
    items = []
    for i in range(n):
        toks = ids_of(tk, "Boston") + [proc.eos_token_id]
        rows = np.sort(np.random.default_rng(i).integers(0, 1025, size=(len(toks), 6)), axis=0).astype(np.float32)
        rows[:, 4:] = 512                                                      # no skew: axis-aligned character boxes in the crop
        items.append((i, i, toks, [0.5] * len(toks), rows))
    return pred, flat, items


def test_the_identity_quad_gives_the_existing_paths_characters():
    rect = [[20, 30], [220, 30], [220, 70], [20, 70]]
    quad = tuple((float(x), float(y)) for x, y in rect)
    pred, flat, items = _assembly_case([quad, None], [rect, rect])
    got = pred._assemble_batch(flat, items, False, True, 1025)
    pred0, flat0, _ = _assembly_case(None, [rect, rect])
    ref = pred0._assemble_batch(flat0, items, False, True, 1025)
    assert [g.rectified for g in got] == [True, False] and all(r.rectified is None for r in ref)
    strip = lambda d: {k: v for k, v in d.items() if k != "rectified"}
    for g, r in zip(got, ref):
        assert g.text == "Boston" and strip(g.model_dump()) == r.model_dump()
        assert "rectified" in g.model_dump() and "rectified" not in r.model_dump() and "rectified" not in r.model_fields_set
    for it, g in zip(items, got):                                              # the single-line form agrees with the batch form
        one = pred._assemble_line(flat, *it, False, True, 1025)
        assert one.model_dump() == g.model_dump() and one.model_fields_set == g.model_fields_set


def test_a_character_box_of_a_tilted_line_lands_on_the_hand_computed_page_quad():
    from surya_amd.recognition import assemble
    c, s = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
    p0 = (50.0, 40.0)
    W, H = 120, 20
    quad = (p0, (p0[0] + W * c, p0[1] + W * s), (p0[0] + W * c - H * s, p0[1] + W * s + H * c), (p0[0] - H * s, p0[1] + H * c))
    assert quad_size(quad) == (W, H)
    # a rotation is affine: crop point (u, v) sits at p0 + u (c, s) + v (-s, c) on the page
    box = np.array([[[10.0, 2.0], [22.0, 2.0], [22.0, 18.0], [10.0, 18.0]],
                    [[-7.0, -3.0], [130.0, 5.0], [125.0, 26.0], [60.0, 20.0]]])     # the second one leaves the crop: clamped first
    clamped = np.stack([np.clip(box[..., 0], 0, W), np.clip(box[..., 1], 0, H)], axis=-1)
    want = np.stack([p0[0] + clamped[..., 0] * c - clamped[..., 1] * s, p0[1] + clamped[..., 0] * s + clamped[..., 1] * c], axis=-1)
    got = assemble.quad_to_page(box.copy(), quad, (1.0, 1.0))
    assert np.array_equal(got, np.trunc(np.round(want, 6)))
    got2 = assemble.quad_to_page(box.copy(), quad, (2.0, 4.0))                 # the high-res rescale, then int() truncation
    assert np.array_equal(got2, np.stack([np.trunc(np.round(want[..., 0], 6) * 0.5), np.trunc(np.round(want[..., 1], 6) * 0.25)], axis=-1))
    # ... and through the assembly of a line: its characters are tilted quads on the page, outside the polygon's bounding-box clamp
    poly = [[int(x), int(y)] for x, y in quad]
    pred, flat, items = _assembly_case([quad], [poly])
    line = pred._assemble_batch(flat, items, False, False, 1025)[0]
    assert line.rectified is True and line.polygon == [[float(x), float(y)] for x, y in poly] and len(line.chars) == 6
    from surya_amd.recognition.postprocess import prediction_to_polygon_batch
    P = prediction_to_polygon_batch(items[0][4][None], [(H, W, 3)], 1025, 512).astype(np.float64)[0]
    for j, ch in enumerate(line.chars):
        assert ch.polygon == assemble.quad_to_page(P[j].copy(), quad, (1.0, 1.0)).tolist()
        top = np.array(ch.polygon[1]) - np.array(ch.polygon[0])
        assert top[0] == 0 or abs(math.degrees(math.atan2(top[1], top[0])) - 30.0) < 15.0          # (integer corners: roughly 30 degrees)
    one = pred._assemble_line(flat, *items[0], False, False, 1025)
    assert one.model_dump() == line.model_dump()


def test_rectified_is_present_by_the_rule_and_absent_from_the_serialised_form_otherwise():
    from surya_amd.recognition.assemble import _LINE_FIELDS
    from surya_amd.recognition.schema import TextLine
    ln = TextLine(text="x", polygon=[[0, 0], [1, 0], [1, 1], [0, 1]], confidence=0.5, chars=[])
    assert ln.rectified is None and "rectified" not in ln.model_dump() and "rectified" not in ln.model_dump_json()
    ln.rectified = False
    assert ln.model_dump()["rectified"] is False and TextLine.model_validate_json(ln.model_dump_json()) == ln
    assert "rectified" in TextLine.model_json_schema()["properties"] and "rectified" in _LINE_FIELDS
    # a blank line (<NOP>) of a rectifying call reports it too
    pred, flat, items = _assembly_case([QUADS["tilt17"], None], [[[1, 1], [9, 1], [9, 5], [1, 5]]] * 2)
    items = [(i, i, [pred.processor.no_output_token], [0.5], np.zeros((1, 6), np.float32)) for i in range(2)]
    assert [g.rectified for g in pred._assemble_batch(flat, items, False, False, 1025)] == [True, False]


# --------------------------------------------------------------------------------------------------------------- transport
@pytest.mark.parametrize("rank", [0, 1])
def test_shard_lines_deals_the_quads_with_the_lines(monkeypatch, rank):
    import torch
    from surya_amd import dist as sdist
    monkeypatch.setattr(sdist, "collectives_on", lambda group=None: True)
    monkeypatch.setattr(sdist, "world_info", lambda group=None: (rank, 2))
    monkeypatch.setattr(sdist, "collective_device", lambda dev, group=None: "cpu")
    monkeypatch.setattr(sdist, "assert_same_inputs", lambda *a, **k: None)
    monkeypatch.setattr(sdist, "gather_line_outputs", lambda toks, scores, boxes, mine, n_total, max_tokens, **k: (toks, scores, boxes))
    pred, img = _predictor(True), _page_image()
    pred.rectify = 3.0
    polys = [[tilted(100, 50, 60 + 4 * i, 12, 4.0 * i - 8.0) for i in range(7)]]
    flat = pred.slice_bboxes([img], ["ocr_with_boxes"], polygons=polys)
    want = [tuple(map(tuple, p)) if abs(4.0 * i - 8.0) >= 3.0 else None for i, p in enumerate(polys[0])]
    assert [s.quad for s in flat["slices"]] == want and flat["quads"] == want
    seen = {}

    def loop(local, rbs, math_mode):
        seen.update(local)
        m = len(local["slices"])
        return [[5]] * m, torch.zeros((m, 6, 6)), [[0.5]] * m
    pred.prediction_loop = loop
    pred._top_k = None
    pred.sharded_prediction_loop(flat, 4, True)
    assert [s.quad for s in seen["slices"]] == [want[i] for i in range(rank, 7, 2)] and seen["pages"] is flat["pages"]


def test_a_page_sharded_rank_rectifies_its_own_pages(monkeypatch):
    from surya_amd import dist as sdist
    from surya_amd.recognition.schema import OCRResult
    monkeypatch.setattr(sdist, "world_info", lambda group=None: (1, 2))
    monkeypatch.setattr(sdist, "collective_device", lambda dev, group=None: "cpu")
    monkeypatch.setattr(sdist, "assert_same_inputs", lambda *a, **k: None)
    monkeypatch.setattr(sdist, "gather_objects", lambda local, mine, n, group=None: list(local))
    pred = _predictor(True)
    pred.shard_pages, pred.rectify = True, True
    quads = [[[int(x), int(y)] for x, y in tilted(100, 50, 80, 12, 5.0 * i)] for i in range(5)]
    pages = [_page_image() for _ in range(5)]
    index_of = {id(p): i for i, p in enumerate(pages)}
    det = lambda images, batch_size=None: [SimpleNamespace(bboxes=[SimpleNamespace(polygon=quads[index_of[id(im)]])]) for im in images]
    got = {}

    def rank_call(images, task_names, det_predictor, dbs, rbs, highres, *a, **kw):
        flat = pred.detect_and_slice_bboxes(images, task_names, det_predictor, dbs, highres or [None] * len(images))
        got["quads"], got["refs"] = flat["quads"], [s.quad for s in flat["slices"]]
        return [OCRResult(text_lines=[], image_bbox=[0, 0, 1, 1]) for _ in images]
    pred._call = rank_call
    pred._call_page_sharded(pages, ["ocr_with_boxes"] * 5, det, None, None, [None] * 5, False, True, False, False)
    mine = [tuple((float(x), float(y)) for x, y in quads[i]) for i in (1, 3)]
    assert got["quads"] == mine and got["refs"] == mine
