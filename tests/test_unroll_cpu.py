"""CPU: unrolling a bent text line along its centre line (surya_amd/common/imageops.py: curve_table, warp_columns, curve_to_page, curve_ok).
A straight horizontal line at integer coordinates reproduces the page's slice byte for byte; a striped page of bent bands unrolls into
straight rows where the bounding rectangle has no clean row; the map back to the page returns the centre line; every refusal; header,
binding and descriptor against each other."""
import os
import re

import numpy as np
import pytest

from surya_amd.common import imageops as io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _page(h, w, pix=3, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, pix), dtype=np.uint8)


@pytest.mark.parametrize("pix", [3, 4])
@pytest.mark.parametrize("box", [(5, 7, 60, 19), (0, 0, 80, 50), (33, 20, 34, 21), (10, 10, 43, 26)])
def test_table_of_a_straight_line_reproduces_the_slice(box, pix):
    x0, y0, x1, y1 = box
    page = _page(50, 80, pix)
    yc = (y0 + y1) / 2
    for points in ([(x0, yc), (x1, yc)], [(x0, yc), ((x0 + x1) / 2, yc), (x1, yc)]):      # one segment, and two collinear ones
        table, out_w, out_h = io.curve_table(points, y1 - y0)
        assert (out_w, out_h) == (x1 - x0, y1 - y0) and table.shape == (out_w, 4) and table.dtype == np.float64
        assert np.array_equal(table[:, 0], np.arange(x0, x1) + 0.5) and (table[:, 1] == yc).all()
        assert (table[:, 2] == 0).all() and (table[:, 3] == 1).all()                      # the normal points down
        crop = io.warp_columns(page, table, out_h)
        assert crop.shape == (out_h, out_w, pix) and crop.dtype == np.uint8
        assert np.array_equal(crop[..., :3], page[y0:y1, x0:x1, :3])
        if pix == 4:
            assert (crop[..., 3] == 0).all()                                              # the fourth byte is 0


def test_warp_columns_is_warp_quad_on_a_straight_tilted_line():
    """A straight centre line is a rectangle: the column table samples where the quad's homography does (to rounding), so the two crops
    agree to a grey level."""
    import math
    page = _page(120, 200, 3, seed=3)
    c, s = math.cos(math.radians(17.0)), math.sin(math.radians(17.0))
    p0, p1, T = (30.0, 40.0), (30.0 + 120 * c, 40.0 + 120 * s), 22.0
    table, W, H = io.curve_table([p0, p1], T)
    nx, ny = -s, c
    quad = [(p0[0] - nx * T / 2, p0[1] - ny * T / 2), (p1[0] - nx * T / 2, p1[1] - ny * T / 2), (p1[0] + nx * T / 2, p1[1] + ny * T / 2),
            (p0[0] + nx * T / 2, p0[1] + ny * T / 2)]
    assert io.quad_size(quad) == (W, H) == (120, 22)
    a = io.warp_columns(page, table, H).astype(np.int64)
    b = io.warp_quad(page, io.quad_homography(quad, W, H), W, H).astype(np.int64)
    assert np.abs(a - b).max() <= 1


def _striped_page(W=400, H=220, A=40.0, t=12, gap=36.0):
    """Three dark bands of thickness t, bent by A over W columns, `gap` apart, on white. Returns (page uint8 [H, W, 3], f of the middle band)."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    bend = A * np.sin(np.pi * (xx + 0.5) / W)
    dark = np.zeros((H, W), bool)
    for k in (-1, 0, 1):
        dark |= np.abs(yy + 0.5 - (90.0 + k * gap + bend)) < t / 2.0
    page = np.where(dark, 0, 255).astype(np.uint8)

    def f(x):
        return 90.0 + A * np.sin(np.pi * np.asarray(x, np.float64) / W)
    return np.repeat(page[..., None], 3, 2), f


def test_striped_page_unrolls_into_straight_rows():
    t = 12
    page, f = _striped_page(t=t)
    xs = np.linspace(0.0, 400.0, 17)
    points = np.stack([xs, f(xs)], 1)
    table, out_w, out_h = io.curve_table(points, 2.2 * t)
    crop = io.warp_columns(page, table, out_h)[..., 0].astype(np.int64)
    v = np.arange(out_h) + 0.5 - out_h / 2                             # a row's offset from the centre line
    core, margin = np.abs(v) < t / 2 - 1.5, (np.abs(v) > t / 2 + 1.5) & (np.abs(v) < 1.5 * t - 1.5)
    assert core.sum() >= 8 and margin.sum() >= 4
    print(f"unrolled {out_w} x {out_h}: darkest value on a margin row {crop[margin].min()}, brightest on a core row {crop[core].max()}")
    assert (crop[core] < 64).all()
    assert (crop[margin] > 192).all()
    # the bounding rectangle of the same band has no row that is dark from end to end
    y0, y1 = int(np.floor(f(0.0) - t / 2)), int(np.ceil(f(200.0) + t / 2))
    rect = page[y0:y1, :, 0]
    assert rect.shape[0] >= 40 + t and not (rect < 64).all(axis=1).any()


def test_round_trip_returns_the_centre_line():
    _, f = _striped_page()
    xs = np.linspace(3.0, 390.0, 17)
    points = np.stack([xs, f(xs)], 1)
    T = 26.4
    out_w, out_h, L = io.curve_size(points, T)
    frame = io._curve_frame(points)
    # the vertices themselves: crop points on the centre row at their arc lengths
    crop_pts = np.stack([frame[2] * out_w / L, np.full(len(xs), out_h / 2)], 1)
    assert np.abs(io.curve_to_page(crop_pts, points, T) - points).max() <= 1e-6
    # every column centre of the centre row lands on its table entry; an offset row moves along the normal by that offset
    table, _, _ = io.curve_table(points, T)
    u = np.arange(out_w) + 0.5
    assert np.abs(io.curve_to_page(np.stack([u, np.full(out_w, out_h / 2)], 1), points, T) - table[:, :2]).max() <= 1e-6
    off = io.curve_to_page(np.stack([u, np.full(out_w, out_h / 2 + 5.0)], 1), points, T)
    assert np.abs(off - (table[:, :2] + 5.0 * table[:, 2:])).max() <= 1e-6
    assert np.abs(np.hypot(table[:, 2], table[:, 3]) - 1.0).max() <= 1e-12 and (table[:, 3] > 0).all()
    # the shape of the argument is kept, points beyond the ends continue the end segments
    quad = io.curve_to_page(np.zeros((3, 4, 2)), points, T)
    assert quad.shape == (3, 4, 2)
    before = io.curve_to_page([[-2.0, out_h / 2]], points, T)[0]
    d0 = (points[1] - points[0]) / np.hypot(*(points[1] - points[0]))
    assert np.abs(before - (points[0] - 2.0 * L / out_w * d0)).max() <= 1e-9


def test_sizes_round_half_up_and_are_at_least_one():
    assert io.curve_size([(0, 0), (3, 4)], 2.5)[:2] == (5, 3) and io.curve_size([(0, 0), (0.2, 0)], 0.3)[:2] == (1, 1)
    assert io.curve_size([(0, 0), (10.49, 0)], 7.49)[:2] == (10, 7)
    t, w, h = io.curve_table([(0, 0), (0.2, 0)], 0.3)
    assert t.shape == (1, 4) and io.warp_columns(_page(4, 4), t, h).shape == (1, 1, 3)


def test_every_refusal_of_curve_ok():
    assert io.curve_ok([(0, 0), (1, 0)], 1) and io.curve_ok(np.array([[0.0, 0.0], [5.0, 1.0], [9.0, 3.0]]), 0.5)
    assert io.curve_ok([[0, 0], [1, 1], [0, 0]], 2.0)                   # a curve may return to a point it left
    for bad in ([], [(0, 0)], None, 5, [(0, 0), (1,)], [(0, 0), (1, 2, 3)], [(0, 0), ("a", 1)], [(0, 0), (float("nan"), 1)],
                [(0, 0), (float("inf"), 1)], [(0, 0), (0, 0)], [(0, 0), (1, 1), (1, 1), (2, 2)], [(0, 0), None]):
        assert not io.curve_ok(bad, 3.0), bad
    for bad in (0, -1.0, float("nan"), float("inf"), None, "3", True):
        assert not io.curve_ok([(0, 0), (1, 0)], bad), bad


def test_header_binding_and_descriptor_agree():
    hdr = open(os.path.join(ROOT, "include", "surya_amd.h")).read()
    run = re.search(r"\bint surya_rec_unroll\(([^;]*)\);", hdr)
    assert run
    args = [" ".join(a.split()) for a in run.group(1).split(",")]
    assert args == ["const uint8_t* pages", "const void* descs", "int n", "const double* tables", "uint8_t* out", "int pixel_stride", "int max_w",
                    "int max_h", "void* stream"]
    src = open(os.path.join(ROOT, "surya_amd", "_lib.py")).read()
    assert "lib.surya_rec_unroll.argtypes, lib.surya_rec_unroll.restype = [p, p, i, p, p, i, i, i, p], C.c_int" in src
    kern = open(os.path.join(ROOT, "surya_amd", "csrc", "rec_unroll.h")).read()
    assert "static_assert(sizeof(UnrollDesc) == 40" in kern and "#pragma clang fp contract(off)" in kern and "warp_sample(" in kern
    rect = open(os.path.join(ROOT, "surya_amd", "csrc", "rec_rectify.h")).read()
    assert rect.count("warp_sample(") == 2                              # its definition and rectify_kernel's call: ONE tap body
    model = open(os.path.join(ROOT, "surya_amd", "csrc", "rec_model.hip")).read()
    assert '#include "rec_unroll.h"' in model and "int surya_rec_unroll(" in model
    from surya_amd.recognition.preprocess_gpu import UNROLL_DESC
    assert UNROLL_DESC.itemsize == 40 and list(UNROLL_DESC.names) == ["page_off", "page_w", "page_h", "out_w", "out_h", "out_off", "table_off"]
    assert [UNROLL_DESC.fields[n][1] for n in UNROLL_DESC.names] == [0, 8, 12, 16, 20, 24, 32]


# ------------------------------------------------------------------------------------------------------------- the predictor's side
def test_curve_type_and_its_scaling():
    c = io.Curve([(0, 0), (10, 0), (20, 5)], 8)
    assert c.points == ((0.0, 0.0), (10.0, 0.0), (20.0, 5.0)) and c.thickness == 8.0 and isinstance(c, tuple) and io.curve_ok(*c)
    assert c.scaled(1, 1) is c
    d = c.scaled(2.0, 2.0)
    assert d.points == ((0.0, 0.0), (20.0, 0.0), (40.0, 10.0)) and abs(d.thickness - 16.0) < 1e-12
    e = io.Curve([(0, 5), (10, 5)], 4).scaled(3.0, 0.5)               # a horizontal line: its normal is vertical, the y factor counts
    assert e.points == ((0.0, 2.5), (30.0, 2.5)) and abs(e.thickness - 2.0) < 1e-12


def test_serialised_keys_of_a_text_line_unchanged_while_none():
    from surya_amd.recognition.schema import TextLine
    line = TextLine(text="ab", polygon=[0, 0, 10, 5], chars=[], confidence=0.5)
    assert line.unrolled is None and "unrolled" not in line.model_dump() and "unrolled" not in line.model_dump_json()
    keys = list(line.model_dump())
    line.unrolled = True
    assert [k for k in line.model_dump() if k not in keys] == ["unrolled"] and line.model_dump()["unrolled"] is True
    assert "unrolled" in TextLine.model_json_schema()["properties"]


def test_unrolled_characters_come_back_as_quads_along_the_bend():
    from surya_amd.recognition.assemble import quad_to_page
    _, f = _striped_page()
    xs = np.linspace(0.0, 400.0, 17)
    curve = io.Curve(np.stack([xs, f(xs)], 1), 26.4)
    W, H, L = io.curve_size(*curve)
    # character boxes in crop coordinates: full height, 20 px wide, every 50 px; one hanging over both ends of the crop
    P = np.array([[[u, 0.0], [u + 20.0, 0.0], [u + 20.0, float(H)], [u, float(H)]] for u in (0.0, 50.0, 200.0, 380.0, W - 10.0)], np.float64)
    P[-1, 1:3, 0] = W + 30.0                                            # clamped into the crop
    out = quad_to_page(P.copy(), curve, (1, 1))
    assert out.shape == P.shape and (out == np.trunc(out)).all()
    table, _, _ = io.curve_table(*curve)
    for q in out:                                                       # every corner lies within thickness / 2 (+ 1 px of truncation) of the centre line
        for x, y in q:
            d = np.hypot(table[:, 0] - x, table[:, 1] - y).min()
            assert d <= H / 2 + 1.0 + 0.5, (x, y, d)
    # the quads tilt with the bend: rising at the left end, level in the middle, falling at the right end
    slope = [(q[1, 1] - q[0, 1]) / max(q[1, 0] - q[0, 0], 1.0) for q in out]
    assert slope[0] > 0.15 and abs(slope[2]) < 0.1 and slope[3] < -0.15
    half = quad_to_page(P.copy(), curve, (2.0, 2.0))                    # a high-resolution copy: back on the detected page
    assert np.abs(half - out / 2).max() <= 1.0


def test_predictor_refusals_before_any_device_work():
    from PIL import Image
    from surya_amd.recognition.predictor import RecognitionPredictor, checked_curve
    pred = RecognitionPredictor.__new__(RecognitionPredictor)
    assert pred.unroll is None and pred._unroll_on() is False
    for bad in (False, 1, 0.5, "yes", [True]):
        pred.unroll = bad
        with pytest.raises(ValueError, match="unroll"):
            pred._unroll_on()
    pred.unroll = True
    assert pred._unroll_on() is True
    im = [Image.new("RGB", (64, 32))]
    polys = [[[[0, 0], [10, 0], [10, 5], [0, 5]], [[0, 10], [10, 10], [10, 15], [0, 15]]]]
    good = [[None, ([(0, 12), (5, 13), (10, 12)], 5)]]
    got = pred._checked_centerlines(good, im, polys)
    assert got[0][0] is None and isinstance(got[0][1], io.Curve) and pred._checked_centerlines(None, im, polys) is None
    with pytest.raises(ValueError, match="polygons="):
        pred._checked_centerlines(good, im, None)
    for wrong_shape in ([], [[None]], [[None, None, None]]):
        with pytest.raises(ValueError, match="one entry per polygon"):
            pred._checked_centerlines(wrong_shape, im, polys)
    for bad in (([(0, 12)], 5), ([(0, 12), (0, 12)], 5), ([(0, 12), (5, float("nan"))], 5), ([(0, 12), (5, 13)], 0), ([(0, 12), (5, 13)], -2.0),
                ([(0, 12), (5, 13)],), 7, ([(0, 12), (5, 13)], "5")):
        with pytest.raises(ValueError, match="image 0, line 1"):
            pred._checked_centerlines([[None, bad]], im, polys)
    assert checked_curve("x", None) is None
