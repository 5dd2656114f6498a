"""CPU: the rules of tiled detection (surya_amd/detection/tiling.py) -- grid, seams and ownership as properties over every small axis and
as the worked table, against the plain-numpy statement of tests/det_tile_ref.py; the refusals of DetTiling; a line across three seams
stays one box; the two C entry points as header, binding and descriptor layout state them."""
import os
import re

import numpy as np
import pytest

import det_tile_ref as tr
from surya_amd.detection import heatmap as hm
from surya_amd.detection import tiling as tl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("P", [32, 64])
def test_grid_and_seam_properties(P):
    for overlap in (0, 1, 16, P // 2):
        for M in range(1, 401):
            u = tl.axis_offsets(M, P, overlap)
            sp = tl.axis_spans(M, P, overlap)
            assert u == tr.offsets(M, P, overlap) and sp == tr.spans(M, P, overlap)
            assert all(a < b for a, b in zip(u, u[1:])), (M, overlap, u)                       # distinct and ascending
            assert u[0] == 0 and (u[-1] + P >= M) and all(b <= a + P for a, b in zip(u, u[1:]))      # the tiles cover [0, M)
            assert (len(u) == 1) == (M <= P)
            if len(u) > 1:
                assert u[-1] == M - P                                                          # the last tile ends with the map
                assert all(a + P - b >= overlap for a, b in zip(u, u[1:])), (M, overlap, u)    # neighbours share >= overlap pixels
            assert sp[0][1] == 0 and sp[-1][2] == M and all(a[2] == b[1] for a, b in zip(sp, sp[1:]))    # the spans partition [0, M)
            for off, a, b in sp:
                assert a < b and off <= a and b <= min(off + P, M), (M, overlap, sp)       # a span is not empty and lies inside its tile


def test_the_worked_table():
    cases = [(200, 64, 16, [0, 48, 96, 136], [56, 104, 148]), (65, 64, 16, [0, 1], [32]), (63, 64, 16, [0], []), (64, 64, 16, [0], []),
             (330, 128, 32, [0, 96, 192, 202], [112, 208, 261])]
    for M, P, ov, offs, sm in cases:
        assert tl.axis_offsets(M, P, ov) == offs and tr.offsets(M, P, ov) == offs
        assert tl.axis_seams(offs, M, P) == [0] + sm + [M] and tr.seams(M, P, ov) == sm


def test_page_plan_and_scaled_size():
    assert tl.scaled_size(520, 700, 0.5) == (260, 350) and tl.scaled_size(521, 701, 0.5) == (261, 351) and tl.scaled_size(1, 1, 0.01) == (1, 1)
    pl = tl.page_plan(300, 200, 128, tl.DetTiling(1.0, 32))
    assert pl.map_size == (300, 200) and pl.grid == (3, 2) and pl.n_tiles == 6 and pl.pitch == 300
    assert [t[:2] for t in pl.tiles()] == [(0, 0), (96, 0), (172, 0), (0, 72), (96, 72), (172, 72)]
    assert tl.page_plan(131, 330, 128, tl.DetTiling(1.0, 32)).pitch == 132
    assert tl.page_plan(100, 90, 128, tl.DetTiling(1.0, 32)).tiles() == [(0, 0, (0, 100), (0, 90))]


@pytest.mark.parametrize("shape,P,overlap", [((2, 160, 200), 64, 16), ((1, 65, 131), 64, 0), ((2, 63, 64), 64, 16), ((1, 130, 129), 64, 1),
                                             ((2, 200, 97), 32, 16)])
def test_numpy_stitch_of_numpy_cuts_is_the_map(shape, P, overlap):
    m = np.random.default_rng(5).random(shape, dtype=np.float32)
    tiles = tr.cut_map(m, P, overlap, fill=-1.0)
    out = tr.stitch(tiles, shape[2], shape[1], P, overlap)
    assert out.shape == (shape[0], shape[1], (shape[2] + 3) & ~3)
    assert np.array_equal(out[:, :, : shape[2]], m) and not out[:, :, shape[2]:].any()
    # stitched in two halves into one array == stitched at once; cells of the other half stay as they were
    half = set(range(len(tiles) // 2))
    part = tr.stitch(tiles, shape[2], shape[1], P, overlap, out=np.full_like(out, 7.0), only=half)
    if len(tiles) > 1:
        assert (part == 7.0).any()
    assert np.array_equal(tr.stitch(tiles, shape[2], shape[1], P, overlap, out=part, only=set(range(len(tiles))) - half), out)


def test_numpy_cut_pads_white():
    page = np.random.default_rng(1).integers(0, 255, (70, 90, 3), dtype=np.uint8)
    t = tr.cut_grid(page, 64, 16, 4)
    assert t.shape == (4, 64, 64, 4) and not t[..., 3].any()
    assert np.array_equal(t[3, :, :, :3], page[6:70, 26:90])
    w = tr.cut_window(page, 60, 50, 64, 3)
    assert np.array_equal(w[:20, :30], page[50:, 60:]) and (w[20:] == 255).all() and (w[:, 30:] == 255).all()


def test_refusals():
    for bad in (0.0, -0.5, 1.5, float("nan"), "1", None, True):
        with pytest.raises(ValueError):
            tl.DetTiling(scale=bad)
    for bad in (-1, 1.5, "8", None, True):
        with pytest.raises(ValueError):
            tl.DetTiling(overlap=bad)
    assert tl.DetTiling(scale=1, overlap=0).check(64).overlap == 0
    assert tl.check_tiling(tl.DetTiling(0.25, 32), 64).scale == 0.25
    with pytest.raises(ValueError):
        tl.check_tiling(tl.DetTiling(1.0, 33), 64)
    for bad in ((1.0, 128), {"scale": 1.0}, 1.0, "tile"):
        with pytest.raises(ValueError):
            tl.check_tiling(bad, 1024)


def test_predictor_refuses_before_any_device_work():
    """`tiling` is checked first thing in the call paths: a predictor without a model or a device refuses all the same."""
    from surya_amd.detection.predictor import DetectionPredictor, DetTiling, SegformerImageProcessor
    pred = DetectionPredictor.__new__(DetectionPredictor)
    pred.processor = SegformerImageProcessor({"height": 64, "width": 64})
    assert pred.tiling is None and DetTiling is tl.DetTiling
    for bad in ((1.0, 16), DetTiling(1.0, 33)):
        pred.tiling = bad
        with pytest.raises(ValueError):
            pred._detect([])
        with pytest.raises(ValueError):
            list(pred._iter_detect_device([]))


def test_a_line_across_three_seams_stays_one_box():
    m = tr.bar_map()
    assert m.shape == (160, 200) and tr.seams(200, 64, 16) == [56, 104, 148]
    tiles = tr.cut_map(m[None], 64, 16)
    assert len(tiles) == 4 * 3
    st = tr.stitch(tiles, 200, 160, 64, 16)
    assert np.array_equal(st[0], m)
    boxes, conf = hm.detect_boxes(st[0], 0.6, 0.35)
    assert len(boxes) == 1
    b = np.asarray(boxes[0])
    assert (b.min(0) == (17, 63)).all() and (b.max(0) == (184, 78)).all(), b


def test_header_and_bindings_agree():
    from surya_amd import _lib as L
    from surya_amd.detection.model import CUT_DESC, STITCH_DESC
    hdr = open(os.path.join(ROOT, "include", "surya_amd.h")).read()
    cut = re.search(r"\bint surya_det_cut_tiles_u8\(([^;]*)\);", hdr)
    st = re.search(r"\bint surya_det_stitch_tiles\(([^;]*)\);", hdr)
    assert cut and st
    cut_args = [a.strip() for a in cut.group(1).split(",")]
    st_args = [a.strip() for a in st.group(1).split(",")]
    assert cut_args == ["const void* descs", "int n", "uint8_t* dst", "int n_tiles", "int tile_size", "int dst_pix", "void* stream"]
    assert st_args == ["const float* heat", "int n_tiles", "int labels", "int tile_size", "const void* descs", "int n", "void* stream"]
    if os.path.exists(L.LIB_PATH):
        lib = L.bind_det_tile(L.lib())
        assert len(lib.surya_det_cut_tiles_u8.argtypes) == 7 and len(lib.surya_det_stitch_tiles.argtypes) == 7
    assert CUT_DESC.itemsize == 32 and "32 bytes, C layout" in hdr and STITCH_DESC.itemsize == 64 and "64 bytes, C layout" in hdr
    assert {n: CUT_DESC.fields[n][1] for n in CUT_DESC.names} == {"src": 0, "w": 8, "h": 12, "pix": 16, "x0": 20, "y0": 24, "tile": 28}
    assert {n: STITCH_DESC.fields[n][1] for n in STITCH_DESC.names} == {
        "dst": 0, "pitch": 8, "plane_stride": 16, "tile": 24, "tx0": 28, "ty0": 32, "tw": 36, "th": 40, "dx0": 44, "dy0": 48, "planes": 52,
        "pad_cols": 56, "reserved": 60}
    core = open(os.path.join(ROOT, "surya_amd", "csrc", "det_tile.h")).read()
    assert "sizeof(CutDesc) == 32" in core and "sizeof(StitchDesc) == 64" in core
