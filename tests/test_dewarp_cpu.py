"""CPU: flattening of curled pages. warp_mesh (surya_amd/common/imageops.py) against an independent scalar-loop statement, EQUAL; the host
build of csrc/page_warp_core.h against numpy, source positions bit-equal, and every descriptor refusal; fit_mesh
(surya_amd/detection/dewarp.py) on planted fields -- the bounds are the issue's: the residual of every true centre line after from_page at
most 1.0 px and at most a tenth of its sag before (2.0 px and an eighth through the detector's host arm); straight skewed lines are left
alone; refusals; the point maps; header, binding and core header against each other."""
import os
import re
import subprocess
import tempfile
import types

import numpy as np
import pytest

import dewarp_ref as R
from surya_amd.common import imageops as io
from surya_amd.detection import dewarp as dw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MESHES = {"zero": lambda W, H, c: R.zero_mesh(W, H, c), "shift": lambda W, H, c: R.shift_mesh(W, H, c),
          "random": lambda W, H, c: R.random_mesh(W, H, c, seed=W + c)}


# ------------------------------------------------------------------------------------------------------------------- warp_mesh
@pytest.mark.parametrize("pix", [3, 4])
@pytest.mark.parametrize("cell", [16, 32])
@pytest.mark.parametrize("size", R.PAGES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_warp_mesh_equals_the_scalar_statement(size, cell, pix):
    W, H = size
    pg = R.page(W, H, pix)
    for name, make in MESHES.items():
        mesh = make(W, H, cell)
        if name == "random":
            io.check_mesh(mesh, cell, (W, H))
        got = io.warp_mesh(pg, mesh, cell)
        assert got.shape == pg.shape and got.dtype == np.uint8
        want = R.scalar_warp_mesh(pg, mesh, cell)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (name, len(bad), bad[:4].tolist())
        if pix == 4:
            assert (got[..., 3] == 0).all()
        if name == "zero":
            assert np.array_equal(got[..., :3], pg[..., :3])
        if name == "shift":                                             # (3, -2): the shifted page, borders replicated
            ys, xs = np.clip(np.arange(H) - 2, 0, H - 1), np.clip(np.arange(W) + 3, 0, W - 1)
            assert np.array_equal(got[..., :3], pg[ys][:, xs][..., :3])


@pytest.mark.parametrize("cell", [16, 32])
@pytest.mark.parametrize("size", R.PAGES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_build_source_positions_are_bit_equal_to_numpy(size, cell):
    W, H = size
    for make in (R.zero_mesh, R.shift_mesh, lambda w, h, c: R.random_mesh(w, h, c, seed=w + c), R.off_page_mesh, R.huge_mesh):
        mesh = make(W, H, cell)
        nx, ny = R.numpy_sources(W, H, mesh, cell)
        hx, hy = R.host_sources(W, H, mesh, cell)
        px, py = R.scalar_sources(W, H, mesh, cell)
        assert np.array_equal(nx.view(np.uint64), hx.view(np.uint64)) and np.array_equal(ny.view(np.uint64), hy.view(np.uint64))
        assert np.array_equal(nx.view(np.uint64), px.view(np.uint64)) and np.array_equal(ny.view(np.uint64), py.view(np.uint64))


def test_every_descriptor_refusal_of_the_host_build():
    from surya_amd.recognition.preprocess_gpu import MESH_DESC
    lib = R.host_lib()
    assert lib.page_warp_desc_bytes() == MESH_DESC.itemsize == 40
    good = np.zeros(1, MESH_DESC)
    good[0] = (8, 100, 50, 32, 0, 16, 4)

    def ok(pix=3, max_w=100, max_h=50, **edit):
        d = good.copy()
        for k, v in edit.items():
            d[k][0] = v
        return lib.page_warp_desc_ok(d.ctypes.data, pix, max_w, max_h)
    assert ok() == 1 and ok(pix=4) == 1
    for cell in range(16, 1025, 16):
        assert ok(cell=cell) == 1
    for edit in ({"w": 0}, {"w": -1}, {"h": 0}, {"w": 101}, {"h": 51}, {"cell": 0}, {"cell": 8}, {"cell": 24}, {"cell": 1040}, {"cell": -16},
                 {"reserved": 1}, {"reserved": -1}, {"page_off": -8}, {"out_off": -4}, {"mesh_off": -2}, {"mesh_off": 5}):
        assert ok(**edit) == 0, edit
    assert ok(max_w=99) == 0 and ok(max_h=49) == 0
    assert ok(page_off=6) == 1 and ok(pix=4, page_off=6) == 0 and ok(out_off=2) == 1 and ok(pix=4, out_off=2) == 0


def test_the_native_program_runs_clean_under_the_host_sanitizers():
    """The stand-alone program (its own main) under -fsanitize=address,undefined; never loaded into Python."""
    out = os.path.join(tempfile.mkdtemp(prefix="page_warp_asan_"), "page_warp_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "native", "page_warp_host.cpp"), "-o", out], check=True)
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


# -------------------------------------------------------------------------------------------------------------------- fit_mesh
@pytest.mark.parametrize("name,tilt", [("A", 0.0), ("B", 0.0), ("A", 0.03)])
def test_fit_mesh_flattens_planted_fields(name, tilt):
    W, H, make = R.FIELDS[name]
    f = make(W, H)
    lines = R.planted_lines(W, H, f, tilt)
    assert len(lines) >= 20 and all(len(ln) == 18 for ln in lines) and lines[2][-1, 0] == 0.55 * W
    mesh = dw.fit_mesh(lines, (W, H), dw.Dewarp(cell=64))
    assert mesh is not None and mesh.shape == io.mesh_shape((W, H), 64) and not mesh[..., 0].any()
    io.check_mesh(mesh, 64, (W, H))
    res = R.residuals(lines, f, tilt, mesh, 64)
    print(f"field {name}, tilt {tilt}: sag before max {res[:, 0].max():.2f} px (min {res[:, 0].min():.2f}); residual after max "
          f"{res[:, 1].max():.3f} px; worst ratio {(res[:, 1] / res[:, 0]).max():.4f}; slopes after {res[:, 2].min():.4f} .. {res[:, 2].max():.4f}")
    assert (res[:, 1] <= 1.0).all()
    assert (res[:, 1] <= res[:, 0] / 10.0).all()
    if tilt:
        # the tilt survives (dewarp composes with straighten): it adds `tilt` to every slope sample, so to their median, so every
        # flattened line runs steeper by `tilt` than the same line of the untilted page
        plain = R.residuals(lines0 := R.planted_lines(W, H, f), f, 0.0, dw.fit_mesh(lines0, (W, H), dw.Dewarp(cell=64)), 64)
        print(f"slope after, tilted minus plain: {(res[:, 2] - plain[:, 2]).min():.5f} .. {(res[:, 2] - plain[:, 2]).max():.5f}")
        assert np.abs(res[:, 2] - plain[:, 2] - tilt).max() <= 0.002


def _skewed_lines(W=1024, H=1024, slope=0.04, n=12):
    return [np.array([[60.0, 80.0 + 70.0 * k + slope * 60.0], [950.0 - 40.0 * (k % 3), 80.0 + 70.0 * k + slope * (950.0 - 40.0 * (k % 3))]])
            for k in range(n)]


def test_straight_skewed_lines_are_left_alone():
    from surya_amd.common.geometry import PolygonBox
    from surya_amd.detection.heatmap import TextDetectionResult
    lines = _skewed_lines()
    mesh = dw.fit_mesh(lines, (1024, 1024), dw.Dewarp())
    assert mesh is not None and np.abs(mesh).max() <= 1e-9
    flat = dw.fit_mesh(lines, (1024, 1024), dw.Dewarp(keep_skew=False))      # without keep_skew the slope is taken out: a shear
    assert flat is not None and np.abs(flat[..., 1]).max() > 10.0
    # through the public call: skewed quads (42 px down over 840) fit a mesh of rounding noise, and the page comes back as the object it was
    boxes = [PolygonBox(polygon=[[60, 80 + 70 * k], [900, 122 + 70 * k], [900, 142 + 70 * k], [60, 100 + 70 * k]]) for k in range(10)]
    r = TextDetectionResult(bboxes=boxes, vertical_lines=[], heatmap=None, affinity_map=None, image_bbox=[0, 0, 1024, 1024])
    pg = R.page(1024, 1024, 3)
    (got,) = dw.dewarp([pg], results=[r])
    assert got.image is pg and got.mesh is None and got.n_lines == 10 and got.max_shift == 0.0 and got.cell == 64
    pts = np.array([[3.5, 7.25], [900.0, -4.0]])
    assert np.array_equal(got.to_page(pts), pts) and np.array_equal(got.from_page(pts), pts)


def test_too_few_lines_and_too_few_intervals_give_none():
    W, H, make = R.FIELDS["A"]
    lines = R.planted_lines(W, H, make(W, H))
    assert dw.fit_mesh(lines[:5], (W, H), dw.Dewarp()) is None and dw.fit_mesh(lines[:6], (W, H), dw.Dewarp()) is not None
    assert dw.fit_mesh(lines[:6], (W, H), dw.Dewarp(min_lines=7)) is None
    assert dw.fit_mesh([], (W, H), dw.Dewarp()) is None
    one_interval = [np.array([[60.0, 50.0 + 30 * k], [130.0, 51.0 + 30 * k]]) for k in range(8)]       # only [64, 128] lies inside
    assert dw.fit_mesh(one_interval, (W, H), dw.Dewarp()) is None
    steep = [np.array([[0.0, 40.0 * k], [1024.0, 40.0 * k + 1228.8 * (k % 2)]]) for k in range(10)]      # every other line beyond max_slope
    assert dw.fit_mesh(steep, (W, H), dw.Dewarp(keep_skew=False)) is None                                # five lines are left
    assert dw.fit_mesh(steep, (W, H), dw.Dewarp(keep_skew=False, min_lines=5)) is not None


def test_shuffled_lines_give_an_equal_mesh():
    W, H, make = R.FIELDS["B"]
    lines = R.planted_lines(W, H, make(W, H))
    want = dw.fit_mesh(lines, (W, H), dw.Dewarp())
    rng = np.random.default_rng(3)
    for _ in range(3):
        order = rng.permutation(len(lines))
        got = dw.fit_mesh([lines[k][::-1] if k % 2 else lines[k] for k in order], (W, H), dw.Dewarp())     # (and right to left)
        assert np.array_equal(got, want)


def test_a_folding_field_gives_none():
    # lines 20 px apart whose slopes alternate between +0.45 and -0.45: integrated over 1024 px neighbouring rows cross many times over
    lines = [np.array([[0.0, 200.0 + 20.0 * k], [1024.0, 200.0 + 20.0 * k + (460.8 if k % 2 else -460.8)]]) for k in range(12)]
    assert dw.fit_mesh(lines, (1024, 1024), dw.Dewarp(keep_skew=False)) is None


def test_page_lines_takes_centre_lines_and_mid_lines_and_ignores_vertical_and_short_ones():
    from surya_amd.common.geometry import PolygonBox, TextBox
    from surya_amd.detection.heatmap import ColumnLine, TextDetectionResult
    bent = TextBox(polygon=[[10, 10], [210, 10], [210, 40], [10, 40]])
    bent.centerline, bent.thickness = [[10.0, 20.0], [110.0, 30.0], [210.0, 20.0]], 12.0
    backwards = TextBox(polygon=[[10, 100], [210, 100], [210, 120], [10, 120]])
    backwards.centerline, backwards.thickness = [[210.0, 110.0], [110.0, 114.0], [10.0, 110.0]], 12.0
    straight = PolygonBox(polygon=[[10, 200], [210, 210], [210, 230], [10, 220]])
    upright = PolygonBox(polygon=[[300, 10], [320, 10], [320, 210], [300, 210]])                # its mid-line runs along x but is 20 long, 200 thick
    turned = PolygonBox(polygon=[[420, 10], [420, 210], [400, 210], [400, 10]])                  # a line read top to bottom: the chord runs along y
    short = PolygonBox(polygon=[[500, 10], [560, 10], [560, 30], [500, 30]])                      # 60 long, 20 thick: below 4 thicknesses
    down = TextBox(polygon=[[600, 10], [640, 10], [640, 300], [600, 300]])
    down.centerline, down.thickness = [[620.0, 10.0], [626.0, 150.0], [620.0, 300.0]], 12.0       # a vertical centre line
    vertical = ColumnLine(polygon=[[700, 0], [720, 0], [720, 900], [700, 900]], vertical=True, horizontal=False)
    r = TextDetectionResult(bboxes=[bent, backwards, straight, upright, turned, short, down], vertical_lines=[vertical], heatmap=None,
                            affinity_map=None, image_bbox=[0, 0, 1024, 1024])
    lines = dw.page_lines(r)
    assert len(lines) == 3
    assert np.array_equal(lines[0], np.array(bent.centerline)) and np.array_equal(lines[1], np.array(backwards.centerline)[::-1])
    assert np.array_equal(lines[2], np.array([[10.0, 210.0], [210.0, 220.0]]))
    assert len(dw.page_lines(r, dw.Dewarp(min_length=2.5))) == 4                                  # the short one is 3 thicknesses long


def test_every_refusal_of_check_dewarp_and_check_mesh():
    ok = dw.check_dewarp(dw.Dewarp())
    assert (ok.cell, ok.min_lines, ok.min_length, ok.max_slope, ok.keep_skew) == (64, 6, 4.0, 0.5, True)
    for bad in (0, 8, 24, 1040, -16, 64.0, "64", None, True):
        with pytest.raises(ValueError, match="cell"):
            dw.check_dewarp(dw.Dewarp(cell=bad))
    for bad in (0, -3, 6.0, "6", None, True):
        with pytest.raises(ValueError, match="min_lines"):
            dw.check_dewarp(dw.Dewarp(min_lines=bad))
    for bad in (0, -0.1, float("nan"), float("inf"), "4", None, True):
        with pytest.raises(ValueError, match="min_length"):
            dw.check_dewarp(dw.Dewarp(min_length=bad))
        with pytest.raises(ValueError, match="max_slope"):
            dw.check_dewarp(dw.Dewarp(max_slope=bad))
    for bad in (0, 1, None, "yes"):
        with pytest.raises(ValueError, match="keep_skew"):
            dw.check_dewarp(dw.Dewarp(keep_skew=bad))
    for bad in (64, {"cell": 64}, "dewarp", None):
        with pytest.raises(ValueError, match="Dewarp"):
            dw.check_dewarp(bad)
        with pytest.raises(ValueError, match="Dewarp"):
            dw.fit_mesh([], (64, 64), bad)
    # check_mesh
    good = R.random_mesh(131, 97, 32, 1)
    assert io.check_mesh(good, 32, (131, 97)) is good and good.shape == (5, 6, 2)
    for cell in (0, 8, 24, 1040, 32.0, None, True):
        with pytest.raises(ValueError, match="cell"):
            io.check_mesh(good, cell, (131, 97))
    for bad in (good.astype(np.float32), good[:-1], good[:, :-1], good[..., :1], good.tolist(), None, np.zeros((5, 6, 2), np.int64)):
        with pytest.raises(ValueError, match="shape"):
            io.check_mesh(bad, 32, (131, 97))
    with pytest.raises(ValueError, match="shape"):
        io.check_mesh(good, 32, (97, 131))
    with pytest.raises(ValueError, match="size"):
        io.check_mesh(good, 32, (0, 97))
    for v in (np.nan, np.inf, -np.inf):
        m = good.copy()
        m[2, 3, 1] = v
        with pytest.raises(ValueError, match="finite"):
            io.check_mesh(m, 32, (131, 97))
    for (j, i, c), v in (((2, 3, 0), 60.0), ((2, 3, 0), -60.0), ((2, 3, 1), 47.0), ((0, 0, 1), 32.0 + good[1, 0, 1])):   # the last: equal, not increasing
        m = good.copy()
        m[j, i, c] = v
        with pytest.raises(ValueError, match="folds"):
            io.check_mesh(m, 32, (131, 97))


def test_dewarp_refuses_bad_calls_before_any_work():
    pg = R.page(33, 16, 3)
    with pytest.raises(ValueError, match="exactly one"):
        dw.dewarp([pg])
    with pytest.raises(ValueError, match="exactly one"):
        dw.dewarp([pg], results=[None], meshes=[None])
    with pytest.raises(ValueError, match="1 images, 2 meshes"):
        dw.dewarp([pg], meshes=[None, None])
    with pytest.raises(ValueError, match="cell"):
        dw.dewarp([pg], meshes=[None], options=dw.Dewarp(cell=20))
    with pytest.raises(ValueError, match="shape"):
        dw.dewarp([pg], meshes=[R.zero_mesh(33, 16, 32)], options=dw.Dewarp(cell=16))
    with pytest.raises(ValueError, match="uint8"):
        dw.dewarp([pg.astype(np.float32)], meshes=[None])


def test_dewarp_host_arm_with_given_meshes():
    from PIL import Image
    W, H, cell = 131, 97, 32
    pg = R.page(W, H, 3)
    mesh = R.random_mesh(W, H, cell, 9)
    im = Image.fromarray(pg)
    rgbx = np.dstack([pg, pg[..., :1]])
    a, b, c, d = dw.dewarp([im, pg, rgbx, im], meshes=[mesh, None, mesh, R.zero_mesh(W, H, cell)], options=dw.Dewarp(cell=cell))
    want = io.warp_mesh(pg, mesh, cell)
    assert np.array_equal(np.asarray(a.image), want) and np.array_equal(np.asarray(c.image), want) and a.image.size == (W, H)
    assert a.mesh is mesh and a.cell == cell and a.n_lines == 0 and a.max_shift == float(np.abs(mesh[..., 1]).max())
    assert b.image is pg and b.mesh is None and d.image is im and d.mesh is None            # None and all zero: untouched, the same objects


# ------------------------------------------------------------------------------------------------------------------ point maps
def test_point_maps_round_trip():
    W, H, make = R.FIELDS["A"]
    mesh = dw.fit_mesh(R.planted_lines(W, H, make(W, H)), (W, H), dw.Dewarp())
    rng = np.random.default_rng(8)
    for m, cell, size in ((mesh, 64, (W, H)), (R.random_mesh(131, 97, 16, 4) * 0.5, 16, (131, 97))):
        io.check_mesh(m, cell, size)
        pts = rng.uniform(-0.1, 1.1, (500, 2)) * np.array(size, np.float64)                    # (beyond the page: the edge cells extrapolate)
        there = io.mesh_to_page(pts, m, cell)
        back = io.mesh_from_page(there, m, cell)
        err = float(np.abs(back - pts).max())
        print(f"cell {cell}: round trip {err:.2e} px, largest displacement {np.abs(there - pts).max():.2f} px")
        assert err <= 1e-6
        assert float(np.abs(io.mesh_to_page(io.mesh_from_page(pts, m, cell), m, cell) - pts).max()) <= 1e-6
    # the maps are the ones warp_mesh samples through: a pixel centre goes where its value was read
    sx, sy = R.numpy_sources(131, 97, m, 16)
    u, v = np.meshgrid(np.arange(131) + 0.5, np.arange(97) + 0.5)
    assert np.abs(io.mesh_to_page(np.stack([u, v], -1), m, 16) - np.stack([sx + 0.5, sy + 0.5], -1)).max() <= 1e-9
    d = dw.Dewarped(None, m, 16, 0)
    assert np.array_equal(d.to_page(pts), there) and d.to_page(pts.reshape(10, 50, 2)).shape == (10, 50, 2)


# ------------------------------------------------------------------------------------------------- through the detector's host arm
@pytest.mark.parametrize("name", ["A", "B"])
def test_through_the_detectors_host_arm(name):
    from surya_amd.detection import pagepost as pp
    from surya_amd.detection.centerline import Centerlines
    W, H, make = R.FIELDS[name]
    f = make(W, H)
    lines = R.planted_lines(W, H, f)
    heat = R.bar_map(W, H, lines, f, thickness=10)
    extra = pp.CenterlineExtra(types.SimpleNamespace(centerlines=Centerlines()))
    extra.check([])
    result, infos = pp.host_page([extra], heat, None, (W, H), (W, H))
    assert len(result.bboxes) == len(lines) and infos[0]["n_curved"] >= len(lines) // 2
    found = dw.page_lines(result)
    assert len(found) == len(lines)
    mesh = dw.fit_mesh(found, (W, H), dw.Dewarp(cell=64))
    assert mesh is not None
    res = R.residuals(lines, f, 0.0, mesh, 64)
    print(f"field {name} through the host arm: {infos[0]}; sag before max {res[:, 0].max():.2f} px; residual after max {res[:, 1].max():.3f} px; "
          f"worst ratio {(res[:, 1] / res[:, 0]).max():.4f}")
    assert (res[:, 1] <= 2.0).all()
    assert (res[:, 1] <= res[:, 0] / 8.0).all()


# --------------------------------------------------------------------------------------------------------------------- surface
def test_header_bindings_and_core_agree():
    from surya_amd import _lib as L
    from surya_amd.recognition.preprocess_gpu import MESH_DESC
    hdr = open(os.path.join(ROOT, "include", "surya_amd.h")).read()
    run = re.search(r"\bint surya_warp_mesh\(([^;]*)\);", hdr)
    assert run
    args = [" ".join(a.split()) for a in run.group(1).split(",")]
    assert args == ["const uint8_t* pages", "const void* descs", "int n", "const double* meshes", "uint8_t* out", "int pixel_stride", "int max_w",
                    "int max_h", "void* stream"]
    assert "{ int64 page_off; int32 w, h; int32 cell, reserved (0); int64 out_off (bytes into out);" in hdr and "-- 40 bytes, C layout" in hdr
    assert MESH_DESC.names == ("page_off", "w", "h", "cell", "reserved", "out_off", "mesh_off") and MESH_DESC.itemsize == 40
    assert [MESH_DESC.fields[n][1] for n in MESH_DESC.names] == [0, 8, 12, 16, 20, 24, 32]
    src = open(os.path.join(ROOT, "surya_amd", "_lib.py")).read()
    assert "lib.surya_warp_mesh.argtypes, lib.surya_warp_mesh.restype = [p, p, i, p, p, i, i, i, p], C.c_int" in src
    if os.path.exists(L.LIB_PATH):
        assert hasattr(L.lib(), "surya_warp_mesh")
    core = open(os.path.join(ROOT, "surya_amd", "csrc", "page_warp_core.h")).read()
    assert "sizeof(MeshDesc) == 40" in core and f"MESH_MIN_CELL = {io.MESH_MIN_CELL};" in core and f"MESH_MAX_CELL = {io.MESH_MAX_CELL};" in core
    assert re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", core) == ["math.h", "stdint.h"]
    kern = open(os.path.join(ROOT, "surya_amd", "csrc", "page_warp.h")).read()
    assert '#include "page_warp_core.h"' in kern and "mesh_source(" in kern and "warp_sample(" in kern and "fp contract(off)" in kern
    model = open(os.path.join(ROOT, "surya_amd", "csrc", "rec_model.hip")).read()
    assert '#include "page_warp.h"' in model and "int surya_warp_mesh(" in model
