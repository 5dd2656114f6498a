"""Cases, generators, a per-pixel brute-force statement and mutants of the centre-line tests (tests/test_det_centerline_cpu.py,
tests/test_gpu_det_centerline_ops.py, tests/test_gpu_det_centerlines.py). The rule is surya_amd/detection/centerline.py (numpy); this file
states its profile half a second time, pixel by pixel in plain Python, builds the host harness of csrc/det_centerline_core.h and makes maps."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np
from scipy import ndimage

import det_post_ref as P
from surya_amd.detection import centerline as cl
from surya_amd.detection import heatmap as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT_T, LOW_T = P.TEXT, P.LOW
TEXT, BLANK = np.float32(0.9), np.float32(0.02)
# the adversarial pages of det_post_ref the issue names
ADVERSARIAL = ("serpentine_s", "comb_top_s", "comb_bottom_s", "comb_bottom_r", "nested_s", "many_a", "big_a", "big_b", "frame_s")
MUTANTS = ("bin_extent_minus_1", "last_column_dropped", "axis_tie_flipped", "dropped_counted", "lo_hi_swapped")
# (H, W, A, t) of the planted curved bands
BANDS = ((96, 256, 27, 9), (64, 256, 15, 5), (64, 100, 12, 5), (200, 1000, 60, 11))
_host = None


# --------------------------------------------------------------------------------------------------------------------- brute force
def _components(heat, mutant=None):
    """[(pixels [(y, x)] in raster order, kept)] of the 4-connected components of heat > low, raster order of the first pixel."""
    heat = np.asarray(heat, np.float32)
    tt, lt = hm.get_dynamic_thresholds(heat, TEXT_T, LOW_T)
    labels, count = ndimage.label(heat > lt, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    ys, xs = np.nonzero(labels)
    pix = [[] for _ in range(count)]
    for y, x in zip(ys.tolist(), xs.tolist()):
        pix[labels[y, x] - 1].append((y, x))
    out = []
    for pts in pix:
        kept = len(pts) >= 10 and max(heat[y, x] for y, x in pts) >= tt
        out.append((pts, kept or mutant == "dropped_counted"))
    return out


def brute_page(heat, knots, mutant=None) -> dict:
    """Rule A pixel by pixel, in Python integers. mutant: one deliberate mistake (MUTANTS)."""
    comps = [pts for pts, kept in _components(heat, mutant) if kept]
    out = cl.empty_profile(len(comps), knots)
    for i, pts in enumerate(comps):
        x0, x1 = min(x for _, x in pts), max(x for _, x in pts)
        y0, y1 = min(y for y, _ in pts), max(y for y, _ in pts)
        horizontal = (x1 - x0 > y1 - y0) if mutant == "axis_tie_flipped" else (x1 - x0 >= y1 - y0)
        origin, extent = (x0, x1 - x0 + 1) if horizontal else (y0, y1 - y0 + 1)
        cnt, sm, lo, hi = [0] * knots, [0] * knots, [cl.EMPTY_LO] * knots, [cl.EMPTY_HI] * knots
        for y, x in pts:
            t, p = (x - origin, y) if horizontal else (y - origin, x)
            if mutant == "last_column_dropped" and t == extent - 1:
                continue
            k = (t * knots) // (extent - 1) if mutant == "bin_extent_minus_1" and extent > 1 else (t * knots) // extent
            k = min(k, knots - 1)                                      # (only the mutant's last column needs it)
            cnt[k] += 1
            sm[k] += p
            lo[k], hi[k] = min(lo[k], p), max(hi[k], p)
        if mutant == "lo_hi_swapped":
            lo, hi = hi, lo
        out["cnt"][i], out["sum"][i], out["lo"][i], out["hi"][i] = cnt, sm, lo, hi
        out["axis"][i], out["box"][i] = 0 if horizontal else 1, (x0, x1, y0, y1)
    return out


def same(a: dict, b: dict) -> bool:
    return all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]) for k in ("cnt", "sum", "lo", "hi", "axis", "box"))


# ------------------------------------------------------------------------------------------------------------- the kernel's inputs
def workspace_inputs(heat, max_boxes):
    """What surya_det_centerlines reads of a surya_det_boxes workspace, made on the host for one page: (label int32 [H * W] = the root's
    raster index or -1, area int32 [H * W] = at a root its compact index or -1 (other words: poison), comp [max_boxes] of
    det_post_ref.COMP_DT, count = kept components, or -1 when there are more than max_boxes)."""
    heat = np.asarray(heat, np.float32)
    H, W = heat.shape
    label = np.full(H * W, -1, np.int32)
    area = np.full(H * W, 0x5A5A5A5A, np.int32)
    comp = np.zeros(max_boxes, P.COMP_DT)
    n = 0
    comps = _components(heat)
    over = sum(kept for _, kept in comps) > max_boxes
    for pts, kept in comps:
        root = pts[0][0] * W + pts[0][1]
        for y, x in pts:
            label[y * W + x] = root
        if over:
            area[root] = len(pts)                                      # an overflowed page keeps the areas: select never ran
            continue
        area[root] = n if kept else -1
        if kept:
            comp[n] = (min(x for _, x in pts), max(x for _, x in pts), min(y for y, _ in pts), max(y for y, _ in pts), len(pts),
                       max(heat[y, x] for y, x in pts))
            n += 1
    return label, area, comp, (-1 if over else n)


def host_lib():
    """det_centerline_core.h compiled for the host (tests/native/det_centerline_host.cpp), once per process."""
    global _host
    if _host is None:
        out = os.path.join(tempfile.mkdtemp(prefix="det_centerline_host_"), "libdet_centerline_host.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out, os.path.join(ROOT, "tests", "native", "det_centerline_host.cpp")],
                       check=True)
        _host = C.CDLL(out)
        _host.det_centerline_host.argtypes = [C.c_void_p] * 3 + [C.c_int] * 5 + [C.c_void_p] * 5
        _host.det_centerline_host.restype = C.c_int
    return _host


def host_page(heat, knots, max_boxes=None) -> dict:
    """The host build over `workspace_inputs`, trimmed to the page's count (box: from comp)."""
    heat = np.asarray(heat, np.float32)
    H, W = heat.shape
    if max_boxes is None:
        max_boxes = max(1, sum(kept for _, kept in _components(heat)))
    label, area, comp, count = workspace_inputs(heat, max_boxes)
    cnt, sm = np.full((max_boxes, knots), 7, np.uint32), np.full((max_boxes, knots), 7, np.uint64)
    lo, hi, axis = np.full((max_boxes, knots), 7, np.int32), np.full((max_boxes, knots), 7, np.int32), np.full(max_boxes, 7, np.int32)
    rc = host_lib().det_centerline_host(label.ctypes.data, area.ctypes.data, comp.ctypes.data, count, H, W, max_boxes, knots, cnt.ctypes.data,
                                        sm.ctypes.data, lo.ctypes.data, hi.ctypes.data, axis.ctypes.data)
    assert rc == 0, rc
    n = max(count, 0)
    e = cl.empty_profile(max_boxes - n, knots)                         # beyond the count: empty bins, axis -1
    assert np.array_equal(cnt[n:], e["cnt"]) and np.array_equal(sm[n:], e["sum"]) and np.array_equal(lo[n:], e["lo"])
    assert np.array_equal(hi[n:], e["hi"]) and np.array_equal(axis[n:], e["axis"])
    box = np.stack([comp[k][:n].astype(np.int32) for k in ("x0", "x1", "y0", "y1")], 1).reshape(n, 4)
    return {"cnt": cnt[:n], "sum": sm[:n], "lo": lo[:n], "hi": hi[:n], "axis": axis[:n], "box": box}


# ------------------------------------------------------------------------------------------------------------------------- maps
def random_mask(rng, H, W, density=0.5):
    """Blobby random text: a smoothed field thresholded, so that components of every size and both axes occur."""
    f = ndimage.uniform_filter(rng.random((H, W)), size=3, mode="constant")
    return np.where(f > np.quantile(f, 1.0 - density), TEXT, BLANK).astype(np.float32)


def band_map(H, W, A, t, y0=None, tilt_deg=0.0, second_gap=None):
    """fp32 [H][W]: the band |y + 0.5 - f(x + 0.5)| < t / 2, f = y0 + A sin(pi x / W) + tan(tilt) (x - W / 2). second_gap: a second,
    parallel band that far below the first. Returns (map, f)."""
    y0 = (H - A) / 2.0 if y0 is None else y0
    s = np.tan(np.radians(tilt_deg))

    def f(x):
        return y0 + A * np.sin(np.pi * np.asarray(x, np.float64) / W) + s * (np.asarray(x, np.float64) - W / 2.0)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    text = np.abs(yy + 0.5 - f(xx + 0.5)) < t / 2.0
    if second_gap is not None:
        text |= np.abs(yy + 0.5 - f(xx + 0.5) - second_gap) < t / 2.0
    return np.where(text, TEXT, BLANK).astype(np.float32), f


def polyline_at(points, x):
    """y of the piecewise-linear curve `points` [(x, y)] (x increasing) at the abscissae x."""
    pts = np.asarray(points, np.float64)
    return np.interp(x, pts[:, 0], pts[:, 1])


@functools.lru_cache(maxsize=None)
def adversarial(name):
    return P.page(name)


def bent_page(H, W, t=7, pitch=44, A=14.0):
    """fp32 [H][W]: bent bands of thickness t every `pitch` rows (f = y0 + A sin(pi x / W), margins of 10 columns), every third one
    straight. What the predictor tests plant into the detector's page maps."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    text = np.zeros((H, W), bool)
    for k, y0 in enumerate(np.arange(12.0, H - A - t - 4, pitch)):
        f = y0 + (0.0 if k % 3 == 2 else A) * np.sin(np.pi * (xx + 0.5) / W)
        text |= (np.abs(yy + 0.5 - f) < t / 2.0) & (xx >= 10) & (xx < W - 10)
    return np.where(text, TEXT, BLANK).astype(np.float32)
