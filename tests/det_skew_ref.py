"""Cases and generators of the page-skew tests (tests/test_det_skew_cpu.py, tests/test_gpu_det_skew_ops.py, tests/test_gpu_det_skew.py).
The reference itself is surya_amd/detection/skew.py (plain numpy); this file only makes maps and builds the host harness."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANTS = (-12.0, -3.25, -0.5, 0.0, 0.75, 2.0, 7.5, 14.0)
TEXT, BLANK = 0.9, 0.02
_host = None


def host_lib():
    """det_skew_core.h compiled for the host (tests/native/det_skew_host.cpp), once per process."""
    global _host
    if _host is None:
        out = os.path.join(tempfile.mkdtemp(prefix="det_skew_host_"), "libdet_skew_host.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out, os.path.join(ROOT, "tests", "native", "det_skew_host.cpp")],
                       check=True)
        _host = C.CDLL(out)
        _host.det_skew_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _host.det_skew_host.restype = C.c_int
    return _host


def host_scores(heat, threshold, cs):
    heat = np.ascontiguousarray(heat, np.float32)
    cs = np.ascontiguousarray(cs, np.int32).reshape(-1, 2)
    scores, n = np.zeros(len(cs), np.uint64), C.c_int32(-1)
    rc = host_lib().det_skew_host(heat.ctypes.data, heat.shape[0], heat.shape[1], threshold, cs.ctypes.data, len(cs), scores.ctypes.data,
                                  C.addressof(n))
    assert rc == 0, rc
    return scores, n.value


def band_map(angle, size=256, band=6, pitch=20, seed=0, margin=24):
    """fp32 [size, size] (size: an int, or (H, W)): text bands `band` px high every `pitch` px with ragged right ends, rotated about the
    centre so that the baselines run at `angle` degrees (y down: positive = down to the right). Text is 0.9, the rest 0.02."""
    H, W = (size, size) if isinstance(size, int) else size
    rng = np.random.default_rng(seed)
    t = np.radians(angle)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    u = (x - cx) * np.cos(t) + (y - cy) * np.sin(t) + cx              # the pixel in the upright page
    v = -(x - cx) * np.sin(t) + (y - cy) * np.cos(t) + cy
    line = np.floor(v / pitch).astype(np.int64)
    ends = rng.integers(W // 2, W - margin, size=4 * max(H, W))       # ragged right ends, one per line
    end = ends[np.clip(line + max(H, W), 0, len(ends) - 1)]
    text = ((v - line * pitch) < band) & (u >= margin) & (u < end) & (v >= margin) & (v < H - margin)
    return np.where(text, np.float32(TEXT), np.float32(BLANK)).astype(np.float32)


def random_mask(rng, H, W, density=0.2):
    return np.where(rng.random((H, W)) < density, np.float32(TEXT), np.float32(BLANK)).astype(np.float32)


def corner_map(H, W):
    """Text in the four corners only: the largest and the smallest value of the bin arithmetic."""
    m = np.full((H, W), BLANK, np.float32)
    m[0, 0] = m[0, W - 1] = m[H - 1, 0] = m[H - 1, W - 1] = TEXT
    return m


def random_table(rng, n):
    from surya_amd.detection import skew as sk
    return sk.coeffs(rng.uniform(-45.0, 45.0, n))
