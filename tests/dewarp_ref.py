"""Cases, generators and an independent scalar-loop statement of the page-flattening tests (tests/test_dewarp_cpu.py,
tests/test_gpu_warp_mesh_ops.py, tests/test_gpu_dewarp.py). The rule is surya_amd/common/imageops.py (warp_mesh) and
surya_amd/detection/dewarp.py (fit_mesh); this file states warp_mesh a second time, pixel by pixel in plain Python floats, builds the host
harness of csrc/page_warp_core.h, and plants curled pages whose true field is known."""
import ctypes as C
import functools
import math
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PAGES = [(1, 1), (17, 5), (33, 16), (131, 97)]                 # (W, H)


# ------------------------------------------------------------------------------------------------------------------------ meshes
def mesh_dims(W, H, cell):
    return (H + cell - 1) // cell + 1, (W + cell - 1) // cell + 1


def zero_mesh(W, H, cell):
    return np.zeros(mesh_dims(W, H, cell) + (2,), np.float64)


def shift_mesh(W, H, cell, dx=3.0, dy=-2.0):
    m = zero_mesh(W, H, cell)
    m[..., 0], m[..., 1] = dx, dy
    return m


def random_mesh(W, H, cell, seed):
    """Displacements within +-0.45 cell: neighbouring nodes differ by less than a cell, so the mesh cannot fold."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.45 * cell, 0.45 * cell, mesh_dims(W, H, cell) + (2,))


def off_page_mesh(W, H, cell):
    """Every edge of the output reads beyond the page: the left column of nodes far to the left, the right far to the right, likewise
    top and bottom (a single cell: one corner each)."""
    m = zero_mesh(W, H, cell)
    m[:, 0, 0], m[:, -1, 0] = -(W + 9.25), W + 7.5
    m[0, :, 1], m[-1, :, 1] = -(H + 6.75), H + 11.5
    return m


def huge_mesh(W, H, cell):
    m = zero_mesh(W, H, cell)
    m[..., 0], m[..., 1] = 1e12, -1e12
    m[0, 0] = (-1e12, 1e12)
    return m


def page(W, H, pix, seed=5):
    return np.random.default_rng(seed + W * 131 + H).integers(0, 256, size=(H, W, pix), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------- the rule, one pixel at a time
def _cubic(t, a=-0.75):
    w0 = ((a * (t + 1) - 5 * a) * (t + 1) + 8 * a) * (t + 1) - 4 * a
    w1 = ((a + 2) * t - (a + 3)) * t * t + 1
    w2 = ((a + 2) * (1 - t) - (a + 3)) * (1 - t) * (1 - t) + 1
    return [w0, w1, w2, 1.0 - w0 - w1 - w2]


def _rint(x):
    return round(x)                                             # Python rounds halves to even, as rint does


def scalar_sources(W, H, mesh, cell):
    """(sx, sy) float64 [H, W] by the issue's words, Python floats."""
    sx, sy = np.zeros((H, W)), np.zeros((H, W))
    for v in range(H):
        for u in range(W):
            X, Y = u + 0.5, v + 0.5
            i, j = u // cell, v // cell
            fx, fy = (X - i * cell) / cell, (Y - j * cell) / cell
            d = []
            for c in range(2):
                top = float(mesh[j, i, c]) * (1 - fx) + float(mesh[j, i + 1, c]) * fx
                bot = float(mesh[j + 1, i, c]) * (1 - fx) + float(mesh[j + 1, i + 1, c]) * fx
                d.append(top * (1 - fy) + bot * fy)
            sx[v, u], sy[v, u] = (X + d[0]) - 0.5, (Y + d[1]) - 0.5
    return sx, sy


def scalar_warp_mesh(page_u8, mesh, cell):
    H, W, C_ = page_u8.shape
    sx, sy = scalar_sources(W, H, mesh, cell)
    out = np.zeros((H, W, C_), np.uint8)
    clampi = lambda x, hi: 0 if x < 0 else (hi if x > hi else x)     # noqa: E731
    for v in range(H):
        for u in range(W):
            x, y = float(sx[v, u]), float(sy[v, u])
            fx, fy = math.floor(x), math.floor(y)
            wx, wy = _cubic(x - fx), _cubic(y - fy)
            bx, by = int(min(max(fx, -4.0), W + 4.0)), int(min(max(fy, -4.0), H + 4.0))
            for c in range(3):
                acc = None
                for jj in range(4):
                    row = page_u8[clampi(by - 1 + jj, H - 1)]
                    h = None
                    for k in range(4):
                        p = float(row[clampi(bx - 1 + k, W - 1), c]) * wx[k]
                        h = p if h is None else h + p
                    p = h * wy[jj]
                    acc = p if acc is None else acc + p
                out[v, u, c] = int(min(max(_rint(acc), 0), 255))
    return out


# --------------------------------------------------------------------------------------------------------------- the host build
_host = None


def host_lib():
    """page_warp_core.h compiled for the host (tests/native/page_warp_host.cpp), once per process."""
    global _host
    if _host is None:
        out = os.path.join(tempfile.mkdtemp(prefix="page_warp_host_"), "libpage_warp_host.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", out,
                        os.path.join(ROOT, "tests", "native", "page_warp_host.cpp")], check=True)
        _host = C.CDLL(out)
        _host.page_warp_sources.argtypes = [C.c_int] * 3 + [C.c_void_p] * 3
        _host.page_warp_sources.restype = C.c_int
        _host.page_warp_desc_ok.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        _host.page_warp_desc_ok.restype = C.c_int
        _host.page_warp_desc_bytes.restype = C.c_int
    return _host


def host_sources(W, H, mesh, cell):
    m = np.ascontiguousarray(mesh, np.float64)
    sx, sy = np.zeros((H, W)), np.zeros((H, W))
    assert host_lib().page_warp_sources(W, H, cell, m.ctypes.data, sx.ctypes.data, sy.ctypes.data) == 0
    return sx, sy


def numpy_sources(W, H, mesh, cell):
    """Where imageops.warp_mesh reads the page: its own arithmetic, caught at _sample_cubic."""
    from surya_amd.common import imageops
    seen = {}
    real = imageops._sample_cubic

    def spy(page_u8, sx, sy, w, h):
        seen["s"] = (np.array(sx), np.array(sy))
        return real(page_u8, sx, sy, w, h)
    imageops._sample_cubic = spy
    try:
        imageops.warp_mesh(np.zeros((H, W, 3), np.uint8), mesh, cell)
    finally:
        imageops._sample_cubic = real
    return seen["s"]


# -------------------------------------------------------------------------------------------------------------- planted fields
def field_a(W, H):
    return lambda x, y: 30.0 * np.sin(np.pi * x / W) * (0.6 + 0.4 * y / H)


def field_b(W, H):
    return lambda x, y: 40.0 * np.exp(-x / (0.25 * W)) * (1.0 + 0.3 * y / H)


FIELDS = {"A": (1024, 1024, field_a), "B": (1024, 1400, field_b)}


def planted_lines(W, H, field, tilt=0.0, points=18, x0=0.05, x1=0.95, gap=45.0, first=60.0, margin=70.0):
    """The centre lines of a curled page: flat lines `gap` apart from y = `first`, each displaced by field(x, its flat ordinate) (+ tilt x);
    `points` points per line; every third line ends at 0.55 W (a paragraph's short last line)."""
    lines, y0, k = [], first, 0
    while y0 <= H - margin:
        xs = np.linspace(x0 * W, (0.55 if k % 3 == 2 else x1) * W, points)
        lines.append(np.stack([xs, y0 + field(xs, y0) + tilt * xs], 1))
        y0 += gap
        k += 1
    return lines


def dense(line, field, tilt=0.0, n=400):
    """The TRUE centre line the polyline samples, densely (the flat ordinate is recovered from the first point)."""
    x0, xs = line[0, 0], np.linspace(line[0, 0], line[-1, 0], n)
    # y0 + field(x0, y0) + tilt x0 = line[0, 1] is linear in y0 for both planted fields: two evaluations solve it
    f0, f1 = field(x0, 0.0), field(x0, 1.0)
    y0 = (line[0, 1] - tilt * x0 - f0) / (1.0 + (f1 - f0))
    return np.stack([xs, y0 + field(xs, y0) + tilt * xs], 1)


def line_residual(pts):
    """(largest distance of the points from their own least-squares line, that line's slope)."""
    a, b = np.polyfit(pts[:, 0], pts[:, 1], 1)
    return float(np.abs(pts[:, 1] - (a * pts[:, 0] + b)).max() / math.hypot(1.0, a)), float(a)


def residuals(lines, field, tilt, mesh, cell):
    """Per true centre line (sag before, residual after from_page, slope after)."""
    from surya_amd.common.imageops import mesh_from_page
    out = []
    for ln in lines:
        true = dense(ln, field, tilt)
        before, _ = line_residual(true)
        after, slope = line_residual(mesh_from_page(true, mesh, cell) if mesh is not None else true)
        out.append((before, after, slope))
    return np.array(out)


def bar_map(W, H, lines, field, tilt=0.0, thickness=10):
    """A float32 text map with one bar `thickness` pixels thick along every true centre line (1.0 inside, 0.0 outside)."""
    m = np.zeros((H, W), np.float32)
    for ln in lines:
        true = dense(ln, field, tilt, n=int(ln[-1, 0] - ln[0, 0]) * 2)
        xs = np.arange(int(math.ceil(ln[0, 0])), int(math.floor(ln[-1, 0])))
        yc = np.interp(xs + 0.5, true[:, 0], true[:, 1])
        top = np.rint(yc - thickness / 2.0).astype(np.int64)
        for x, t in zip(xs, top):
            m[max(t, 0): max(t + thickness, 0), x] = 1.0
    return m


@functools.lru_cache(maxsize=None)
def field_b_page():
    """(page uint8 [1400, 1024, 3], mesh at cell 64): the field-B page of the device tests -- dark bars along the planted lines on a
    light, textured ground -- and the mesh fitted from its lines."""
    from surya_amd.detection.dewarp import Dewarp, fit_mesh
    W, H, make = FIELDS["B"]
    f = make(W, H)
    lines = planted_lines(W, H, f)
    rng = np.random.default_rng(77)
    pg = rng.integers(200, 256, size=(H, W, 3), dtype=np.uint8)
    pg[bar_map(W, H, lines, f) > 0] = rng.integers(0, 60, size=3, dtype=np.uint8)
    mesh = fit_mesh(lines, (W, H), Dewarp())
    assert mesh is not None
    pg.setflags(write=False)
    mesh.setflags(write=False)
    return pg, mesh
