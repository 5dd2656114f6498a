"""cv2-free image primitives used on the host side of the hot path.

OpenCV is not in this image, so these are numpy restatements of the published algorithms:
  * resize_cubic / resize_lanczos4: separable resampling with OpenCV's geometry (half-pixel centres
    `src = (dst + 0.5) * scale - 0.5`, replicate border, no antialiasing -- what cv2.resize does for
    INTER_CUBIC (Keys a = -0.75) and INTER_LANCZOS4 (8 taps)).
  * fill_convex_poly_mask: even-odd scanline fill of an integer polygon, boundary pixels included
    (cv2.fillPoly convention).
They are NOT pinned against cv2 (absent); the parity boundary of the model path is downstream of them
(image_tiles / pixel_values), and both oracle and HIP path consume the same arrays.
"""
from __future__ import annotations

import math

import numpy as np


def _cubic_weights(t: np.ndarray, a: float = -0.75) -> np.ndarray:
    """Keys cubic kernel weights for taps at offsets -1, 0, 1, 2 given fractional position t in [0, 1)."""
    w = np.empty(t.shape + (4,), np.float64)
    w[..., 0] = ((a * (t + 1) - 5 * a) * (t + 1) + 8 * a) * (t + 1) - 4 * a
    w[..., 1] = ((a + 2) * t - (a + 3)) * t * t + 1
    w[..., 2] = ((a + 2) * (1 - t) - (a + 3)) * (1 - t) * (1 - t) + 1
    w[..., 3] = 1.0 - w[..., 0] - w[..., 1] - w[..., 2]
    return w


def _lanczos4_weights(t: np.ndarray) -> np.ndarray:
    """8-tap Lanczos (a = 4) weights for taps at offsets -3..4, normalised to sum 1 (OpenCV interpolateLanczos4)."""
    offs = np.arange(-3, 5, dtype=np.float64)
    x = t[..., None] - offs                       # distance from each tap to the sample point
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(np.abs(x) < 1e-12, 1.0, np.sinc(x) * np.sinc(x / 4.0))
    w[np.abs(x) >= 4.0] = 0.0
    return w / w.sum(-1, keepdims=True)


def _resample_axis(img: np.ndarray, out_len: int, axis: int, kind: str) -> np.ndarray:
    in_len = img.shape[axis]
    if in_len == out_len:
        return img
    scale = in_len / out_len
    src = (np.arange(out_len, dtype=np.float64) + 0.5) * scale - 0.5
    base = np.floor(src)
    t = src - base
    if kind == "cubic":
        w, first = _cubic_weights(t), -1
    else:
        w, first = _lanczos4_weights(t), -3
    taps = w.shape[-1]
    idx = np.clip(base[:, None].astype(np.int64) + first + np.arange(taps)[None, :], 0, in_len - 1)   # replicate
    moved = np.moveaxis(img, axis, 0).astype(np.float64)
    gathered = moved[idx]                          # [out_len, taps, ...]
    wshape = (out_len, taps) + (1,) * (gathered.ndim - 2)
    out = (gathered * w.reshape(wshape)).sum(1)
    return np.moveaxis(out, 0, axis)


def resize(img: np.ndarray, new_w: int, new_h: int, kind: str) -> np.ndarray:
    """float image [H, W, C] -> [new_h, new_w, C]; kind in {'cubic', 'lanczos4'}; result float32."""
    out = _resample_axis(img, new_w, 1, kind)
    out = _resample_axis(out, new_h, 0, kind)
    return out.astype(np.float32)


def fill_poly_mask(h: int, w: int, pts) -> np.ndarray:
    """uint8 mask [h, w] = 1 inside / on the boundary of the polygon with integer vertices `pts` (x, y)."""
    pts = np.asarray(pts, np.float64)
    n = len(pts)
    mask = np.zeros((h, w), np.uint8)
    if n < 3 or h == 0 or w == 0:
        return mask
    ys = np.arange(h, dtype=np.float64)
    # boundary: rasterise each edge densely
    for i in range(n):
        x0, y0 = pts[i]
        x1, y1 = pts[(i + 1) % n]
        steps = int(max(abs(x1 - x0), abs(y1 - y0))) + 1
        xs = np.rint(np.linspace(x0, x1, steps + 1)).astype(np.int64)
        yy = np.rint(np.linspace(y0, y1, steps + 1)).astype(np.int64)
        ok = (xs >= 0) & (xs < w) & (yy >= 0) & (yy < h)
        mask[yy[ok], xs[ok]] = 1
    # interior: even-odd rule per scanline at pixel centres
    for y in range(h):
        xints = []
        for i in range(n):
            x0, y0 = pts[i]
            x1, y1 = pts[(i + 1) % n]
            if y0 == y1:
                continue
            lo, hi = (y0, y1) if y0 < y1 else (y1, y0)
            if lo <= ys[y] < hi:
                xints.append(x0 + (ys[y] - y0) * (x1 - x0) / (y1 - y0))
        xints.sort()
        for a, b in zip(xints[0::2], xints[1::2]):
            xa, xb = int(np.ceil(a)), int(np.floor(b))
            if xb >= xa:
                mask[y, max(xa, 0): min(xb, w - 1) + 1] = 1
    return mask


# ------------------------------------------------------------------------------------------ quadrilateral rectification
# A rotated text line is a quadrilateral p0..p3, clockwise in image coordinates, whose vertex order is the reading direction: p0 -> p1
# is the top edge, read left to right. Vertex coordinates are grid-line coordinates (pixel i covers [i, i + 1)), the convention under
# which slice_and_pad_poly cuts [min, max). The rule is stated here once; csrc/rec_rectify.h restates warp_quad per pixel.
def quad_size(quad):
    """(W, H) of the upright crop of a quad: the longer of each pair of opposite edges, rounded half up, at least 1."""
    p = [(float(x), float(y)) for x, y in quad]             # (plain float64 arithmetic: this runs several times per line of a call)
    n = lambda a, b: math.sqrt((p[a][0] - p[b][0]) ** 2 + (p[a][1] - p[b][1]) ** 2)
    return max(1, int(max(n(1, 0), n(2, 3)) + 0.5)), max(1, int(max(n(3, 0), n(2, 1)) + 0.5))


def quad_ok(quad) -> bool:
    """Four vertices, strictly convex and clockwise in image coordinates (every cross product of consecutive edges > 0): what can be
    rectified. Three points, a bow-tie, zero area and a counter-clockwise quad cannot."""
    try:
        if len(quad) != 4 or any(len(v) != 2 for v in quad):
            return False
        p = [(float(v[0]), float(v[1])) for v in quad]
    except (TypeError, ValueError):
        return False
    if not all(math.isfinite(c) for v in p for c in v):
        return False
    for i in range(4):
        a, b, c = p[i], p[(i + 1) % 4], p[(i + 2) % 4]
        if not (b[0] - a[0]) * (c[1] - b[1]) - (b[1] - a[1]) * (c[0] - b[0]) > 0:
            return False
    return True


def rectify_threshold(value):
    """A `rectify` setting as a threshold in degrees: None is off, True is 0, a non-negative finite number is itself. ValueError else."""
    if value is None:
        return None
    if value is True:
        return 0.0
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not 0 <= value < float("inf"):
        raise ValueError(f"rectify must be None, True or a non-negative number of degrees, got {value!r}")
    return float(value)


def should_rectify(coords, threshold) -> bool:
    """THE decision whether a line's slice is warped from its polygon (`coords`, as the slices are cut from: page pixels) instead of
    being cut as the polygon's bounding rectangle: rectification is on (`threshold`, degrees, not None), the polygon is a rectifiable
    quad (quad_ok), it is not an axis-aligned rectangle in canonical order (that crop is today's, bit for bit), and its top edge
    p0 -> p1 is tilted by at least the threshold. No orientation is guessed: the vertex order is the reading direction."""
    if threshold is None or coords is None or len(coords) != 4 or not quad_ok(coords):
        return False
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = ((float(c[0]), float(c[1])) for c in coords)
    if y0 == y1 and x1 == x2 and y2 == y3 and x3 == x0 and x0 < x1 and y1 < y2:     # canonical order: p0 is the top-left corner
        return False
    return abs(math.degrees(math.atan2(y1 - y0, x1 - x0))) >= threshold


def quad_homography(quad, W: int, H: int) -> np.ndarray:
    """float64 [9], row-major with h[8] = 1: the projective map that takes the rectangle corners (0,0), (W,0), (W,H), (0,H) to p0..p3."""
    return quad_homographies([quad], [W], [H])[0]


def quad_homographies(quads, Ws, Hs) -> np.ndarray:
    """quad_homography of n quads at once, float64 [n, 9]: the n 8 x 8 systems are built as arrays and solved by one stacked
    numpy.linalg.solve (the same LAPACK solve per system, so a row does not depend on its neighbours)."""
    p = np.asarray(quads, np.float64).reshape(-1, 4, 2)
    n = len(p)
    W, H = np.asarray(Ws, np.float64).reshape(n), np.asarray(Hs, np.float64).reshape(n)
    zero = np.zeros(n)
    u, v = np.stack([zero, W, W, zero], 1), np.stack([zero, zero, H, H], 1)          # [n, 4]: the rectangle corners
    x, y = p[..., 0], p[..., 1]
    A = np.zeros((n, 4, 2, 8), np.float64)
    A[:, :, 0, 0], A[:, :, 0, 1], A[:, :, 0, 2], A[:, :, 0, 6], A[:, :, 0, 7] = u, v, 1.0, -u * x, -v * x
    A[:, :, 1, 3], A[:, :, 1, 4], A[:, :, 1, 5], A[:, :, 1, 6], A[:, :, 1, 7] = u, v, 1.0, -u * y, -v * y
    h = np.linalg.solve(A.reshape(n, 8, 8), p.reshape(n, 8, 1))[..., 0]
    return np.concatenate([h, np.ones((n, 1))], axis=1)


def warp_quad(page_u8: np.ndarray, h9, W: int, H: int) -> np.ndarray:
    """uint8 [H, W, C] (C = the page's pixel stride, 3 or 4): output pixel (u, v) samples the page at the image of (u + 0.5, v + 0.5)
    under h9, minus 0.5 on both axes (half-pixel centres, as every resampler here); 4 x 4 cubic taps (a = -0.75) around floor() of that
    point, tap indices clamped to the page (replicate border); float64 products summed in tap order, the horizontal pass per tap row
    first, then the vertical taps; rint (half to even), clamp to 0..255. With stride 4 the X byte is written as 0."""
    h = np.asarray(h9, np.float64).reshape(9)
    ph, pw, C = page_u8.shape
    U = (np.arange(W, dtype=np.float64) + 0.5)[None, :]
    V = (np.arange(H, dtype=np.float64) + 0.5)[:, None]
    w = h[6] * U + h[7] * V + h[8]
    sx = (h[0] * U + h[1] * V + h[2]) / w - 0.5
    sy = (h[3] * U + h[4] * V + h[5]) / w - 0.5
    return _sample_cubic(page_u8, sx, sy, W, H)


def _sample_cubic(page_u8: np.ndarray, sx: np.ndarray, sy: np.ndarray, W: int, H: int) -> np.ndarray:
    """The sampling half of warp_quad and warp_columns: sx, sy float64 [H, W] = where every output pixel reads the page (pixel-index
    coordinates); taps, sums, rounding as warp_quad says."""
    ph, pw, C = page_u8.shape
    fx, fy = np.floor(sx), np.floor(sy)
    wx, wy = _cubic_weights(sx - fx), _cubic_weights(sy - fy)                  # [H, W, 4]
    # (the base is clamped before it becomes an integer: far outside the page every tap is the border pixel anyway)
    bx = np.clip(fx, -4.0, pw + 4.0).astype(np.int64)
    by = np.clip(fy, -4.0, ph + 4.0).astype(np.int64)
    xi = [np.clip(bx - 1 + k, 0, pw - 1) for k in range(4)]
    yi = [np.clip(by - 1 + k, 0, ph - 1) for k in range(4)]
    acc = None
    for j in range(4):
        hrow = None
        for k in range(4):
            prod = page_u8[yi[j], xi[k], :3].astype(np.float64) * wx[..., k, None]
            hrow = prod if hrow is None else hrow + prod
        prod = hrow * wy[..., j, None]
        acc = prod if acc is None else acc + prod
    out = np.zeros((H, W, C), np.uint8)
    out[..., :3] = np.clip(np.rint(acc), 0.0, 255.0).astype(np.uint8)
    return out


# ------------------------------------------------------------------------------------------------ unrolling along a curve
# A BENT text line is a centre line -- points (x, y) in grid-line coordinates of the page, ordered along the reading direction -- and a
# thickness: the height of the band around the centre line that holds the line. Unrolling samples the band column by column along the
# arc length into an upright crop. The rule is stated here once; csrc/rec_unroll.h restates warp_columns per pixel.
def curve_ok(points, thickness) -> bool:
    """At least two points of two finite numbers each, no segment of zero length, a finite positive thickness: what can be unrolled."""
    try:
        if len(points) < 2 or any(len(v) != 2 for v in points):
            return False
        p = [(float(v[0]), float(v[1])) for v in points]
        t = float(thickness)
    except (TypeError, ValueError):
        return False
    if isinstance(thickness, (bool, str, bytes)) or not all(math.isfinite(c) for v in p for c in v) or not (math.isfinite(t) and t > 0.0):
        return False
    return all(a != b for a, b in zip(p[:-1], p[1:]))


class Curve(tuple):
    """(points, thickness) of a line that is read from its unrolled crop: points a tuple of (x, y) floats in the pixels its slice is cut
    from, thickness a float. A tuple of its own type, so that the places that hold "the quad a line was warped from" can hold it too."""
    __slots__ = ()

    def __new__(cls, points, thickness):
        return super().__new__(cls, (tuple((float(p[0]), float(p[1])) for p in points), float(thickness)))

    points = property(lambda self: self[0])
    thickness = property(lambda self: self[1])

    def scaled(self, sx: float, sy: float) -> "Curve":
        """The curve in an image sx x sy times as large: points by the two factors, the thickness by the median length of the scaled
        unit normals at the vertices (TextBox.rescale's rule)."""
        if sx == 1 and sy == 1:
            return self
        pts = self[0]
        ks = []
        for i in range(len(pts)):
            a, b = pts[max(i - 1, 0)], pts[min(i + 1, len(pts) - 1)]
            tx, ty = b[0] - a[0], b[1] - a[1]
            n = math.hypot(tx, ty)
            if n > 0.0:
                ks.append(math.hypot(-ty / n * sx, tx / n * sy))
        return Curve([(x * sx, y * sy) for x, y in pts], self[1] * (float(np.median(ks)) if ks else 1.0))


def _curve_frame(points):
    """(P [m, 2], segment lengths [m - 1], cumulative arc length [m], unit tangents [m - 1, 2], vertex normals [m, 2]). A segment's normal
    is (-ty, tx): it points DOWN for text read left to right. A vertex normal is the normalised sum of the adjacent segments' normals."""
    P = np.asarray(points, np.float64).reshape(-1, 2)
    seg = np.diff(P, axis=0)
    ln = np.hypot(seg[:, 0], seg[:, 1])
    cum = np.concatenate([[0.0], np.cumsum(ln)])
    tang = seg / ln[:, None]
    nseg = np.stack([-tang[:, 1], tang[:, 0]], 1)
    vn = np.concatenate([nseg[:1], nseg[:-1] + nseg[1:], nseg[-1:]])
    nv = np.hypot(vn[:, 0], vn[:, 1])
    vn = np.where(nv[:, None] > 0.0, vn / np.where(nv > 0.0, nv, 1.0)[:, None], np.concatenate([nseg[:1], nseg[1:], nseg[-1:]]))    # (a hairpin: the next segment's)
    return P, ln, cum, tang, vn


def _curve_at(frame, s):
    """Centre C [n, 2] and unit normal N [n, 2] at arc lengths s [n]: C linear on its segment (the end segments continue beyond the ends),
    N interpolated between the vertex normals (held beyond the ends) and renormalised."""
    P, ln, cum, tang, vn = frame
    s = np.asarray(s, np.float64).reshape(-1)
    i = np.clip(np.searchsorted(cum, s, side="right") - 1, 0, len(ln) - 1)
    d = s - cum[i]
    C = P[i] + d[:, None] * tang[i]
    f = np.clip(d / ln[i], 0.0, 1.0)
    N = vn[i] * (1.0 - f)[:, None] + vn[i + 1] * f[:, None]
    nn = np.hypot(N[:, 0], N[:, 1])
    N = np.where(nn[:, None] > 0.0, N / np.where(nn > 0.0, nn, 1.0)[:, None], vn[i])
    return C, N


def curve_size(points, thickness):
    """(out_w, out_h, L) of the unrolled crop: the arc length and the thickness, rounded half up, at least 1."""
    _, ln, _, _, _ = _curve_frame(points)
    L = float(ln.sum())
    return max(1, int(L + 0.5)), max(1, int(float(thickness) + 0.5)), L


def curve_table(points, thickness):
    """(table float64 [out_w][4] = (Cx, Cy, Nx, Ny) per output column, out_w, out_h): column u sits at arc length
    s = (u + 0.5) * L / out_w."""
    out_w, out_h, L = curve_size(points, thickness)
    C, N = _curve_at(_curve_frame(points), (np.arange(out_w, dtype=np.float64) + 0.5) * L / out_w)
    return np.ascontiguousarray(np.concatenate([C, N], 1)), out_w, out_h


def warp_columns(page_u8: np.ndarray, table, out_h: int) -> np.ndarray:
    """uint8 [out_h, out_w, C]: output pixel (u, v) samples the page at C(u) + (v + 0.5 - out_h / 2) * N(u) - 0.5 per axis; from there
    warp_quad's words exactly (4 x 4 Keys taps around floor, base clamped, tap indices clamped to the page, float64 products summed in
    tap order, the horizontal pass first, rint, clamp; the fourth byte 0 with stride 4)."""
    t = np.asarray(table, np.float64).reshape(-1, 4)
    d = ((np.arange(out_h, dtype=np.float64) + 0.5) - out_h / 2)[:, None]
    sx = t[None, :, 0] + d * t[None, :, 2] - 0.5
    sy = t[None, :, 1] + d * t[None, :, 3] - 0.5
    return _sample_cubic(page_u8, sx, sy, len(t), out_h)


def curve_to_page(P, points, thickness) -> np.ndarray:
    """Points P [..., 2] (float64) of the unrolled crop, in its grid-line coordinates, onto the page: (u, v) -> C(s) + (v - out_h / 2) N(s)
    at the continuous arc length s = u * L / out_w -- the map warp_columns samples through, so a crop pixel's centre lands where its
    value was read."""
    out_w, out_h, L = curve_size(points, thickness)
    P = np.asarray(P, np.float64)
    flat = P.reshape(-1, 2)
    C, N = _curve_at(_curve_frame(points), flat[:, 0] * L / out_w)
    return (C + (flat[:, 1] - out_h / 2)[:, None] * N).reshape(P.shape)


# ------------------------------------------------------------------------------------------------ flattening through a mesh
# A CURLED page is flattened through a warp mesh: a coarse grid of displacements over the OUTPUT, cell x cell pixels per cell. For a page
# of W x H pixels gw = ceil(W / cell), gh = ceil(H / cell); the mesh is float64 [gh + 1, gw + 1, 2], entry (j, i) the displacement (dx, dy)
# at output point (i * cell, j * cell), grid-line coordinates. An output point reads the page at itself plus the displacement, bilinear
# inside a cell. The rule is stated here once; csrc/page_warp_core.h + page_warp.h restate warp_mesh per pixel (detection/dewarp.py fits
# a mesh from text-line centre lines).
MESH_MIN_CELL, MESH_MAX_CELL = 16, 1024          # csrc/page_warp_core.h: a multiple of 16, so that a 16 x 16 output tile lies in one cell


def mesh_shape(size, cell: int):
    """(gh + 1, gw + 1, 2) of the mesh of a page of size (W, H)."""
    return -(-int(size[1]) // cell) + 1, -(-int(size[0]) // cell) + 1, 2


def check_mesh(mesh, cell, size) -> np.ndarray:
    """The refusals of a mesh for a page of size (W, H), by ValueError: `cell` not a multiple of 16 in 16 .. 1024; not a float64 array of
    mesh_shape; non-finite entries; a mesh that FOLDS -- i * cell + dx not strictly increasing along i, or j * cell + dy not strictly
    increasing along j (which is also what makes mesh_from_page converge: a displacement varies by less than a cell per cell)."""
    if isinstance(cell, bool) or not isinstance(cell, (int, np.integer)) or not MESH_MIN_CELL <= cell <= MESH_MAX_CELL or cell % 16:
        raise ValueError(f"mesh cell must be a multiple of 16 in {MESH_MIN_CELL} .. {MESH_MAX_CELL}, got {cell!r}")
    if len(size) != 2 or min(int(size[0]), int(size[1])) <= 0:
        raise ValueError(f"mesh: the page size is (W, H) with both positive, got {size!r}")
    want = mesh_shape(size, int(cell))
    if not isinstance(mesh, np.ndarray) or mesh.dtype != np.float64 or mesh.shape != want:
        raise ValueError(f"mesh: a page of {int(size[0])} x {int(size[1])} at cell {cell} takes a float64 array of shape {want}, got "
                         f"{getattr(mesh, 'dtype', type(mesh).__name__)} {getattr(mesh, 'shape', '')}")
    if not np.isfinite(mesh).all():
        raise ValueError("mesh: non-finite entries")
    gx = np.arange(want[1], dtype=np.float64)[None, :] * cell + mesh[..., 0]
    gy = np.arange(want[0], dtype=np.float64)[:, None] * cell + mesh[..., 1]
    if not (np.diff(gx, axis=1) > 0).all() or not (np.diff(gy, axis=0) > 0).all():
        raise ValueError("mesh: it folds (i * cell + dx must increase strictly along i, j * cell + dy along j)")
    return mesh


def _mesh_bilinear(m: np.ndarray, i, j, fx, fy) -> np.ndarray:
    """THE bilinear form, per component: top = m[j, i] (1 - fx) + m[j, i + 1] fx, bot one row down, d = top (1 - fy) + bot fy."""
    gx, gy = (1.0 - fx)[..., None], (1.0 - fy)[..., None]
    fx, fy = fx[..., None], fy[..., None]
    top = m[j, i] * gx + m[j, i + 1] * fx
    bot = m[j + 1, i] * gx + m[j + 1, i + 1] * fx
    return top * gy + bot * fy


def warp_mesh(page_u8: np.ndarray, mesh, cell: int) -> np.ndarray:
    """uint8 [H, W, C], the page's own size: output pixel (u, v) has X = u + 0.5, Y = v + 0.5, cell i = u // cell, j = v // cell,
    fx = (X - i * cell) / cell, fy likewise, displacement d = _mesh_bilinear, and samples the page at sx = (X + dx) - 0.5,
    sy = (Y + dy) - 0.5 (float64, in this order); from there warp_quad's words exactly (_sample_cubic). The VALUES of the mesh are not
    judged here (check_mesh does that): far outside the page every tap is the border pixel."""
    m = np.asarray(mesh, np.float64)
    H, W, _ = page_u8.shape
    assert m.shape == mesh_shape((W, H), cell), (m.shape, (W, H), cell)
    u, v = np.arange(W, dtype=np.int64)[None, :], np.arange(H, dtype=np.int64)[:, None]
    X, Y = u.astype(np.float64) + 0.5, v.astype(np.float64) + 0.5
    i, j = u // cell, v // cell
    fx = np.broadcast_to((X - (i * cell).astype(np.float64)) / float(cell), (H, W))
    fy = np.broadcast_to((Y - (j * cell).astype(np.float64)) / float(cell), (H, W))
    d = _mesh_bilinear(m, np.broadcast_to(i, (H, W)), np.broadcast_to(j, (H, W)), fx, fy)
    sx = (X + d[..., 0]) - 0.5
    sy = (Y + d[..., 1]) - 0.5
    return _sample_cubic(page_u8, sx, sy, W, H)


def _mesh_disp(points: np.ndarray, m: np.ndarray, cell: int) -> np.ndarray:
    """The displacement at continuous output points [n, 2]: the cell index is floor(x / cell) clamped to the mesh, the fractions are not
    clamped, so points outside the page extrapolate its edge cells."""
    gh, gw = m.shape[0] - 1, m.shape[1] - 1
    i = np.clip(np.floor(points[:, 0] / cell), 0, gw - 1).astype(np.int64)
    j = np.clip(np.floor(points[:, 1] / cell), 0, gh - 1).astype(np.int64)
    fx = (points[:, 0] - (i * cell).astype(np.float64)) / float(cell)
    fy = (points[:, 1] - (j * cell).astype(np.float64)) / float(cell)
    return _mesh_bilinear(m, i, j, fx, fy)


def mesh_to_page(points, mesh, cell: int) -> np.ndarray:
    """Points [..., 2] (x, y) of the flattened output, grid-line coordinates -> the page, float64: p + d(p), the map warp_mesh samples
    through (an output pixel's centre lands where its value was read)."""
    P = np.asarray(points, np.float64)
    flat = P.reshape(-1, 2)
    return (flat + _mesh_disp(flat, np.asarray(mesh, np.float64), cell)).reshape(P.shape)


def mesh_from_page(points, mesh, cell: int) -> np.ndarray:
    """The inverse of mesh_to_page by fixed-point iteration q <- p - d(q) from q = p, until the largest step is below 1e-9, for at most
    50 rounds (a mesh that passes check_mesh contracts)."""
    P = np.asarray(points, np.float64)
    flat = P.reshape(-1, 2)
    m = np.asarray(mesh, np.float64)
    q = flat.copy()
    for _ in range(50):
        nq = flat - _mesh_disp(q, m, cell)
        step = float(np.abs(nq - q).max()) if len(q) else 0.0
        q = nq
        if step < 1e-9:
            break
    return q.reshape(P.shape)


def page_pixels(image) -> np.ndarray:
    """uint8 [H, W, 3 or 4] pixels of a PIL RGB page. Pillow stores RGB as 4 bytes per pixel; np.asarray(image) repacks that to
    3 (~2-3 ms per 1024^2 page under the GIL: 128 pages cost more host time than their detection forward pass). When Pillow can
    export its memory through the Arrow C interface (>= 11.2, single-block images) and pyarrow is present, the page's OWN memory
    is returned as an RGBX view instead -- no copy; the device kernels read either stride."""
    try:
        import pyarrow as pa
        if image.mode == "RGB" and hasattr(image, "__arrow_c_array__"):
            a = pa.array(image)
            v = a.values.to_numpy(zero_copy_only=True)
            if v.dtype == np.uint8 and v.size == image.size[0] * image.size[1] * 4:
                return v.reshape(image.size[1], image.size[0], 4)
    except Exception:                                   # multi-block images, exotic builds: fall through to the copying path
        pass
    return np.ascontiguousarray(np.asarray(image, dtype=np.uint8))


_COPY_POOL = None


def copy_pool():
    """One small thread pool per process for staging copies and page views (thread start-up costs ~0.7 ms each: never per call)."""
    global _COPY_POOL
    if _COPY_POOL is None:
        from concurrent.futures import ThreadPoolExecutor
        import os
        _COPY_POOL = ThreadPoolExecutor(max(1, min(8, os.cpu_count() or 1)), thread_name_prefix="surya-amd-copy")
    return _COPY_POOL


def parallel_copy(dsts, srcs, min_bytes: int = 4 << 20) -> None:
    """dsts[i][...] = srcs[i] for numpy arrays of equal shapes. Pages are 3-8 MB each and a call stages 16-128 of them into pinned
    memory: one memcpy stream moves ~10 GB/s, i.e. 6 ms per 16 RGBX pages at 1024^2 -- as long as the detector's forward pass takes for
    five of them. numpy releases the GIL inside a contiguous copy, so a few threads run them side by side."""
    total = sum(int(s_.nbytes) for s_ in srcs)
    if len(srcs) < 2 or total < min_bytes:
        for d, s_ in zip(dsts, srcs):
            d[...] = s_
        return

    def one(i):
        dsts[i][...] = srcs[i]

    list(copy_pool().map(one, range(len(srcs))))



# --------------------------------------------------------------------------------------------------- contrast adjustment
# Pillow's ImageOps.autocontrast(crop, cutoff, preserve_tone=True, mask) restated in numpy, byte for byte (tests/test_reread_cpu.py
# holds it to Pillow's own function); csrc/adjust_core.h + rec_adjust.h restate it once more for the device.
def autocontrast_bounds(hist, cutoff: int):
    """(lo, hi) of a 256-bin histogram: `cutoff` percent of the counts removed from the low end, then from the high end of what is
    left, then the first and the last bin that still holds something (255, 0 for an empty histogram)."""
    h = [int(v) for v in hist]
    n = sum(h)
    for rng in (range(256), range(255, -1, -1)):
        cut = n * int(cutoff) // 100
        for i in rng:
            if cut <= 0:
                break
            take = min(cut, h[i])
            h[i] -= take
            cut -= take
    lo = next((i for i in range(256) if h[i]), 255)
    hi = next((i for i in range(255, -1, -1) if h[i]), 0)
    return lo, hi


def autocontrast_lut(lo: int, hi: int) -> np.ndarray:
    """The 256-entry uint8 table for bounds (lo, hi): the identity when hi <= lo, else int(i * scale + offset) clamped to 0..255 with
    scale = 255.0 / (hi - lo), offset = -lo * scale in float64 (for (0, 25) lut[25] is 254, as in Pillow)."""
    if hi <= lo:
        return np.arange(256, dtype=np.uint8)
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return np.clip((np.arange(256, dtype=np.float64) * scale + offset).astype(np.int64), 0, 255).astype(np.uint8)


def autocontrast_crop(crop_u8: np.ndarray, mask, cutoff: int, with_bounds: bool = False):
    """The contrast-adjusted copy of a padded uint8 crop [h, w, 3]: the histogram of the luma (Pillow's convert("L")) over the pixels
    `mask` keeps ([h, w], non-zero = counted; None = all), autocontrast_bounds, autocontrast_lut, the table applied to every channel
    of every pixel, the pad included. `cutoff` is an integer percent in 0..49."""
    if isinstance(cutoff, bool) or not isinstance(cutoff, (int, np.integer)) or not 0 <= cutoff <= 49:
        raise ValueError(f"cutoff must be an integer percent in 0..49, got {cutoff!r}")
    crop_u8 = np.asarray(crop_u8)
    if crop_u8.dtype != np.uint8 or crop_u8.ndim != 3 or crop_u8.shape[2] != 3:
        raise ValueError("autocontrast_crop takes a uint8 [h, w, 3] crop")
    c = crop_u8.astype(np.int64)
    luma = (19595 * c[..., 0] + 38470 * c[..., 1] + 7471 * c[..., 2] + 32768) >> 16
    if mask is not None:
        luma = luma[np.asarray(mask) != 0]
    lo, hi = autocontrast_bounds(np.bincount(luma.reshape(-1), minlength=256), int(cutoff))
    out = autocontrast_lut(lo, hi)[crop_u8]
    return (out, (lo, hi)) if with_bounds else out
