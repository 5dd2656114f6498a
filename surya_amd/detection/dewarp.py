"""Flattening of curled pages: a warp mesh fitted from text-line centre lines, and the page resampled through it (`dewarp`; the warp:
surya_warp_mesh / imageops.warp_mesh, kernel csrc/page_warp.h). Host, float64, numpy only.

This is the page model of leptonica's dewarp module: the text lines of a flat page run straight, so their centre lines give a vertical
disparity field, and the page is resampled through it. It is the counterpart of `straighten` (detection/skew.py): skew is the part of
the field that is one constant slope, and it is left alone here (keep_skew), so the two compose.

The fit (fit_mesh) is a SLOPE field integrated along x, not a displacement per line. A line's displacement can only be measured against
something -- its own chord, say -- and then two neighbouring lines of different extent (a full line above a short last line of a
paragraph) disagree about the same piece of page by the difference of their chords; a coarse mesh cannot represent a field that jumps
between neighbours. The SLOPE of the text at a place does not depend on which part of the line was detected.

1. Slope samples. For every line and every column interval [i * cell, (i + 1) * cell] inside the line's x-extent:
   (ordinate, slope) = ((y(x_i) + y(x_{i+1})) / 2, (y(x_{i+1}) - y(x_i)) / cell), y(.) the polyline, linear between its points.
2. Base slope. base = the median of all slopes (keep_skew: a page of straight skewed lines is left alone), else 0. Samples with
   |slope - base| > max_slope are dropped.
3. Field per interval. S[j, i] = np.interp(j * cell, ordinates, slopes - base) over the interval's samples sorted by ordinate (held
   constant above the first and below the last); intervals without samples are filled by np.interp across i, per row, held beyond the ends.
4. Refusal. Fewer than min_lines lines that gave a sample, or fewer than two intervals with samples: None.
5. Integration. D[:, 0] = 0, D[:, i + 1] = D[:, i] + cell * S[:, i]; then per row the mean of D at the two nodes of the reference interval
   is subtracted. The reference interval is the one with the most samples (ties: nearest the page centre, then the lower index): there
   the page stays where it is.
6. Inversion. D is indexed by PAGE ordinate: page point (x_i, y_j) belongs at y_j - D. A mesh is indexed by OUTPUT ordinate, so per column
   dy[:, i] = np.interp(y_j, y_j - D[:, i], D[:, i]); a column whose y_j - D is not increasing gives None.
7. dx = 0 everywhere (no horizontal model: foreshortening towards the gutter is out of scope; the mesh and the kernel carry dx already).

The result does not depend on the order of the lines. Accuracy on real scans is unmeasured: no trained checkpoint is here.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from ..common.imageops import check_mesh, mesh_from_page, mesh_shape, mesh_to_page, warp_mesh


@dataclass(frozen=True)
class Dewarp:
    """What `dewarp` and `fit_mesh` take. cell: the mesh cell size, a multiple of 16 in 16 .. 1024. min_lines: the fewest usable lines for a
    fit. min_length: the shortest usable line, in thicknesses. max_slope: the largest slope sample kept (against the base slope).
    keep_skew: leave the page's median slope in place (`straighten` removes that)."""
    cell: int = 64
    min_lines: int = 6
    min_length: float = 4.0
    max_slope: float = 0.5
    keep_skew: bool = True


ZERO_MESH = 1e-9                # px: a mesh with no larger entry moves nothing (`dewarp` returns such a page untouched)


def _number(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, float)) and math.isfinite(v)


def check_dewarp(options) -> Dewarp:
    """The refusals of `dewarp`'s options, before any work."""
    if not isinstance(options, Dewarp):
        raise ValueError(f"dewarp options must be a Dewarp, got {type(options).__name__}")
    if isinstance(options.cell, bool) or not isinstance(options.cell, int) or not 16 <= options.cell <= 1024 or options.cell % 16:
        raise ValueError(f"Dewarp.cell must be a multiple of 16 in 16 .. 1024, got {options.cell!r}")
    if isinstance(options.min_lines, bool) or not isinstance(options.min_lines, int) or options.min_lines < 1:
        raise ValueError(f"Dewarp.min_lines must be an integer >= 1, got {options.min_lines!r}")
    if not _number(options.min_length) or not options.min_length > 0.0:
        raise ValueError(f"Dewarp.min_length must be a positive number of thicknesses, got {options.min_length!r}")
    if not _number(options.max_slope) or not options.max_slope > 0.0:
        raise ValueError(f"Dewarp.max_slope must be a positive number, got {options.max_slope!r}")
    if not isinstance(options.keep_skew, bool):
        raise ValueError(f"Dewarp.keep_skew must be True or False, got {options.keep_skew!r}")
    return options


def page_lines(result, options: Dewarp = Dewarp()) -> List[np.ndarray]:
    """One polyline (float64 [m, 2], running left to right) per usable box of a TextDetectionResult. A TextBox with a `centerline` gives
    that polyline; any other box the mid-line of its quad, (p0 + p3) / 2 -> (p1 + p2) / 2 (straight lines matter: they pin the flat
    part of the page). Usable: the chord runs more along x than along y (one running right to left is reversed), and it is at least
    min_length thicknesses long -- the thickness is TextBox.thickness, or the quad's height (the mean of its two side edges). The
    result's `vertical_lines` are never looked at."""
    options = check_dewarp(options)
    lines = []
    for box in result.bboxes:
        p = np.asarray(box.polygon, np.float64)
        cl, thick = getattr(box, "centerline", None), getattr(box, "thickness", None)
        if cl is not None and len(cl) >= 2:
            pts = np.asarray(cl, np.float64).reshape(-1, 2)
        else:
            pts = np.stack([(p[0] + p[3]) / 2.0, (p[1] + p[2]) / 2.0])
        if cl is None or thick is None:
            thick = 0.5 * (float(np.hypot(*(p[3] - p[0]))) + float(np.hypot(*(p[2] - p[1]))))
        if not np.isfinite(pts).all() or not (math.isfinite(thick) and thick > 0.0):
            continue
        cx, cy = pts[-1] - pts[0]
        if not abs(cx) > abs(cy):
            continue
        if cx < 0:
            pts = pts[::-1]
        if math.hypot(cx, cy) < options.min_length * float(thick):
            continue
        lines.append(np.ascontiguousarray(pts))
    return lines


def _reference_interval(counts: np.ndarray, cell: int, width: int) -> int:
    best = counts.max()
    ties = np.nonzero(counts == best)[0]
    dist = np.abs((ties + 0.5) * cell - 0.5 * width)
    return int(ties[np.argmin(dist)])                                  # (argmin: the first, i.e. the lower index, of equal distances)


def fit_mesh(lines, page_size, options: Dewarp = Dewarp()) -> Optional[np.ndarray]:
    """The mesh (float64, imageops.mesh_shape) of a page of size (W, H) from its text lines' polylines, or None: the module's rule."""
    options = check_dewarp(options)
    W, H = int(page_size[0]), int(page_size[1])
    if W <= 0 or H <= 0:
        raise ValueError(f"fit_mesh: the page size is (W, H) with both positive, got {page_size!r}")
    cell = options.cell
    nj, ni, _ = mesh_shape((W, H), cell)
    gw = ni - 1
    per = [[] for _ in range(gw)]                                       # per interval: (ordinate, slope)
    contributed = []
    for li, line in enumerate(lines):
        P = np.asarray(line, np.float64).reshape(-1, 2)
        if len(P) < 2 or not np.isfinite(P).all():
            continue
        if P[-1, 0] < P[0, 0]:
            P = P[::-1]
        if not (np.diff(P[:, 0]) > 0).all():                            # y(x) is a function only along an x-monotone polyline
            continue
        i0, i1 = int(math.ceil(P[0, 0] / cell)), int(math.floor(P[-1, 0] / cell))
        i0, i1 = max(i0, 0), min(i1, gw)
        if i1 <= i0:
            continue
        y = np.interp(np.arange(i0, i1 + 1, dtype=np.float64) * cell, P[:, 0], P[:, 1])
        for k, i in enumerate(range(i0, i1)):
            per[i].append((0.5 * (y[k] + y[k + 1]), (y[k + 1] - y[k]) / cell, li))
    allv = np.array([s for iv in per for s in iv], np.float64).reshape(-1, 3)
    if len(allv) == 0:
        return None
    base = float(np.median(allv[:, 1])) if options.keep_skew else 0.0
    yj = np.arange(nj, dtype=np.float64) * cell
    S = np.zeros((nj, gw), np.float64)
    counts = np.zeros(gw, np.int64)
    for i, iv in enumerate(per):
        a = np.array(iv, np.float64).reshape(-1, 3)
        a = a[np.abs(a[:, 1] - base) <= options.max_slope]
        counts[i] = len(a)
        if len(a):
            contributed.extend(a[:, 2].astype(np.int64).tolist())
            order = np.lexsort((a[:, 1], a[:, 0]))                      # by ordinate, then by slope: no trace of the lines' order
            S[:, i] = np.interp(yj, a[order, 0], a[order, 1] - base)
    have = np.nonzero(counts > 0)[0]
    if len(set(contributed)) < options.min_lines or len(have) < 2:
        return None
    idx = np.arange(gw, dtype=np.float64)
    for j in range(nj):
        S[j] = np.interp(idx, have.astype(np.float64), S[j, have])
    D = np.zeros((nj, ni), np.float64)
    for i in range(gw):
        D[:, i + 1] = D[:, i] + cell * S[:, i]
    r = _reference_interval(counts, cell, W)
    D = D - (0.5 * (D[:, r] + D[:, r + 1]))[:, None]
    mesh = np.zeros((nj, ni, 2), np.float64)
    for i in range(ni):
        out_y = yj - D[:, i]
        if not (np.diff(out_y) > 0).all():
            return None
        mesh[:, i, 1] = np.interp(yj, out_y, D[:, i])
    try:
        return check_mesh(mesh, cell, (W, H))
    except ValueError:
        return None


class Dewarped:
    """One page of `dewarp`: .image (PIL RGB; the caller's own object for a page left as it is), .mesh (float64, flattened -> page
    displacements, None for a page left as it is), .cell, .n_lines (the polylines the fit saw; 0 with a caller's mesh), .max_shift (the
    largest |dy| of the mesh, 0.0 without one) and the two point maps."""

    def __init__(self, image, mesh, cell: int, n_lines: int):
        self.image, self.mesh, self.cell, self.n_lines = image, mesh, cell, n_lines
        self.max_shift = 0.0 if mesh is None else float(np.abs(mesh[..., 1]).max())

    def to_page(self, points) -> np.ndarray:
        """Points [..., 2] (x, y) of the flattened image -> the page, float64."""
        return np.array(points, np.float64) if self.mesh is None else mesh_to_page(points, self.mesh, self.cell)

    def from_page(self, points) -> np.ndarray:
        """Points [..., 2] (x, y) of the page -> the flattened image, float64 (imageops.mesh_from_page)."""
        return np.array(points, np.float64) if self.mesh is None else mesh_from_page(points, self.mesh, self.cell)


def _size(im):
    return (int(im.shape[1]), int(im.shape[0])) if isinstance(im, np.ndarray) else (int(im.size[0]), int(im.size[1]))


def dewarp(images, results=None, meshes=None, options: Dewarp = Dewarp(), device=None) -> List[Dewarped]:
    """Flatten every curled page. images: PIL images (or uint8 [H, W, 3 | 4] arrays), as `straighten` takes them. Exactly one of
    `results` (a TextDetectionResult per page, best from a call with `DetectionPredictor.centerlines` set: page_lines, then fit_mesh) and
    `meshes` (the caller's own float64 array per page at options.cell, or None; each goes through check_mesh). A page without a mesh --
    the fit refused, None was given -- or whose mesh is all zero (no entry beyond ZERO_MESH = 1e-9 px: a page of straight skewed lines
    fits the rounding noise of its equal slopes) comes back untouched: the SAME object, mesh None, identity maps. The
    output has the page's size and is sampled as imageops.warp_mesh samples (4 x 4 cubic taps, replicate border). device: a torch device
    = the pages go up once and ONE surya_warp_mesh call warps them (uint8-equal to the host rule); None = the host rule. Polygons found
    on a flattened page go back through `to_page`."""
    from PIL import Image
    options = check_dewarp(options)
    images = list(images)
    if (results is None) == (meshes is None):
        raise ValueError("dewarp takes exactly one of results= and meshes=")
    given = list(results if meshes is None else meshes)
    if len(given) != len(images):
        raise ValueError(f"dewarp: {len(images)} images, {len(given)} {'results' if meshes is None else 'meshes'}")
    for im in images:
        if isinstance(im, np.ndarray) and not (im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] in (3, 4)):
            raise ValueError("dewarp: a pixel array is uint8 [H, W, 3 | 4]")
    fitted, n_lines = [], []
    for im, g in zip(images, given):
        if meshes is not None:
            fitted.append(None if g is None else check_mesh(g, options.cell, _size(im)))
            n_lines.append(0)
        else:
            lines = page_lines(g, options)
            fitted.append(fit_mesh(lines, _size(im), options))
            n_lines.append(len(lines))
    todo = [i for i, m in enumerate(fitted) if m is not None and float(np.abs(m).max()) > ZERO_MESH]
    out: List[Optional[Dewarped]] = [Dewarped(im, None, options.cell, n) for im, n in zip(images, n_lines)]
    if not todo:
        return out
    from .skew import _pixels
    px = [_pixels(images[i]) for i in todo]
    ms = [fitted[i] for i in todo]
    if device is None:
        warped = [warp_mesh(p, m, options.cell) for p, m in zip(px, ms)]
    else:
        warped = _dewarp_device(px, ms, options.cell, device)
    for i, wp, m in zip(todo, warped, ms):
        out[i] = Dewarped(Image.fromarray(np.ascontiguousarray(wp[..., :3])), m, options.cell, n_lines[i])
    return out


def _dewarp_device(px, ms, cell, device):
    """One upload, one surya_warp_mesh call (one descriptor per page), one download."""
    import ctypes as C

    import torch

    from .. import _lib as L
    from ..recognition.preprocess_gpu import MESH_DESC
    if not torch.cuda.is_available():
        raise L.SuryaAmdError("dewarp(device=...) needs a GPU (MI355X); device=None runs the host rule")
    lib = L.lib()
    dev = torch.device("cuda:0" if device == "cuda" else device)
    pix = 4 if all(p.shape[2] == 4 for p in px) else 3
    px = [p if p.shape[2] == pix else np.ascontiguousarray(p[..., :3]) for p in px]
    al = lambda n: (n + 255) & ~255                                     # noqa: E731
    off = np.concatenate([[0], np.cumsum([al(p.nbytes) for p in px])]).astype(np.int64)
    mesh_off = np.concatenate([[0], np.cumsum([m.size for m in ms])]).astype(np.int64)      # (every mesh holds an even count of doubles)
    stage = torch.empty(int(off[-1]), dtype=torch.uint8, pin_memory=True)
    sv = stage.numpy()
    for p, o in zip(px, off[:-1]):
        sv[int(o): int(o) + p.nbytes] = p.reshape(-1)
    desc = np.zeros(len(px), MESH_DESC)
    for k, p in enumerate(px):
        desc[k] = (int(off[k]), p.shape[1], p.shape[0], cell, 0, int(off[k]), int(mesh_off[k]))
    torch.cuda.set_device(dev)
    d_pages = stage.to(dev, non_blocking=True)
    d_meshes = torch.from_numpy(np.concatenate([m.reshape(-1) for m in ms])).to(dev)
    d_out = torch.empty(int(off[-1]), dtype=torch.uint8, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L.check(lib.surya_warp_mesh(L.ptr(d_pages), desc.ctypes.data_as(C.c_void_p), C.c_int(len(px)), L.ptr(d_meshes), L.ptr(d_out), C.c_int(pix),
                                C.c_int(max(p.shape[1] for p in px)), C.c_int(max(p.shape[0] for p in px)), stream), "surya_warp_mesh")
    host = d_out.cpu().numpy()
    return [host[int(o): int(o) + p.nbytes].reshape(p.shape) for o, p in zip(off[:-1], px)]
