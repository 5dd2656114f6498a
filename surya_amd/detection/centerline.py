"""Centre lines of bent text lines from the heat map: the rule, stated once (DetectionPredictor.centerlines; kernels:
csrc/det_centerline.h, bin arithmetic: csrc/det_centerline_core.h).

A. The profile (integers only; device, host build and numpy agree bit for bit). For every component `detect_boxes` keeps (4-connected
   component of heat > low_text with >= 10 pixels and max >= text_threshold, raster order of the first pixel), inclusive bounding box
   x0..x1, y0..y1:
   1. axis = 0 (bins along x, perpendicular coordinate p = y) when x1 - x0 >= y1 - y0, else 1 (bins along y, p = x).
   2. t = the pixel's coordinate along the axis minus the box origin, extent = the box length along the axis (<= 8192).
   3. A pixel of the component falls into bin k = (t * knots) // extent.
   4. Per bin: cnt (uint32) pixels, sum (uint64) of p, lo / hi (int32) = min / max of p; an empty bin holds 0, 0, 0x7fffffff, -1.
B. The curve (`finish`, float64, on the host from one component's integers):
   1. Bin k covers the columns t = ceil(k * extent / knots) .. ceil((k + 1) * extent / knots) - 1. An occupied bin gives the knot
      (origin + mean t of those columns + 0.5, sum / cnt + 0.5) in grid-line coordinates (pixel i covers [i, i + 1)).
   2. The polyline of the knots is extended linearly, from its first two and last two knots, to the box ends x0 and x1 + 1.
   3. Local thickness at a knot = cnt / columns of the bin, times the cosine of the polyline's slope there (the slope between the knot's
      two neighbours on the extended polyline). T = the median of the local thicknesses.
   4. The component is CURVED when the largest distance of a knot from the chord through the polyline's two end points is
      >= min_sag * T and the chord is >= min_length * T long. Fewer than three occupied bins: never. axis = 1: never unless
      `vertical` -- a centre line gives a vertical line's reading direction as top to bottom, which would be a guess.
   5. A curved component's box gets `centerline` = the extended polyline, ordered by increasing axis coordinate, and `thickness` =
      T + int(sqrt(T)): the reference's dilation rule (dilation_of: a (int(sqrt(min(w, h))) + 1)-square) applied to the line's own
      thickness instead of its box. PolygonBox.rescale takes both to page pixels with the factors of the corners.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

MAX_DIM = 8192                  # csrc/det_centerline_core.h CL_MAX_DIM
MIN_KNOTS, MAX_KNOTS = 2, 64    # ... CL_MIN_KNOTS, CL_MAX_KNOTS
EMPTY_LO, EMPTY_HI = 0x7FFFFFFF, -1


@dataclass(frozen=True)
class Centerlines:
    """What `DetectionPredictor.centerlines` takes. knots in 2 .. 64: bins along a line. min_sag, min_length: a line is bent when its
    centre line leaves its chord by min_sag thicknesses and the chord is min_length thicknesses long. vertical: also vertical lines."""
    knots: int = 16
    min_sag: float = 0.35
    min_length: float = 4.0
    vertical: bool = False


def _number(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, float)) and math.isfinite(v)


def check_centerlines(cl) -> Centerlines:
    """The refusals of DetectionPredictor.centerlines, before any device work."""
    if not isinstance(cl, Centerlines):
        raise ValueError(f"DetectionPredictor.centerlines must be None or a Centerlines, got {type(cl).__name__}")
    if isinstance(cl.knots, bool) or not isinstance(cl.knots, int) or not (MIN_KNOTS <= cl.knots <= MAX_KNOTS):
        raise ValueError(f"Centerlines.knots must be an integer in {MIN_KNOTS} .. {MAX_KNOTS}, got {cl.knots!r}")
    if not _number(cl.min_sag) or not cl.min_sag > 0.0:
        raise ValueError(f"Centerlines.min_sag must be a positive number of thicknesses, got {cl.min_sag!r}")
    if not _number(cl.min_length) or not cl.min_length > 0.0:
        raise ValueError(f"Centerlines.min_length must be a positive number of thicknesses, got {cl.min_length!r}")
    if not isinstance(cl.vertical, bool):
        raise ValueError(f"Centerlines.vertical must be a bool, got {cl.vertical!r}")
    return cl


def empty_profile(n: int, knots: int) -> dict:
    return {"cnt": np.zeros((n, knots), np.uint32), "sum": np.zeros((n, knots), np.uint64), "lo": np.full((n, knots), EMPTY_LO, np.int32),
            "hi": np.full((n, knots), EMPTY_HI, np.int32), "axis": np.full(n, -1, np.int32), "box": np.zeros((n, 4), np.int32)}


def profile_page(linemap: np.ndarray, text_threshold: float, low_text: float, knots: int) -> dict:
    """The numpy statement of surya_det_centerlines for one map [H][W]: rule A over scipy.ndimage labels, for the components
    heatmap.detect_boxes keeps, in its order. Returns cnt uint32 [n][knots], sum uint64, lo / hi int32, axis int32 [n] and box int32
    [n][4] = (x0, x1, y0, y1)."""
    from scipy import ndimage

    from .heatmap import get_dynamic_thresholds
    linemap = np.asarray(linemap)
    if linemap.dtype != np.float32:
        linemap = linemap.astype(np.float32)
    assert linemap.ndim == 2 and max(linemap.shape) <= MAX_DIM and MIN_KNOTS <= knots <= MAX_KNOTS
    text_threshold, low_text = get_dynamic_thresholds(linemap, text_threshold, low_text)
    labels, count = ndimage.label(linemap > low_text, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    slices = ndimage.find_objects(labels)
    rows = []
    for k in range(1, count + 1):
        sl = slices[k - 1]
        comp = labels[sl] == k
        if int(comp.sum()) < 10 or np.max(linemap[sl][comp]) < text_threshold:
            continue
        y0, x0 = sl[0].start, sl[1].start
        y1, x1 = sl[0].stop - 1, sl[1].stop - 1
        ys, xs = np.nonzero(comp)
        ys, xs = ys.astype(np.int64) + y0, xs.astype(np.int64) + x0
        axis = 0 if x1 - x0 >= y1 - y0 else 1
        a, p = (xs, ys) if axis == 0 else (ys, xs)
        origin, extent = (x0, x1 - x0 + 1) if axis == 0 else (y0, y1 - y0 + 1)
        b = ((a - origin) * knots) // extent
        cnt = np.bincount(b, minlength=knots)
        sm = np.zeros(knots, np.int64)
        np.add.at(sm, b, p)
        lo, hi = np.full(knots, EMPTY_LO, np.int64), np.full(knots, EMPTY_HI, np.int64)
        np.minimum.at(lo, b, p)
        np.maximum.at(hi, b, p)
        rows.append((cnt, sm, lo, hi, axis, (x0, x1, y0, y1)))
    out = empty_profile(len(rows), knots)
    for i, (cnt, sm, lo, hi, axis, box) in enumerate(rows):
        out["cnt"][i], out["sum"][i], out["lo"][i], out["hi"][i], out["axis"][i], out["box"][i] = cnt, sm.astype(np.uint64), lo, hi, axis, box
    return out


def bin_columns(extent: int, knots: int):
    """(first, last) column t of every bin, int64 [knots] each; last < first for a bin no column falls into (knots > extent)."""
    k = np.arange(knots, dtype=np.int64)
    first = -((-k * extent) // knots)
    last = -((-(k + 1) * extent) // knots) - 1
    return first, last


def finish(cnt, sm, lo, hi, axis, box, cl: Centerlines) -> Optional[Tuple[np.ndarray, float]]:
    """Rule B for one component: (points float64 [m][2] as (x, y) in grid-line coordinates of the map, thickness) when it is curved, else
    None. lo / hi take no part in the rule; they are carried for callers that want the band's envelope."""
    axis = int(axis)
    if axis < 0 or (axis == 1 and not cl.vertical):
        return None
    cnt = np.asarray(cnt).astype(np.float64)
    occ = np.nonzero(cnt > 0)[0]
    if len(occ) < 3:
        return None
    x0, x1, y0, y1 = (int(v) for v in box)
    origin, extent = (x0, x1 - x0 + 1) if axis == 0 else (y0, y1 - y0 + 1)
    first, last = bin_columns(extent, len(cnt))
    cols = (last - first + 1)[occ].astype(np.float64)
    a = origin + 0.5 * (first + last)[occ].astype(np.float64) + 0.5
    p = np.asarray(sm).astype(np.float64)[occ] / cnt[occ] + 0.5
    a_lo, a_hi = float(origin), float(origin + extent)
    p_lo = p[0] + (p[1] - p[0]) / (a[1] - a[0]) * (a_lo - a[0])
    p_hi = p[-1] + (p[-1] - p[-2]) / (a[-1] - a[-2]) * (a_hi - a[-1])
    A, P = np.concatenate([[a_lo], a, [a_hi]]), np.concatenate([[p_lo], p, [p_hi]])
    slope = (P[2:] - P[:-2]) / (A[2:] - A[:-2])
    T = float(np.median(cnt[occ] / cols / np.sqrt(1.0 + slope * slope)))
    da, dp = A[-1] - A[0], P[-1] - P[0]
    chord = math.hypot(da, dp)
    sag = float(np.max(np.abs((a - A[0]) * dp - (p - P[0]) * da)) / chord)
    if not (T > 0.0 and sag >= cl.min_sag * T and chord >= cl.min_length * T):
        return None
    pts = np.stack([A, P], 1) if axis == 0 else np.stack([P, A], 1)
    return pts, T + int(math.sqrt(T))


def attach(boxes, prof: dict, cl: Centerlines) -> int:
    """Rule B over one page: boxes[i] (PolygonBox, still in MAP coordinates, in the profile's order) gets centerline / thickness when its
    component is curved. Returns the number of curved components."""
    n = 0
    for i, bo in enumerate(boxes):
        got = finish(prof["cnt"][i], prof["sum"][i], prof["lo"][i], prof["hi"][i], prof["axis"][i], prof["box"][i], cl)
        if got is not None:
            bo.centerline, bo.thickness = got[0].tolist(), float(got[1])
            n += 1
    return n
