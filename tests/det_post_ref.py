"""Test infrastructure: the heat-map -> boxes kernels (csrc/det_post.h, surya_det_boxes) one stage at a time: adversarial cases, a staged
reference of everything ONE call leaves in the caller's workspace, and the mutants that reference must tell apart. Built like
gemm_ops_ref.py / attn_ops_ref.py; here nothing rounds except the threshold formula, so every bound is "equal".

reference(case, mutant=None) -> per call, per page, a dict in plain numpy / scipy (integers, float64, math.fsum):
    thresholds   k = int(N * 0.9); `prefix` = bits of the value at ascending rank k; `rank` = what is left of k inside the last radix bin
                 (k - #{v < v_k}); cnt_gt = #{v > v_k}; sum_gt = fsum of those; avg = float32((sum_gt + (N - k - cnt_gt) v_k) / (N - k)), the
                 product exact in float64 (24 + 21 bits); text_thr / low_thr by thr_formula(): post_thresholds_kernel's float32 operations
                 (division, clip, sqrt, product, clip -- each correctly rounded, so numpy float32 gives the same bits)
    labels       -1 or the smallest raster index of the pixel's 4-connected component of heat > low_thr (scipy.ndimage.label, then min index)
    statistics   at every root: area, bounding box, bits of the max value
    selection    kept roots (area >= 10, max >= text_thr) in raster order; area_final (compact index / -1 at every root); the CompStats
                 rows; dilated rows and their exclusive prefix (rowoff); n_sel, n_rows, max_conf, overflow; blk = exclusive (count, rows)
                 prefix per 4096-pixel scan block
    row extremes rmin / rmax, n_rows entries: a kept component's slice holds its source rows' leftmost / rightmost pixel first, then
                 (0x7fffffff, -1) for the rows only the dilation adds (post_scatter_kernel's fill)
    boxes, conf  from the stages above: dilated row extremes -> heatmap.min_area_rect_points -> detect_boxes' own tail. They are NOT taken
                 from heatmap.detect_boxes; tests/test_det_post_stages_cpu.py holds them equal to it and to the native harness.
A page that overflows max_boxes keeps the raw areas (post_scatter_kernel returns first) and has no component table, rows or boxes.

Cases: background 1/16 and foreground 3/4 unless a family needs other values, so whatever the dynamic thresholds come to (low in [0.1, 0.35],
text <= 0.6) the mask is the drawn one and the top-10 % mean is an exact dyadic sum. Pages with other values are listed in NON_DYADIC; the ones
that are drawn from a generator are redrawn (seed by seed, _draw) until numpy's float32 pairwise mean gives the exact mean's thresholds.

MUTANTS are deliberately wrong evaluations of the reference; each case lists the ones it kills (`kills`), and
tests/test_det_post_stages_cpu.py holds every mutant to at least one case. Not a conftest; never imported by the product."""
from __future__ import annotations

import ctypes as C
import functools
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
from scipy import ndimage

from surya_amd.detection import heatmap as hm

F = np.float32
BG, FG = F(1 / 16), F(3 / 4)
TEXT, LOW = 0.6, 0.35                     # settings.DETECTOR_TEXT_THRESHOLD / DETECTOR_BLANK_THRESHOLD
SCAN_PIX = 4096                           # det_post.h SCAN_PIX
IMAX = 0x7FFFFFFF
SENT = F(-7.0)                            # boxes / conf before a call
SENT_COUNT = -77                          # count before a call
WS_FILL = 0xA5                            # every workspace byte before a call
POST_SMALL_ROWS, POST_LDS_ROWS = 255, 2555

# order of surya_det_boxes_workspace_layout's offsets (include/surya_amd.h)
LAYOUT_WORDS = ("st", "hist", "psum", "pcnt", "label", "area", "minx", "maxx", "miny", "maxy", "maxv", "blk", "comp", "rowoff", "rmin", "rmax",
                "big", "big_stride", "total", "sizeof_page_state", "sizeof_comp_stats")

MUTANTS = ("row_wrap", "conn8", "low_ge", "text_gt", "area9", "root_max", "order_top", "rank_off", "ties_above", "dil_swap", "carry_dropped",
           "rows_not_reset")


class PageState(C.Structure):             # det_post.h PageState
    _fields_ = [("rank", C.c_uint32), ("prefix", C.c_uint32), ("cnt_gt", C.c_uint32), ("n_sel", C.c_int32), ("n_rows", C.c_int32),
                ("overflow", C.c_int32), ("text_thr", C.c_float), ("low_thr", C.c_float), ("max_conf", C.c_float), ("pad_", C.c_float),
                ("sum_gt", C.c_double)]


class CompStats(C.Structure):             # det_post_core.h CompStats
    _fields_ = [("x0", C.c_int32), ("x1", C.c_int32), ("y0", C.c_int32), ("y1", C.c_int32), ("area", C.c_int32), ("maxv", C.c_float)]


PAGE_STATE_DT = np.dtype([("rank", "<u4"), ("prefix", "<u4"), ("cnt_gt", "<u4"), ("n_sel", "<i4"), ("n_rows", "<i4"), ("overflow", "<i4"),
                          ("text_thr", "<f4"), ("low_thr", "<f4"), ("max_conf", "<f4"), ("pad_", "<f4"), ("sum_gt", "<f8")])
COMP_DT = np.dtype([("x0", "<i4"), ("x1", "<i4"), ("y0", "<i4"), ("y1", "<i4"), ("area", "<i4"), ("maxv", "<f4")])


def workspace_layout(lib, B, H, W, max_boxes) -> Dict[str, int]:
    """surya_det_boxes_workspace_layout as a dict (LAYOUT_WORDS + n_blk + row_cap); the struct mirrors above must have the library's sizes."""
    off = (C.c_size_t * len(LAYOUT_WORDS))()
    n_blk, row_cap = C.c_int(0), C.c_int(0)
    rc = lib.surya_det_boxes_workspace_layout(B, H, W, max_boxes, off, len(LAYOUT_WORDS), C.byref(n_blk), C.byref(row_cap))
    assert rc == 0, rc
    L = {n: int(v) for n, v in zip(LAYOUT_WORDS, off)}
    L["n_blk"], L["row_cap"] = n_blk.value, row_cap.value
    assert L["sizeof_page_state"] == C.sizeof(PageState) == PAGE_STATE_DT.itemsize, L["sizeof_page_state"]
    assert L["sizeof_comp_stats"] == C.sizeof(CompStats) == COMP_DT.itemsize, L["sizeof_comp_stats"]
    return L


def bits(v) -> np.ndarray:
    return np.asarray(v, F).view(np.uint32)


def f32_step(v) -> float:
    """Distance from float32 v to its neighbours (the larger one)."""
    v = F(v)
    return float(max(np.nextafter(v, F(np.inf)) - v, v - np.nextafter(v, F(-np.inf))))


# ------------------------------------------------------------------------------------------------------------------ reference
def thr_formula(avg, text=TEXT, low=LOW) -> Tuple[np.float32, np.float32]:
    """post_thresholds_kernel from `avg` on, float32 operation by float32 operation."""
    sc = F(avg) / F(0.7)
    sc = min(max(sc, F(0)), F(1))
    sc = np.sqrt(F(sc))
    tt = min(max(F(text) * sc, F(0.15)), F(0.8))
    lt = min(max(F(low) * sc, F(0.1)), F(0.6))
    return F(tt), F(lt)


def _thresholds(heat, mutant):
    flat = heat.ravel()
    N = flat.size
    k = int(N * 0.9)
    kk = k + 1 if mutant == "rank_off" else k
    vk = np.partition(flat, kk)[kk]
    above = flat >= vk if mutant == "ties_above" else flat > vk
    cnt = int(above.sum())
    vals = flat[above].astype(np.float64)
    sum_gt = math.fsum(vals)
    exact = math.fsum(list(vals) + [(N - k - cnt) * float(vk)])          # the product is exact in float64
    avg = F(exact / (N - k))
    tt, lt = thr_formula(avg)
    return dict(k=k, rank=kk - int((flat < vk).sum()), prefix=int(bits(vk)), cnt_gt=cnt, sum_gt=sum_gt, avg=avg, text_thr=tt, low_thr=lt)


def _labels(mask, mutant):
    """int32 [N]: -1 or the component's root (smallest raster index; the largest under root_max)."""
    H, W = mask.shape
    st = np.ones((3, 3), int) if mutant == "conn8" else [[0, 1, 0], [1, 1, 1], [0, 1, 0]]
    lab, n = ndimage.label(mask, structure=st)
    lab = lab.ravel()
    parent = np.arange(n + 1)
    if mutant == "row_wrap":                       # a run ending at x = W - 1 continues at x = 0 of the next row
        def find(a):
            while parent[a] != a:
                a = parent[a]
            return a
        for y in range(H - 1):
            a, b = lab[y * W + W - 1], lab[(y + 1) * W]
            if a and b:
                ra, rb = find(a), find(b)
                parent[max(ra, rb)] = min(ra, rb)
        for a in range(1, n + 1):
            parent[a] = find(a)
    idx = np.flatnonzero(lab)
    ids = parent[lab[idx]]
    if mutant == "root_max":
        root_of = np.full(n + 1, -1, np.int64)
        np.maximum.at(root_of, ids, idx)
    else:
        root_of = np.full(n + 1, IMAX, np.int64)
        np.minimum.at(root_of, ids, idx)
    out = np.full(H * W, -1, np.int32)
    out[idx] = root_of[ids]
    return out


def _dilation(x0, x1, y0, y1, H, mutant):
    k = math.isqrt(min(x1 - x0 + 1, y1 - y0 + 1)) + 1         # int(np.sqrt(min(w, h))) + 1
    hi = k // 2
    lo = k - 1 - hi
    if mutant == "dil_swap":
        lo, hi = hi, lo
    return lo, hi, max(0, y0 - lo), min(H - 1, y1 + hi)


def _box_from_rows(Ls, Rs, Y0, Y1):
    """min_area_rect_points of the dilated row extremes, then detect_boxes' tail (heatmap.py, the lines after min_area_rect_points)."""
    ys = np.arange(Y0, Y1 + 1)
    ext = np.concatenate([np.column_stack((Ls, ys)), np.column_stack((Rs, ys))])
    hull_m = len(hm._convex_hull(ext.astype(np.float64)))
    box = hm.min_area_rect_points(ext)
    bw, bh = np.linalg.norm(box[0] - box[1]), np.linalg.norm(box[1] - box[2])
    if abs(1 - max(bw, bh) / (min(bw, bh) + 1e-5)) <= 0.1:
        l, r, t, b = Ls.min(), Rs.max(), Y0, Y1
        box = np.array([[l, t], [r, t], [r, b], [l, b]], dtype=np.float32)
    c = box.mean(0)
    ang = np.arctan2(box[:, 1] - c[1], box[:, 0] - c[0])
    box = box[np.argsort(ang)]
    box = np.roll(box, -int(box.sum(axis=1).argmin()), 0)
    return box.astype(np.float32), hull_m


def ref_page(heat: np.ndarray, max_boxes: int, mutant: Optional[str] = None) -> dict:
    H, W = heat.shape
    N = H * W
    r = _thresholds(heat, mutant)
    mask = heat >= r["low_thr"] if mutant == "low_ge" else heat > r["low_thr"]
    label = _labels(mask, mutant)
    fg = np.flatnonzero(label >= 0)
    roots, inv = np.unique(label[fg], return_inverse=True)
    n = len(roots)
    xs, ys, vals = fg % W, fg // W, heat.ravel()[fg]
    area = np.bincount(inv, minlength=n).astype(np.int32)
    minx, miny = np.full(n, IMAX, np.int32), np.full(n, IMAX, np.int32)
    maxx, maxy = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    maxv = np.zeros(n, F)
    np.minimum.at(minx, inv, xs); np.maximum.at(maxx, inv, xs)
    np.minimum.at(miny, inv, ys); np.maximum.at(maxy, inv, ys)
    np.maximum.at(maxv, inv, vals)
    r.update(label=label, roots=roots.astype(np.int32), area=area, minx=minx, maxx=maxx, miny=miny, maxy=maxy, maxv=bits(maxv).copy())
    # selection, raster order of the roots
    keep = area >= (9 if mutant == "area9" else 10)
    keep &= (maxv > r["text_thr"]) if mutant == "text_gt" else (maxv >= r["text_thr"])
    kept = np.flatnonzero(keep)
    if mutant == "order_top":                      # cv2 labels by the first pixel in raster order, not by the bounding box
        kept = kept[np.lexsort((minx[kept], miny[kept]))]
    n_sel = len(kept)
    dil = [_dilation(minx[c], maxx[c], miny[c], maxy[c], H, mutant) for c in kept]
    rows = np.array([d[3] - d[2] + 1 for d in dil], np.int32).reshape(-1)
    rowoff = (np.cumsum(rows) - rows).astype(np.int32)
    n_rows = int(rows.sum())
    n_blk = (N + SCAN_PIX - 1) // SCAN_PIX
    blk = np.zeros((n_blk, 2), np.int64)
    np.add.at(blk[:, 0], roots[kept] // SCAN_PIX, 1)
    np.add.at(blk[:, 1], roots[kept] // SCAN_PIX, rows)
    blk = np.cumsum(blk, 0) - blk
    if mutant == "carry_dropped" and n_blk > 256:  # post_scan_kernel's second round of 256 blocks starts from zero
        blk[256:] -= blk[256].copy()
    overflow = int(n_sel > max_boxes or n_rows > min(N, 1 << 30))
    r.update(n_sel=n_sel, n_rows=n_rows, overflow=overflow, blk=blk.astype(np.int32), kept=roots[kept].astype(np.int32))
    area_final = area.copy()
    comp = np.zeros(n_sel, COMP_DT)
    rmin, rmax = np.full(n_rows, IMAX, np.int32), np.full(n_rows, -1, np.int32)
    boxes, conf, hull_m = np.zeros((0, 4, 2), F), np.zeros(0, F), []
    max_conf = F(0)
    if not overflow:
        area_final[:] = -1
        area_final[kept] = np.arange(n_sel)
        for f, src in (("x0", minx), ("x1", maxx), ("y0", miny), ("y1", maxy), ("area", area), ("maxv", maxv)):
            comp[f] = src[kept]
        max_conf = F(maxv[kept].max()) if n_sel else F(0)
        ci = area_final[inv]                       # compact index of every foreground pixel's component
        on = ci >= 0
        pos = rowoff[ci[on]] + ys[on] - miny[kept][ci[on]]
        np.minimum.at(rmin, pos, xs[on].astype(np.int32))
        np.maximum.at(rmax, pos, xs[on].astype(np.int32))
        bl = []
        for j, c in enumerate(kept):
            lo, hi, Y0, Y1 = dil[j]
            h = maxy[c] - miny[c] + 1
            smin, smax = rmin[rowoff[j]: rowoff[j] + h].astype(np.int64), rmax[rowoff[j]: rowoff[j] + h].astype(np.int64)
            Ls, Rs = np.full(Y1 - Y0 + 1, IMAX, np.int64), np.full(Y1 - Y0 + 1, -1, np.int64)
            for d in range(-hi, lo + 1):           # source row Y + d reaches dilated row Y (det_post_core.h dilated_row)
                Y = np.arange(miny[c], maxy[c] + 1) - d
                ok = (Y >= Y0) & (Y <= Y1)
                Ls[Y[ok] - Y0] = np.minimum(Ls[Y[ok] - Y0], smin[ok])
                Rs[Y[ok] - Y0] = np.maximum(Rs[Y[ok] - Y0], smax[ok])
            b, m = _box_from_rows(np.maximum(Ls - lo, 0), np.minimum(Rs + hi, W - 1), Y0, Y1)
            bl.append(b); hull_m.append(m)
        if n_sel:
            boxes = np.stack(bl)
            conf = (maxv[kept] / max_conf).astype(F) if max_conf > 0 else maxv[kept]
    r.update(area_final=area_final.astype(np.int32), comp=comp, rows=rows, rowoff=rowoff, max_conf=max_conf, rmin=rmin, rmax=rmax,
             boxes=boxes, conf=conf, hull_m=hull_m)
    return r


STAGE_KEYS = ("rank", "prefix", "cnt_gt", "sum_gt", "avg", "text_thr", "low_thr", "label", "roots", "area", "minx", "maxx", "miny", "maxy", "maxv",
              "kept", "area_final", "comp", "rows", "rowoff", "n_sel", "n_rows", "overflow", "max_conf", "blk", "rmin", "rmax", "boxes", "conf")


def stages_differ(a: dict, b: dict) -> List[str]:
    """Names of the stages at which two page references differ (exact comparison, floats by value)."""
    out = []
    for key in STAGE_KEYS:
        x, y = np.asarray(a[key]), np.asarray(b[key])
        if x.shape != y.shape or not np.array_equal(x, y):
            out.append(key)
    return out


# ---------------------------------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    name: str
    pages: Tuple[str, ...]                 # page names (PAGES), one shape per case
    max_boxes: int = 512
    second: Tuple[str, ...] = ()           # a second call with these pages on the same workspace
    kills: Tuple[str, ...] = ()
    overflows: Tuple[int, ...] = ()        # pages of the first call that must report -1


def _blank(H, W, bg=BG):
    return np.full((H, W), bg, F)


def _run(m, start, n, v=FG):
    """n pixels from raster index `start`, cut at the end of the row it starts in."""
    W = m.shape[1]
    end = min(start + n, (start // W + 1) * W)
    m.ravel()[start:end] = v


def _seg(m, y0, x0, y1, x1, v=FG):
    m[min(y0, y1): max(y0, y1) + 1, min(x0, x1): max(x0, x1) + 1] = v


def page_wrap(H, W, phase):
    """A 10-pixel run ending at x = W - 1 and, in the next row, one starting at x = 0; every third row, so the three phases put the pair at
    every row: with W % 64 = 4 the row boundary falls on every fourth lane of a wave segment. Separate components, all kept."""
    m = _blank(H, W)
    for y in range(phase, H - 1, 3):
        m[y, W - 10:] = FG
        m[y + 1, :10] = FG
    return m


def page_segments(H, W):
    """Runs placed by raster index around the multiples of 64 (post_init_kernel's wave segments): across one, starting on lane 63, ending
    on lane 0; and runs of exactly 64, 65 and 128 pixels, aligned and not, where the row is long enough. Every other row."""
    m = _blank(H, W)
    kinds = [(-5, 10), (-1, 10), (-9, 10), (0, 64), (-3, 64), (0, 65), (-1, 65), (0, 128), (-7, 128), (-63, 64), (-64, 65)]
    i = 0
    for y in range(1, H - 1, 2):
        lo, hi = y * W, (y + 1) * W
        for t in range(len(kinds)):                          # the next kind that fits into this row at one of its multiples of 64
            off, n = kinds[(i + t) % len(kinds)]
            fits = [q for q in range(-(-lo // 64) * 64, hi + 64, 64) if q + off >= lo and q + off + n <= hi]
            if fits:
                _run(m, fits[0] + off, n)
                i += t + 1
                break
    return m


def page_spiral(H, W):
    m = _blank(H, W)
    t, l, b, r = 1, 1, H - 2, W - 2
    y, x = t, l
    while r - l >= 3 and b - t >= 3:
        _seg(m, y, x, t, r); _seg(m, t, r, b, r); _seg(m, b, r, b, l); _seg(m, b, l, t + 2, l)
        y, x = t + 2, l
        t, l, b, r = t + 2, l + 2, b - 2, r - 2
    return m


def page_comb(H, W, bottom):
    """Teeth every second column joined by one bar: at the bottom the teeth are labelled apart and re-linked by the last row."""
    m = _blank(H, W)
    m[2: H - 2, 2: W - 2: 2] = FG
    m[H - 3 if bottom else 2, 2: W - 2] = FG
    return m


def page_nested(H, W):
    """U shapes and inverted ones nested with one pixel between them, and a hook whose first pixel lies right of a block's but whose
    bounding box starts left of it (raster order of the roots is not the order of the bounding boxes)."""
    m = _blank(H, W)
    t, l, b, r = 12, 2, H - 3, W - 3
    i = 0
    while r - l >= 6 and b - t >= 6:
        _seg(m, t, l, b, l); _seg(m, t, r, b, r)
        _seg(m, b if i % 2 == 0 else t, l, b if i % 2 == 0 else t, r)
        t, l, b, r = t + 2, l + 2, b - 2, r - 2
        i += 1
    _seg(m, 2, 8, 4, 13)                                     # block: root (2, 8)
    _seg(m, 2, 30, 8, 31); _seg(m, 8, 2, 9, 31)              # hook: root (2, 30), bounding box from x = 2
    return m


def page_serpentine(H, W):
    m = _blank(H, W)
    m[0::2, :] = FG
    for y in range(1, H, 2):
        m[y, W - 1 if (y // 2) % 2 == 0 else 0] = FG
    return m


def page_checker(H, W):
    m = _blank(H, W)
    yy, xx = np.mgrid[0:H, 0:W]
    m[(yy + xx) % 2 == 0] = FG
    return m


def page_diagonal(H, W):
    """One-pixel diagonals (8-connected only: nothing reaches area 10) and a two-wide staircase (4-connected: one component)."""
    m = _blank(H, W)
    n = min(H, W // 2) - 4
    for i in range(n):
        m[2 + i, 2 + i] = FG
        m[2 + i, W - 3 - i] = FG
    for i in range(n // 2):
        m[H - 3 - i, W // 2 - n // 2 + i: W // 2 - n // 2 + i + 2] = FG
    return m


def page_filters(H, W):
    """Top-10 % mean 3/4 -> scale clipped to exactly 1: text_thr = float32(0.6), low_thr = float32(0.35). Under a bar of 3/4: blocks of area
    9, 10, 11; components at 1/2 whose maximum is the text threshold / one float32 step below; a neighbour pixel at the low threshold / one
    step above; two blocks parted by one column at the low threshold; near-squares on both sides of detect_boxes' 0.1 rule."""
    assert H >= 64 and W >= 128
    T, Lo = F(TEXT), F(LOW)
    m = _blank(H, W)
    m[0:8, :] = FG                                           # 8 W pixels >= N - k of them: the whole top tenth
    _seg(m, 11, 2, 13, 4); _seg(m, 11, 8, 12, 12); _seg(m, 11, 16, 11, 26)            # 9, 10, 11
    _seg(m, 11, 30, 12, 35, F(0.5)); m[12, 33] = T                                    # max == text_thr: kept
    _seg(m, 11, 40, 12, 45, F(0.5)); m[12, 43] = np.nextafter(T, F(0))                # one step below: dropped
    _seg(m, 11, 50, 12, 55); m[11, 56] = Lo                                           # pixel at low_thr: background
    _seg(m, 11, 60, 12, 65); m[11, 66] = np.nextafter(Lo, F(1))                       # one step above: foreground
    _seg(m, 11, 70, 13, 73); _seg(m, 11, 75, 13, 78); m[11:14, 74] = Lo               # two components
    _seg(m, 16, 2, 17, 6, F(0.5)); m[16, 2] = T; m[17, 6] = np.nextafter(T, F(0))     # both: kept by the one at the threshold
    for x, w in ((4, 20), (34, 22), (64, 23), (94, 26)):                              # 20 rows high: dilated 24 x (w + 4)
        _seg(m, 24, x, 43, x + w - 1)
    for x, h in ((4, 12), (24, 13), (44, 14), (64, 15)):                              # 12 columns wide
        _seg(m, 47, x, 47 + h - 1, x + 11)
    return m


def page_dark(H, W):
    """Top-10 % mean far below 0.7: both clamps (0.15 / 0.1). Components at 1/8 pass the low clamp and fail the text clamp; 1/4 is kept."""
    m = _blank(H, W, F(1 / 64))
    _seg(m, 5, 5, 6, 10, F(1 / 8)); _seg(m, 5, 20, 6, 25, F(1 / 4)); _seg(m, 20, 0, 20, 11, F(1 / 8)); _seg(m, 30, W - 12, 31, W - 1, F(1 / 4))
    return m


def page_equal(H, W):
    return _blank(H, W, F(5 / 8))                            # one component touching all four borders; every value ties at rank k


def page_plateau(H, W):
    """~73 % at 1/16, then a plateau of 1/2 that spans rank k (~24 % of the page), 3/4 above it."""
    m = _blank(H, W)
    N = H * W
    a, b = int(N * 0.734), N - 192
    m.ravel()[a:b] = F(0.5)
    m.ravel()[b:] = FG
    assert a < int(N * 0.9) < b - 1 and b - a > 1500
    return m


def page_zero_one(H, W):
    m = _blank(H, W, F(0.0))
    for y in (3, 9, 17, 30, H - 1):
        m[y, 7:27] = F(1.0)
    m[40:43, 0:5] = F(1.0)
    return m


def page_lowbits(H, W, shift, seed):
    """0.5 + j 2^-24 2^shift, j random: shift 0 -> the values differ in bits [9:0] only (third histogram level), shift 10 -> in bits
    [20:10] only (second level). One component: the whole page."""
    rng = np.random.default_rng(seed)
    j = rng.integers(0, 1 << (10 if shift == 0 else 11), (H, W))
    return (0.5 + j * 2.0 ** (shift - 24)).astype(F)


def page_edges(H, W):
    """Lines on the four borders, among them a one-pixel column at x = W - 1 (the frame that touches all four borders is page_frame)."""
    m = _blank(H, W)
    m[0, 5:41] = FG; m[H - 1, 20: W - 4] = FG; m[35:56, 0] = FG; m[10:30, W - 1] = FG
    m[5:9, W - 2:] = FG                                      # two wide, at the right border
    return m


def page_frame(H, W):
    m = _blank(H, W)
    m[0, :] = FG; m[H - 1, :] = FG; m[:, 0] = FG; m[:, W - 1] = FG
    _seg(m, 10, 10, 12, 14)                                  # inside it: area 15
    return m


def page_squares(H, W):
    """Rectangles turned by 45 degrees, |dx + dy| <= a and |dx - dy| <= b: the minimum-area rectangle of a square one is near-square, so
    detect_boxes replaces it by the upright bounding box; from b / a ~ 1.1 on the turned rectangle stays (both sides of the 0.1 rule)."""
    m = _blank(H, W)
    yy, xx = np.mgrid[0:H, 0:W]
    for i, b in enumerate((8, 9, 10, 12, 14)):
        for cy, aa, bb in ((17, 8, b), (46, b, 8)):
            dx, dy = xx - (14 + 25 * i), yy - cy
            m[(np.abs(dx + dy) <= aa) & (np.abs(dx - dy) <= bb)] = FG
    return m


def page_many(H, W):
    """More than 256 kept components: 10-pixel runs, every second row (post_boxes_kernel<0>'s grid-stride; > max_boxes = 256 overflows)."""
    m = _blank(H, W)
    for y in range(0, H, 2):
        for x in range(0, W - 9, 12):
            m[y, x: x + 10] = FG
    return m


def _zigzag(m, cx, amp, period, x_thick=3):
    """Full-height triangular zigzag whose amplitude follows an ellipse: non-convex, 4-connected, and its hull follows the ellipse (a
    vertex per peak)."""
    H = m.shape[0]
    y = np.arange(H + 1)
    env = amp * np.sqrt(np.clip(1 - ((y - H / 2) / (H / 2)) ** 2, 0, 1))
    tri = 2 * np.abs(2 * ((y / period) % 1) - 1) - 1
    x = np.rint(cx + env * tri).astype(int)
    for r in range(H):
        m[r, min(x[r], x[r + 1]): max(x[r], x[r + 1]) + x_thick] = FG


def page_big_a(H, W):
    """> 2^20 pixels, 265 scan blocks: a class-1 zigzag (whole-LDS launch, hull > 64 vertices), text-line sized runs in scan blocks before
    and after block 256 (post_scan_kernel's carry), a 300-row rule (class 1, straight)."""
    m = _blank(H, W)
    _zigzag(m, 250, 200, 24)
    for y in list(range(4, 200, 6)) + list(range(1000, 1100, 6)) + list(range(2036, 2096, 4)):
        m[y, 470:500] = FG
        m[y, 4:16] = FG
    m[300:600, 508:510] = FG
    return m


def page_big_b(H, W):
    """Taller than POST_LDS_ROWS: a class-2 zigzag (workspace scratch), a 400-row rule (class 1), runs (class 0)."""
    m = _blank(H, W)
    _zigzag(m, 20, 17, 16, 2)
    m[100:500, 50:52] = FG
    for y in range(10, H, 97):
        m[y, 56:67] = FG
    return m


def _draw(build, *args):
    """A generated non-dyadic page, redrawn seed by seed until numpy's float32 mean of the top tenth gives the thresholds of the exact mean
    and rank k is no tie with rank k + 1 (a condition on the INPUT; the staged reference itself never changes)."""
    for seed in range(64):
        m = build(*args, seed)
        r = _thresholds(m, None)
        tt, lt = hm.get_dynamic_thresholds(m, TEXT, LOW)
        s = np.sort(m.ravel())
        if bits(tt) == bits(r["text_thr"]) and bits(lt) == bits(r["low_thr"]) and s[r["k"]] != s[r["k"] + 1]:
            return m
    raise AssertionError(f"no seed of {build.__name__}{args} meets numpy's thresholds")


S, A, R, TALL, BIG = (61, 68), (64, 128), (40, 260), (2600, 68), (2100, 516)
PAGES = {
    "wrap0": (page_wrap, S, 0), "wrap1": (page_wrap, S, 1), "wrap2": (page_wrap, S, 2),
    "segments_s": (page_segments, S), "segments_a": (page_segments, A), "segments_r": (page_segments, R),
    "spiral_s": (page_spiral, S), "spiral_r": (page_spiral, R), "comb_top_s": (page_comb, S, False), "comb_bottom_s": (page_comb, S, True),
    "comb_bottom_r": (page_comb, R, True), "nested_s": (page_nested, S), "serpentine_s": (page_serpentine, S), "checker_s": (page_checker, S),
    "diagonal_s": (page_diagonal, S), "filters_a": (page_filters, A), "dark_s": (page_dark, S), "equal_s": (page_equal, S),
    "plateau_a": (page_plateau, A), "zero_one_s": (page_zero_one, S), "low10_s": (_draw, page_lowbits, *S, 0), "mid11_s": (_draw, page_lowbits, *S, 10),
    "edges_s": (page_edges, S), "frame_s": (page_frame, S), "many_a": (page_many, A), "squares_a": (page_squares, A), "big_a": (page_big_a, BIG), "big_b": (page_big_b, TALL),
}
NON_DYADIC = ("filters_a", "low10_s", "mid11_s")              # values off the 1/64 grid: thresholds held to the device's own avg


@functools.lru_cache(maxsize=None)
def page(name: str) -> np.ndarray:
    fn, *args = PAGES[name]
    m = fn(*args) if fn is _draw else fn(*args[0], *args[1:])
    m = np.ascontiguousarray(m, F)
    m.setflags(write=False)
    return m


CASES = [
    Case("wrap", ("wrap0", "wrap1", "wrap2"), kills=("row_wrap", "dil_swap")),
    Case("topology_a", ("spiral_s", "comb_bottom_s", "nested_s"), second=("serpentine_s", "checker_s", "diagonal_s"),
         kills=("root_max", "order_top", "rows_not_reset")),
    Case("topology_b", ("serpentine_s", "checker_s", "diagonal_s"), kills=("conn8", "root_max")),
    Case("topology_c", ("comb_top_s", "segments_s", "frame_s"), kills=("root_max",)),
    Case("segments_a", ("segments_a", "many_a", "filters_a"), kills=("text_gt", "low_ge", "area9")),
    Case("overflow", ("filters_a", "many_a", "segments_a"), max_boxes=256, overflows=(1,), second=("many_a", "plateau_a", "filters_a")),
    Case("thresholds_a", ("dark_s", "equal_s", "zero_one_s")),
    Case("thresholds_b", ("low10_s", "mid11_s", "edges_s"), kills=("rank_off",)),
    Case("plateau", ("plateau_a", "segments_a", "squares_a"), kills=("ties_above",)),
    Case("rows_260", ("segments_r", "comb_bottom_r", "spiral_r")),
    Case("big_a", ("big_a",), kills=("carry_dropped",)),
    Case("big_b", ("big_b",)),
]
CASE_BY_NAME = {c.name: c for c in CASES}


@functools.lru_cache(maxsize=None)
def reference(case_name: str, mutant: Optional[str] = None):
    """[call][page] -> ref_page dict. rows_not_reset acts on the second call: a slice entry keeps the first call's extreme where that call
    left one at the same place of the page's rmin / rmax."""
    case = CASE_BY_NAME[case_name]
    calls = []
    for names in (case.pages, case.second) if case.second else (case.pages,):
        calls.append([ref_page(page(n), case.max_boxes, None if mutant == "rows_not_reset" else mutant) for n in names])
    if mutant == "rows_not_reset" and case.second:
        for i, (old, new) in enumerate(zip(calls[0], calls[1])):
            new = dict(new)
            n = min(len(old["rmin"]), len(new["rmin"]))
            new["rmin"], new["rmax"] = new["rmin"].copy(), new["rmax"].copy()
            new["rmin"][:n] = np.minimum(new["rmin"][:n], old["rmin"][:n])
            new["rmax"][:n] = np.maximum(new["rmax"][:n], old["rmax"][:n])
            calls[1][i] = new
    return calls


def killed(case_name: str, mutant: str) -> List[str]:
    """Stages at which the mutant's evaluation of the case differs from the reference's."""
    out = []
    for ca, cb in zip(reference(case_name), reference(case_name, mutant)):
        for pa, pb in zip(ca, cb):
            out += stages_differ(pa, pb)
    return out
