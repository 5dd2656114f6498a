"""Device-side line pre-processing: page pixels -> image_tiles in one library call (csrc/rec_prep.h).

The host computes only integers here -- which page, which rectangle / polygon, the sizes scale_to_fit and the x28 round-up
produce (surya/common/surya/processor/__init__.py:141-230 arithmetic) and where each line's patch rows go; cropping, the
outside-polygon pad, both resizes, normalisation and patchify run on the GPU. Pages cross PCIe once as uint8.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib as L
from ..common.imageops import curve_size, curve_table, page_pixels, parallel_copy, quad_homographies, quad_size  # noqa: F401  (page_pixels is re-exported: the predictor and tests import it from here)

# must match sa::prep::LineDesc (csrc/rec_prep.h); align=True reproduces the C layout (8-byte longs after the int block)
LINE_DESC = np.dtype([("page_off", np.int64), ("page_w", np.int32), ("page_h", np.int32), ("x0", np.int32), ("y0", np.int32),
                      ("cw", np.int32), ("ch", np.int32), ("has_poly", np.int32), ("poly", np.float32, (8,)), ("mid_w", np.int32),
                      ("mid_h", np.int32), ("out_w", np.int32), ("out_h", np.int32), ("mask_off", np.int64), ("mid_off", np.int64),
                      ("tile_row", np.int64)], align=True)
assert LINE_DESC.itemsize == 112, LINE_DESC.itemsize
# must match sa::prep::RectifyDesc (csrc/rec_rectify.h): one per rectified line, a HOST array (surya_rec_rectify copies it into kernel arguments)
RECTIFY_DESC = np.dtype([("page_off", np.int64), ("page_w", np.int32), ("page_h", np.int32), ("out_w", np.int32), ("out_h", np.int32),
                         ("out_off", np.int64), ("h", np.float64, (9,))], align=True)
assert RECTIFY_DESC.itemsize == 104, RECTIFY_DESC.itemsize
# must match sa::prep::UnrollDesc (csrc/rec_unroll.h): one per unrolled line, a HOST array like RECTIFY_DESC; table_off counts doubles
UNROLL_DESC = np.dtype([("page_off", np.int64), ("page_w", np.int32), ("page_h", np.int32), ("out_w", np.int32), ("out_h", np.int32),
                        ("out_off", np.int64), ("table_off", np.int64)], align=True)
assert UNROLL_DESC.itemsize == 40, UNROLL_DESC.itemsize
# must match sa::pagewarp::MeshDesc (csrc/page_warp_core.h): one per flattened page, a HOST array like RECTIFY_DESC; mesh_off counts doubles
MESH_DESC = np.dtype([("page_off", np.int64), ("w", np.int32), ("h", np.int32), ("cell", np.int32), ("reserved", np.int32),
                      ("out_off", np.int64), ("mesh_off", np.int64)], align=True)
assert MESH_DESC.itemsize == 40, MESH_DESC.itemsize
# must match sa::adjust::AdjustDesc (csrc/adjust_core.h): one per contrast-adjusted line, a HOST array like RECTIFY_DESC
ADJUST_DESC = np.dtype([("src_off", np.int64), ("src_w", np.int32), ("src_h", np.int32), ("x0", np.int32), ("y0", np.int32), ("w", np.int32),
                        ("h", np.int32), ("cutoff", np.int32), ("has_poly", np.int32), ("poly", np.float32, (8,)), ("out_off", np.int64),
                        ("mask_off", np.int64)], align=True)
assert ADJUST_DESC.itemsize == 88, ADJUST_DESC.itemsize
ADJUST_WORK_BYTES = 1280                                   # per line of a surya_rec_adjust_contrast call: 256 counters, then the LUT


@dataclass
class LineRef:
    """A line of a page by reference (no pixels): what RecognitionPredictor's `flat["slices"]` holds on the device path.
    `shape` is the shape the cropped array would have (slice_bboxes_from_image / slice_and_pad_poly), which is all the
    predictor reads from a slice besides its pixels (width sort, polygon scaling)."""
    page: int
    x0: int
    y0: int
    x1: int
    y1: int
    poly: Optional[Tuple[Tuple[int, int], ...]] = None      # absolute page coordinates, 4 vertices
    # a line that is RECTIFIED (RecognitionPredictor.rectify): four (x, y) floats in page coordinates, clockwise, p0 -> p1 the top edge in
    # reading direction. Its pixels are warp_quad's (common/imageops.py) of the quad, its shape quad_size's; `poly` is then not read.
    quad: Optional[Tuple[Tuple[float, float], ...]] = None
    # a line read from its CONTRAST-ADJUSTED crop (RecognitionPredictor.reread): the cutoff, an integer percent in 0..49. Its pixels are
    # autocontrast_crop's (common/imageops.py) of the padded crop it would have been read from -- the rectified one for a line with a `quad`.
    adjust: Optional[int] = None
    # a line that is UNROLLED along its centre line (RecognitionPredictor.unroll): an imageops.Curve in page coordinates. Its pixels are
    # warp_columns' (common/imageops.py) of the curve's table, its shape curve_size's; `poly` and `quad` are then not read.
    curve: Optional[tuple] = None

    @property
    def shape(self):
        if self.curve is not None:
            w, h, _ = curve_size(*self.curve)
            return (h, w, 3)
        if self.quad is not None:
            w, h = quad_size(self.quad)
            return (h, w, 3)
        return (max(self.y1 - self.y0, 0), max(self.x1 - self.x0, 0), 3)

    @property
    def size(self):
        return self.shape[0] * self.shape[1] * 3


def bbox_ref(page: int, page_w: int, page_h: int, bbox) -> LineRef:
    """The rectangle slice_bboxes_from_image cuts (surya/input/processing.py:35-54: clip at 0, at least 1 px, clip to the page)."""
    b = [max(int(v), 0) for v in bbox]
    if b[3] <= b[1]:
        b[3] = b[1] + 1
    if b[2] <= b[0]:
        b[2] = b[0] + 1
    b[2], b[3] = min(b[2], page_w), min(b[3], page_h)
    return LineRef(page, b[0], b[1], b[2], b[3])


def poly_ref(page: int, page_w: int, page_h: int, coords) -> LineRef:
    """The bounding rectangle slice_and_pad_poly cuts (:64-101) + the polygon for the pad mask. numpy slicing clips at the
    page's far edges (and a negative start would wrap, which no caller produces: detection boxes are fitted to the page)."""
    pts = tuple((int(c[0]), int(c[1])) for c in coords)
    x0, y0 = min(p[0] for p in pts), min(p[1] for p in pts)
    x1, y1 = max(p[0] for p in pts), max(p[1] for p in pts)
    return LineRef(page, max(x0, 0), max(y0, 0), min(x1, page_w), min(y1, page_h), pts)


def quad_ref(page: int, page_w: int, page_h: int, coords) -> LineRef:
    """poly_ref of a line that is rectified: the same reference with the quad the pixels are warped from."""
    ln = poly_ref(page, page_w, page_h, coords)
    ln.quad = tuple((float(c[0]), float(c[1])) for c in coords)
    return ln


def curve_ref(page: int, page_w: int, page_h: int, coords, curve) -> LineRef:
    """poly_ref of a line that is unrolled: the same reference with the curve the pixels are unrolled along."""
    ln = poly_ref(page, page_w, page_h, coords)
    ln.curve = curve
    return ln


def fit_sizes(h: int, w: int, max_size, min_size=(168, 168), factor: int = 28):
    """(mid_h, mid_w) after scale_to_fit and (out_h, out_w) after the round-up to multiples of `factor`."""
    cur, mx, mn = w * h, max_size[0] * max_size[1], min_size[0] * min_size[1]
    mw, mh = w, h
    if cur > mx:
        s = (mx / cur) ** 0.5
        mw, mh = math.floor(w * s), math.floor(h * s)
    elif cur < mn:
        s = (mn / cur) ** 0.5
        mw, mh = math.ceil(w * s), math.ceil(h * s)
    return (mh, mw), (math.ceil(mh / factor) * factor, math.ceil(mw / factor) * factor)


class DevicePreprocessor:
    def __init__(self, device, patch_size: int = 14, merge_size: int = 2, pad_value: float = 255.0,
                 mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
        if not torch.cuda.is_available():
            raise L.SuryaAmdError("DevicePreprocessor needs a GPU (MI355X)")
        self.lib = L.lib()
        self.device = torch.device(device)
        self.ps, self.merge, self.pad = patch_size, merge_size, float(pad_value)
        self.mean = (C.c_float * 3)(*[float(np.float32(m)) for m in mean])
        self.std = (C.c_float * 3)(*[float(np.float32(s)) for s in std])

    def __call__(self, pages: Sequence[np.ndarray], lines: Sequence[LineRef], max_sizes: Sequence[Tuple[int, int]]):
        """pages: uint8 [H, W, 3] (RGB) or [H, W, 4] (RGBX) arrays; lines: LineRefs into them; max_sizes: the task's img_size per line.
        Returns (tiles cuda fp32 [sum P, 3 ps^2], tile_offs int64 [n + 1], grids [(gh, gw)]).
        Lines with a `quad` are rectified first (surya_rec_rectify, once per call): their upright crops are written into an arena behind the
        pages and each then is an ordinary line whose page is its crop. Lines with `adjust` set get their contrast-adjusted, padded crops
        behind those (surya_rec_adjust_contrast, once per call, after the rectification) and are read from them likewise; the call's
        (lo, hi) bounds stay in `last_adjust_bounds` (device int32 [n_adjusted, 2], in line order). A call without a quad and without an
        adjusted line allocates and launches what it always did. Lines with a `curve` are unrolled likewise (surya_rec_unroll, once per call,
        from the tables of all of them in one device array): the arena holds the rectified crops, then the unrolled ones, then the adjusted
        copies."""
        n = len(lines)
        f = self.ps * self.merge
        offs, total = [], 0
        pix = 4 if pages and all(pg.shape[2] == 4 for pg in pages) else 3
        if pix == 3:                                   # mixed strides: repack the RGBX views
            pages = [pg if pg.shape[2] == 3 else np.ascontiguousarray(pg[..., :3]) for pg in pages]
        for pg in pages:
            assert pg.dtype == np.uint8 and pg.ndim == 3 and pg.shape[2] == pix
            offs.append(total)
            total += pg.size
        # rectified lines: their upright crops are written behind the pages, each at a 4-byte-aligned offset, as pages of their own
        n_rect = sum(1 for ln in lines if ln.quad is not None and ln.curve is None)
        unr = [i for i, ln in enumerate(lines) if ln.curve is not None]
        rdesc = np.zeros(n_rect, RECTIFY_DESC)
        arena, r, max_rw, max_rh = (total + 3) & ~3, 0, 0, 0
        adj = [i for i, ln in enumerate(lines) if ln.adjust is not None]
        adesc, amask_bytes = np.zeros(len(adj), ADJUST_DESC), 0
        desc = np.zeros(n, LINE_DESC)
        tile_offs = np.zeros(n + 1, np.int64)
        grids, mask_bytes, mid_floats, max_mid_w = [], 0, 0, 0
        for i, (ln, mx) in enumerate(zip(lines, max_sizes)):
            ph, pw = pages[ln.page].shape[:2]
            h, w = ln.y1 - ln.y0, ln.x1 - ln.x0
            if ln.curve is not None:
                w, h, _ = curve_size(*ln.curve)
            elif ln.quad is not None:
                w, h = quad_size(ln.quad)
            if h <= 0 or w <= 0:
                raise ValueError("empty line crop on the device pre-processing path (caller substitutes a blank page)")
            (mh, mw), (oh, ow) = fit_sizes(h, w, mx, factor=f)
            d = desc[i]
            if ln.curve is not None:                   # the line's page is its unrolled crop, placed behind the rectified ones below
                d["page_w"], d["page_h"], d["cw"], d["ch"] = w, h, w, h
            elif ln.quad is not None:                  # the line's page is its rectified crop
                rd = rdesc[r]
                rd["page_off"], rd["page_w"], rd["page_h"], rd["out_w"], rd["out_h"], rd["out_off"] = offs[ln.page], pw, ph, w, h, arena
                d["page_off"], d["page_w"], d["page_h"], d["cw"], d["ch"] = arena, w, h, w, h
                arena += (w * h * pix + 3) & ~3
                r, max_rw, max_rh = r + 1, max(max_rw, w), max(max_rh, h)
            else:
                d["page_off"], d["page_w"], d["page_h"] = offs[ln.page], pw, ph
                d["x0"], d["y0"], d["cw"], d["ch"] = ln.x0, ln.y0, w, h
            if ln.quad is None and ln.curve is None and ln.poly is not None and len(ln.poly) >= 3:
                if len(ln.poly) != 4:
                    raise ValueError("device pre-processing handles 4-point polygons")
                d["has_poly"] = 1
                d["poly"] = np.asarray([(x - ln.x0, y - ln.y0) for x, y in ln.poly], np.float32).reshape(-1)
                if ln.adjust is None:
                    d["mask_off"] = mask_bytes
                    mask_bytes += h * w
            d["mid_w"], d["mid_h"], d["out_w"], d["out_h"] = mw, mh, ow, oh
            if (mh, mw) != (h, w):
                d["mid_off"] = mid_floats
                mid_floats += mh * mw * 3
                max_mid_w = max(max_mid_w, mw)
            d["tile_row"] = tile_offs[i]
            gh, gw = oh // self.ps, ow // self.ps
            grids.append((gh, gw))
            tile_offs[i + 1] = tile_offs[i] + gh * gw
        # unrolled lines, behind every rectified crop: one table per line, all of them in one array of doubles
        udesc, tables, t_at, max_uw, max_uh = np.zeros(len(unr), UNROLL_DESC), [], 0, 0, 0
        for k, i in enumerate(unr):
            d, ud, ln = desc[i], udesc[k], lines[i]
            ph, pw = pages[ln.page].shape[:2]
            table, w, h = curve_table(*ln.curve)
            ud["page_off"], ud["page_w"], ud["page_h"], ud["out_w"], ud["out_h"], ud["out_off"], ud["table_off"] = offs[ln.page], pw, ph, w, h, arena, t_at
            d["page_off"] = arena
            arena += (w * h * pix + 3) & ~3
            tables.append(table.reshape(-1))
            t_at += table.size
            max_uw, max_uh = max(max_uw, w), max(max_uh, h)
        # adjusted lines, behind every rectified and every unrolled crop: what the line would have been read from is the source, the line's page its adjusted copy
        for k, i in enumerate(adj):
            d, ad = desc[i], adesc[k]
            w, h = int(d["cw"]), int(d["ch"])
            ad["src_off"], ad["src_w"], ad["src_h"], ad["x0"], ad["y0"] = d["page_off"], d["page_w"], d["page_h"], d["x0"], d["y0"]
            ad["w"], ad["h"], ad["cutoff"], ad["out_off"] = w, h, lines[i].adjust, arena
            if d["has_poly"]:                          # the pad is in the adjusted pixels: the mask moves to the adjustment
                ad["has_poly"], ad["poly"], ad["mask_off"] = 1, d["poly"], amask_bytes
                amask_bytes += h * w
                d["has_poly"], d["poly"] = 0, 0
            d["page_off"], d["page_w"], d["page_h"], d["x0"], d["y0"] = arena, w, h, 0, 0
            arena += (w * h * pix + 3) & ~3
        if n_rect:                                     # all homographies of the call in one stacked solve
            rdesc["h"] = quad_homographies([ln.quad for ln in lines if ln.quad is not None and ln.curve is None], rdesc["out_w"], rdesc["out_h"])
        torch.cuda.set_device(self.device)
        # pinned staging straight from torch's caching host allocator (a pageable buffer + .pin_memory() would allocate, fault in and
        # copy the pages' ~3 MB each a second time)
        host = torch.empty(max(total, 1), dtype=torch.uint8, pin_memory=True)
        hv = host.numpy()
        parallel_copy([hv[o: o + pg.size].reshape(pg.shape) for pg, o in zip(pages, offs)], list(pages))   # 3-8 MB each: side by side
        if n_rect or adj or unr:
            d_pages = torch.empty(arena, dtype=torch.uint8, device=self.device)
            d_pages[:host.numel()].copy_(host, non_blocking=True)
        else:
            d_pages = host.to(self.device, non_blocking=True)
        d_desc = torch.from_numpy(desc.view(np.uint8).reshape(-1)).to(self.device)
        d_mask = torch.empty(max(mask_bytes, 1), dtype=torch.uint8, device=self.device)
        d_mid = torch.empty(max(mid_floats, 1), dtype=torch.float32, device=self.device)
        tiles = torch.empty((int(tile_offs[-1]), 3 * self.ps * self.ps), dtype=torch.float32, device=self.device)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        if n_rect:
            L.check(self.lib.surya_rec_rectify(L.ptr(d_pages), rdesc.ctypes.data_as(C.c_void_p), C.c_int(n_rect), L.ptr(d_pages), C.c_int(pix),
                                               C.c_int(max_rw), C.c_int(max_rh), stream), "surya_rec_rectify")
        d_tables = None
        if unr:
            d_tables = torch.from_numpy(np.concatenate(tables)).to(self.device)
            L.check(self.lib.surya_rec_unroll(L.ptr(d_pages), udesc.ctypes.data_as(C.c_void_p), C.c_int(len(unr)), L.ptr(d_tables), L.ptr(d_pages),
                                              C.c_int(pix), C.c_int(max_uw), C.c_int(max_uh), stream), "surya_rec_unroll")
        if adj:
            d_amask = torch.empty(max(amask_bytes, 1), dtype=torch.uint8, device=self.device)
            d_work = torch.empty(len(adj) * ADJUST_WORK_BYTES, dtype=torch.uint8, device=self.device)
            self.last_adjust_bounds = torch.empty((len(adj), 2), dtype=torch.int32, device=self.device)
            L.check(self.lib.surya_rec_adjust_contrast(L.ptr(d_pages), adesc.ctypes.data_as(C.c_void_p), C.c_int(len(adj)), L.ptr(d_pages),
                                                       L.ptr(d_amask), L.ptr(d_work), L.ptr(self.last_adjust_bounds), C.c_int(pix), stream),
                    "surya_rec_adjust_contrast")
        L.check(self.lib.surya_rec_preprocess(L.ptr(d_pages), L.ptr(d_desc), C.c_int(n), L.ptr(d_mask), L.ptr(d_mid), L.ptr(tiles),
                                              C.c_int(self.ps), C.c_int(self.merge), C.c_float(self.pad), self.mean, self.std,
                                              C.c_int(int(mask_bytes > 0)), C.c_int(max_mid_w), C.c_int(pix), stream),
                "surya_rec_preprocess")
        self._keep = (d_pages, d_desc, d_mask, d_mid, host, d_tables) + ((d_amask, d_work) if adj else ())      # alive until the stream has consumed them
        return tiles, tile_offs, grids
