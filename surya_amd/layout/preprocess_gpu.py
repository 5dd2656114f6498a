"""Device-side page pre-processing of the layout family: uint8 pages -> the encoder's pixel_values in one library call
(surya_layout_preprocess, csrc/layout_prep.h).

The host only names, per output image, a page and a rectangle of it (a slicer strip or the whole page); the crop, the cubic resize
to the model size, the rounding to uint8, 1/255 and the normalisation run on the GPU, bit-identical to LayoutImageProcessor. Pages
cross PCIe once as uint8, staged through a pinned buffer that is reused across calls.
"""
from __future__ import annotations

import ctypes as C
import time
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib as L
from ..common.imageops import page_pixels, parallel_copy

# must match sa::lprep::PageDesc (csrc/layout_prep.h, include/surya_amd.h)
PAGE_DESC = np.dtype([("page_off", np.int64), ("page_w", np.int32), ("page_h", np.int32), ("x0", np.int32), ("y0", np.int32),
                      ("cw", np.int32), ("ch", np.int32)], align=True)
assert PAGE_DESC.itemsize == 32, PAGE_DESC.itemsize

Rect = Tuple[int, int, int, int]            # (x0, y0, x1, y1), PIL's crop box


def page_descriptors(shapes: Sequence[Tuple[int, int]], offsets: Sequence[int], rects: Sequence[Tuple[int, Rect]]) -> np.ndarray:
    """PAGE_DESC [n] for rects = [(page index, crop box)] into pages of shapes [(h, w)] at byte offsets `offsets`."""
    desc = np.zeros(len(rects), PAGE_DESC)
    for i, (p, (x0, y0, x1, y1)) in enumerate(rects):
        h, w = shapes[p]
        if not (0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h):
            raise ValueError(f"crop box {(x0, y0, x1, y1)} is empty or outside its {w} x {h} page")
        desc[i] = (offsets[p], w, h, x0, y0, x1 - x0, y1 - y0)
    return desc


class LayoutDevicePreprocessor:
    """pixel_values for the layout / table engine from pages on the device. `timing = True` records, per call, the host staging time
    (descriptors, copies into the pinned buffer) and a hipEvent pair around the kernel in `timings` (tools/layout_call_bench.py)."""

    def __init__(self, device):
        if not torch.cuda.is_available():
            raise L.SuryaAmdError("LayoutDevicePreprocessor needs a GPU (MI355X)")
        self.lib = L.lib()
        self.device = torch.device(device)
        self._host: Optional[torch.Tensor] = None         # pinned staging, grown on demand
        self._uploaded: Optional[torch.cuda.Event] = None  # the last upload out of it has finished once this has
        self.timing = False
        self.timings: List[Tuple[float, torch.cuda.Event, torch.cuda.Event]] = []

    def __call__(self, pieces: Sequence[Tuple[object, Rect]], image_processor) -> torch.Tensor:
        """pieces: [(PIL RGB page, crop box)] -> cuda fp32 [n, 3, H, W] as image_processor (a LayoutImageProcessor) would compute it
        from the cropped images."""
        pages, index, rects = [], {}, []
        for image, box in pieces:
            k = id(image)
            if k not in index:
                index[k] = len(pages)
                pages.append(image)
            rects.append((index[k], tuple(box)))
        size = (image_processor.max_size["height"], image_processor.max_size["width"])
        return self.run([page_pixels(im) for im in pages], rects, size, image_processor.image_mean, image_processor.image_std)

    def run(self, pages: Sequence[np.ndarray], rects: Sequence[Tuple[int, Rect]], size: Tuple[int, int], mean, std) -> torch.Tensor:
        """pages: uint8 [h, w, 3] (RGB) or [h, w, 4] (RGBX) arrays; rects: [(page index, crop box)]; size: (H, W) of the output."""
        t0 = time.perf_counter()
        n = len(rects)
        H, W = int(size[0]), int(size[1])
        out = torch.empty((n, 3, H, W), dtype=torch.float32, device=self.device)
        if n == 0:
            return out
        pix = 4 if all(pg.shape[2] == 4 for pg in pages) else 3
        if pix == 3:                                   # mixed strides: repack the RGBX views
            pages = [pg if pg.shape[2] == 3 else np.ascontiguousarray(pg[..., :3]) for pg in pages]
        offs, total = [], 0
        for pg in pages:
            assert pg.dtype == np.uint8 and pg.ndim == 3 and pg.shape[2] == pix
            offs.append(total)
            total += pg.size
        desc = page_descriptors([pg.shape[:2] for pg in pages], offs, rects)
        mean_c = (C.c_float * 3)(*[float(v) for v in np.asarray(mean, np.float32)])
        std_c = (C.c_float * 3)(*[float(v) for v in np.asarray(std, np.float32)])
        torch.cuda.set_device(self.device)
        stream = torch.cuda.current_stream(self.device)
        if self._uploaded is not None:
            self._uploaded.synchronize()               # the previous call's upload has left the staging buffer
        if self._host is None or self._host.numel() < total:
            self._host = torch.empty(max(total, 2 * (self._host.numel() if self._host is not None else 0)), dtype=torch.uint8, pin_memory=True)
        hv = self._host.numpy()
        parallel_copy([hv[o: o + pg.size].reshape(pg.shape) for pg, o in zip(pages, offs)], list(pages))
        d_pages = self._host[:total].to(self.device, non_blocking=True)
        self._uploaded = torch.cuda.Event()
        self._uploaded.record(stream)
        t1 = time.perf_counter()
        if self.timing:
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record(stream)
        L.check(self.lib.surya_layout_preprocess(L.ptr(d_pages), C.c_size_t(total), desc.ctypes.data_as(C.c_void_p), C.c_int(n),
                                                 C.c_int(pix), mean_c, std_c, C.c_int(H), C.c_int(W), L.ptr(out),
                                                 C.c_void_p(stream.cuda_stream)), "surya_layout_preprocess")
        if self.timing:
            ev1.record(stream)
            self.timings.append(((t1 - t0) * 1e3, ev0, ev1))
        self._keep = d_pages                           # alive until the stream has consumed it
        return out


def device_preprocessor(predictor, image_processor) -> Optional[LayoutDevicePreprocessor]:
    """The predictor's device pre-processing, or None where the host chain runs: LAYOUT_PREPROCESS_HOST=1 (predictor.device_preprocess
    False), a model that is not the HIP engine on a GPU (host stand-ins of the tests, the table oracle), or an image processor that is
    not the family's own (a caller replaced it)."""
    from .model import HipLayoutModel
    from .predictor import LayoutImageProcessor
    model = predictor.model
    if not getattr(predictor, "device_preprocess", False) or not isinstance(model, HipLayoutModel) or model.device.type != "cuda":
        return None
    if type(image_processor) is not LayoutImageProcessor:
        return None
    prep = getattr(predictor, "device_prep", None)
    if prep is None or prep.device != model.device:
        prep = predictor.device_prep = LayoutDevicePreprocessor(model.device)
    return prep
