"""Host side of the device LANCZOS resize of detection pages (csrc/resample.h, SURVEY 8(f) rank 2, detection side).

The reference resizes every page twice with Pillow -- `img.thumbnail(size, LANCZOS)` then `img.resize(size, LANCZOS)`
(surya/detection/__init__.py:50-57) -- on the host, ~10-20 ms per page. Pillow's 8-bit resampler (src/libImaging/Resample.c,
Pillow is an installed dependency, not part of the reference tree) is integer arithmetic once its coefficient tables exist:
    support = 3 * max(scale, 1); per output position the taps lanczos((x - center + 0.5) / max(scale, 1)) over
    [int(center - support + 0.5), int(center + support + 0.5)) clipped to the image, normalised to sum 1 in float64, then
    rounded to 22-bit fixed point; each pass accumulates int32 from 2^21 and stores clip8(acc >> 22); horizontal pass first,
    its uint8 result feeds the vertical pass.
This module computes the sizes and the fixed-point tables exactly as Pillow does (math.sin = the same libm); the kernels apply
them. Only what the GPU path covers is restated: RGB pages. `plan()` covers the pages whose thumbnail is plain LANCZOS and returns
None for anything else.

Pages whose thumbnail shrinks an axis by 4x or more: `plan_chain()`. `thumbnail(..., reducing_gap=2.0)` = Image.resize with
    fx = int(w / tw / 2.0) or 1, fy = int(h / th / 2.0) or 1; when either exceeds 1 an `Image.reduce((fx, fy))` box reduction
    (src/libImaging/Reduce.c) runs first, then the LANCZOS passes over the reduced image with box = (0, 0, w / fx, h / fy):
    scale = (in1 - in0) / out, center = in0 + (xx + 0.5) * scale, the tap window clipped to the reduced SIZE (not to in1).
    The box reaches the C code as float32, the tables are float64 from there on.
reduce(): output ceil(w / fx) x ceil(h / fy); a pixel = ((sum + n // 2) * (2^24 // n)) >> 24 in uint32 over the n source pixels that
    exist in its fx x fy block (ragged last column / row / corner: their own n). 2^24 // n is the FLOOR: for n not a power of two one
    block sum per output level comes out one below (sum + n // 2) // n.
`reduce_reference` states that in numpy (the checker of csrc/resample.h's reduce kernels; Pillow is its checker). Still left to Pillow
in both planners: images more than 100 times as tall as wide.
"""
from __future__ import annotations

import math
from functools import lru_cache
from typing import List, Optional, Tuple

import numpy as np

PRECISION_BITS = 32 - 8 - 2


def _lanczos(x: float) -> float:
    if -3.0 <= x < 3.0:
        if x == 0.0:
            return 1.0
        a, b = x * math.pi, x / 3.0 * math.pi
        return (math.sin(a) / a) * (math.sin(b) / b) if b != 0.0 else math.sin(a) / a
    return 0.0


@lru_cache(maxsize=256)
def lanczos_coeffs(in_size: int, out_size: int, in0: float = 0.0, in1: Optional[float] = None) -> Tuple[np.ndarray, np.ndarray, int]:
    """precompute_coeffs + normalize_coeffs_8bpc for the source span [in0, in1) of an axis of in_size pixels (default: the whole
    axis, box = (0, in_size)): bounds int32 [out, 2] = (first source index, tap count), taps int32 [out, ksize] in 22-bit fixed
    point. The span is float32 in Pillow's C signature (a fractional in1 follows a ragged reduce())."""
    f0 = np.float32(in0)
    f1 = np.float32(in_size if in1 is None else in1)
    in0 = float(f0)
    scale = filterscale = float(f1 - f0) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 3.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = in0 + (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        w = [_lanczos((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            kk[xx, x] = int(-0.5 + v * one) if v < 0 else int(0.5 + v * one)
        bounds[xx] = (xmin, xmax)
    return bounds, kk, ksize


def thumbnail_size(w: int, h: int, size: Tuple[int, int]) -> Optional[Tuple[int, int]]:
    """Image.thumbnail's preserve_aspect_ratio: the size the first resize goes to, or None when the image already fits."""
    x, y = int(math.floor(size[0])), int(math.floor(size[1]))
    if x >= w and y >= h:
        return None
    aspect = w / h

    def round_aspect(number, key):
        return max(min(math.floor(number), math.ceil(number), key=key), 1)

    if x / y >= aspect:
        x = round_aspect(y * aspect, key=lambda n: abs(aspect - n / y))
    else:
        y = round_aspect(x / aspect, key=lambda n: 0 if n == 0 else abs(aspect - x / n))
    return x, y


Box = Tuple[float, float, float, float]


def plan_chain(w: int, h: int, size: Tuple[int, int]) -> Optional[list]:
    """The steps of `thumbnail(size, LANCZOS)` + `resize(size, LANCZOS)`, thumbnail's reduce() pre-pass included, as a list of
    ("reduce", fx, fy) and ("resize", (w, h), box) -- box None = the whole image, else (0, 0, w / fx, h / fy) on the reduced image --
    (empty = already at `size`), or None for the tall images Pillow resizes in two calls."""
    steps: list = []
    cw, ch = w, h
    t = thumbnail_size(w, h, size)
    if t is not None and t != (w, h):
        if h > w * 100 and t[1] < h:
            return None
        fx, fy = int(w / t[0] / 2.0) or 1, int(h / t[1] / 2.0) or 1          # Image.resize(t, reducing_gap=2.0)
        box = None
        if fx > 1 or fy > 1:
            steps.append(("reduce", fx, fy))
            box = (0.0, 0.0, w / fx, h / fy)
        steps.append(("resize", t, box))
        cw, ch = t
    if (cw, ch) != tuple(size):
        if ch > cw * 100 and size[1] < ch:
            return None
        steps.append(("resize", (int(size[0]), int(size[1])), None))
    return steps


def plan(w: int, h: int, size: Tuple[int, int]) -> Optional[List[Tuple[int, int]]]:
    """`plan_chain` for the pages whose thumbnail is plain LANCZOS: the list of (w, h) targets the two resizes go to (empty =
    already at `size`), or None when Pillow would reduce first or resize a tall image in two calls."""
    steps = plan_chain(w, h, size)
    if steps is None or any(s[0] == "reduce" for s in steps):
        return None
    return [s[1] for s in steps]


def reduce_reference(img: np.ndarray, fx: int, fy: int) -> np.ndarray:
    """numpy statement of ImagingReduce for uint8 [H, W, C] -> [ceil(H / fy), ceil(W / fx), C] (the checker of the reduce kernels;
    Pillow itself is the checker of this function)."""
    h, w, c = img.shape
    oh, ow = -(-h // fy), -(-w // fx)
    pad = np.zeros((oh * fy, ow * fx, c), np.uint32)
    pad[:h, :w] = img
    s = pad.reshape(oh, fy, ow, fx, c).sum((1, 3), dtype=np.uint32)
    nx, ny = np.full(ow, fx, np.uint32), np.full(oh, fy, np.uint32)
    if w % fx:
        nx[-1] = w % fx
    if h % fy:
        ny[-1] = h % fy
    n = (ny[:, None] * nx[None, :])[..., None]
    return (((s + n // 2) * ((1 << 24) // n)) >> 24).astype(np.uint8)          # uint32: (255.5 n) * (2^24 / n) < 2^32


def resample_reference(img: np.ndarray, out_w: int, out_h: int, box: Optional[Box] = None) -> np.ndarray:
    """numpy statement of ImagingResample for uint8 [H, W, C] (the checker of the kernels in tests; Pillow itself is the
    checker of this function). box: the source rectangle (x0, y0, x1, y1), default the whole image."""
    h, w, c = img.shape
    x0_, y0_, x1_, y1_ = (0.0, 0.0, float(w), float(h)) if box is None else box
    cur = img
    if out_w != w or x0_ != 0 or x1_ != w:
        b, kk, _ = lanczos_coeffs(w, out_w, x0_, x1_)
        out = np.empty((h, out_w, c), np.uint8)
        for xx in range(out_w):
            x0, n = int(b[xx, 0]), int(b[xx, 1])
            acc = (cur[:, x0:x0 + n].astype(np.int64) * kk[xx, :n].astype(np.int64)[None, :, None]).sum(1) + (1 << (PRECISION_BITS - 1))
            out[:, xx] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
        cur = out
    if out_h != h or y0_ != 0 or y1_ != h:
        b, kk, _ = lanczos_coeffs(h, out_h, y0_, y1_)
        out = np.empty((out_h, cur.shape[1], c), np.uint8)
        for yy in range(out_h):
            y0, n = int(b[yy, 0]), int(b[yy, 1])
            acc = (cur[y0:y0 + n].astype(np.int64) * kk[yy, :n].astype(np.int64)[:, None, None]).sum(0) + (1 << (PRECISION_BITS - 1))
            out[yy] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
        cur = out
    return cur
