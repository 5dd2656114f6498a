"""Page skew from the heat map, and straightening: the rules, stated once (DetectionPredictor.skew, `straighten`; kernels: csrc/det_skew.h,
bin arithmetic: csrc/det_skew_core.h; the warp: surya_rec_rectify / imageops.warp_quad).

The estimator is the projection profile with the differential-square-sum criterion (Postl; leptonica's pixFindSkew), over integers.

1. Mask. Pixel (x, y) of an fp32 map [H][W] is text iff heat > threshold (strict, as the labelling). threshold >= 0, so the zero pad
   columns of a stitched map never count.
2. Candidates live in PAGE space. `skew` is the angle in degrees of the text baseline in the page, image coordinates with y down:
   positive = the lines run down to the right (clockwise on screen). The candidates are k * step for |k| <= floor(max_angle / step). The
   detector's map is the page scaled by (sx, sy) = (page_w / map_w, page_h / map_h), which are not equal in general, so a baseline at phi
   in the page is a baseline at theta = atan(tan(phi) * sx / sy) in the map: every page gets its own coefficient table from the one
   candidate list.
3. Coefficients, per map angle theta: c = rint(cos(theta) * 65536), s = rint(sin(theta) * 65536), float64 on the host, stored as int32.
   c > 0 and |s| <= c, i.e. |theta| <= 45 degrees. The device evaluates no trigonometry and no floating-point product.
4. Bin. r = (y * c - x * s + off) >> 16 with off = (W - 1) * max(s, 0): int32 arithmetic, |value| < 2^31 for H, W <= 8192. nb = H + W
   bins; P[r] = text pixels in bin r.
5. Score. score(theta) = sum_{r = 0}^{nb - 2} (P[r + 1] - P[r])^2 in uint64: a pure function of the mask and (c, s).
6. Choice (float64). Best = the FIRST maximum of the scores; when it is interior it is refined by the parabola through its two
   neighbours, the shift clamped to +- step / 2. skew_confidence = 1 - median(scores) / best. Fewer than min_pixels text pixels, or all
   scores equal: no estimate (None, None).
7. Straightening a page of size (w, h) by phi: the output is (W', H') = (ceil(w |cos| + h |sin| - 1e-9), ceil(w |sin| + h |cos| - 1e-9)),
   nothing is cut off; output point (u, v) samples the page at C_page + R(phi) ((u, v) - C_out), centres in grid-line coordinates.
   `straighten_matrix` returns that map as the nine numbers of a surya_rec_rectify descriptor; host and device use the same nine.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

FRAC = 65536
MAX_DIM = 8192                  # csrc/det_skew_core.h SKEW_MAX_DIM
MAX_ANGLES = 1024               # ... SKEW_MAX_ANGLES


@dataclass(frozen=True)
class SkewEstimate:
    """What `DetectionPredictor.skew` takes. max_angle in (0, 45] and step > 0, degrees, page space; at most 1024 candidates.
    min_pixels: a page with fewer text pixels has no estimate. threshold: the mask's, None = settings.DETECTOR_BLANK_THRESHOLD."""
    max_angle: float = 15.0
    step: float = 0.25
    min_pixels: int = 256
    threshold: Optional[float] = None


def _number(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, float)) and math.isfinite(v)


def candidate_angles(est: SkewEstimate) -> np.ndarray:
    """float64 [2 k + 1]: -k * step .. k * step, k = floor(max_angle / step) (a hair of slack, so 15 / 0.25 is 60)."""
    k = int(math.floor(est.max_angle / est.step + 1e-9))
    return np.arange(-k, k + 1, dtype=np.float64) * float(est.step)


def map_angles(angles, page_size, map_size) -> np.ndarray:
    """Page-space angles (degrees) as angles of the map: theta = atan(tan(phi) * sx / sy), (sx, sy) = page / map."""
    sx, sy = page_size[0] / map_size[0], page_size[1] / map_size[1]
    return np.degrees(np.arctan(np.tan(np.radians(np.asarray(angles, np.float64))) * (sx / sy)))


def page_angle(theta, page_size, map_size) -> float:
    """The inverse of map_angles for one angle: phi = atan(tan(theta) * sy / sx)."""
    sx, sy = page_size[0] / map_size[0], page_size[1] / map_size[1]
    return math.degrees(math.atan(math.tan(math.radians(theta)) * (sy / sx)))


def check_skew(est, pages: Sequence[Tuple[Tuple[int, int], Tuple[int, int]]] = ()) -> SkewEstimate:
    """The refusals of DetectionPredictor.skew, before any device work. pages: (page size, map size) of every page of the call; a page
    whose extreme candidate would lie beyond +-45 degrees in its map is refused by its index."""
    if not isinstance(est, SkewEstimate):
        raise ValueError(f"DetectionPredictor.skew must be None or a SkewEstimate, got {type(est).__name__}")
    if not _number(est.max_angle) or not (0.0 < est.max_angle <= 45.0):
        raise ValueError(f"SkewEstimate.max_angle must be in (0, 45] degrees, got {est.max_angle!r}")
    if not _number(est.step) or not est.step > 0.0:
        raise ValueError(f"SkewEstimate.step must be a positive number of degrees, got {est.step!r}")
    if isinstance(est.min_pixels, bool) or not isinstance(est.min_pixels, int) or est.min_pixels < 0:
        raise ValueError(f"SkewEstimate.min_pixels must be an integer >= 0, got {est.min_pixels!r}")
    if est.threshold is not None and (not _number(est.threshold) or est.threshold < 0.0):
        raise ValueError(f"SkewEstimate.threshold must be None or a number >= 0, got {est.threshold!r}")
    n = 2 * int(math.floor(est.max_angle / est.step + 1e-9)) + 1
    if n > MAX_ANGLES:
        raise ValueError(f"SkewEstimate: {n} candidates (max_angle {est.max_angle} / step {est.step}), at most {MAX_ANGLES}")
    top = candidate_angles(est)[-1]
    for i, (page_size, map_size) in enumerate(pages):
        if min(*page_size, *map_size) <= 0:
            raise ValueError(f"SkewEstimate: page {i} has an empty size {page_size} or map {map_size}")
        theta = float(map_angles([top], page_size, map_size)[0])
        if theta > 45.0:
            raise ValueError(f"SkewEstimate: page {i} ({page_size[0]} x {page_size[1]} on a {map_size[0]} x {map_size[1]} map): the candidate "
                             f"{top} degrees is {theta:.2f} degrees in the map, beyond 45; lower max_angle for pages of this shape")
    return est


def coeffs(theta_deg) -> np.ndarray:
    """int32 [n, 2] = (c, s) of map angles in degrees. ValueError unless c > 0 and |s| <= c."""
    t = np.radians(np.asarray(theta_deg, np.float64).reshape(-1))
    c, s = np.rint(np.cos(t) * FRAC), np.rint(np.sin(t) * FRAC)
    if not ((c > 0) & (np.abs(s) <= c)).all():
        raise ValueError("skew coefficients need |theta| <= 45 degrees")
    return np.stack([c, s], 1).astype(np.int32)


def coeff_table(angles, page_size, map_size) -> np.ndarray:
    """The table of one page: the page-space candidates as (c, s) of their map angles, int32 [n, 2]."""
    return coeffs(map_angles(angles, page_size, map_size))


def skew_scores(heat: np.ndarray, threshold: float, cs: np.ndarray):
    """The numpy reference of surya_det_skew for one map [H][W]: (scores uint64 [n], n_text)."""
    heat = np.asarray(heat)
    assert heat.ndim == 2 and max(heat.shape) <= MAX_DIM and threshold >= 0
    H, W = heat.shape
    nb = H + W
    ys, xs = np.nonzero(heat > np.float32(threshold))
    ys, xs = ys.astype(np.int64), xs.astype(np.int64)
    cs = np.asarray(cs, np.int64).reshape(-1, 2)
    out = np.zeros(len(cs), np.uint64)
    for k, (c, s) in enumerate(cs):
        r = (ys * c - xs * s + (W - 1) * max(int(s), 0)) >> 16
        r = r[(r >= 0) & (r < nb)]                                   # a bin outside [0, nb) is not counted
        P = np.bincount(r, minlength=nb).astype(np.int64)
        d = np.diff(P)
        out[k] = np.uint64(int((d * d).sum()))
    return out, int(len(ys))


def choose(scores, n_text: int, angles, step: float, min_pixels: int):
    """(skew, skew_confidence) from one page's scores, or (None, None): rule 6."""
    s = np.asarray(scores).astype(np.float64)
    if n_text < min_pixels or len(s) == 0 or (s == s[0]).all():
        return None, None
    i = int(np.argmax(s))                                            # the first maximum
    angle = float(angles[i])
    if 0 < i < len(s) - 1:
        den = s[i - 1] - 2.0 * s[i] + s[i + 1]
        if den < 0.0:
            shift = 0.5 * (s[i - 1] - s[i + 1]) / den * step
            angle += min(max(shift, -0.5 * step), 0.5 * step)
    return float(angle), float(1.0 - np.median(s) / s[i])


def estimate(heat: np.ndarray, est: SkewEstimate, page_size, threshold: float, map_size=None):
    """The host statement of one page: (skew, skew_confidence, n_text). map_size: the valid (w, h) of the map when the array is wider
    (the pad columns of a stitched map), default the array's own."""
    H, W = heat.shape
    angles = candidate_angles(est)
    scores, n_text = skew_scores(heat, threshold, coeff_table(angles, page_size, map_size or (W, H)))
    return (*choose(scores, n_text, angles, est.step, est.min_pixels), n_text)


# ------------------------------------------------------------------------------------------------------------------- straightening
def straighten_size(w: int, h: int, phi: float) -> Tuple[int, int]:
    c, s = abs(math.cos(math.radians(phi))), abs(math.sin(math.radians(phi)))
    return max(1, math.ceil(w * c + h * s - 1e-9)), max(1, math.ceil(w * s + h * c - 1e-9))


def straighten_matrix(w: int, h: int, phi: float) -> np.ndarray:
    """float64 [9], a surya_rec_rectify descriptor's h (h[6] = h[7] = 0, h[8] = 1): output point (u, v) of the straightened page ->
    C_page + R(phi) ((u, v) - C_out) in the page, grid-line coordinates. THE map of host and device straightening and of to_page."""
    W, H = straighten_size(w, h, phi)
    c, s = math.cos(math.radians(phi)), math.sin(math.radians(phi))
    cx, cy, ox, oy = 0.5 * w, 0.5 * h, 0.5 * W, 0.5 * H
    return np.array([c, -s, cx - c * ox + s * oy, s, c, cy - s * ox - c * oy, 0.0, 0.0, 1.0], np.float64)


_IDENTITY = np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0], np.float64)


def _apply(h9, points) -> np.ndarray:
    p = np.asarray(points, np.float64)
    m = np.asarray(h9, np.float64).reshape(3, 3)
    return p @ m[:2, :2].T + m[:2, 2]


class Straightened:
    """One page of `straighten`: .image (PIL RGB), .angle (the rotation applied, 0.0 for a page left as it is), .matrix (float64 [9],
    straightened -> page) and the two point maps."""

    def __init__(self, image, angle: float, matrix: np.ndarray):
        self.image, self.angle, self.matrix = image, angle, matrix

    def to_page(self, points) -> np.ndarray:
        """Points [..., 2] (x, y) of the straightened image -> the page, float64."""
        return _apply(self.matrix, points)

    def from_page(self, points) -> np.ndarray:
        """Points [..., 2] (x, y) of the page -> the straightened image, float64 (the inverse of the same matrix)."""
        inv = np.linalg.inv(self.matrix.reshape(3, 3))
        return _apply(inv.reshape(9), points)


def _pixels(im) -> np.ndarray:
    if isinstance(im, np.ndarray):
        assert im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] in (3, 4), "a pixel array is uint8 [H, W, 3 | 4]"
        return np.ascontiguousarray(im)
    from ..common.imageops import page_pixels
    return page_pixels(im if im.mode == "RGB" else im.convert("RGB"))


def straighten(images, angles, device=None, min_angle: float = 0.1) -> List[Straightened]:
    """Rotate every page by its skew so that its baselines run horizontally. images: PIL images (or uint8 [H, W, 3 | 4] arrays); angles: one
    per page, degrees as `TextDetectionResult.skew` reports them. An angle of None, or below `min_angle` in magnitude, returns the page
    untouched with an identity transform. The output holds the whole page (rule 7) and is sampled as imageops.warp_quad samples: 4 x 4
    cubic taps, replicate border, float64 sums in its tap order -- so the corner triangles that lie outside the page repeat the page's
    edge pixels; they are not white and not transparent. device: a torch device = the pages go up once and ONE surya_rec_rectify call
    warps them (uint8-equal to the host rule); None = the host rule. Polygons found on a straightened page go back through `to_page`."""
    from PIL import Image
    from ..common.imageops import warp_quad
    images, angles = list(images), list(angles)
    if len(images) != len(angles):
        raise ValueError(f"straighten: {len(images)} images, {len(angles)} angles")
    for a in angles:
        if a is not None and (not _number(a) or abs(a) >= 90.0):
            raise ValueError(f"straighten: an angle is None or a number of degrees inside (-90, 90), got {a!r}")
    todo = [i for i, a in enumerate(angles) if a is not None and abs(a) >= min_angle]
    out: List[Optional[Straightened]] = [None] * len(images)
    for i, im in enumerate(images):
        if i not in todo:
            out[i] = Straightened(Image.fromarray(im[..., :3]) if isinstance(im, np.ndarray) else im, 0.0, _IDENTITY.copy())
    if not todo:
        return out
    px = [_pixels(images[i]) for i in todo]
    mats = [straighten_matrix(p.shape[1], p.shape[0], float(angles[i])) for p, i in zip(px, todo)]
    sizes = [straighten_size(p.shape[1], p.shape[0], float(angles[i])) for p, i in zip(px, todo)]
    if device is None:
        warped = [warp_quad(p, m, W, H) for p, m, (W, H) in zip(px, mats, sizes)]
    else:
        warped = _straighten_device(px, mats, sizes, device)
    for i, wp, m in zip(todo, warped, mats):
        out[i] = Straightened(Image.fromarray(np.ascontiguousarray(wp[..., :3])), float(angles[i]), m)
    return out


def _straighten_device(px, mats, sizes, device):
    """One upload, one surya_rec_rectify call (one descriptor per page), one download."""
    import ctypes as C

    import torch

    from .. import _lib as L
    from ..recognition.preprocess_gpu import RECTIFY_DESC
    if not torch.cuda.is_available():
        raise L.SuryaAmdError("straighten(device=...) needs a GPU (MI355X); device=None runs the host rule")
    lib = L.lib()
    dev = torch.device("cuda:0" if device == "cuda" else device)
    pix = 4 if all(p.shape[2] == 4 for p in px) else 3
    px = [p if p.shape[2] == pix else np.ascontiguousarray(p[..., :3]) for p in px]
    al = lambda n: (n + 255) & ~255                                     # noqa: E731
    in_off = np.concatenate([[0], np.cumsum([al(p.nbytes) for p in px])]).astype(np.int64)
    out_bytes = [W * H * pix for W, H in sizes]
    out_off = np.concatenate([[0], np.cumsum([al(b) for b in out_bytes])]).astype(np.int64)
    stage = torch.empty(int(in_off[-1]), dtype=torch.uint8, pin_memory=True)
    sv = stage.numpy()
    for p, o in zip(px, in_off[:-1]):
        sv[int(o): int(o) + p.nbytes] = p.reshape(-1)
    desc = np.zeros(len(px), RECTIFY_DESC)
    for k, (p, m, (W, H)) in enumerate(zip(px, mats, sizes)):
        desc[k] = (int(in_off[k]), p.shape[1], p.shape[0], W, H, int(out_off[k]), m)
    torch.cuda.set_device(dev)
    d_pages = stage.to(dev, non_blocking=True)
    d_out = torch.empty(int(out_off[-1]), dtype=torch.uint8, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L.check(lib.surya_rec_rectify(L.ptr(d_pages), desc.ctypes.data_as(C.c_void_p), C.c_int(len(px)), L.ptr(d_out), C.c_int(pix),
                                  C.c_int(max(W for W, _ in sizes)), C.c_int(max(H for _, H in sizes)), stream), "surya_rec_rectify")
    host = d_out.cpu().numpy()
    return [host[int(o): int(o) + b].reshape(H, W, pix) for o, b, (W, H) in zip(out_off[:-1], out_bytes, sizes)]
