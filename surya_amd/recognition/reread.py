"""Re-read doubtful lines as other pictures (RecognitionPredictor.reread): after a call's first pass is assembled,
every doubtful line is read once more per variant -- its contrast-adjusted crop, its quad turned by 90 / 180 / 270 degrees -- in ONE more
`generate` run under the line's own task, input text and per-line options, and the best candidate takes the line's place.

Everything here is host logic over the call's flat line table (predictor.new_flat); pixels are touched only by the slices it builds:
LineRefs on the device path (`adjust` / `quad`, preprocess_gpu.py), arrays on the host path (autocontrast_crop / warp_quad)."""
from __future__ import annotations

import dataclasses
import time
from collections import namedtuple
from typing import Optional, Tuple

import numpy as np

from ..common.imageops import autocontrast_crop, fill_poly_mask, page_pixels, quad_homography, quad_ok, quad_size, warp_quad
from . import options
from .schema import LineReading

VARIANTS = ("original", "contrast", "rot90", "rot180", "rot270")
_Page = namedtuple("_Page", "size")


class Reread:
    """`pred.reread = Reread(below=0.6, contrast=2, rotations=(180,))`: re-read every line whose reading is doubtful -- non-empty with a
    confidence under `below` (a float, required), or under a pattern / lexicon it did not meet -- as its contrast-adjusted crop
    (`contrast`: the cutoff percent of Pillow's autocontrast, 0..49, or None) and / or turned by the quarter turns in `rotations` (a tuple
    drawn from 90, 180, 270, no repeats). At least one variant must be named. TypeError / ValueError for anything else."""

    def __init__(self, below, contrast: Optional[int] = None, rotations: Tuple[int, ...] = ()):
        if isinstance(below, bool) or not isinstance(below, (int, float)):
            raise TypeError(f"Reread.below must be a float, got {type(below).__name__}")
        if below != below:
            raise ValueError("Reread.below must not be NaN")
        if contrast is not None:
            if isinstance(contrast, bool) or not isinstance(contrast, int):
                raise TypeError(f"Reread.contrast must be None or an integer percent, got {type(contrast).__name__}")
            if not 0 <= contrast <= 49:
                raise ValueError(f"Reread.contrast must be in 0..49, got {contrast}")
        if isinstance(rotations, (str, bytes)) or not isinstance(rotations, (tuple, list)):
            raise TypeError(f"Reread.rotations must be a tuple drawn from 90, 180, 270, got {type(rotations).__name__}")
        for r in rotations:
            if isinstance(r, bool) or not isinstance(r, int):
                raise TypeError(f"Reread.rotations holds integers, got {type(r).__name__}")
            if r not in (90, 180, 270):
                raise ValueError(f"Reread.rotations are drawn from 90, 180, 270, got {r}")
        if len(set(rotations)) != len(rotations):
            raise ValueError(f"Reread.rotations names a turn twice: {tuple(rotations)}")
        if contrast is None and not rotations:
            raise ValueError("Reread needs at least one variant: contrast= or rotations=")
        self.below, self.contrast, self.rotations = float(below), contrast, tuple(rotations)

    def __repr__(self):
        return f"Reread(below={self.below!r}, contrast={self.contrast!r}, rotations={self.rotations!r})"

    @property
    def variants(self) -> tuple:
        """The variant names of this setting, in candidate order."""
        return (("contrast",) if self.contrast is not None else ()) + tuple(f"rot{r}" for r in (90, 180, 270) if r in self.rotations)


def checked(value):
    """A `reread` attribute validated for a call: None or a Reread (its constructor has checked the values; they are checked again here,
    since attributes can be assigned). TypeError for anything else."""
    if value is None:
        return None
    if not isinstance(value, Reread):
        raise TypeError(f"reread must be None or a Reread, got {type(value).__name__}")
    return Reread(value.below, value.contrast, value.rotations)


# ------------------------------------------------------------------------------------------------------- gate and choice
def has_constraint(line) -> bool:
    return line.pattern_matched is not None or line.lexicon_index is not None


def constraint_met(line) -> bool:
    return line.pattern_matched is True or (line.lexicon_index is not None and line.lexicon_index >= 0)


def doubtful(line, below: float) -> bool:
    """A non-empty reading under `below`, or a pattern / lexicon that was not met. An empty line without a constraint is not doubtful:
    its confidence is 1 by convention."""
    if has_constraint(line) and not constraint_met(line):
        return True
    return line.text != "" and (line.confidence if line.confidence is not None else 0.0) < below


def choose(candidates) -> int:
    """The index of the winner among a line's candidates (the first reading first): the constraint is met (where the line has one), the
    text is non-empty, then the higher confidence; the earlier candidate wins every tie."""
    def key(line):
        conf = line.confidence if line.confidence is not None else 0.0
        return (constraint_met(line) if has_constraint(line) else True, line.text != "", conf)
    best = 0
    for i in range(1, len(candidates)):
        if key(candidates[i]) > key(candidates[best]):
            best = i
    return best


# ------------------------------------------------------------------------------------------------------------- variants
def rolled(quad, k: int) -> tuple:
    """The quad with vertex k first: read from it, the line is its crop turned counter-clockwise by k quarter turns (np.rot90(crop, k))."""
    q = [tuple(float(c) for c in v) for v in quad]
    return tuple(q[(i + k) % 4] for i in range(4))


def base_quad(kind, poly_px, first_quad, clipped=None):
    """The quad a line's turned variants are rolled from: the quad the first pass warped it from; else, for a `bboxes=` line, its clipped
    rectangle's corners; else its polygon if that is a rectifiable quad (quad_ok). None: the line gets no turned variant."""
    if first_quad is not None:
        return tuple(tuple(float(c) for c in v) for v in first_quad)
    if kind == "bbox":
        x0, y0, x1, y1 = clipped
        poly_px = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    if poly_px is None or len(poly_px) != 4 or not quad_ok(poly_px):
        return None
    return tuple((float(v[0]), float(v[1])) for v in poly_px)


def line_variants(setting: Reread, quad) -> list:
    """[(variant name, ("adjust", cutoff) | ("quad", rolled quad))] of one line, in candidate order; `quad`: base_quad's."""
    out = []
    if setting.contrast is not None:
        out.append(("contrast", ("adjust", setting.contrast)))
    for r in (90, 180, 270):
        if r in setting.rotations and quad is not None:
            out.append((f"rot{r}", ("quad", rolled(quad, r // 90))))
    return out


def clip_bbox(bbox, page_w, page_h) -> tuple:
    """The rectangle slice_bboxes_from_image cuts (preprocess_gpu.bbox_ref's arithmetic)."""
    b = [max(int(v), 0) for v in bbox]
    if b[3] <= b[1]:
        b[3] = b[1] + 1
    if b[2] <= b[0]:
        b[2] = b[0] + 1
    return b[0], b[1], min(b[2], page_w), min(b[3], page_h)


def source_polygon(polygon, scale):
    """A line's polygon in the pixels of the image its crop is cut from (predictor.page_lines' arithmetic for a high-resolution copy)."""
    if tuple(scale) == (1, 1):
        return polygon
    return [[int(p[0] * scale[0]), int(p[1] * scale[1])] for p in polygon]


def host_contrast(slice_f32, kind, poly_px, first_quad, cutoff):
    """The host path's contrast variant of a first-pass slice (float32 pixels of integer value): autocontrast_crop of the padded crop,
    the histogram over the polygon's mask for a polygon line that was not rectified."""
    crop = np.asarray(slice_f32)
    if crop.size == 0:
        return crop
    u8 = np.ascontiguousarray(crop[..., :3]).astype(np.uint8)
    mask = None
    if kind == "poly" and first_quad is None and poly_px is not None and len(poly_px) >= 3:
        pts = [(int(c[0]), int(c[1])) for c in poly_px]
        x0, y0 = min(p[0] for p in pts), min(p[1] for p in pts)
        mask = fill_poly_mask(u8.shape[0], u8.shape[1], [(x - x0, y - y0) for x, y in pts])
    return autocontrast_crop(u8, mask, cutoff).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------- second pass
def second_pass(pred, setting: Reread, flat, orig_of, text_lines, sources, kind, recognition_batch_size, return_words, drop_repeated_text,
                math_mode, stamps):
    """`text_lines` (by original position) of a call's first pass -> the same list with every doubtful line replaced by its best candidate.
    flat: the call's line table after the first pass (slices / task_names / input_text / the options' integers by line id, polygons /
    res_scales / quads by original position); orig_of[k]: original position of line id k; sources[p]: the PIL image page p's crops are cut
    from; kind: "bbox" for a `bboxes=` call, else "poly"."""
    t0 = time.perf_counter()
    for line in text_lines:
        line.variant = "original"
        line.__pydantic_fields_set__.add("variant")
    id_of = {o: k for k, o in enumerate(orig_of)}
    page_of = []
    for p, n in enumerate(flat["slice_map"]):
        page_of.extend([p] * n)
    picked = [o for o, line in enumerate(text_lines) if doubtful(line, setting.below)]
    stamps.update(reread_lines=float(len(picked)), reread_ms=0.0)
    pred.last_reread_candidates = {}
    if not picked:
        return text_lines
    from .preprocess_gpu import LineRef, quad_ref
    device = isinstance(flat["slices"][0], LineRef)           # the call's one decision (prepare_lines dispatches on the first slice)
    first_quads, first_curves = flat.get("quads"), flat.get("curves")
    pages, page_idx, host_pages = [], {}, {}
    slices, ids, owner, names, quads2, curves2 = [], [], [], [], [], []
    for o in picked:
        k, pg = id_of[o], page_of[o]
        src = sources[pg]
        poly_px = source_polygon(flat["polygons"][o], flat["res_scales"][o])
        fq = None if first_quads is None else first_quads[o]
        fc = None if first_curves is None else first_curves[o]       # an unrolled line: its contrast variant is its unrolled crop's, its
        clipped = None                                               # turned variants read the line's quad as always
        if kind == "bbox":
            pl = flat["polygons"][o]
            clipped = clip_bbox([pl[0][0], pl[0][1], pl[2][0], pl[2][1]], src.size[0], src.size[1])
        for name, (what, arg) in line_variants(setting, base_quad(kind, poly_px, fq, clipped)):
            if device:
                if pg not in page_idx:                        # only the pages that hold a doubtful line travel again
                    page_idx[pg] = len(pages)
                    pages.append(page_pixels(src))
                if what == "adjust":
                    sl = dataclasses.replace(flat["slices"][k], page=page_idx[pg], adjust=arg)
                else:
                    sl = quad_ref(page_idx[pg], src.size[0], src.size[1], arg)
            elif what == "adjust":
                sl = host_contrast(flat["slices"][k], kind, poly_px, fq if fc is None else fc, arg)
            else:
                if pg not in host_pages:
                    host_pages[pg] = page_pixels(src)
                w, h = quad_size(arg)
                sl = warp_quad(host_pages[pg], quad_homography(arg, w, h), w, h)[..., :3].astype(np.float32)
            slices.append(sl)
            ids.append(k)
            owner.append(o)
            names.append(name)
            quads2.append(arg if what == "quad" else fq)
            curves2.append(fc if what == "adjust" else None)
    if not slices:
        return text_lines
    from .predictor import new_flat
    flat2 = new_flat()
    flat2.update(slices=slices, slice_map=[len(slices)], polygons=[flat["polygons"][o] for o in owner],
                 res_scales=[flat["res_scales"][o] for o in owner], task_names=[flat["task_names"][k] for k in ids],
                 input_text=[flat["input_text"][k] for k in ids], **options.take(flat, ids))
    if device:
        flat2["pages"] = pages
    any_quad = any(q is not None for q in quads2)
    if any_quad or first_quads is not None:
        flat2["quads"] = quads2
    if first_curves is not None:
        flat2["curves"] = curves2
    span = max(s.size[0] for s in sources), max(s.size[1] for s in sources)
    sub = {}
    results = pred._read_flat([_Page(span)], flat2, None, recognition_batch_size, False, return_words, drop_repeated_text, sub,
                              time.perf_counter(), lambda f: pred.prepare_lines(f, math_mode), math_mode)
    read = results[0].text_lines
    assert len(read) == len(slices)
    by_owner = {}
    for o, name, q, line in zip(owner, names, quads2, read):
        if first_quads is None and q is None:                 # a call without `rectify`: only a turned reading says it was warped
            line.rectified = None
            line.__pydantic_fields_set__.discard("rectified")
        line.variant = name
        line.__pydantic_fields_set__.add("variant")
        by_owner.setdefault(o, []).append(line)
    pred.last_reread_candidates = {}                          # original position -> every candidate's TextLine, for diagnostics and tests
    for o, more in by_owner.items():
        cands = pred.last_reread_candidates[o] = [text_lines[o]] + more
        readings = [LineReading(variant=c.variant, text=c.text, confidence=c.confidence) for c in cands]
        win = cands[choose(cands)]
        win.readings = readings
        win.__pydantic_fields_set__.add("readings")
        text_lines[o] = win
    stamps["reread_ms"] = (time.perf_counter() - t0) * 1e3
    stamps["reread_variants"] = float(len(slices))
    return text_lines
