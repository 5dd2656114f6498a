"""RecognitionPredictor: drop-in for surya.recognition.RecognitionPredictor on MI355X.

Same call signature, class attributes and output schema as the reference
(surya/recognition/__init__.py:77-102, 773-942). What changes is below the plugin seam:
  * `self.model` is a HipRecModel (libsurya_amd.so); prefill / decode / process_outputs and the KV-cache merge
    (reference :294-471, cache.py) are single library calls on a slot-based cache;
  * prompts are pre-processed once up front (thread pool) and their tiles stay resident in HBM;
  * the continuous-batching policy is the reference's (:539-599: prefill when more than `min_prefill_ratio` of the
    slots are empty, same stop rules), but decode runs `RECOGNITION_STEPS_PER_SYNC` device-resident steps per host
    round trip. Per-line outputs do not depend on batch composition: attention and positions are per-sequence, every GEMM
    tile shape walks K in the same order, and the split-K slice count / lm_head partial width depend on the weight shape only
    (tests/test_gpu_fullsize.py demands identical tokens, boxes and scores across slot counts); in fp32 mode the emitted
    tokens are bit-identical to the oracle's.
There is no CPU fallback: without the HIP library and a GPU, construction raises.
"""
from __future__ import annotations

import os
import time
import zlib
from concurrent.futures import ThreadPoolExecutor
from contextlib import contextmanager
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch
from PIL import Image

from ..common.imageops import (Curve, curve_ok, curve_table, fill_poly_mask, quad_homography, quad_size, rectify_threshold, should_rectify,
                               warp_columns, warp_quad)
from ..common.predictor import BasePredictor, gc_paused
from ..settings import settings
from . import assemble, options, reread as rereading
from .loader import RecognitionModelLoader, rec_config_from_reference_json  # noqa: F401  (re-exported)
from .loop import FEED_END, DeviceLoop
from .preprocess_gpu import DevicePreprocessor, LineRef, bbox_ref, curve_ref, page_pixels, poly_ref, quad_ref
from .postprocess import sort_text_lines
from .reread import Reread  # noqa: F401  (re-exported: pred.reread = Reread(...))
from .schema import LineRanking, OCRResult, RankedCandidate, RankResult, TaskNames, TextLine


# ------------------------------------------------------------------------------------------------ input slicing
def convert_if_not_rgb(images: List[Image.Image]) -> List[Image.Image]:
    return [im if im.mode == "RGB" else im.convert("RGB") for im in images]


def slice_bboxes_from_image(image: np.ndarray, bboxes) -> List[np.ndarray]:
    """Axis-aligned crops, boxes clipped into the page (surya/input/processing.py:35-54)."""
    lines = []
    for bbox in bboxes:
        b = np.clip(np.array(bbox, dtype=np.int32), 0, None)
        if b[3] <= b[1]:
            b[3] = b[1] + 1
        if b[2] <= b[0]:
            b[2] = b[0] + 1
        b[2] = min(b[2], image.shape[1])
        b[3] = min(b[3], image.shape[0])
        lines.append(image[b[1]: b[3], b[0]: b[2]].copy())
    return lines


def slice_and_pad_poly(image: np.ndarray, coordinates) -> np.ndarray:
    """Crop the polygon's bounding box and paint everything outside the polygon with the pad value
    (surya/input/processing.py:64-101; fillPoly replaced by common.imageops.fill_poly_mask)."""
    pts = [(int(c[0]), int(c[1])) for c in coordinates]
    x0, y0 = min(p[0] for p in pts), min(p[1] for p in pts)
    x1, y1 = max(p[0] for p in pts), max(p[1] for p in pts)
    crop = image[y0:y1, x0:x1].copy()
    h, w = crop.shape[:2]
    if y1 <= y0 or x1 <= x0 or len(pts) < 3 or h == 0 or w == 0:
        return crop
    mask = fill_poly_mask(h, w, [(x - x0, y - y0) for x, y in pts])
    crop[mask == 0] = settings.RECOGNITION_PAD_VALUE
    return crop


def slice_polys_from_image(image: np.ndarray, polys) -> List[np.ndarray]:
    return [slice_and_pad_poly(image, p) for p in polys]


def slice_polys(polys, threshold, page=None, pg: int = -1, arr=None, curves=None):
    """The slices of one page's polygons (in the pixels of the image they are cut from) and, with rectification on (`threshold` not
    None), per polygon the quad it is warped from or None -- the ONE place where should_rectify is asked, for every call path. Device
    path (`page`: the page's uint8 pixels, registered as page `pg`): LineRefs; host path (`arr`: the image processor's array of the
    same page): arrays, a rectified one being warp_quad's pixels as float32. curves (a call with `unroll` set): per polygon None or the
    Curve the line is unrolled along, in the same pixels; such a line is read from warp_columns' crop and is not asked about rectification."""
    bent = [None] * len(polys) if curves is None else curves
    quads = None if threshold is None else [tuple((float(c[0]), float(c[1])) for c in pl) if bent[i] is None and should_rectify(pl, threshold)
                                            else None for i, pl in enumerate(polys)]
    slices = []
    for i, pl in enumerate(polys):
        q = None if quads is None else quads[i]
        if bent[i] is not None:
            if arr is None:
                h, w = page.shape[:2]
                slices.append(curve_ref(pg, w, h, pl, bent[i]))
            else:
                table, _, out_h = curve_table(*bent[i])
                slices.append(warp_columns(page, table, out_h)[..., :3].astype(np.float32))
        elif arr is None:
            h, w = page.shape[:2]
            slices.append(quad_ref(pg, w, h, pl) if q is not None else poly_ref(pg, w, h, pl))
        elif q is not None:
            w, h = quad_size(q)
            slices.append(warp_quad(page, quad_homography(q, w, h), w, h)[..., :3].astype(np.float32))
        else:
            slices.append(slice_and_pad_poly(arr, pl))
    return slices, quads


def checked_curve(where: str, given):
    """One entry of `RecognitionPredictor.centerlines` (None, or (points, thickness)) as a Curve; ValueError naming the line for what curve_ok refuses."""
    if given is None:
        return None
    try:
        points, thickness = given
    except (TypeError, ValueError):
        raise ValueError(f"{where}: a centre line is None or (points, thickness), got {given!r}") from None
    if not curve_ok(points, thickness):
        raise ValueError(f"{where}: the centre line cannot be unrolled (at least two finite points, no zero-length segment, a positive "
                         f"thickness), got {given!r}")
    return Curve(points, thickness)


def detected_curves(det_pred, scale):
    """The Curves of one detected page's boxes (DetectionPredictor.centerlines), in the pixels the crops are cut from; None per straight line."""
    out = []
    for k, b in enumerate(det_pred.bboxes):
        pts, th = getattr(b, "centerline", None), getattr(b, "thickness", None)
        out.append(None if pts is None or th is None else checked_curve(f"detected line {k}", (pts, th)).scaled(scale[0], scale[1]))
    return out


def new_flat() -> dict:
    """The lines of one call, flattened over its pages. By line id (sorted / admission order): slices, task_names, input_text;
    by ORIGINAL position (page order): polygons, res_scales; slice_map holds the line count per page. The device path adds "pages";
    a call with `rectify` set adds "quads", by original position: the quad a line was warped from (in the pixels its slice came
    from), None for a line that took the ordinary path; a call with `unroll` set adds "curves" likewise: the Curve a line was unrolled
    along."""
    return {"slices": [], "slice_map": [], "polygons": [], "task_names": [], "input_text": [], "res_scales": []}


def page_lines(det_pred, image, highres):
    """One page's detected polygons -> (the polygons, the image its crops are cut from, the polygons in that image's pixels, its
    scale against the detected page). With a high-resolution copy of the page the crops come from the copy."""
    polygons = [p.polygon for p in det_pred.bboxes]
    if not highres:
        return polygons, image, polygons, (1, 1)
    ws, hs = highres.size[0] / image.size[0], highres.size[1] / image.size[1]
    return polygons, highres, [[[int(p[0] * ws), int(p[1] * hs)] for p in poly] for poly in polygons], (ws, hs)


def inputs_fingerprint(shapes, chunks) -> list:
    """What every rank of a sharded call must agree on (dist.assert_same_inputs): the item count, a CRC of the items' (h, w) or
    (w, h) pairs and a CRC of sample bytes."""
    shapes = np.asarray(shapes, np.int64).reshape(-1, 2)
    return [len(shapes), zlib.crc32(shapes.tobytes()), zlib.crc32(b"".join(chunks))]


def per_image_lists(arg, name, n_images) -> list:
    """An `allowlist` / `blocklist` / `pattern` argument as one entry per image: None, a str, or a list with one None / str per line."""
    if arg is None or isinstance(arg, str):
        return [arg] * n_images
    if not isinstance(arg, (list, tuple)):
        raise TypeError(f"{name} must be a str or a list with one entry per image, got {type(arg).__name__}")
    if len(arg) != n_images:
        raise ValueError(f"{name} has {len(arg)} entries for {n_images} images")
    for e in arg:
        if e is None or isinstance(e, str):
            continue
        if not isinstance(e, (list, tuple)) or not all(x is None or isinstance(x, str) for x in e):
            raise TypeError(f"an entry of {name} is None, a str, or a list of None / str per line")
    return list(arg)


class LexiconKey(tuple):
    """One lexicon of a call, hashable: its entries in order. (A type of its own, so that a list per line is told from a lexicon.)"""


def _as_lexicon(x):
    """x as a LexiconKey if it is a lexicon -- a non-empty list / tuple of str -- else None."""
    if isinstance(x, (list, tuple)) and len(x) > 0 and all(isinstance(e, str) for e in x):
        return LexiconKey(x)
    return None


def per_image_lexicons(arg, n_images, name="lexicon") -> list:
    """A `lexicon` (or, under its `name`, `boost_words`) argument as one entry per image: None, a LexiconKey, or a list with one None / LexiconKey per line. The argument is a
    list of str (one lexicon for every line), or a list with one entry per image: None, a list of str, or a list per line of None /
    list of str."""
    if arg is None:
        return [None] * n_images
    if isinstance(arg, str) or not isinstance(arg, (list, tuple)):
        raise TypeError(f"{name} must be a list of str or a list with one entry per image, got {type(arg).__name__}")
    if len(arg) == 0:
        raise ValueError(f"{name} is an empty list: a {name} needs at least one entry")
    whole = _as_lexicon(arg)
    if whole is not None:
        return [whole] * n_images
    if len(arg) != n_images:
        raise ValueError(f"{name} has {len(arg)} entries for {n_images} images")
    out = []
    for i, e in enumerate(arg):
        if e is None:
            out.append(None)
            continue
        if isinstance(e, str) or not isinstance(e, (list, tuple)):
            raise TypeError(f"an entry of {name} is None, a list of str, or a list of None / list of str per line")
        key = _as_lexicon(e)
        if key is not None:
            out.append(key)
            continue
        lines = []
        for x in e:
            k = None if x is None else _as_lexicon(x)
            if x is not None and k is None:
                if isinstance(x, (list, tuple)) and len(x) == 0:
                    raise ValueError(f"image {i}: a {name} is an empty list: it needs at least one entry")
                raise TypeError(f"an entry of {name} is None, a list of str, or a list of None / list of str per line")
            lines.append(k)
        out.append(lines)
    return out


def given_lists(allowlist=None, blocklist=None, pattern=None, lexicon=None, boost_words=None, boost_weight=None) -> dict:
    """The list arguments of a call that were given, as keywords: `_call` is reached positionally by the page-sharded path and by
    stand-ins, so the lists go by keyword and only when given (allowlist and blocklist together; boost_weight with boost_words)."""
    lists = {} if allowlist is None and blocklist is None else {"allowlist": allowlist, "blocklist": blocklist}
    lists.update((k, v) for k, v in (("pattern", pattern), ("lexicon", lexicon), ("boost_words", boost_words)) if v is not None)
    if boost_words is not None:
        lists["boost_weight"] = boost_weight
    return lists


def list_for_pages(name, arg, n_images, pages) -> list:
    """List argument `name` of a call over n_images, for the images `pages` only, back in argument form (one entry per image; a
    lexicon as a list, not a key)."""
    if name in ("allowlist", "blocklist", "pattern"):
        per = per_image_lists(arg, name, n_images)
        return [per[i] for i in pages]
    per = per_image_lexicons(arg, n_images, name)
    return [None if per[i] is None else [None if k is None else list(k) for k in per[i]] if isinstance(per[i], list) else list(per[i])
            for i in pages]


class LineConstraints:
    """The allowlist / blocklist / pattern arguments of one call, resolved: `table` holds the call's distinct token masks (MaskTable:
    identical sets are merged), `per_image[i]` the mask id of every line of image i (an int) or one id per line (a list). `lines_known`
    is False on the detector paths, where the per-line form cannot be matched to lines that do not exist yet. With patterns:
    `patterns` is the call's PatternTables (recognition/pattern.py), compiled once, whose states' allowed sets are further rows of
    `table`, and `per_image_state[i]` the start state of image i's lines in the same two forms (-1 = no pattern). A line with a
    pattern has mask id -1: its start state names its row. With lexicons: `lexicons` is the call's LexiconTables
    (recognition/lexicon.py), compiled once, and `per_image_lex[i]` the lexicon start state of image i's lines in the same two forms
    (-1 = no lexicon). A line takes a lexicon, a pattern, or an allowlist / blocklist, never two. A lexicon needs a mask table on the
    device, so a call whose only constraints are lexicons gets one row that allows everything and that no line names. With boosted
    decoding: `boost` is the call's BoostTables (recognition/boost.py), compiled once for the call's distinct lists, whose word-unit
    set is one more row of `table` (boost.word_row; so the table is never empty), and `per_image_root[i]` the root state of image i's
    lines in the same two forms (-1 = not boosted). A boosted line takes no allowlist / blocklist; other lines of the call may."""

    def __init__(self, tokenizer, allowlist, blocklist, n_images, line_counts, vocab_size=None, limit=None, pattern=None, lexicon=None,
                 boost_words=None):
        from .tokenizer import MaskTable
        self.table = MaskTable(tokenizer, vocab_size, limit)
        allow, block = per_image_lists(allowlist, "allowlist", n_images), per_image_lists(blocklist, "blocklist", n_images)
        pats = per_image_lists(pattern, "pattern", n_images)
        self.per_image, per_image_pat = [], []
        for i, (a, b, p) in enumerate(zip(allow, block, pats)):
            if not any(isinstance(x, (list, tuple)) for x in (a, b, p)):
                if p is not None and (a is not None or b is not None):
                    raise ValueError(f"image {i}: a line takes a pattern or an allowlist / blocklist, not both")
                self.per_image.append(self.table.id_for(a, b))
                per_image_pat.append(p)
                continue
            if line_counts is None:
                raise ValueError("a per-line allowlist / blocklist / pattern needs bboxes or polygons: with det_predictor the lines are not known yet")
            n = line_counts[i]
            a = list(a) if isinstance(a, (list, tuple)) else [a] * n
            b = list(b) if isinstance(b, (list, tuple)) else [b] * n
            p = list(p) if isinstance(p, (list, tuple)) else [p] * n
            if len(a) != n or len(b) != n or len(p) != n:
                raise ValueError(f"image {i} has {n} lines but its allowlist / blocklist / pattern entry has {len(a)} / {len(b)} / {len(p)}")
            for j, (x, y, z) in enumerate(zip(a, b, p)):
                if z is not None and (x is not None or y is not None):
                    raise ValueError(f"image {i}, line {j}: a line takes a pattern or an allowlist / blocklist, not both")
            self.per_image.append([self.table.id_for(x, y) for x, y in zip(a, b)])
            per_image_pat.append(p)
        distinct = list(dict.fromkeys(z for p in per_image_pat for z in (p if isinstance(p, list) else [p]) if z is not None))
        self.patterns, self.per_image_state = None, None
        if distinct:
            from .pattern import compile_patterns
            self.patterns = compile_patterns(tokenizer, distinct, vocab_size, extra_mask_rows=self.table)
            start = {z: s for z, s in zip(self.patterns.patterns, self.patterns.starts)}
            start[None] = -1
            self.per_image_state = [[start[z] for z in p] if isinstance(p, list) else start[p] for p in per_image_pat]
        self.lexicons, self.per_image_lex = None, None
        lex = per_image_lexicons(lexicon, n_images)
        if any(x is not None for x in lex):
            self._add_lexicons(tokenizer, lex, per_image_pat, line_counts, vocab_size)
        self.boost, self.per_image_root = None, None
        bw = per_image_lexicons(boost_words, n_images, "boost_words")
        if any(x is not None for x in bw):
            self._add_boost(tokenizer, bw, line_counts, vocab_size)

    def _add_boost(self, tokenizer, bw, line_counts, vocab_size):
        if self.patterns is not None or self.lexicons is not None:
            raise ValueError("boost_words is not available with pattern or lexicon")
        for i, (x, ids) in enumerate(zip(bw, self.per_image)):
            if x is None:
                continue
            if not isinstance(x, list) and not isinstance(ids, list):
                if ids != -1:
                    raise ValueError(f"image {i}: a boosted line takes no allowlist / blocklist")
                continue
            if line_counts is None:
                raise ValueError("per-line boost_words need bboxes or polygons: with det_predictor the lines are not known yet")
            n = line_counts[i]
            x, ids = (v if isinstance(v, list) else [v] * n for v in (x, ids))
            if len(x) != n:
                raise ValueError(f"image {i} has {n} lines but its boost_words entry has {len(x)}")
            for j, (k, y) in enumerate(zip(x, ids)):
                if k is not None and y != -1:
                    raise ValueError(f"image {i}, line {j}: a boosted line takes no allowlist / blocklist")
        distinct = list(dict.fromkeys(k for x in bw for k in (x if isinstance(x, list) else [x]) if k is not None))
        from .boost import compile_boost
        self.boost = compile_boost(tokenizer, distinct, vocab_size)
        self.boost.word_row = self.table.add_row(self.boost.word_mask, "allowlists / blocklists (boost_words take one row)")
        root = {k: r for k, r in zip(distinct, self.boost.roots)}
        root[None] = -1
        self.per_image_root = [[root[k] for k in x] if isinstance(x, list) else root[x] for x in bw]

    def _add_lexicons(self, tokenizer, lex, per_image_pat, line_counts, vocab_size):
        for i, (lx, ids, p) in enumerate(zip(lex, self.per_image, per_image_pat)):
            if lx is None:
                continue
            if not any(isinstance(x, list) for x in (lx, ids, p)):
                if ids != -1 or p is not None:
                    raise ValueError(f"image {i}: a line takes a lexicon, a pattern or an allowlist / blocklist, never two")
                continue
            if line_counts is None:
                raise ValueError("a per-line lexicon needs bboxes or polygons: with det_predictor the lines are not known yet")
            n = line_counts[i]
            lx, ids, p = (x if isinstance(x, list) else [x] * n for x in (lx, ids, p))
            if len(lx) != n:
                raise ValueError(f"image {i} has {n} lines but its lexicon entry has {len(lx)}")
            for j, (x, y, z) in enumerate(zip(lx, ids, p)):
                if x is not None and (y != -1 or z is not None):
                    raise ValueError(f"image {i}, line {j}: a line takes a lexicon, a pattern or an allowlist / blocklist, never two")
        distinct = list(dict.fromkeys(k for x in lex for k in (x if isinstance(x, list) else [x]) if k is not None))
        from .lexicon import compile_lexicons
        self.lexicons = compile_lexicons(tokenizer, distinct, vocab_size)
        start = {k: s for k, s in zip(distinct, self.lexicons.starts)}
        start[None] = -1
        self.per_image_lex = [[start[k] for k in x] if isinstance(x, list) else start[x] for x in lex]
        if len(self.table) == 0:                              # the engine keeps lexicon rows behind a mask table: one row nobody names
            V = tokenizer.vocab_size if vocab_size is None else int(vocab_size)
            bits = np.zeros((V + 31) // 32 * 32, bool)
            bits[:V] = True
            self.table.add_row(np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1).astype(np.uint32))

    def __bool__(self):
        return len(self.table) > 0

    def line_ids(self, slice_map, per_image=None) -> list:
        """One id per line, in page order, for pages of slice_map[i] lines."""
        out = []
        for ids, n in zip(self.per_image if per_image is None else per_image, slice_map):
            out.extend(ids if isinstance(ids, list) else [ids] * n)
        return out

    # line_ids for the other options' integers (-1 = no pattern / no lexicon / not boosted); a call with that option only
    def line_states(self, slice_map) -> list:
        return self.line_ids(slice_map, self.per_image_state)

    def line_lexicon_starts(self, slice_map) -> list:
        return self.line_ids(slice_map, self.per_image_lex)

    def line_boost_roots(self, slice_map) -> list:
        return self.line_ids(slice_map, self.per_image_root)


class AssemblyHandover(ThreadPoolExecutor):
    """One call's assembly worker. Output assembly is host work of the same order as the device loop itself; it runs on one worker
    thread WHILE the device decodes the next lines: the lines that stopped at a synchronisation point (`on_done` each, then `on_flush`)
    are handed over together (batched numpy work, `_assemble_batch`). The scheduler thread spends most of its time blocked in
    hipEventSynchronize (GIL released), which is when the worker runs. `orig_of[k]`: the original position of line id k."""

    def __init__(self, pred, flat, orig_of, drop_repeated_text, return_words):
        self.pred, self.flat, self.orig_of = pred, flat, orig_of
        self.options = (drop_repeated_text, return_words, pred.model.cfg.bbox_size)
        super().__init__(1)                                    # (as a context manager: the worker is joined on the way out)
        self.futures, self.pending = [], []

    def assemble(self, batch):
        # batch = [(line id, tokens, scores, bbox_rows)]: the lines that stopped at one synchronisation point
        if self.pred._beam is not None:                        # a beam-search call: [(line id, hypotheses)]
            return assemble.assemble_beam_batch(self.pred.processor, self.flat, [(b[0], self.orig_of[b[0]], b[1]) for b in batch], *self.options)
        return self.pred._assemble_batch(self.flat, [(b[0], self.orig_of[b[0]]) + tuple(b[1:]) for b in batch], *self.options)

    def on_done(self, k, tokens, sc=None, bbox_rows=None, *alts):
        # alts: (alternative ids [T, 4], probabilities [T, 4]) of a call with top_k, else nothing
        if sc is None:                                         # a beam-search call: `tokens` is the line's hypothesis list
            self.pending.append((k, list(tokens)))
            return
        self.pending.append((k, list(tokens), list(sc), bbox_rows.copy()) + ((alts,) if alts else ()))

    def on_flush(self):
        if self.pending:
            batch = self.pending[:]
            self.pending.clear()
            self.futures.append(([b[0] for b in batch], self.submit(self.assemble, batch)))

    def finish(self, stamps, t_loop) -> list:
        """After the loop: hand over what is pending, wait for the worker; the TextLines by ORIGINAL position."""
        self.on_flush()
        t2 = time.perf_counter()
        text_lines = self.place((ks, f.result()) for ks, f in self.futures)
        stamps.update(device_loop_ms=(t2 - t_loop) * 1e3, assemble_tail_ms=(time.perf_counter() - t2) * 1e3)
        return text_lines

    def place(self, groups) -> list:
        """groups = [(line ids, their TextLines)] -> the TextLines by ORIGINAL position, every position filled."""
        text_lines = [None] * len(self.orig_of)
        for ks, lines in groups:
            for k, line in zip(ks, lines):
                text_lines[self.orig_of[k]] = line
        assert all(t is not None for t in text_lines)
        return text_lines


@dataclass
class RecognitionPrompt:
    id: int
    task_name: str
    image: np.ndarray
    text: Optional[str]
    math_mode: bool


class RecognitionPredictor(BasePredictor):
    model_loader_cls = RecognitionModelLoader
    batch_size = settings.RECOGNITION_BATCH_SIZE
    torch_dtype = None
    default_batch_sizes = {"cpu": 32, "mps": 64, "cuda": 256, "xla": 128}
    encoder_chunk_size: int = 4096
    encoder_chunk_sizes = {"cpu": 4096, "mps": 4096, "cuda": 32768, "xla": 32768}
    min_prefill_ratio: float = settings.RECOGNITION_MIN_PREFILL_RATIO
    min_trim_length: int = 50        # kept for API compatibility; the slot cache has no left padding to trim
    tasks = {
        TaskNames.ocr_with_boxes: {"needs_bboxes": True, "img_size": (1024, 256), "max_tokens": 224},
        TaskNames.ocr_without_boxes: {"needs_bboxes": False, "img_size": (1024, 256), "max_tokens": 224},
        TaskNames.block_without_boxes: {"needs_bboxes": False, "img_size": (1024, 512), "max_tokens": 768},
    }

    # Multi-GPU: when set, ONE call's lines are dealt over the ranks of `process_group` (default group if
    # None) and the results all-gathered; every rank must pass the same inputs (checked). Off by default.
    shard_lines: bool = settings.SURYA_AMD_SHARD
    process_group = None
    # Line crops are cut, padded, resized, normalised and patchified on the device (surya_rec_preprocess): the host keeps page
    # pixels as uint8 and describes lines by reference. RECOGNITION_PREPROCESS_HOST=1 selects the host (numpy) chain instead.
    device_preprocess: bool = not settings.RECOGNITION_PREPROCESS_HOST

    preprocess_workers: int = min(8, os.cpu_count() or 1)   # threads of the host pre-processing chain

    def line_budget(self, task) -> int:
        """Token budget of one line of `task`."""
        return settings.RECOGNITION_MAX_TOKENS or self.tasks[task]["max_tokens"]

    # --------------------------------------------------------------------------------------------- slicing
    def _page(self, flat: dict, image) -> int:
        """Device path: register a page (uint8 HWC) once, return its index for LineRefs."""
        flat.setdefault("pages", []).append(page_pixels(image))
        return len(flat["pages"]) - 1

    def detect_and_slice_bboxes(self, images, task_names, det_predictor, detection_batch_size=None, highres_images=None):
        det_predictions = det_predictor(images, batch_size=detection_batch_size)
        flat = new_flat()
        thr = rectify_threshold(self.rectify)
        if thr is not None:
            flat["quads"] = []
        unroll = self._unroll_on()
        if unroll:
            flat["curves"] = []
        for det_pred, image, highres, task in zip(det_predictions, images, highres_images, task_names):
            polygons, src, polys_px, scale = page_lines(det_pred, image, highres)
            curves = detected_curves(det_pred, scale) if unroll else None
            if self.device_preprocess:
                pg = self._page(flat, src)
                slices, quads = slice_polys(polys_px, thr, flat["pages"][pg], pg, curves=curves)
            elif thr is None and not unroll:
                slices = slice_polys_from_image(self.processor.image_processor(src), polys_px)
            else:
                slices, quads = slice_polys(polys_px, thr, page_pixels(src), arr=self.processor.image_processor(src), curves=curves)
            if thr is not None:
                flat["quads"].extend(quads)
            if unroll:
                flat["curves"].extend(curves)
            flat["slice_map"].append(len(slices))
            flat["slices"].extend(slices)
            flat["polygons"].extend(polygons)
            flat["task_names"].extend([task] * len(slices))
            flat["res_scales"].extend([scale] * len(polygons))
        flat["input_text"] = [None] * len(flat["slices"])
        return flat

    def slice_bboxes(self, images, task_names, bboxes=None, polygons=None, input_text=None) -> dict:
        assert bboxes is not None or polygons is not None
        flat = new_flat()
        # ONE decision for the whole call (prepare_lines dispatches on the type of the first slice): the device path takes 4-point
        # polygons only, so a single polygon with another vertex count anywhere sends every image of the call down the host path
        dev = self.device_preprocess and (polygons is None or all(len(pl) == 4 for page in polygons for pl in page))
        thr = rectify_threshold(self.rectify)
        if thr is not None:
            flat["quads"] = []
        unroll, given = self._unroll_on(), self._curves_given
        if unroll:
            flat["curves"] = []
        for idx, image in enumerate(images):
            arr = None if dev else self.processor.image_processor(image)
            pg = self._page(flat, image) if dev else -1
            curves = None
            if unroll:                                        # (validated by __call__, before any device work)
                n_lines = len(polygons[idx] if polygons is not None else bboxes[idx])
                curves = [None] * n_lines if given is None or polygons is None else list(given[idx])
                flat["curves"].extend(curves)
            if polygons is not None:
                polys = polygons[idx]
                if curves is not None and any(c is not None for c in curves):
                    slices, quads = (slice_polys(polys, thr, flat["pages"][pg], pg, curves=curves) if dev
                                     else slice_polys(polys, thr, page_pixels(image), arr=arr, curves=curves))
                    if thr is not None:
                        flat["quads"].extend(quads)
                elif thr is None:
                    slices = ([poly_ref(pg, image.size[0], image.size[1], pl) for pl in polys] if dev
                              else slice_polys_from_image(arr, polys))
                else:
                    slices, quads = slice_polys(polys, thr, flat["pages"][pg], pg) if dev else slice_polys(polys, thr, page_pixels(image), arr=arr)
                    flat["quads"].extend(quads)
            else:
                slices = ([bbox_ref(pg, image.size[0], image.size[1], b) for b in bboxes[idx]] if dev
                          else slice_bboxes_from_image(arr, bboxes[idx]))
                polys = [[[b[0], b[1]], [b[2], b[1]], [b[2], b[3]], [b[0], b[3]]] for b in bboxes[idx]]
                if thr is not None:                           # `bboxes=` lines are never rectified
                    flat["quads"].extend([None] * len(slices))
            flat["slice_map"].append(len(slices))
            flat["slices"].extend(slices)
            flat["polygons"].extend(polys)
            flat["task_names"].extend([task_names[idx]] * len(slices))
            flat["input_text"].extend([None] * len(slices) if input_text is None else input_text[idx])
        n = len(flat["slices"])
        assert n == sum(flat["slice_map"]) == len(flat["polygons"]) == len(flat["input_text"]) == len(flat["task_names"])
        flat["res_scales"] = [(1, 1)] * n
        return flat

    def prepare_input(self, task_names, images, input_text, math_modes):
        """Area clamp + prompt assembly per crop (reference :259-292)."""
        batch = []
        for image, text, task, math_mode in zip(images, input_text, task_names, math_modes):
            size = self.tasks[task]["img_size"]
            if image.size == 0:     # the reference catches cv2.error here and substitutes a blank crop (:272-278)
                image = np.zeros((size[1], size[0], 3), dtype=np.float32)
            else:
                image = self.processor.scale_to_fit(image, size)
            text = text or ""
            if len(text) > self.tasks[task]["max_tokens"]:
                text = ""
            batch.append({"task": task, "inputs": [{"type": "image", "image": image, "rotated": False},
                                                   {"type": "text", "text": text.strip(), "math": math_mode}]})
        return batch

    def preprocess_prompts_device(self, prompts: List[RecognitionPrompt], pages):
        """Device path: prompts whose `image` is a LineRef -> one surya_rec_preprocess call; prompt ids on the host."""
        if getattr(self, "_prep", None) is None:
            self._prep = DevicePreprocessor(self.model.device, self.processor.patch_size, self.processor.merge_size,
                                            settings.RECOGNITION_PAD_VALUE, self.processor.image_mean, self.processor.image_std)
        pages = list(pages)
        refs = []
        for p in prompts:
            ln = p.image
            if ln.size == 0:          # the reference substitutes a blank crop of the task size (:272-278): a black page of that size
                size = self.tasks[p.task_name]["img_size"]
                pages.append(np.zeros((size[1], size[0], 3), np.uint8))
                ln = LineRef(len(pages) - 1, 0, 0, size[0], size[1])
            refs.append(ln)
        tiles, offs, grids = self._prep(pages, refs, [self.tasks[p.task_name]["img_size"] for p in prompts])
        m2 = self.processor.merge_size ** 2
        ids = []
        for p, (gh, gw) in zip(prompts, grids):
            text = p.text or ""
            if len(text) > self.tasks[p.task_name]["max_tokens"]:
                text = ""
            ids.append(self.processor.prompt_ids(gh * gw // m2, p.task_name, text.strip(), p.math_mode, False))
        return tiles, offs, grids, ids

    def preprocess_prompts(self, prompts: List[RecognitionPrompt]):
        """All prompts -> (device tiles [sum P, 588], per-prompt tile offsets, grids, prompt ids)."""
        def one(p):
            b = self.prepare_input([p.task_name], [p.image], [p.text], [p.math_mode])
            return self.processor(b)

        if len(prompts) > 4 and self.preprocess_workers > 1:
            with ThreadPoolExecutor(self.preprocess_workers) as ex:
                outs = list(ex.map(one, prompts))
        else:
            outs = [one(p) for p in prompts]
        counts = [o["image_tiles"].shape[0] for o in outs]
        offs = np.zeros(len(outs) + 1, np.int64)
        offs[1:] = np.cumsum(counts)
        host = torch.from_numpy(np.concatenate([o["image_tiles"] for o in outs], 0))
        tiles = host.pin_memory().to(self.model.device, non_blocking=True) if host.numel() else host.to(self.model.device)
        grids = [tuple(int(x) for x in o["grid_hw"][0]) for o in outs]
        ids = [o["input_ids"][0] for o in outs]
        return tiles, offs, grids, ids

    # ------------------------------------------------------------------------------------------- hot loop
    def prepare_lines(self, flat: dict, math_mode: bool = True) -> dict:
        """Host half of the loop: build prompts, pre-process every crop, upload the tiles (they stay in HBM)."""
        prompts, max_tokens = [], {}
        for idx, (img, txt, task) in enumerate(zip(flat["slices"], flat["input_text"], flat["task_names"])):
            prompts.append(RecognitionPrompt(id=idx, task_name=task, text=txt, image=img, math_mode=math_mode))
            max_tokens[idx] = self.line_budget(task)
        if prompts and isinstance(prompts[0].image, LineRef):
            tiles, tile_offs, grids, prompt_ids = self.preprocess_prompts_device(prompts, flat.get("pages", []))
        else:
            tiles, tile_offs, grids, prompt_ids = self.preprocess_prompts(prompts)
        prep = {"prompts": prompts, "max_tokens": max_tokens, "tiles": tiles, "tile_offs": tile_offs, "grids": grids,
                "prompt_ids": prompt_ids, **options.take(flat)}      # ... and every per-line option of the call: its table, one integer per line
        if flat.get("forced_ids") is not None:                # align(): one forced id list per line
            prep["forced_ids"] = flat["forced_ids"]
            if flat.get("fan"):                               # rank(): a LIST of id lists per line, one slot each behind one prefill
                prep["fan"] = True
        return prep

    def generate(self, prep: dict | None, recognition_batch_size: int | None = None, on_done=None, on_flush=None, feed=None) -> tuple:
        """Device half: one DeviceLoop (loop.py, which documents on_done / on_flush / feed) run until every line stopped (reference
        :501-607). A streamed call states its token budget up front in the first dict (`overall_max_tokens`)."""
        if recognition_batch_size is None:
            recognition_batch_size = self.get_batch_size()
        first = prep if prep is not None else {}
        overall_max_tokens = int(first.get("overall_max_tokens") or max(first["max_tokens"].values()))
        proc = self.processor
        # (keywords only for what is on: a stand-in loop keeps its signature.) `extra`: the one extra output set of the run, if any
        more, extra = ({"alternatives": True}, options.ALTERNATIVES) if self._top_k is not None else ({}, None)
        if first.get("forced_ids") is not None:
            more, extra = ({"forced": True, "fan": True} if first.get("fan") else {"forced": True}), options.FORCED      # rank(): a list of candidates per line
        elif self._beam is not None:
            more, extra = {"beam": self._beam}, None
        extra = options.option_extra(first) or extra
        if first.get("store_mode") is not None:               # encode() / EncodedLines: the lines leave their prompts in the store, or come out of it
            more = dict(more, store=first["store_mode"])
        loop = DeviceLoop(self.model, proc.eos_token_id, proc.pad_token_id, proc.no_output_token,
                          min(recognition_batch_size, self.model.max_slots), overall_max_tokens, self.min_prefill_ratio,
                          on_done=on_done, on_flush=on_flush, feed=feed, **more)
        loop.run(prep)
        # the loop's own dense bookkeeping (ids [n, cap], scores [n, cap], lengths): what the sharded loop packs for its all_gather
        # without walking the per-line lists again
        from ..dist import PackedLines
        self.last_packed = (PackedLines(loop.tok_mat, loop.line_len), PackedLines(loop.sc_mat, loop.line_len))
        if extra is not None:                                 # ... and the extra set's matrices likewise: last_forced / last_boost / last_alternatives
            setattr(self, extra.last, tuple(PackedLines(getattr(loop, f.attr), loop.line_len) for f in extra.fields))
        return loop.predicted_tokens, torch.from_numpy(loop.batch_bboxes), loop.scores

    def prediction_loop(self, flat: dict, recognition_batch_size: int | None = None, math_mode: bool = True) -> tuple:
        return self.generate(self.prepare_lines(flat, math_mode), recognition_batch_size)

    def sharded_prediction_loop(self, flat: dict, recognition_batch_size: int | None = None, math_mode: bool = True) -> tuple:
        """One process per GPU (torch.distributed initialised by the caller, e.g. torchrun), used when `shard_lines` is set:
        every rank holds the same width-sorted line list (verified with a fingerprint all_gather), pre-processes and
        recognises only the lines dealt to it round-robin, and all ranks get all results back through ONE all_gather
        (surya_amd/dist.py). No collective touches the per-step data path. Single process: plain loop."""
        from .. import dist as sdist
        group = self.process_group
        rank, world = sdist.world_info(group)
        slices = flat["slices"]
        n = len(slices)
        if not sdist.collectives_on(group):                  # one rank (unless a forced 1-rank group, dist.force_collectives)
            return self.prediction_loop(flat, recognition_batch_size, math_mode)
        dev = sdist.collective_device(self.model.device, group)
        if n and isinstance(slices[0], LineRef):              # device path: lines are references into the uploaded pages
            probe = [np.asarray([(l.page, l.x0, l.y0, l.x1, l.y1) for l in slices], np.int64).tobytes()]
            probe += [pg.reshape(-1)[:4096].tobytes() for pg in flat.get("pages", [])[:16]]
        else:
            probe = [np.ascontiguousarray(slices[i]).tobytes()[:4096] for i in range(0, n, max(1, n // 16))]
        sdist.assert_same_inputs(inputs_fingerprint([s.shape[:2] for s in slices], probe), group, dev)
        if n == 0:
            return self.prediction_loop(flat, recognition_batch_size, math_mode)
        mine = sdist.shard_indices(n, world, rank)
        local = {k: [flat[k][i] for i in mine] for k in ("slices", "input_text", "task_names")}
        if "pages" in flat:
            local["pages"] = flat["pages"]
        local.update(options.take(flat, mine))                # every rank holds the whole tables; the lines' integers travel with the lines
        max_tokens = max(self.line_budget(t) for t in flat["task_names"])
        # the extra output set that rides in the same collective: a boosted call's plain readings, else the alternatives of top_k
        extra = options.option_extra(flat) or (options.ALTERNATIVES if self._top_k is not None else None)
        more = None
        if mine:
            self.last_packed = None                          # only what generate() sets DURING this call counts (a stand-in prediction_loop
            toks, boxes, scores = self.prediction_loop(local, recognition_batch_size, math_mode)      # must not gather an earlier call's arrays)
            packed = getattr(self, "last_packed", None)
            if packed is not None and len(packed[0]) == len(toks):      # generate()'s dense arrays: no per-token Python in the pack
                toks, scores = packed
            self.last_packed = None                          # (and the [n, cap] matrices are not pinned on the predictor between calls)
            if extra is not None:
                more = getattr(self, extra.last, None)
                setattr(self, extra.last, None)
            boxes = boxes.numpy()
            if boxes.shape[1] < max_tokens:
                boxes = np.pad(boxes, ((0, 0), (0, max_tokens - boxes.shape[1]), (0, 0)))
        else:
            toks, scores, boxes = [], [], np.zeros((0, max_tokens, 6), np.float32)
        if extra is None:
            toks, scores, boxes = sdist.gather_line_outputs(toks, scores, boxes, mine, n, max_tokens, device=dev, group=group)
            return toks, torch.from_numpy(boxes), scores
        # the set's two arrays ride in the collective's [n, T, A] places: the alternatives as they are, the plain readings as one
        # "alternative" per token (boost_words exclude top_k)
        if more is None:
            more = tuple(sdist.PackedLines(a, np.zeros(0, np.int64)) for a in options.empty_rows(extra, 0, (max_tokens,)))
        scalar = not extra.fields[0].tail
        if scalar:
            more = tuple(sdist.PackedLines(pl.data[:, :, None], pl.lens) for pl in more)
        toks, scores, boxes, *more = sdist.gather_line_outputs(toks, scores, boxes, mine, n, max_tokens, device=dev, group=group, alts=tuple(more))
        setattr(self, extra.last, tuple(sdist.PackedLines(pl.data[:, :, 0], pl.lens) if scalar else pl for pl in more))
        return toks, torch.from_numpy(boxes), scores

    # ------------------------------------------------------------------------------------- output assembly
    # (assemble.py; the call paths reach it through these names, so a stand-in set on the instance takes effect)
    def get_bboxes_text(self, flat, predicted_tokens, scores, predicted_polygons, drop_repeated_text=False) -> list:
        return assemble.get_bboxes_text(self.processor, flat, predicted_tokens, scores, predicted_polygons, drop_repeated_text)

    _chars_of = staticmethod(assemble.chars_of)

    def _assemble_line(self, flat, sorted_pos, orig, tokens, sc, bbox_rows, drop_repeated_text, return_words, bbox_size) -> TextLine:
        return assemble.assemble_line(self.processor, flat, sorted_pos, orig, tokens, sc, bbox_rows, drop_repeated_text, return_words, bbox_size)

    def _assemble_batch(self, flat, items, drop_repeated_text, return_words, bbox_size) -> List[TextLine]:
        return assemble.assemble_batch(self.processor, flat, items, drop_repeated_text, return_words, bbox_size)

    @staticmethod
    def _page_results(images, slice_map, text_lines, sort_lines) -> List[OCRResult]:
        """The lines (by original position) regrouped per page."""
        results, start = [], 0
        for image, count in zip(images, slice_map):
            lines = text_lines[start:start + count]
            start += count
            if sort_lines:
                lines = sort_text_lines(lines)
            results.append(OCRResult(text_lines=lines, image_bbox=[0, 0, image.size[0], image.size[1]]))
        return results

    def __call__(self, images: List[Image.Image], task_names: List[str] | None = None, det_predictor=None,
                 detection_batch_size: int | None = None, recognition_batch_size: int | None = None,
                 highres_images: List[Image.Image] | None = None, bboxes: List[List[List[int]]] | None = None,
                 polygons: List[List[List[List[int]]]] | None = None, input_text: List[List[str | None]] | None = None,
                 sort_lines: bool = False, math_mode: bool = True, return_words: bool = False,
                 drop_repeated_text: bool = False, allowlist=None, blocklist=None) -> List[OCRResult]:
        """`self.top_k` (an attribute like `shard_lines`: the call's signature ends with the two lists; None = off, else 2..4): every
        TextChar also carries `alternatives`, the top_k most likely readings of the token it takes its confidence from, best first
        (entry 0 is the character's own), with `allowlist` / `blocklist` the most likely ALLOWED readings. Texts, confidences and boxes
        do not change. Anything else raises ValueError before any device work.

        `allowlist` / `blocklist` (not in the reference; keywords after its own arguments) restrict the characters a line may
        contain -- "0123456789.,-" for a numeric column. Each is a str for every line of the call, or a list with one entry per image:
        None, a str, or a list with one None / str per bbox / polygon of that image (not with det_predictor: the lines are not known
        yet). A line takes one of the two, not both. Tokens and confidences are the reference's process_outputs on logits whose
        disallowed ids are -inf, so a confidence is the softmax over the allowed set; EOS, pad and no-output stay allowed, formatting and
        math tags do not under an allowlist (OCRTokenizer.token_mask). Stop rules, sorting and assembly are unchanged.

        `self.pattern` (an attribute like `top_k`, for the same reason; None = off; the forms of `allowlist`: a str for every line of the
        calls that follow, or one entry per image of the call: None, a str, or a list with one None / str per bbox / polygon) constrains a
        line to a regular expression -- r"\\d{2}/\\d{2}/\\d{4}" for a date column -- with the semantics of re.fullmatch on the line's text
        (recognition/pattern.py documents the supported subset; anything else raises ValueError before any device work). The allowed
        characters then depend on the position in the line: the line follows the pattern's automaton on the device, one step per token,
        with no host round trip. A line takes `pattern` or `allowlist` / `blocklist`, not both; a call may mix lines of either kind and
        unconstrained ones. `TextLine.pattern_matched` is True iff the line ended where the pattern accepts; a line cut by the token
        budget, the repeat rule or the no-output token reports False and keeps its partial text; None without a pattern. Confidences
        are softmax values over the set allowed at that position. `top_k` works with it. ValueError with `beam_width`, and in `align`.

        `self.lexicon` (an attribute like `pattern`; None = off; a list of str for every line of the calls that follow, or one entry per
        image of the call: None, a list of str, or a list with one None / list of str per bbox / polygon) reads a line as exactly one
        entry of a word list -- a city, a surname, a product code, one of the 40 000 postal codes -- with re.fullmatch semantics. Entries
        are taken verbatim: no case folding, no Unicode normalisation, no stripping; duplicates are allowed. The call's lexicons are
        compiled once into a minimised automaton (recognition/lexicon.py; 10^5 entries are fine) that every line follows on the device,
        with no host round trip. A line takes a lexicon, a pattern, or an allowlist / blocklist, never two; a call may mix all of them
        with unconstrained lines. `TextLine.lexicon_index` is the index, in the line's own list, of the entry read (the first for a
        duplicate); -1 for a line cut by the token budget, the repeat rule or the no-output token, which keeps its partial text, a
        proper prefix of an entry; None without a lexicon. `top_k` works with it. ValueError, before any device work, with `beam_width`,
        in `align`, for an empty list, an empty entry and an entry the model's vocabulary cannot write.

        `self.boost_words` (an attribute like `lexicon`, in the same three forms; None = off) PREFERS the entries of a word list -- drug
        names, surnames, part numbers -- without forbidding anything else: wherever the tokens so far could be the beginning of an
        entry that began at a word boundary, the entry's next character gets `self.boost_weight` (logit units, a finite float >= 0,
        required, no default) added to its logit. Entries are verbatim and may hold spaces and punctuation. The line still reads every
        word that is not listed. A boost that was spent on a match that then died is not taken back, so use a moderate weight.
        `TextLine.boost_matches` lists the entries (indices in the line's own list) that were read in full, in order of completion;
        `TextChar.plain` is the character the model would have emitted without the boost, `TextChar.plain_confidence` the emitted
        character's probability without it; confidences are softmax values of the boosted distribution. All three are None on lines
        that are not boosted. Other lines of the call may carry allowlists; a boosted line takes none. ValueError, before any device
        work, with `top_k`, `beam_width`, `pattern` or `lexicon`, without `boost_weight`, and in `align`.

        `self.rectify` (an attribute like `top_k`; None = off, True = every tilted line, or a non-negative threshold in degrees): a line
        that came with a 4-point polygon (`polygons=` or `det_predictor=`, never `bboxes=`) which is strictly convex and clockwise, is not
        an axis-aligned rectangle in canonical order and whose top edge p0 -> p1 is tilted by at least the threshold is warped to an
        upright crop (common/imageops.py: warp_quad) instead of being cut as its bounding rectangle; every other line takes today's path
        with today's bits. The vertex order is the reading direction: a caller who knows a line is vertical or upside down says so with
        the order of its vertices; nothing is guessed. Characters of a warped line are tilted quads on the page, `TextLine.polygon` stays
        the polygon that came in, `TextLine.rectified` says whether the line was warped (None while `rectify` is None). It works with every
        decoding option, dtype and KV mode, and in `align`: nothing behind the image tiles changes. ValueError, before any device work,
        for any other value.

        `self.beam_width` (an attribute like `top_k`; None = greedy, else 2..4): beam search on the device. Every TextLine carries
        `hypotheses`, its up to beam_width best readings as LineHypothesis(text, confidence, log_prob, finished, chars) -- finished
        readings by log_prob descending, then the ones the token budget or the repeat rule cut -- each assembled like a line
        (`drop_repeated_text` and `return_words` apply to each). The TextLine itself is hypothesis 0 and its `log_prob` is set; it is
        the most likely whole reading, which may differ from the greedy one. log_prob is the sum of the tokens' log-probabilities,
        eos included, without length normalisation: comparable with `align`'s. `recognition_batch_size` keeps meaning KV slots, and a
        line takes beam_width of them, so a beam call decodes recognition_batch_size // beam_width lines at a time. `allowlist` /
        `blocklist` work with it (the readings are made of allowed characters). ValueError before any device work for another value,
        together with `top_k` (the alternatives arrays serve the beams), or on a model running MXFP8 decode weights or the fp8 KV cache;
        NotImplementedError with `shard_lines`, `shard_pages` or a process group. With `det_predictor` a beam call detects all pages
        before it recognises (no streamed detection). `align` is unaffected.

        `self.reread` (an attribute like `rectify`; None = off, else a recognition.reread.Reread: `pred.reread = Reread(below=0.6,
        contrast=2, rotations=(180,))`): after the call's lines are read and assembled as always, every DOUBTFUL line -- a non-empty text
        with `confidence < below`, or a pattern / lexicon that was not met -- is read once more per variant, all of them in one more run
        of the loop under the line's own task, input text and per-line options and the call's `top_k` / `beam_width` / `math_mode`:
        "contrast" is the line's own crop (padded, or rectified if the first pass rectified it) after Pillow's
        ImageOps.autocontrast(cutoff=contrast, preserve_tone=True) over the polygon's pixels; "rot90" / "rot180" / "rot270" are the
        line's quad -- the rectangle for a `bboxes=` line -- with its vertex list rolled by 1 / 2 / 3, read through the rectify path whatever
        `rectify` says (a polygon that is no rectifiable quad gets none). Candidates are the first reading, then the variants in that
        order; the winner meets its constraint (where the line has one), has a non-empty text, then the highest confidence, the earlier
        one on a tie, and its whole TextLine takes the line's place (`polygon` stays the one that came in; a turned winner's characters
        are tilted quads on the page). `TextLine.variant` names the winner, `TextLine.readings` lists every candidate of a line that was
        re-read as LineReading(variant, text, confidence); both are None while `reread` is None. `last_timing` gains `reread_ms` and
        `reread_lines`. TypeError / ValueError for a bad value, NotImplementedError with `shard_lines`, `shard_pages` or a process group,
        before any device work; ValueError naming `reread` in `align`, `rank`, `encode` and the methods of EncodedLines: a stored prompt
        holds no pixels to adjust or turn.

        `self.unroll` (an attribute like `rectify`; None = off, or True): a line that carries a CENTRE LINE is read from its unrolled crop
        (common/imageops.py: curve_table, warp_columns -- the band of `thickness` around the centre line, sampled column by column along
        the arc length) instead of its bounding rectangle or its rectified quad; every other line is handled as always. The centre line
        comes with the detection (`det_predictor=` whose `centerlines` is set: TextBox.centerline / .thickness) or with
        `self.centerlines` (an attribute like `pattern`, for the same reason: the call's signature ends with the two lists), a list
        parallel to `polygons=` -- one list per image, one entry per polygon: None or (points, thickness) in page pixels, points ordered in
        reading direction. Characters of an unrolled line are tilted quads that follow the bend, `TextLine.polygon` stays the polygon that came
        in, `TextLine.unrolled` says whether the line was unrolled (None while `unroll` is None). It works with every decoding option,
        dtype and KV mode: nothing behind the image tiles changes. A turned `reread` variant of an unrolled line reads the line's quad as
        always. ValueError, before any device work, for another value of `unroll`, for `centerlines` without `polygons=` or of another
        shape, and, naming the line, for a centre line with fewer than two points, a non-finite value, a zero-length segment or a
        non-positive thickness."""
        top_k, beam, pattern, lexicon, boost_words, boost_weight = self._checked_modes()
        setting = rereading.checked(self.reread)
        if setting is not None and (self.shard_lines or self.shard_pages or self.process_group is not None):
            raise NotImplementedError("a call with reread runs on one rank: unset shard_lines / shard_pages / process_group")
        given = self._checked_centerlines(self.centerlines, images, polygons)
        with self._modes(top_k, beam, setting):
            self._curves_given = given
            try:
                return self._call_gc_paused(images, task_names, det_predictor, detection_batch_size, recognition_batch_size, highres_images,
                                            bboxes, polygons, input_text, sort_lines, math_mode, return_words, drop_repeated_text, allowlist,
                                            blocklist, pattern, lexicon, boost_words, boost_weight)
            finally:
                self._curves_given = None

    def _checked_modes(self) -> tuple:
        """The attributes a reading call runs under -- (top_k, beam_width, pattern, lexicon, boost_words, boost_weight) -- validated as
        `__call__` documents, before any device work."""
        top_k = self.top_k
        if top_k is not None and (isinstance(top_k, bool) or not isinstance(top_k, int) or not 2 <= top_k <= 4):
            raise ValueError(f"top_k must be None or an integer in 2..4, got {top_k!r}")
        beam = self._check_beam_width(top_k)
        rectify_threshold(self.rectify)                       # ValueError for a bad value, before any device work
        self._unroll_on()
        pattern = self.pattern
        if pattern is not None and beam is not None:
            raise ValueError("pattern is not available with beam_width: a beam would have to inherit its parent's automaton state")
        lexicon = self.lexicon
        if lexicon is not None and beam is not None:
            raise ValueError("lexicon is not available with beam_width: a beam would have to inherit its parent's automaton state and row")
        boost_words, boost_weight = self.boost_words, self.boost_weight
        if boost_words is not None:
            for name, v in (("top_k", top_k), ("beam_width", beam), ("pattern", pattern), ("lexicon", lexicon)):
                if v is not None:
                    raise ValueError(f"boost_words is not available with {name}: the boosted head runs the masked and the plain greedy "
                                     f"lm_head epilogues and owns the slot's mask row")
            if boost_weight is None:
                raise ValueError("boost_words needs boost_weight, the boost in logit units (a finite float >= 0); it has no default")
            if isinstance(boost_weight, bool) or not isinstance(boost_weight, (int, float)) or not 0 <= boost_weight < float("inf"):
                raise ValueError(f"boost_weight must be a finite float >= 0, got {boost_weight!r}")
        return top_k, beam, pattern, lexicon, boost_words, boost_weight

    @contextmanager
    def _modes(self, top_k=None, beam=None, reread=None):
        """The validated top_k and beam_width for the length of a call: `_call`, `generate` and the loops are reached positionally by the
        page-sharded path and by stand-ins and read them from here. align() and rank() park both: they report `greedy`, not
        alternatives, and one reading, the given one, whatever beam_width says."""
        saved = self._top_k, self._beam, self._reread
        self._top_k, self._beam, self._reread = top_k, beam, reread
        try:
            yield
        finally:
            self._top_k, self._beam, self._reread = saved
            if top_k is not None:
                self.last_alternatives = None

    def _unroll_on(self) -> bool:
        """`self.unroll` validated (None or True); ValueError for anything else, before any device work."""
        if self.unroll is not None and self.unroll is not True:
            raise ValueError(f"unroll must be None or True, got {self.unroll!r}")
        return self.unroll is True

    def _checked_centerlines(self, centerlines, images, polygons):
        """`self.centerlines` for a call as per-image lists of None / Curve; ValueError naming the line, before any device work."""
        if centerlines is None:
            return None
        if polygons is None:
            raise ValueError("centerlines goes with polygons=: one entry (None, or (points, thickness)) per polygon")
        if len(centerlines) != len(images) or any(len(c) != len(pl) for c, pl in zip(centerlines, polygons)):
            raise ValueError("centerlines needs one list per image with one entry per polygon of that image")
        return [[checked_curve(f"image {i}, line {k}", c) for k, c in enumerate(page)] for i, page in enumerate(centerlines)]

    def _check_beam_width(self, top_k):
        """`self.beam_width` validated for a call (None: off), before any device work."""
        beam = self.beam_width
        if beam is None:
            return None
        if isinstance(beam, bool) or not isinstance(beam, int) or not 2 <= beam <= 4:
            raise ValueError(f"beam_width must be None or an integer in 2..4, got {beam!r}")
        if top_k is not None:
            raise ValueError("beam_width and top_k exclude each other: the alternatives arrays serve the beams")
        if self.shard_lines or self.shard_pages or self.process_group is not None:
            raise NotImplementedError("a beam-search call runs on one rank: unset shard_lines / shard_pages / process_group")
        if getattr(self.model, "decode_fp8", False):
            raise ValueError("beam_width is not available with MXFP8 decode weights (RECOGNITION_DECODE_FP8 / set_decode_fp8)")
        if getattr(self.model, "kv_fp8", False):
            raise ValueError("beam_width is not available with the fp8 KV cache (RECOGNITION_KV_FP8 / set_kv_fp8)")
        return beam

    def forced_ids(self, text: str, task: str) -> List[int]:
        """The ids `align` forces for one line: the tokenizer's ids of the text for the line's task, then eos."""
        return [int(t) for t in self.processor.ocr_tokenizer(text, task)["input_ids"][0]] + [int(self.processor.eos_token_id)]

    def _forced_call_checks(self, what, arg, arg_lists, images, per_line, task_names, bboxes, polygons):
        """What `align` and `rank` refuse before any device work; -> (the bbox / polygon lists, the task names)."""
        rectify_threshold(self.rectify)                       # ValueError for a bad value, before any device work
        if self.reread is not None:
            raise ValueError(f"reread does not apply to {what}(): the text is given, there is no reading to doubt (set reread = None)")
        if self.pattern is not None:
            raise ValueError(f"pattern does not apply to {what}(): forced decoding reads no allowed set (set pattern = None)")
        if self.lexicon is not None:
            raise ValueError(f"lexicon does not apply to {what}(): forced decoding reads no allowed set (set lexicon = None)")
        if self.boost_words is not None:
            raise ValueError(f"boost_words do not apply to {what}(): the text is given, there is nothing to prefer (set boost_words = None)")
        if getattr(self, "_poisoned", None):
            raise RuntimeError(self._poisoned)
        if self.shard_lines or self.shard_pages or self.process_group is not None:
            raise NotImplementedError(f"{what}() runs on one rank: unset shard_lines / shard_pages / process_group")
        given = polygons if polygons is not None else bboxes
        if given is None:
            raise ValueError(f"{what}() needs bboxes or polygons: the lines the {arg} belong to")
        if task_names is None:
            task_names = [TaskNames.ocr_with_boxes] * len(images)
        if not (len(images) == len(per_line) == len(given) == len(task_names)):
            raise ValueError(f"{what}(): {len(images)} images, {len(per_line)} {arg_lists}, {len(given)} bbox / polygon lists, {len(task_names)} task names")
        for t in task_names:
            if t not in self.tasks:
                raise ValueError(f"task {t!r} is not supported. Supported tasks are {list(self.tasks)}")
        return given, task_names

    def _forced_line_ids(self, where, text, task) -> List[int]:
        """`forced_ids` of one text of a line of `task`, checked against the budget, SA_MAX_FORCED_TOKENS and the vocabulary."""
        from .. import _lib as L
        if not isinstance(text, str):
            raise ValueError(f"{where}: the text must be a str, got {type(text).__name__}")
        ids = self.forced_ids(text, task)
        budget, vocab = self.line_budget(task), getattr(self.model, "vocab", None)
        if len(ids) > budget:
            raise ValueError(f"{where}: {len(ids)} tokens (eos included) exceed the token budget {budget} of task {task}")
        if len(ids) > L.SA_MAX_FORCED_TOKENS:
            raise ValueError(f"{where}: {len(ids)} tokens exceed SA_MAX_FORCED_TOKENS = {L.SA_MAX_FORCED_TOKENS}")
        if vocab is not None and max(ids) >= vocab:
            raise ValueError(f"{where}: token id {max(ids)} is outside the model's vocabulary of {vocab}")
        return ids

    def align(self, images: List[Image.Image], texts: List[List[str]], task_names: List[str] | None = None,
              bboxes: List[List[List[int]]] | None = None, polygons: List[List[List[List[int]]]] | None = None,
              recognition_batch_size: int | None = None, math_mode: bool = True, return_words: bool = False) -> List[OCRResult]:
        """Align known transcriptions: texts[i][j] is the text of image i's j-th bbox / polygon (one of the two is required). Every
        line is decoded with its own tokens forced (`forced_ids`) instead of the model's choices, so the result holds the GIVEN text,
        read back through the tokenizer, with per-character polygons predicted from the forced prefix and per-character `confidence`
        = p(character | image, preceding text); a line's `confidence` is computed as in `__call__`. Two more fields:
        `TextLine.log_prob`, the sum of the log-probabilities of the line's tokens, eos included (p(eos | text) says whether the model
        thinks the line is complete), and `TextChar.greedy`, the model's own reading (text, probability, token id) at the token the
        character takes its confidence from -- the character itself where the model agrees. ValueError, naming image and line, for
        a count mismatch, a line longer than its task's token budget or than SA_MAX_FORCED_TOKENS, or an id outside the model's
        vocabulary. Not with `shard_lines` or a process group: multi-rank alignment is not supported. Allow-lists and `top_k`
        do not apply to an aligned call, and a set `pattern` raises ValueError: the text is given, there is nothing to constrain."""
        given, task_names = self._forced_call_checks("align", "texts", "text lists", images, texts, task_names, bboxes, polygons)
        forced = self._align_forced(texts, given, task_names)
        with self._modes(), gc_paused():
            return self._align(convert_if_not_rgb(images), forced, task_names, bboxes, polygons, recognition_batch_size, math_mode, return_words)

    def _align_forced(self, texts, given, task_names) -> list:
        """The forced id list of every line of an `align` call, in page order; `given` holds one entry per line and image."""
        forced = []
        for i, (tx, gv, task) in enumerate(zip(texts, given, task_names)):
            if len(tx) != len(gv):
                raise ValueError(f"image {i} has {len(gv)} lines but {len(tx)} texts")
            for j, text in enumerate(tx):
                forced.append(self._forced_line_ids(f"image {i}, line {j}", text, task))
        return forced

    def _align(self, images, forced, task_names, bboxes, polygons, recognition_batch_size, math_mode, return_words) -> List[OCRResult]:
        flat = self.slice_bboxes(images, bboxes=bboxes, polygons=polygons, input_text=None, task_names=task_names)
        return self._align_flat(images, flat, forced, recognition_batch_size, return_words, lambda f: self.prepare_lines(f, math_mode))

    def _align_flat(self, images, flat, forced, recognition_batch_size, return_words, prepare) -> List[OCRResult]:
        """`align` from the sliced lines on. `images`: anything with `.size` per page; `prepare(flat)`: the loop's dict of the lines
        (prepare_lines, or EncodedLines' dict of restored lines, which sorts flat["enc_ids"] with the slices)."""
        t_call = time.perf_counter()
        stamps = self.last_timing = {}
        if len(flat["slices"]) == 0:
            return []
        flat["forced"], flat["forced_ids"] = True, forced     # by line id like the slices: sorted with them below
        order = sorted(range(len(flat["slices"])), key=lambda i: -flat["slices"][i].shape[1])
        for key in ("slices", "input_text", "task_names", "forced_ids") + (("enc_ids",) if "enc_ids" in flat else ()):
            flat[key] = [flat[key][i] for i in order]
        with AssemblyHandover(self, flat, order, False, return_words) as hand:
            t0 = time.perf_counter()
            prep = prepare(flat)
            t1 = time.perf_counter()
            self.generate(prep, recognition_batch_size, on_done=hand.on_done, on_flush=hand.on_flush)
            stamps["prepare_ms"] = (t1 - t0) * 1e3
            text_lines = hand.finish(stamps, t1)
        results = self._page_results(images, flat["slice_map"], text_lines, False)
        stamps["total_ms"] = (time.perf_counter() - t_call) * 1e3
        return results

    def rank(self, images: List[Image.Image], candidates: List[List[List[str]]], task_names: List[str] | None = None,
             bboxes: List[List[List[int]]] | None = None, polygons: List[List[List[List[int]]]] | None = None,
             recognition_batch_size: int | None = None, math_mode: bool = True) -> List[RankResult]:
        """Rank candidate texts: candidates[i][j] is the non-empty list of texts the caller holds for image i's j-th bbox / polygon (one
        of the two is required). Every line is encoded and prefilled ONCE and takes one KV slot per distinct candidate, each forced to
        its candidate's `forced_ids` as in `align`; equal id lists within a line are scored once and reported at every index that named
        them. The result holds, per line, RankedCandidate(index, text, log_prob, n_tokens, probability, greedy_match) sorted by
        log_prob descending, then index ascending, and `best`, the caller's index of the first: log_prob is `align`'s
        TextLine.log_prob for the same line and text, probability its softmax over the line's distinct candidates. No characters,
        polygons or words are assembled. ValueError, naming image and line, as in `align`, and for an empty candidate list or a line
        with more distinct candidates than the slots in use (min(recognition_batch_size, the model's slots): one line is not split over
        several prefills); a set `pattern` / `lexicon` / `boost_words` raises ValueError too. Not with `shard_lines` or a process group.
        `rectify` applies; `top_k` and `beam_width` do not."""
        given, task_names = self._forced_call_checks("rank", "candidates", "candidate lists", images, candidates, task_names, bboxes, polygons)
        lines = self._rank_candidates(candidates, given, task_names, recognition_batch_size)
        with self._modes(), gc_paused():
            return self._rank(convert_if_not_rgb(images), lines, task_names, bboxes, polygons, recognition_batch_size, math_mode)

    def _rank_candidates(self, candidates, given, task_names, recognition_batch_size) -> list:
        """Per line of a `rank` call, in page order: (its texts, its distinct id lists, text index -> distinct index)."""
        slots = recognition_batch_size if recognition_batch_size is not None else self.get_batch_size()
        slots = min(slots, self.model.max_slots)
        lines = []                                            # per line: (its texts, its distinct id lists, text index -> distinct index)
        for i, (cs, gv, task) in enumerate(zip(candidates, given, task_names)):
            if len(cs) != len(gv):
                raise ValueError(f"image {i} has {len(gv)} lines but {len(cs)} candidate lists")
            for j, texts in enumerate(cs):
                if isinstance(texts, str) or len(texts) == 0:
                    raise ValueError(f"image {i}, line {j}: the candidates must be a non-empty list of str")
                distinct, where, index = [], {}, []
                for k, text in enumerate(texts):
                    ids = self._forced_line_ids(f"image {i}, line {j}, candidate {k}", text, task)
                    if tuple(ids) not in where:
                        where[tuple(ids)] = len(distinct)
                        distinct.append(ids)
                    index.append(where[tuple(ids)])
                if len(distinct) > slots:
                    raise ValueError(f"image {i}, line {j}: {len(distinct)} distinct candidates exceed the {slots} slots in use "
                                     f"(recognition_batch_size / the model's slots)")
                lines.append((list(texts), distinct, index))
        return lines

    def _rank(self, images, lines, task_names, bboxes, polygons, recognition_batch_size, math_mode) -> List[RankResult]:
        flat = self.slice_bboxes(images, bboxes=bboxes, polygons=polygons, input_text=None, task_names=task_names)
        return self._rank_flat(images, flat, lines, recognition_batch_size, lambda f: self.prepare_lines(f, math_mode))

    def _rank_flat(self, images, flat, lines, recognition_batch_size, prepare) -> List[RankResult]:
        """`rank` from the sliced lines on; `images` and `prepare` as in `_align_flat`."""
        t_call = time.perf_counter()
        stamps = self.last_timing = {}
        n = len(flat["slices"])
        assert n == len(lines)
        scored = {}                                           # sorted position -> per distinct candidate (greedy ids, probabilities, log-probabilities)
        if n:
            flat["forced_ids"], flat["fan"] = [ln[1] for ln in lines], True      # by line id like the slices: sorted with them below
            order = sorted(range(n), key=lambda i: -flat["slices"][i].shape[1])
            for key in ("slices", "input_text", "task_names", "forced_ids") + (("enc_ids",) if "enc_ids" in flat else ()):
                flat[key] = [flat[key][i] for i in order]
            t0 = time.perf_counter()
            prep = prepare(flat)
            t1 = time.perf_counter()
            self.generate(prep, recognition_batch_size, on_done=scored.__setitem__)
            stamps.update(prepare_ms=(t1 - t0) * 1e3, device_loop_ms=(time.perf_counter() - t1) * 1e3)
            assert len(scored) == n
        rankings = [None] * n
        for k in range(n):
            o = order[k]
            texts, distinct, index = lines[o]
            lp = np.asarray([np.sum(np.asarray(r[2], np.float64)) for r in scored[k]], np.float64)     # set_log_prob's sum
            e = np.exp(lp - lp.max())
            prob = e / e.sum()
            match = [len(r[0]) == len(ids) and bool(np.array_equal(np.asarray(r[0], np.int64), np.asarray(ids, np.int64)))
                     for r, ids in zip(scored[k], distinct)]
            cands = [RankedCandidate(index=c, text=texts[c], log_prob=float(lp[d]), n_tokens=len(distinct[d]), probability=float(prob[d]),
                                     greedy_match=match[d]) for c, d in enumerate(index)]
            cands.sort(key=lambda r: (-r.log_prob, r.index))
            rankings[o] = LineRanking(polygon=flat["polygons"][o], candidates=cands, best=cands[0].index)
        results, start = [], 0
        for image, count in zip(images, flat["slice_map"]):
            results.append(RankResult(lines=rankings[start:start + count], image_bbox=[0, 0, image.size[0], image.size[1]]))
            start += count
        stamps["total_ms"] = (time.perf_counter() - t_call) * 1e3
        return results

    def encode(self, images: List[Image.Image], task_names: List[str] | None = None, bboxes: List[List[List[int]]] | None = None,
               polygons: List[List[List[List[int]]]] | None = None, input_text: List[List[str | None]] | None = None,
               highres_images: List[Image.Image] | None = None, math_mode: bool = True, recognition_batch_size: int | None = None,
               det_predictor=None):
        """Encode lines once and keep them on the device: the lines are sliced (honouring `self.rectify`), resized, patchified, run through
        the vision encoder and prefilled as in `__call__`, and every prompt's KV rows stay in the model's prompt store. The result, an
        EncodedLines (recognition/encoded.py), reads (`enc.read`), ranks (`enc.rank`) and aligns (`enc.align`) those lines as often as
        asked, all of them or a subset (`lines=`), with the results of `__call__` / `rank` / `align` on the same inputs bit for bit, and
        without the encoder and the prefill. It holds device memory (about the prompt's rows per line) until `release()`, the end of its
        `with` block, or its collection. `highres_images` is accepted and unused, as in `__call__` with bboxes or polygons. ValueError, before
        any device work, with `det_predictor` (run the detector and pass `polygons=`) and on a model running the fp8 KV cache;
        NotImplementedError with `shard_lines`, `shard_pages` or a process group."""
        from .encoded import EncodedLines
        return EncodedLines.encode(self, images, task_names, bboxes, polygons, input_text, math_mode, recognition_batch_size, det_predictor)

    top_k: int | None = None          # alternatives per character (2..4), None = off: RecognitionPredictor.top_k = 3, or on an instance
    _top_k = None                     # the running call's validated top_k (see __call__)
    beam_width: int | None = None     # readings per line (2..4), None = greedy: RecognitionPredictor.beam_width = 3, or on an instance
    _beam = None                      # the running call's validated beam_width (see __call__)
    pattern = None                    # regex per call / image / line (see __call__), None = off: set on an instance, e.g. pred.pattern = r"\d+"
    lexicon = None                    # word list per call / image / line (see __call__), None = off: pred.lexicon = ["Alabama", "Alaska", ...]
    boost_words = None                # word list per call / image / line to PREFER (see __call__), None = off: pred.boost_words = ["Paracetamol", ...]
    boost_weight = None               # ... and the boost in logit units, a finite float >= 0: required with boost_words, no default
    rectify = None                    # warp tilted 4-point polygons upright (see __call__): None = off, True, or a threshold in degrees: pred.rectify = 2.0
    unroll = None                     # read bent lines from crops unrolled along their centre lines (see __call__): None = off, or True
    centerlines = None                # centre lines given with `polygons=` (see __call__): per image a list with None or (points, thickness) per polygon
    _curves_given = None              # the running call's validated `centerlines` (see __call__): per image, per line None or a Curve
    reread = None                     # re-read doubtful lines as other pictures (see __call__): None = off, or Reread(below=0.6, contrast=2, rotations=(180,))
    _reread = None                    # the running call's validated Reread (see __call__)
    last_boost = None
    last_alternatives = None
    last_forced = None                # align(): (greedy ids, greedy probabilities, forced log-probabilities) per line id, like last_packed

    def _call_gc_paused(self, images, task_names, det_predictor, detection_batch_size, recognition_batch_size, highres_images,
                        bboxes, polygons, input_text, sort_lines, math_mode, return_words, drop_repeated_text, allowlist, blocklist,
                        pattern=None, lexicon=None, boost_words=None, boost_weight=None):
        # the whole call runs with the cyclic GC paused (gc_paused): slicing, scheduling and assembly allocate ~10^6 acyclic objects
        with gc_paused():
            return self._call(images, task_names, det_predictor, detection_batch_size, recognition_batch_size, highres_images,
                              bboxes, polygons, input_text, sort_lines, math_mode, return_words, drop_repeated_text,
                              **given_lists(allowlist, blocklist, pattern, lexicon, boost_words, boost_weight))

    def _constraints(self, allowlist, blocklist, images, bboxes, polygons, pattern=None, lexicon=None, boost_words=None):
        """The call's LineConstraints, or None for a call without lists, patterns, lexicons or boost_words (or whose entries are all None)."""
        if allowlist is None and blocklist is None and pattern is None and lexicon is None and boost_words is None:
            return None
        given = polygons if polygons is not None else bboxes
        if given is not None and len(given) != len(images):
            raise ValueError("You need to pass in one list of bboxes / polygons for each image")
        counts = None if given is None else [len(g) for g in given]
        from .. import _lib as L
        cons = LineConstraints(self.processor.ocr_tokenizer, allowlist, blocklist, len(images), counts,
                               vocab_size=getattr(self.model, "vocab", None), limit=L.SA_MAX_TOKEN_MASKS, pattern=pattern,
                               lexicon=lexicon, boost_words=boost_words)
        return cons if cons else None

    def _call(self, images, task_names, det_predictor, detection_batch_size, recognition_batch_size, highres_images, bboxes,
              polygons, input_text, sort_lines, math_mode, return_words, drop_repeated_text, allowlist=None, blocklist=None,
              pattern=None, lexicon=None, boost_words=None, boost_weight=None) -> List[OCRResult]:
        if getattr(self, "_poisoned", None):
            raise RuntimeError(self._poisoned)
        allowed = self.tasks.keys()
        t_call = time.perf_counter()
        stamps = self.last_timing = {}                    # wall-clock phases of this call in ms (bench.py's e2e leg reports them)
        if task_names is None:
            task_names = [TaskNames.ocr_with_boxes] * len(images)
        assert all(t in allowed for t in task_names), (
            f"One or more tasks in {task_names} is not supported. Supported tasks are {allowed}")
        assert len(images) == len(task_names), "You need to pass in one task name for each image"
        images = convert_if_not_rgb(images)
        if highres_images is not None:
            assert len(images) == len(highres_images), "You need to pass in one highres image for each image"
        highres_images = convert_if_not_rgb(highres_images) if highres_images is not None else [None] * len(images)
        cons = self._constraints(allowlist, blocklist, images, bboxes, polygons, pattern, lexicon, boost_words)
        if cons is not None and cons.boost is not None:
            cons.boost_weight = float(boost_weight)

        if bboxes is None and polygons is None:
            assert det_predictor is not None, (
                "You need to pass in a detection predictor if you don't provide bboxes or polygons")
            if self.shard_pages:
                from .. import dist as sdist
                if sdist.collectives_on(self.process_group):
                    # (lists whose entries are all None -- no `cons` -- are no lists)
                    lists = {} if cons is None else given_lists(allowlist, blocklist, pattern, lexicon, boost_words, boost_weight)
                    return self._call_page_sharded(images, task_names, det_predictor, detection_batch_size, recognition_batch_size,
                                                   highres_images, sort_lines, math_mode, return_words, drop_repeated_text, **lists)
            if self._can_stream(det_predictor):
                return self._call_streamed(images, task_names, det_predictor, detection_batch_size, recognition_batch_size,
                                           highres_images, sort_lines, math_mode, return_words, drop_repeated_text, stamps, t_call, cons=cons)
            flat = self.detect_and_slice_bboxes(images, task_names, det_predictor, detection_batch_size, highres_images)
            if self._reread is not None:                      # the second pass cuts from the images the first pass cut from
                flat["reread_from"] = ([hr if hr is not None else im for im, hr in zip(images, highres_images)], "poly")
        else:
            if bboxes is not None:
                assert len(images) == len(bboxes), "You need to pass in one list of bboxes for each image"
            if polygons is not None:
                assert len(images) == len(polygons), "You need to pass in one list of polygons for each image"
            flat = self.slice_bboxes(images, bboxes=bboxes, polygons=polygons, input_text=input_text, task_names=task_names)
            if self._reread is not None:
                flat["reread_from"] = (images, "poly" if polygons is not None else "bbox")
        return self._read_flat(images, flat, cons, recognition_batch_size, sort_lines, return_words, drop_repeated_text, stamps, t_call,
                               lambda f: self.prepare_lines(f, math_mode), math_mode)

    def _read_flat(self, images, flat, cons, recognition_batch_size, sort_lines, return_words, drop_repeated_text, stamps, t_call, prepare,
                   math_mode=True) -> List[OCRResult]:
        """`_call` from the sliced lines on; `images` and `prepare` as in `_align_flat` (`math_mode` reaches the line-sharded loop only,
        which prepares its own share)."""
        if len(flat["slices"]) == 0:
            return []
        stamps["slice_ms"] = (time.perf_counter() - t_call) * 1e3
        if self._top_k is not None:
            flat["top_k"] = self._top_k
        sorted_keys = ("slices", "input_text", "task_names") + (("enc_ids",) if "enc_ids" in flat else ())
        if cons is not None:                                  # the options' integers are by line id like the slices: sorted with them below
            sorted_keys += options.attach(flat, cons)
        else:                                                 # (a second pass brings its lines' integers with it: reread.second_pass)
            sorted_keys += tuple(o.line_key for o in options.requested(flat) if o.line_key in flat)

        # widest first: the length bucketing that keeps prefill batches homogeneous (reference :847-854); `order[k]` is the original
        # position of sorted line k, so a finished line can be assembled against its own polygon / scale
        order = sorted(range(len(flat["slices"])), key=lambda i: -flat["slices"][i].shape[1])
        for key in sorted_keys:
            flat[key] = [flat[key][i] for i in order]

        with AssemblyHandover(self, flat, order, drop_repeated_text, return_words) as hand:
            if self.shard_lines:
                predicted_tokens, batch_bboxes, scores = self.sharded_prediction_loop(flat, recognition_batch_size, math_mode)
                bb = batch_bboxes.numpy()
                chunks = [range(a, min(a + 256, len(order))) for a in range(0, len(order), 256)]
                la = self.last_alternatives if self._top_k is not None else None
                if options.option_extra(flat) is not None:    # an option's own extra set (the plain readings) travels like the alternatives
                    last = options.option_extra(flat).last
                    la = getattr(self, last, None)
                    setattr(self, last, None)
                alt_of = (lambda k: ()) if la is None else (lambda k: ((la[0].row(k), la[1].row(k)),))
                text_lines = hand.place((ks, hand.assemble([(k, predicted_tokens[k], scores[k], bb[k]) + alt_of(k) for k in ks])) for ks in chunks)
            else:
                t0 = time.perf_counter()
                prep = prepare(flat)
                t1 = time.perf_counter()
                self.generate(prep, recognition_batch_size, on_done=hand.on_done, on_flush=hand.on_flush)
                stamps["prepare_ms"] = (t1 - t0) * 1e3
                text_lines = hand.finish(stamps, t1)
        if self._reread is not None and flat.get("reread_from") is not None:
            text_lines = rereading.second_pass(self, self._reread, flat, order, text_lines, *flat["reread_from"], recognition_batch_size,
                                               return_words, drop_repeated_text, math_mode, stamps)
        results = self._page_results(images, flat["slice_map"], text_lines, sort_lines)
        stamps["total_ms"] = (time.perf_counter() - t_call) * 1e3
        return results

    # ---------------------------------------------------------------------- N > 1: whole pages per rank
    # `shard_lines` deals the LINES of every page over the ranks: every rank detects its share of pages, but then slices, sorts and
    # -- after the all_gather of the token outputs -- assembles ALL lines of ALL pages, so the host work of a call does not shrink with
    # the rank count (128 pages over 8 ranks: ~355 lines of device work per rank against ~2800 lines of assembly on each; VERDICT r04
    # weak #7b), and the streamed detect -> recognise schedule is off. `shard_pages` deals whole PAGES instead: rank r takes pages
    # r, r + world, ... and runs the complete single-rank call on them -- streamed, its own detector batches feeding its own
    # continuous-batching loop, its own assembly -- with no collective on the data path at all. One gather at the end:
    #   gather_page_results = True   every rank gets every page's OCRResult (the drop-in contract; pickled result objects, host cost
    #                                grows with the page count)
    #   gather_page_results = False  results stay partitioned: a rank returns OCRResults for its own pages and None elsewhere; the
    #                                gather carries one small record per page (line count, character count, CRC of the text) so every
    #                                rank can check that each page was processed exactly once (`last_page_summary`)
    shard_pages: bool = False
    gather_page_results: bool = True

    def _call_page_sharded(self, images, task_names, det_predictor, detection_batch_size, recognition_batch_size, highres_images,
                           sort_lines, math_mode, return_words, drop_repeated_text, allowlist=None, blocklist=None, pattern=None,
                           lexicon=None, boost_words=None, boost_weight=None) -> list:
        from .. import dist as sdist
        group = self.process_group
        rank, world = sdist.world_info(group)
        n = len(images)
        dev = sdist.collective_device(self.model.device, group)
        # (a 64 x 16 pixel corner of up to 16 pages: `tobytes()` of whole pages copied several MB per page on every rank, inside the call)
        probe = [images[i].crop((0, 0, min(images[i].size[0], 64), min(images[i].size[1], 16))).tobytes() for i in range(0, n, max(1, n // 16))]
        sdist.assert_same_inputs(inputs_fingerprint([im.size for im in images], probe), group, dev)
        mine = sdist.shard_indices(n, world, rank)
        saved = (self.shard_pages, self.shard_lines, getattr(det_predictor, "shard_pages", False))
        self.shard_pages = self.shard_lines = False
        if hasattr(det_predictor, "shard_pages"):
            det_predictor.shard_pages = False
        # a rank compiles the lists of its own pages (beta is the call's); a call without lists reaches the rank's own call exactly as
        # it always did
        lists = {k: v if k == "boost_weight" else list_for_pages(k, v, n, mine)
                 for k, v in given_lists(allowlist, blocklist, pattern, lexicon, boost_words, boost_weight).items()}
        try:
            hr = [highres_images[i] for i in mine]
            local = self._call([images[i] for i in mine], [task_names[i] for i in mine], det_predictor, detection_batch_size,
                               recognition_batch_size, hr if any(h is not None for h in hr) else None,
                               None, None, None, sort_lines, math_mode, return_words, drop_repeated_text, **lists) if mine else []
        finally:
            self.shard_pages, self.shard_lines = saved[0], saved[1]
            if hasattr(det_predictor, "shard_pages"):
                det_predictor.shard_pages = saved[2]
        if len(local) != len(mine):
            # the single-rank call returns [] when its pages hold no line at all (reference contract, :928-929); this rank's pages then
            # exist all the same: one empty OCRResult per page, so the gather below has an entry for every page of the whole call
            # (a rank dealt only blank pages made those pages None on every rank / tripped the processed-once assert)
            assert len(local) == 0, (len(local), len(mine))
            local = [OCRResult(text_lines=[], image_bbox=[0, 0, images[i].size[0], images[i].size[1]]) for i in mine]
        if self.gather_page_results:
            out = sdist.gather_objects(local, mine, n, group)
            # ... and the call as a whole keeps the single-rank contract: no line anywhere -> []
            return out if any(r is not None and len(r.text_lines) for r in out) else []
        rec = [(len(r.text_lines), sum(len(l.text) for l in r.text_lines), zlib.crc32("\n".join(l.text for l in r.text_lines).encode()))
               for r in local]
        self.last_page_summary = sdist.gather_objects(rec, mine, n, group)
        assert all(x is not None for x in self.last_page_summary), "a page was processed by no rank"
        if not any(x[0] for x in self.last_page_summary):
            return []                                         # no line on any page of the call: the single-rank contract
        out = [None] * n
        for i, r in zip(mine, local):
            out[i] = r
        return out

    # ---------------------------------------------------------------------- streamed detect -> recognise
    # One call, two threads: a producer runs the detector batch by batch (DetectionPredictor.iter_detect) and turns each
    # batch's boxes into a prepared chunk of lines (LineRefs, width sort within the chunk, device pre-processing, prompt ids);
    # the calling thread runs the continuous-batching loop and admits a chunk as soon as it exists, so the recogniser decodes the
    # first pages' lines while the detector still works on the later pages. Both threads launch on the same HIP stream (device
    # work is ordered by submission, no cross-stream hand-off), each waits only on its own events. The reference detects every
    # page before the first crop is recognised (recognition/__init__.py:371-399, 836-845); the order of the work does not enter
    # any result: a line's tokens do not depend on its slot or batch mates, and results are re-assembled by original position.
    stream_detection: bool = settings.RECOGNITION_STREAM_DETECTION

    def _can_stream(self, det_predictor) -> bool:
        """This package's detector on its device post-processing path, one process, and a `__call__` nobody overrode (a subclass that
        filters or edits the results in `__call__` must keep seeing every page before the first crop is cut: serial path)."""
        from ..detection.predictor import DetectionPredictor
        return (self.stream_detection and self.device_preprocess and not self.shard_lines and self._beam is None      # (a beam call: serial)
                and isinstance(det_predictor, DetectionPredictor)
                and type(det_predictor).__call__ is DetectionPredictor.__call__ and type(det_predictor)._call is DetectionPredictor._call
                and type(det_predictor).iter_detect is DetectionPredictor.iter_detect
                # ... nor the pieces iter_detect is made of: a subclass that customises them for __call__ would be silently bypassed
                and type(det_predictor)._detect is DetectionPredictor._detect
                and type(det_predictor)._detect_device is DetectionPredictor._detect_device
                and type(det_predictor)._iter_detect_device is DetectionPredictor._iter_detect_device
                and det_predictor.device_postprocess and not det_predictor.shard_pages)
    def _call_streamed(self, images, task_names, det_predictor, detection_batch_size, recognition_batch_size, highres_images,
                       sort_lines, math_mode, return_words, drop_repeated_text, stamps, t_call, cons=None) -> List[OCRResult]:
        import queue
        import sys
        import threading
        flat = new_flat()
        if self._top_k is not None:
            flat["top_k"] = self._top_k
        if cons is not None:                                  # the options' tables and, no page being there yet, an empty list per option:
            options.attach(flat, cons)                        # assembly replays a line's automaton from the line's integer
        thr = rectify_threshold(self.rectify)
        if thr is not None:
            flat["quads"] = []
        unroll = self._unroll_on()
        if unroll:
            flat["curves"] = []
        orig_of: List[int] = []                               # line id -> original position
        q: "queue.Queue" = queue.Queue()
        overall_max_tokens = max([self.line_budget(t) for t in task_names] or [1])
        det_wall = [0.0]
        stop = threading.Event()

        def produce():
            try:
                if torch.cuda.is_available():
                    torch.cuda.set_device(self.model.device)             # the current device is per thread
                page, t_p = 0, time.perf_counter()
                for dets in det_predictor.iter_detect(images, batch_size=detection_batch_size):
                    if stop.is_set():
                        break
                    pages, refs, polys_all, scales_all, tasks_all, quads_all, curves_all = [], [], [], [], [], [], []
                    first_page = page
                    for det_pred in dets:
                        polygons, src, polys_px, scale = page_lines(det_pred, images[page], highres_images[page])
                        pages.append(page_pixels(src))
                        if thr is None and not unroll:
                            refs.extend(poly_ref(len(pages) - 1, src.size[0], src.size[1], poly) for poly in polys_px)
                        else:
                            curves = detected_curves(det_pred, scale) if unroll else None
                            page_refs, quads = slice_polys(polys_px, thr, pages[-1], len(pages) - 1, curves=curves)
                            refs.extend(page_refs)
                            if thr is not None:
                                quads_all.extend(quads)
                            if unroll:
                                curves_all.extend(curves)
                        polys_all.extend(polygons)
                        scales_all.extend([scale] * len(polygons))
                        tasks_all.extend([task_names[page]] * len(polygons))
                        flat["slice_map"].append(len(polygons))
                        page += 1
                    if not refs:
                        continue
                    base_orig, base_id = len(flat["polygons"]), len(flat["slices"])
                    # widest first inside the chunk: the length bucketing of the reference's global sort (:847-854), per arrival
                    order = sorted(range(len(refs)), key=lambda i: -refs[i].shape[1])
                    prompts = [RecognitionPrompt(id=base_id + k, task_name=tasks_all[i], text=None, image=refs[i], math_mode=math_mode)
                               for k, i in enumerate(order)]
                    tiles, tile_offs, grids, prompt_ids = self.preprocess_prompts_device(prompts, pages)
                    # the options' integers of the chunk's lines (per-call and per-image lists only: one per page), by line id
                    lines = {} if cons is None else {k: [v[i] for i in order] for k, v in
                                                     options.line_part(cons, flat["slice_map"][first_page:], range(first_page, page)).items()}
                    # everything the assembly thread reads about these lines is in place BEFORE the chunk can be admitted
                    flat["polygons"].extend(polys_all)
                    flat["res_scales"].extend(scales_all)
                    if thr is not None:
                        flat["quads"].extend(quads_all)
                    if unroll:
                        flat["curves"].extend(curves_all)
                    flat["slices"].extend(refs[i] for i in order)
                    flat["task_names"].extend(tasks_all[i] for i in order)
                    flat["input_text"].extend([None] * len(order))
                    for k, v in lines.items():
                        flat[k].extend(v)
                    orig_of.extend(base_orig + i for i in order)
                    q.put({"prompts": prompts, "tiles": tiles, "tile_offs": tile_offs, "grids": grids, "prompt_ids": prompt_ids,
                           "max_tokens": {p.id: self.line_budget(p.task_name) for p in prompts}, **lines})
                det_wall[0] = (time.perf_counter() - t_p) * 1e3
                q.put(FEED_END)
            except BaseException as e:                        # surfaces in the calling thread
                q.put(e)

        def feed(block):
            try:
                item = q.get(block)
            except queue.Empty:
                return None
            if isinstance(item, BaseException):
                raise item
            return item

        # the producer's Python work (box lists, line descriptors) must not keep the scheduler from its next launch for a
        # whole default switch interval (5 ms = a decode call of 4 steps)
        old_switch = sys.getswitchinterval()
        sys.setswitchinterval(min(old_switch, 5e-4))
        producer = threading.Thread(target=produce, name="surya-amd-detect", daemon=True)
        try:
            with AssemblyHandover(self, flat, orig_of, drop_repeated_text, return_words) as hand:
                t0 = time.perf_counter()
                producer.start()
                try:
                    first = {"prompts": [], "max_tokens": {}, "overall_max_tokens": overall_max_tokens}
                    if cons is not None:
                        first.update(options.call_part(cons))          # the whole call's tables up front: chunks carry the lines' integers only
                    self.generate(first, recognition_batch_size, on_done=hand.on_done, on_flush=hand.on_flush, feed=feed)
                except BaseException:
                    stop.set()                         # the producer ends after the batch it is working on ...
                    producer.join(timeout=30.0)        # ... and is waited for: it launches detector and pre-processing work on this predictor's
                    if producer.is_alive():            # objects and stream, and a retry of the call must not run beside it
                        self._poisoned = "a streamed call failed and its detector thread did not stop within 30 s: create a new predictor"
                    raise
                producer.join()                        # it has put FEED_END: nothing left to run
                stamps.update(streamed=1.0, detect_thread_ms=det_wall[0])
                text_lines = hand.finish(stamps, t0)
        finally:
            sys.setswitchinterval(old_switch)
        if not text_lines:
            return []
        assert len(flat["slice_map"]) == len(images)
        if self._reread is not None:
            sources = [hr if hr is not None else im for im, hr in zip(images, highres_images)]
            text_lines = rereading.second_pass(self, self._reread, flat, orig_of, text_lines, sources, "poly", recognition_batch_size,
                                               return_words, drop_repeated_text, math_mode, stamps)
        results = self._page_results(images, flat["slice_map"], text_lines, sort_lines)
        stamps["total_ms"] = (time.perf_counter() - t_call) * 1e3
        return results
