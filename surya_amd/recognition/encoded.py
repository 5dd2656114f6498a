"""EncodedLines: lines encoded once and kept on the device (RecognitionPredictor.encode).

Every entry point of the predictor starts with the same steps -- slice, resize, patchify, vision encoder, prompt prefill -- and a caller
who reads a line twice (read, then rank the repairs; read under a pattern, then re-read what did not match with a beam) pays for them
twice. `encode` runs them once: every line's prompt -- its KV rows of every layer and kv head and the hidden row the first token is
computed from -- stays in the model's prompt store (surya_rec_prefill_keep), and `read` / `rank` / `align` land it in decoder slots
again (surya_rec_restore: a copy) and go on from there through the call paths of `__call__` / `rank` / `align`. The copies are exact and
the head pass runs the same kernels on the same row values, so the results are those calls' results bit for bit.

The host hands out the store's rows, as it hands out slots: one RowAllocator per model handle, first fit over a free list, so several
EncodedLines may be live at once and a released one's rows are used again."""
from __future__ import annotations

import time
import weakref
from collections import namedtuple
from typing import List

from ..common.imageops import rectify_threshold
from ..common.predictor import gc_paused
from . import options
from .schema import OCRResult, RankResult, TaskNames

_Page = namedtuple("_Page", "size")                          # what the call paths read of a page once its lines are sliced
_Line = namedtuple("_Line", "id")                            # ... and DeviceLoop.admit of a prompt


class RowAllocator:
    """Row ranges of a store of `capacity` rows: `alloc(rows)` -> the first row of a free range (first fit over the free list, which is
    sorted by row), `free(first)` gives a range back and joins it with free neighbours. When nothing fits, `reserve(new_capacity)` is
    called -- the model's reserve_prompts, which grows the store and keeps its contents -- with at least double the capacity, and the
    new rows join the free list; if it raises, nothing changed."""

    def __init__(self, reserve, capacity: int = 0, chunk: int = 4096):
        self.reserve, self.capacity, self.chunk = reserve, int(capacity), int(chunk)
        self.free_list = [[0, self.capacity]] if self.capacity else []      # [first, rows], ascending, never adjacent
        self.live = {}                                                       # first -> rows

    def alloc(self, rows: int) -> int:
        rows = int(rows)
        assert rows > 0, "a range has at least one row"
        for attempt in (0, 1):
            for blk in self.free_list:
                if blk[1] >= rows:
                    first = blk[0]
                    blk[0] += rows
                    blk[1] -= rows
                    if blk[1] == 0:
                        self.free_list.remove(blk)
                    self.live[first] = rows
                    return first
            assert attempt == 0, "the store grew by what was missing"
            self._grow(rows)

    def _grow(self, rows: int):
        tail = self.free_list[-1] if self.free_list and sum(self.free_list[-1]) == self.capacity else None
        missing = rows - (tail[1] if tail else 0)
        new = max(2 * self.capacity, self.capacity + missing, self.chunk)
        self.reserve(new)                                     # (raises: nothing changed)
        if tail:
            tail[1] += new - self.capacity
        else:
            self.free_list.append([self.capacity, new - self.capacity])
        self.capacity = new

    def free(self, first: int):
        rows = self.live.pop(int(first))
        fl = self.free_list
        i = 0
        while i < len(fl) and fl[i][0] < first:
            i += 1
        fl.insert(i, [int(first), rows])
        if i + 1 < len(fl) and fl[i][0] + fl[i][1] == fl[i + 1][0]:      # joins the block behind it
            fl[i][1] += fl.pop(i + 1)[1]
        if i > 0 and fl[i - 1][0] + fl[i - 1][1] == fl[i][0]:            # ... and the one before it
            fl[i - 1][1] += fl.pop(i)[1]

    @property
    def used(self) -> int:
        return sum(self.live.values())


def rows_of(model) -> RowAllocator:
    """The allocator of `model`'s prompt store: one per handle, made on first use."""
    alloc = getattr(model, "_prompt_rows", None)
    if alloc is None:
        alloc = model._prompt_rows = RowAllocator(model.reserve_prompts)
    return alloc


def _release(model_ref, alloc, first):
    """Forget the entries `first` (those the model holds) and give their rows back. Also the finaliser: it must not hold the object."""
    model = model_ref()
    if model is not None and getattr(model, "handle", None) and first:
        live = [f for f in first if f in alloc.live]
        try:
            model.drop_prompts(live)
        except Exception:                                     # an encode that failed half-way: some of its rows never became entries
            for f in live:
                try:
                    model.drop_prompts([f])
                except Exception:
                    pass
    for f in first:
        if f in alloc.live:
            alloc.free(f)


def _refuse(pred, what, det_predictor=None):
    """What every entry point refuses before any device work."""
    if getattr(pred, "_poisoned", None):
        raise RuntimeError(pred._poisoned)
    if getattr(pred, "reread", None) is not None:
        raise ValueError(f"reread does not apply to {what}(): a stored prompt holds no pixels to adjust or turn (set reread = None)")
    if det_predictor is not None:
        raise ValueError(f"{what}() takes no det_predictor: run the detector first and pass its polygons (polygons=)")
    if pred.shard_lines or pred.shard_pages or pred.process_group is not None:
        raise NotImplementedError(f"{what}() runs on one rank: unset shard_lines / shard_pages / process_group")
    if getattr(pred.model, "kv_fp8", False):
        raise ValueError(f"{what}() is not available with the fp8 KV cache (RECOGNITION_KV_FP8 / set_kv_fp8): the prompt store holds "
                         f"bf16 / fp16 / fp32 rows only")


class EncodedLines:
    """The lines of one `RecognitionPredictor.encode` call, on the device. `line_counts[i]` is the number of lines of image i; `lines=`
    of the methods below is None (all lines) or, per image, a list of line indices: results then hold only those lines, in that order
    (no index twice in a call), and every per-line argument -- candidates, texts, a per-line allowlist -- has one entry per SELECTED
    line. A context manager; `release()` frees the store rows (a finaliser does too), after which every method raises ValueError."""

    def __init__(self, pred, images, flat, first, prompt_ids, grids, task_names):
        self._pred, self._model = weakref.ref(pred), pred.model
        self.dtype, self._handle = pred.model.dtype, pred.model.handle.value
        self._pages = [_Page(tuple(im.size)) for im in images]
        self._task_names = list(task_names)
        self.line_counts = list(flat["slice_map"])
        # the line table, by original position (page order): what assembly and the loop need of a line
        self._slices, self._tasks, self._texts = list(flat["slices"]), list(flat["task_names"]), list(flat["input_text"])
        self._polygons, self._scales = list(flat["polygons"]), list(flat["res_scales"])
        self._quads = list(flat["quads"]) if flat.get("quads") is not None else None
        self._curves = list(flat["curves"]) if flat.get("curves") is not None else None
        self._first, self._prompt_ids, self._grids = list(first), list(prompt_ids), list(grids)
        self._base = [0]
        for n in self.line_counts:
            self._base.append(self._base[-1] + n)
        self._fin = weakref.finalize(self, _release, weakref.ref(pred.model), rows_of(pred.model), list(first))

    # ------------------------------------------------------------------------------------------------ encode
    @classmethod
    def encode(cls, pred, images, task_names, bboxes, polygons, input_text, math_mode, recognition_batch_size, det_predictor=None):
        from .predictor import convert_if_not_rgb
        _refuse(pred, "encode", det_predictor)
        rectify_threshold(pred.rectify)                       # ValueError for a bad value, before any device work
        given = polygons if polygons is not None else bboxes
        if given is None:
            raise ValueError("encode() needs bboxes or polygons: the lines to keep")
        if task_names is None:
            task_names = [TaskNames.ocr_with_boxes] * len(images)
        if not (len(images) == len(given) == len(task_names)) or (input_text is not None and len(input_text) != len(images)):
            raise ValueError(f"encode(): {len(images)} images, {len(given)} bbox / polygon lists, {len(task_names)} task names")
        for t in task_names:
            if t not in pred.tasks:
                raise ValueError(f"task {t!r} is not supported. Supported tasks are {list(pred.tasks)}")
        images = convert_if_not_rgb(images)
        with pred._modes(), gc_paused():                      # greedy, no alternatives: the prompt does not depend on how it is read later
            flat = pred.slice_bboxes(images, task_names, bboxes=bboxes, polygons=polygons, input_text=input_text)
            n = len(flat["slices"])
            order = sorted(range(n), key=lambda i: -flat["slices"][i].shape[1])      # widest first, as every call prefills
            first, prompt_ids, grids = [None] * n, [None] * n, [None] * n
            if n:
                work = dict(flat)
                for key in ("slices", "input_text", "task_names"):
                    work[key] = [flat[key][i] for i in order]
                prep = pred.prepare_lines(work, math_mode)
                model, alloc, taken = pred.model, rows_of(pred.model), []
                try:
                    for ids in prep["prompt_ids"]:
                        taken.append(alloc.alloc(len(ids)))
                    prep["store_first"], prep["store_mode"] = taken, "keep"
                    prep["max_tokens"] = {k: 1 for k in prep["max_tokens"]}      # the prefill's token, then the line stops
                    pred.generate(prep, recognition_batch_size)
                except BaseException:
                    _release(weakref.ref(model), alloc, taken)
                    raise
                for k, g in enumerate(order):
                    first[g], prompt_ids[g], grids[g] = taken[k], prep["prompt_ids"][k], prep["grids"][k]
        return cls(pred, images, flat, first, prompt_ids, grids, task_names)

    # --------------------------------------------------------------------------------------------- lifetime
    @property
    def released(self) -> bool:
        return not self._fin.alive

    def release(self):
        """Forget the entries and give their rows back to the allocator. Idempotent."""
        self._fin()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()
        return False

    def __len__(self):
        return self._base[-1]

    def _usable(self, what, predictor=None):
        """The predictor to run on, after everything a call refuses before any device work."""
        if self.released:
            raise ValueError(f"{what}(): these EncodedLines were released")
        pred = self._pred()
        if pred is None or (predictor is not None and predictor is not pred) or pred.model is not self._model or \
                pred.model.handle.value != self._handle or pred.model.dtype != self.dtype:
            raise ValueError(f"{what}(): these EncodedLines were made by another predictor: their prompts live in that predictor's model")
        _refuse(pred, what)
        return pred

    # ------------------------------------------------------------------------------------------- selection
    def _select(self, lines) -> list:
        """`lines` -> per image the global ids of the selected lines, in the order given."""
        if lines is None:
            return [list(range(a, b)) for a, b in zip(self._base, self._base[1:])]
        if not isinstance(lines, (list, tuple)) or len(lines) != len(self.line_counts):
            raise ValueError(f"lines must be None or a list with one list of line indices per image ({len(self.line_counts)} images)")
        out, seen = [], set()
        for i, (page, n) in enumerate(zip(lines, self.line_counts)):
            if page is None:
                page = range(n)
            ids = []
            for j in page:
                if isinstance(j, bool) or not isinstance(j, int) or not 0 <= j < n:
                    raise ValueError(f"image {i}: line index {j!r} is outside its {n} lines")
                if self._base[i] + j in seen:
                    raise ValueError(f"image {i}: line {j} is named twice (a line is restored once per call)")
                seen.add(self._base[i] + j)
                ids.append(self._base[i] + j)
            out.append(ids)
        return out

    def _flat(self, lines) -> dict:
        """The flat line table (predictor.new_flat) of the selected lines, with their ids under "enc_ids", by line id like the slices."""
        from .predictor import new_flat
        sel = self._select(lines)
        ids = [g for page in sel for g in page]
        flat = new_flat()
        flat["slice_map"] = [len(page) for page in sel]
        for key, src in (("slices", self._slices), ("task_names", self._tasks), ("input_text", self._texts), ("polygons", self._polygons),
                         ("res_scales", self._scales)):
            flat[key] = [src[g] for g in ids]
        if self._quads is not None:
            flat["quads"] = [self._quads[g] for g in ids]
        if self._curves is not None:
            flat["curves"] = [self._curves[g] for g in ids]
        flat["enc_ids"] = ids
        return flat

    def _given(self, flat) -> list:
        """One entry per selected line and image: what the call paths count lines with."""
        return [[None] * n for n in flat["slice_map"]]

    def _prep(self, flat) -> dict:
        """prepare_lines' counterpart for restored lines: no tiles, every line's store row and prompt length instead."""
        pred, ids = self._pred(), flat["enc_ids"]
        prep = {"prompts": [_Line(k) for k in range(len(ids))], "max_tokens": {k: pred.line_budget(t) for k, t in enumerate(flat["task_names"])},
                "tiles": None, "tile_offs": None, "grids": [self._grids[g] for g in ids], "prompt_ids": [self._prompt_ids[g] for g in ids],
                "store_first": [self._first[g] for g in ids], "store_mode": "restore", **options.take(flat)}
        if flat.get("forced_ids") is not None:
            prep["forced_ids"] = flat["forced_ids"]
            if flat.get("fan"):
                prep["fan"] = True
        return prep

    # ----------------------------------------------------------------------------------------------- calls
    def read(self, lines=None, sort_lines: bool = False, return_words: bool = False, drop_repeated_text: bool = False, allowlist=None,
             blocklist=None, recognition_batch_size: int | None = None, predictor=None) -> List[OCRResult]:
        """What `pred(images, bboxes=...)` returns for the selected lines, under the predictor's current `top_k`, `beam_width`, `pattern`,
        `lexicon`, `boost_words` / `boost_weight` and this call's `allowlist` / `blocklist`, with `__call__`'s refusals."""
        pred = self._usable("read", predictor)
        top_k, beam, pattern, lexicon, boost_words, boost_weight = pred._checked_modes()
        flat = self._flat(lines)
        with pred._modes(top_k, beam), gc_paused():
            t_call = time.perf_counter()
            stamps = pred.last_timing = {}
            cons = pred._constraints(allowlist, blocklist, self._pages, self._given(flat), None, pattern, lexicon, boost_words)
            if cons is not None and cons.boost is not None:
                cons.boost_weight = float(boost_weight)
            return pred._read_flat(self._pages, flat, cons, recognition_batch_size, sort_lines, return_words, drop_repeated_text, stamps,
                                   t_call, self._prep)

    def rank(self, candidates, lines=None, recognition_batch_size: int | None = None, predictor=None) -> List[RankResult]:
        """What `pred.rank(images, candidates, bboxes=...)` returns for the selected lines: every entry lands in as many slots as the line
        has distinct candidates, the way `rank` shares one prefill."""
        pred = self._usable("rank", predictor)
        flat = self._flat(lines)
        given, task_names = pred._forced_call_checks("rank", "candidates", "candidate lists", self._pages, candidates, self._task_names,
                                                     self._given(flat), None)
        cand = pred._rank_candidates(candidates, given, task_names, recognition_batch_size)
        with pred._modes(), gc_paused():
            return pred._rank_flat(self._pages, flat, cand, recognition_batch_size, self._prep)

    def align(self, texts, lines=None, return_words: bool = False, recognition_batch_size: int | None = None, predictor=None) -> List[OCRResult]:
        """What `pred.align(images, texts, bboxes=...)` returns for the selected lines."""
        pred = self._usable("align", predictor)
        flat = self._flat(lines)
        given, task_names = pred._forced_call_checks("align", "texts", "text lists", self._pages, texts, self._task_names, self._given(flat), None)
        forced = pred._align_forced(texts, given, task_names)
        with pred._modes(), gc_paused():
            return pred._align_flat(self._pages, flat, forced, recognition_batch_size, return_words, self._prep)
