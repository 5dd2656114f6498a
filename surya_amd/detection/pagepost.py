"""Page map -> result, written once for every route a page map takes. The currency is the PageGroup: pages of equal map
size lie in ONE tensor and share ONE post-processing call, whatever made the maps (`strip_groups` of a `batch_heatmaps` batch, the stitched
maps of `_tiled_batches`). On top of the boxes come the map-derived extras (page skew, centre lines), each one small object with the same five
verbs; PagePost runs them in its device arm (`launch` / `finish`) and in its host arm (`host`: numpy on the downloaded maps, the checker of
the device arm). An extra that is off does not exist here: nothing is launched or allocated for it."""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor
from typing import NamedTuple, Tuple

import numpy as np
import torch
from PIL import Image

from ..settings import settings
from . import centerline as centerline_rule
from . import skew as skew_rule
from .heatmap import detect_boxes, result_from_device_boxes
from .model import HipDetCenterlines, HipDetPost, HipDetSkew
from .tiling import check_tiling


class PageGroup(NamedTuple):
    pages: list                    # their indices within the batch
    maps: torch.Tensor             # cuda fp32 [n, planes, mh, pitch] or [n, mh, pitch]; plane 0 is the text map
    size: Tuple[int, int]          # (mw, mh): the valid part of every map


def strip_groups(heat, split_index, split_heights):
    """The groups of one `batch_heatmaps` batch. heat: [strips, planes, ph, pw]; split_index: page of each strip; split_heights: its valid rows.
    Whole pages share one group, whose tensor is `heat` itself when every page of the batch is whole (no copy on the default path). Tall
    pages are re-assembled from their strips' valid rows (surya/detection/__init__.py:134-151), pages of equal height in one group (a call per
    page was 17 launches + a D2H each: 16 letter pages spent 40 of their 77 ms there, tools/hostbench/det_letter_profile.py)."""
    ph, pw = heat.shape[2], heat.shape[3]
    strips_of = [[i for i, k in enumerate(split_index) if k == page] for page in range(split_index[-1] + 1)]
    groups = []
    whole = [page for page, strips in enumerate(strips_of) if len(strips) == 1]
    if whole:
        groups.append(PageGroup(whole, heat if len(whole) == heat.shape[0] else heat[[strips_of[pg][0] for pg in whole]].contiguous(), (pw, ph)))
    by_height = {}
    for page, strips in enumerate(strips_of):
        if len(strips) > 1:
            by_height.setdefault(sum(split_heights[t] for t in strips), []).append(page)
    for hf, pages in by_height.items():
        full = torch.empty((len(pages), hf, pw), dtype=heat.dtype, device=heat.device)
        for i, page in enumerate(pages):
            r0 = 0
            for t in strips_of[page]:
                full[i, r0: r0 + split_heights[t]] = heat[t, 0, : split_heights[t]]
                r0 += split_heights[t]
        groups.append(PageGroup(pages, full, (pw, hf)))
    return groups


def _image(m):
    return Image.fromarray((m * 255).astype(np.uint8))


def strip_map_images(heat, split_index, split_heights):
    """include_maps of a `batch_heatmaps` batch: page -> (heat image, affinity image), both planes from `heat` as the reference cuts them: a
    page's FIRST strip whole -- an unsplit page shorter than the processor height still gets its full map -- and only the later strips of a
    split page trimmed to their valid rows (detection/__init__.py:134-151). One D2H per batch, when the first page is asked for."""
    host = []

    def images(page):
        host[:] = host or [heat.cpu().numpy()]
        strips = [t for t, k in enumerate(split_index) if k == page]
        rows = [heat.shape[2] if i == 0 else split_heights[t] for i, t in enumerate(strips)]
        return tuple(_image(np.vstack([host[0][t, plane, :r] for t, r in zip(strips, rows)])) for plane in (0, 1))
    return images


def stitched_map_images(groups):
    """include_maps of a `_tiled_batches` batch: the stitched valid region of both planes. One D2H per group, when its first page is asked for."""
    host = {}

    def images(page):
        g, (pages, maps, (mw, mh)) = next((g, group) for g, group in enumerate(groups) if page in group[0])
        if g not in host:
            host[g] = maps.cpu().numpy()
        return tuple(_image(host[g][list(pages).index(page), plane, :mh, :mw]) for plane in (0, 1))
    return images


def _thresholds():
    return settings.DETECTOR_TEXT_THRESHOLD, settings.DETECTOR_BLANK_THRESHOLD


class _Extra:
    """What a map-derived extra provides. `option` / `last`: the predictor's attribute that turns it on / that takes its per-page entries.
    check(images): the refusals, before any device work. launch(post, group, page_sizes): enqueue behind the group's boxes launch, return a
    handle. collect(handle, got): per page of the group what `apply` takes (got: HipDetPost.collect of the same launch). host(heat, map_size,
    page_size): the same from the numpy reference on a downloaded map. apply(raw, target, map_size): onto the page, returns its `last` entry;
    target = the finished result, or with on_boxes the boxes while they are in map coordinates and in the detector's order."""
    on_boxes = False

    def __init__(self, pred):
        self.pred = pred


class SkewExtra(_Extra):
    """DetectionPredictor.skew (detection/skew.py states the rule). Per page travel (scores of every candidate angle, text pixels)."""
    option, last = "skew", "last_skew"

    def check(self, images):
        est = self.est = skew_rule.check_skew(self.pred.skew)
        skew_rule.check_skew(est, self.pred._map_geometry(images))
        self.angles = skew_rule.candidate_angles(est)
        self.threshold = float(settings.DETECTOR_BLANK_THRESHOLD if est.threshold is None else est.threshold)

    def launch(self, post, group, page_sizes):             # every page its own table from the one candidate list
        tables = np.stack([skew_rule.coeff_table(self.angles, ps, group.size) for ps in page_sizes])
        return self.pred._op("_skew_op", HipDetSkew).launch(group.maps, tables, self.threshold)

    def collect(self, pending, got):
        return list(zip(*self.pred._skew_op.collect(pending)))

    def host(self, heat, map_size, page_size):
        return skew_rule.skew_scores(heat, self.threshold, skew_rule.coeff_table(self.angles, page_size, map_size))

    def apply(self, raw, result, map_size):                # the choice: host, float64
        scores, n_text = raw
        angle, conf = skew_rule.choose(scores, int(n_text), self.angles, self.est.step, self.est.min_pixels)
        result.skew, result.skew_confidence = angle, conf
        return {"angle": angle, "confidence": conf, "n_text": int(n_text), "map_size": (int(map_size[0]), int(map_size[1]))}


class CenterlineExtra(_Extra):
    """DetectionPredictor.centerlines (detection/centerline.py states the rule). Per page travels the profile of its kept components."""
    option, last, on_boxes = "centerlines", "last_centerlines", True

    def check(self, images):
        self.cl = centerline_rule.check_centerlines(self.pred.centerlines)

    def launch(self, post, group, page_sizes):             # reads the labels the boxes launch has just left in `post`'s workspace
        return self.pred._op("_cl_op", HipDetCenterlines).launch(post, group.maps, self.cl.knots)

    def collect(self, pending, got):
        return self.pred._cl_op.collect(pending, [len(bx) for bx, _ in got], _thresholds())

    def host(self, heat, map_size, page_size):
        return centerline_rule.profile_page(heat, *_thresholds(), self.cl.knots)

    def apply(self, raw, boxes, map_size):
        return {"n_boxes": len(boxes), "n_curved": centerline_rule.attach(boxes, raw, self.cl)}


def page_result(extras, raws, boxes, confs, map_size, page_size, images=(None, None)):
    """One page: (its result, the `last` entry of every extra). raws: what every extra's `collect` or `host` gave for this page."""
    infos = [None] * len(extras)
    early = [j for j, e in enumerate(extras) if e.on_boxes]

    def attach(bboxes):
        for j in early:
            infos[j] = extras[j].apply(raws[j], bboxes, map_size)
    r = result_from_device_boxes(boxes, confs, list(map_size), page_size, *images, attach=attach if early else None)
    for j, e in enumerate(extras):
        if not e.on_boxes:
            infos[j] = e.apply(raws[j], r, map_size)
    return r, infos


def host_page(extras, text, affinity, map_size, page_size):
    """The host arm for one page: the steps of heatmap.parallel_get_boxes on a downloaded text map (detect_boxes, then the host remainder the
    device arm runs too) with every extra's numpy reference on the same map. affinity: None, or the second plane when the caller wants the
    two map images (the valid region map_size of both: a stitched map is wider than that by its pad columns)."""
    heat = text if text.dtype == np.float32 else text.astype(np.float32)
    mw, mh = map_size
    images = (None, None) if affinity is None else (_image(text[:mh, :mw]), _image(affinity[:mh, :mw]))
    return page_result(extras, [e.host(heat, map_size, page_size) for e in extras], *detect_boxes(heat, *_thresholds()), map_size, page_size, images)


class PagePost:
    """The post stage of one call. Construction runs every refusal of the call (`tiling`, `skew`, `centerlines`): nothing has touched the
    device when it raises."""

    def __init__(self, pred, images):
        self.pred = pred
        if pred.tiling is not None:
            check_tiling(pred.tiling, pred.processor.size["height"])
        # checked in the order the options came to the predictor (a new one last); an extra's `last` list is emptied as ITS check passes
        on = {extra: extra(pred) for extra in (SkewExtra, CenterlineExtra) if getattr(pred, extra.option) is not None}
        for e in on.values():
            e.check(images)
            setattr(pred, e.last, [])
        # The launch order. What reads the workspace of a boxes launch (the centre lines: its labels) goes right behind THAT launch, before the
        # next boxes launch rewrites the workspace; the skew has a workspace of its own and reads only the maps.
        self.extras = [on[extra] for extra in (CenterlineExtra, SkewExtra) if extra in on]

    def _record(self, infos):
        for j, e in enumerate(self.extras):
            getattr(self.pred, e.last).extend(info[j] for info in infos)

    def launch(self, groups, sizes, map_images=None):
        """Device arm: enqueue, per group, boxes -> centre lines -> skew; nothing waits. sizes: the page sizes of the batch. map_images: None, or
        page -> (heat image, affinity image) from the source of the maps (callers that want the maps pay for their D2H, in `finish`)."""
        post = self.pred._op("_post", HipDetPost)
        groups = [PageGroup(*g) for g in groups]                       # a source may yield plain (pages, maps, size) tuples
        launched = []
        for group in groups:
            boxes = post.launch(group.maps, *_thresholds())
            launched.append((boxes, [e.launch(post, group, [sizes[k] for k in group.pages]) for e in self.extras]))
        return groups, sizes, launched, map_images

    def finish(self, pending):
        """Device arm: the results of one launched batch in page order (waits for ITS events only)."""
        groups, sizes, launched, map_images = pending
        out, infos = [None] * len(sizes), [None] * len(sizes)
        for (pages, _, map_size), (boxes, handles) in zip(groups, launched):
            got = self.pred._post.collect(boxes)
            raws = [e.collect(h, got) for e, h in zip(self.extras, handles)]
            for i, (k, (bx, cf)) in enumerate(zip(pages, got)):
                out[k], infos[k] = page_result(self.extras, [r[i] for r in raws], bx, cf, map_size, sizes[k],
                                               map_images(k) if map_images else (None, None))
        self._record(infos)
        return out

    def host(self, pages, n_images):
        """Host arm. pages: (text map, affinity map or None, map size, page size) of every page of the call, in page order, taken while their
        source prepares the next ones. From DETECTOR_MIN_PARALLEL_THRESH images on, on the reference's thread pool."""
        if n_images >= settings.DETECTOR_MIN_PARALLEL_THRESH:
            with ThreadPoolExecutor(max_workers=max(1, min(settings.DETECTOR_POSTPROCESSING_CPU_WORKERS, n_images))) as ex:
                futures = [ex.submit(host_page, self.extras, *page) for page in pages]
            out = [f.result() for f in futures]
        else:
            out = [host_page(self.extras, *page) for page in pages]
        self._record([infos for _, infos in out])
        return [r for r, _ in out]
