"""DetectionPredictor: drop-in for surya.detection.DetectionPredictor on MI355X.

Same call signature / result schema (surya/detection/__init__.py:22-48, detection/schema.py:12-17). The model forward,
sigmoid and x4 upsample run in libsurya_amd.so (HipDetModel); tall-page splitting, PIL resizing and heat-map -> box
post-processing stay on the host as in the reference. No CPU fallback for the model.
"""
from __future__ import annotations

import math
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Generator, List, Tuple

import numpy as np
import torch
from PIL import Image, ImageOps

from ..common.imageops import copy_pool, page_pixels, parallel_copy
from ..common.predictor import BasePredictor, ModelLoader, gc_paused
from ..config import DetConfig, det_config
from ..settings import settings
from .heatmap import TextDetectionResult, detect_boxes, parallel_get_boxes, result_from_device_boxes
from ..common.pil_resample import plan_chain as plan_resize
from .model import CUT_DESC, STITCH_DESC, DeviceResampler, HipDetCenterlines, HipDetModel, HipDetPost, HipDetSkew, HipDetTiler
from . import centerline as centerline_rule
from . import skew as skew_rule
from .centerline import Centerlines  # noqa: F401  (what `DetectionPredictor.centerlines` takes)
from .skew import SkewEstimate, straighten  # noqa: F401  (SkewEstimate: what `DetectionPredictor.skew` takes)
from .tiling import DetTiling, check_tiling, page_plan  # noqa: F401  (DetTiling: what `DetectionPredictor.tiling` takes)


class SegformerImageProcessor:
    """rescale 1/255 + ImageNet normalise -> CHW float32 (surya/detection/processor.py:126-146); `size` from the checkpoint.
    The reference's rescale step multiplies in float64 and rounds to float32 once (transformers' image_transforms.rescale), so the
    scaled pixel is the correctly rounded px / 255; a float32 product px * float32(1/255) is one ulp off for some pixel values
    (found by the live cross-check against the reference's own processor, tests/test_oracle_vs_reference.py)."""
    image_mean = np.array([0.485, 0.456, 0.406], np.float32)
    image_std = np.array([0.229, 0.224, 0.225], np.float32)

    def __init__(self, size=None):
        self.size = size or {"height": 512, "width": 512}

    def __call__(self, image: np.ndarray):
        a = ((image.astype(np.float64) * (1 / 255)).astype(np.float32) - self.image_mean) / self.image_std
        return {"pixel_values": [np.ascontiguousarray(a.transpose(2, 0, 1))]}


def get_total_splits(image_size, height):              # surya/detection/util.py:7-13
    return math.ceil(image_size[1] / height) if image_size[1] > settings.DETECTOR_IMAGE_CHUNK_HEIGHT else 1


def split_image(img: Image.Image, height: int, copy: bool = True):
    """Tall pages (> DETECTOR_IMAGE_CHUNK_HEIGHT px) are cut into `height`-px strips, the last one white-padded
    (surya/detection/util.py:16-36). copy=False hands a page that needs no cutting back as it is (for callers that only read
    its pixels: the reference copies because its prepare_image resizes in place)."""
    ih = img.size[1]
    if ih <= settings.DETECTOR_IMAGE_CHUNK_HEIGHT:
        return [img.copy() if copy else img], [ih]
    parts, heights = [], []
    for i in range(math.ceil(ih / height)):
        top, bottom = i * height, min((i + 1) * height, ih)
        crop = img.crop((0, top, img.size[0], bottom))
        if bottom - top < height:
            crop = ImageOps.pad(crop, (img.size[0], height), color=255, centering=(0, 0))
        parts.append(crop)
        heights.append(bottom - top)
    return parts, heights


def det_config_from_reference_json(raw: dict):
    """Map an EfficientViTConfig config.json (surya/detection/model/config.py:12-52) onto DetConfig."""
    from ..config import DetConfig
    kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in raw.items() if k in DetConfig.__dataclass_fields__}
    kw.setdefault("num_labels", raw.get("num_labels", len(raw.get("id2label", {})) or 2))
    return DetConfig(**{**kw, "name": "checkpoint"})


class DetectionModelLoader(ModelLoader):
    """checkpoint: None / config name (synthetic weights), {"config": DetConfig, "state_dict": ..., "size": int}, or a directory in
    the reference's on-disk format (surya/detection/loader.py:23-63): config.json (EfficientViTConfig), *.safetensors (the
    reference's parameter names) and preprocessor_config.json (SegformerImageProcessor: size, image_mean, image_std)."""

    def __init__(self, checkpoint=None):
        super().__init__(checkpoint)
        ck = checkpoint
        self._mean = self._std = None
        if isinstance(ck, dict):
            self._cfg, self._sd, self._size = ck["config"], ck["state_dict"], int(ck.get("size", 1024))
        elif isinstance(ck, str) and os.path.isdir(ck):
            import json
            from safetensors.torch import load_file
            with open(os.path.join(ck, "config.json")) as f:
                self._cfg = det_config_from_reference_json(json.load(f))
            self._sd = {}
            for fn in sorted(os.listdir(ck)):
                if fn.endswith(".safetensors"):
                    self._sd.update(load_file(os.path.join(ck, fn)))
            if not self._sd:
                raise FileNotFoundError(f"{ck}: no *.safetensors file")
            self._size = 1024
            pp = os.path.join(ck, "preprocessor_config.json")
            if os.path.exists(pp):
                with open(pp) as f:
                    raw = json.load(f)
                size = raw.get("size") or {}
                if size.get("height") != size.get("width"):
                    raise ValueError(f"{pp}: the detector runs on square processor sizes, got {size}")
                self._size = int(size.get("height", 1024))
                self._mean, self._std = raw.get("image_mean"), raw.get("image_std")
        else:
            from ..synth import make_det_weights
            self._cfg = det_config(ck if isinstance(ck, str) else settings.SURYA_AMD_DET_CONFIG)
            self._sd = make_det_weights(self._cfg, 0)
            self._size = int(os.environ.get("SURYA_AMD_DET_SIZE", "1024"))

    def model(self, device=None, dtype=None, max_batch=None) -> HipDetModel:
        if device is None or device == "cuda":
            device = "cuda:0"
        if dtype is None:
            dtype = torch.bfloat16        # the reference picks fp16 on GPUs (detection/loader.py:31); BASELINE asks bf16
        mb = max_batch or settings.DETECTOR_BATCH_SIZE or DetectionPredictor.default_batch_sizes["cuda"]
        bw = False
        if settings.SURYA_AMD_BROADCAST_WEIGHTS:
            from .. import dist as sdist
            bw = sdist.collectives_on()
        return HipDetModel(self._cfg, self._sd, height=self._size, width=self._size, dtype=dtype, device=device, max_batch=mb,
                           broadcast_weights=bw)

    def processor(self, device=None, dtype=None) -> SegformerImageProcessor:
        p = SegformerImageProcessor({"height": self._size, "width": self._size})
        if self._mean is not None:
            p.image_mean = np.asarray(self._mean, np.float32)
        if self._std is not None:
            p.image_std = np.asarray(self._std, np.float32)
        return p


def _one_batch_ahead(launched, finish, eager_first=False):
    """One batch in flight ahead of the one being read: `launched` prepares (PIL convert / resize, pinned staging) and launches batch
    i + 1 while the GPU still works on batch i, whose boxes `finish` only then waits for. eager_first: the FIRST batch is handed over
    as soon as its boxes exist instead of after the second batch has been prepared and launched."""
    prev = None
    for job in launched:
        if prev is not None:
            yield finish(prev)
        prev = job
        if eager_first:
            eager_first = False
            yield finish(prev)
            prev = None
    if prev is not None:
        yield finish(prev)


class DetectionPredictor(BasePredictor):
    model_loader_cls = DetectionModelLoader
    batch_size = settings.DETECTOR_BATCH_SIZE
    default_batch_sizes = {"cpu": 8, "mps": 8, "cuda": 36, "xla": 18}

    # Multi-GPU: when set, ONE call's pages are dealt over the ranks (a page's strips stay on one rank), each
    # rank detects + post-processes its pages and the per-page results (boxes only, a few KB) are all-gathered as objects.
    # Every rank must pass the same pages (checked). Off by default, like RecognitionPredictor.shard_lines.
    shard_pages: bool = settings.SURYA_AMD_SHARD
    process_group = None

    def __call__(self, images: List[Image.Image], batch_size=None, include_maps=False) -> List[TextDetectionResult]:
        with gc_paused():                                  # result objects are acyclic; see common/predictor.py
            return self._call(images, batch_size, include_maps)

    def _call(self, images, batch_size=None, include_maps=False) -> List[TextDetectionResult]:
        if self.shard_pages:
            from ..common.predictor import sharded_over_ranks
            out = sharded_over_ranks(images, lambda mine: self._detect(mine, batch_size, include_maps), self.model.device, self.process_group)
            if out is not None:
                return out
        return self._detect(images, batch_size, include_maps)

    # Heat map -> boxes runs on the device (surya_det_boxes): what leaves the GPU per page is a few hundred 4-point boxes instead
    # of two fp32 maps (8 MB at 1024^2). DETECTOR_POSTPROCESS_HOST=1 keeps the host post-processing of the reference layout
    # (heat maps D2H + surya_amd/detection/heatmap.py on a thread pool): the checker of tests/test_gpu_det.py, not a fallback.
    device_postprocess: bool = not settings.DETECTOR_POSTPROCESS_HOST
    # the double LANCZOS resize of every page on the device, with the box reduction Pillow's thumbnail() puts in front of it for
    # >= 4x shrinks; DETECTOR_RESIZE_HOST=1 keeps Pillow on a thread pool (the checker of tests/test_gpu_resample*.py)
    device_resize: bool = not settings.DETECTOR_RESIZE_HOST
    # how the parts (pages / strips of tall pages) of the last call got to the processor size: resized on the device, by Pillow on
    # the host, or already there. With device_resize, "host" counts only images more than 100 times as tall as wide.
    last_resize_paths = {"device": 0, "host": 0, "ready": 0}

    # Tiled detection (detection/tiling.py states the rules): None = every page, or strip of a tall page, is squeezed onto the processor's
    # square as the reference does; a DetTiling = the page at `scale` times its own resolution is cut into processor-sized tiles on the
    # device, the tiles' heat maps are stitched into ONE page map there (every pixel from the tile that saw it farthest from a cut), and
    # the thresholds, the labelling and the boxes are those of that whole map: a line across a tile border stays one box.
    tiling = None
    # per page of the last tiled call: {"size": (mw, mh) of the scaled page and its map, "grid": (columns, rows), "tiles": their product}
    last_tiling: list = []

    # Page skew (detection/skew.py states the rule): None = nothing is estimated and nothing is launched; a SkewEstimate = every result
    # carries `skew` (degrees, the page's text baselines, positive = down to the right) and `skew_confidence`, estimated from the SAME
    # page map its boxes come from -- the whole tile, the device-side reassembly of a tall page's strips, or the stitched map under
    # `tiling` -- by surya_det_skew, enqueued behind that map's surya_det_boxes. No additional forward pass.
    skew = None
    # per page of the last call with `skew` set: {"angle", "confidence", "n_text" (text pixels of the map), "map_size" (w, h)}
    last_skew: list = []

    # Centre lines of bent text lines (detection/centerline.py states the rule): None = nothing is estimated and nothing is launched; a
    # Centerlines = every box whose component is bent carries `centerline` (points along the line, page pixels) and `thickness` (the height of
    # the band around it), from the labelling of the SAME page map its box comes from: surya_det_centerlines, enqueued behind that map's
    # surya_det_boxes, reads the labels that call left in its workspace. No additional forward pass, no second labelling.
    centerlines = None
    # per page of the last call with `centerlines` set: {"n_boxes" (kept components of the map), "n_curved" (those that got a centre line)}
    last_centerlines: list = []

    def _check_centerlines(self):
        """The refusals of `centerlines` before any device work; returns the checked Centerlines, or None when off."""
        if self.centerlines is None:
            return None
        cli = centerline_rule.check_centerlines(self.centerlines)
        self.last_centerlines = []
        return cli

    def _cl_launch(self, cli, maps):
        """surya_det_centerlines behind the surya_det_boxes launch that just took `maps`."""
        if cli is None:
            return None
        if getattr(self, "_cl_op", None) is None:
            self._cl_op = HipDetCenterlines(self.model.device)
        return self._cl_op.launch(self._post, maps, cli.knots)

    def _cl_collect(self, cpending, got):
        """The profiles of one launch, per page (None when off). got: what HipDetPost.collect returned for the same launch."""
        if cpending is None:
            return [None] * len(got)
        return self._cl_op.collect(cpending, [len(bx) for bx, _ in got], (settings.DETECTOR_TEXT_THRESHOLD, settings.DETECTOR_BLANK_THRESHOLD))

    @staticmethod
    def _cl_result(cli, prof, bx, cf, psize, size, hi=None, ai=None):
        """result_from_device_boxes with the centre lines of one page's profile attached; returns (result, its last_centerlines entry)."""
        if cli is None:
            return result_from_device_boxes(bx, cf, psize, size, hi, ai), None
        info = {}

        def attach(bboxes):
            info["n_boxes"], info["n_curved"] = len(bboxes), centerline_rule.attach(bboxes, prof, cli)
        return result_from_device_boxes(bx, cf, psize, size, hi, ai, attach=attach), info

    def _check_skew(self, images):
        """The refusals of `skew` before any device work; returns the estimate's (candidate angles, mask threshold), or None when off."""
        if self.skew is None:
            return None
        est = skew_rule.check_skew(self.skew)
        P = self.processor.size["height"]
        pw = self.processor.size["width"]
        geo = []
        for im in images:
            w, h = im.size
            if self.tiling is not None:
                geo.append(((w, h), page_plan(w, h, P, self.tiling).map_size))
            else:
                geo.append(((w, h), (pw, h if get_total_splits((w, h), P) > 1 else P)))
        skew_rule.check_skew(est, geo)
        self.last_skew = []
        return skew_rule.candidate_angles(est), float(settings.DETECTOR_BLANK_THRESHOLD if est.threshold is None else est.threshold)

    def _skew_launch(self, sk, maps, page_sizes, map_size):
        """surya_det_skew on the maps a surya_det_boxes launch just took: every page its own table from the one candidate list."""
        if getattr(self, "_skew_op", None) is None:
            self._skew_op = HipDetSkew(self.model.device)
        tables = np.stack([skew_rule.coeff_table(sk[0], ps, map_size) for ps in page_sizes])
        return self._skew_op.launch(maps, tables, sk[1])

    def _skew_set(self, sk, result, scores, n_text, map_size):
        """The choice (host, float64) from one page's scores, onto its result and into last_skew."""
        angle, conf = skew_rule.choose(scores, int(n_text), sk[0], self.skew.step, self.skew.min_pixels)
        result.skew, result.skew_confidence = angle, conf
        return {"angle": angle, "confidence": conf, "n_text": int(n_text), "map_size": (int(map_size[0]), int(map_size[1]))}

    def _skew_host(self, sk, result, heat, page_size, map_size):
        """The checker arm (DETECTOR_POSTPROCESS_HOST): the numpy reference on the downloaded map."""
        scores, n_text = skew_rule.skew_scores(heat, sk[1], skew_rule.coeff_table(sk[0], page_size, map_size))
        return self._skew_set(sk, result, scores, n_text, map_size)

    def _detect(self, images: List[Image.Image], batch_size=None, include_maps=False) -> List[TextDetectionResult]:
        if self.tiling is not None:
            check_tiling(self.tiling, self.processor.size["height"])
        sk = self._check_skew(images)
        cli = self._check_centerlines()
        if self.tiling is not None and not self.device_postprocess:
            return self._detect_tiled_host(images, batch_size, include_maps, sk, cli)
        if self.device_postprocess:
            return self._detect_device(images, batch_size, include_maps)
        gen = self.batch_detection(images, batch_size=batch_size)
        futures = []
        workers = max(1, min(settings.DETECTOR_POSTPROCESSING_CPU_WORKERS, len(images)))

        def one(p, s):
            info = None
            if cli is None:
                r = parallel_get_boxes(p, s, include_maps)
            else:                                          # the same steps (heatmap.py), with the profile of the same map in between
                heat = p[0] if p[0].dtype == np.float32 else p[0].astype(np.float32)
                tt, lt = settings.DETECTOR_TEXT_THRESHOLD, settings.DETECTOR_BLANK_THRESHOLD
                imgs = [Image.fromarray((m * 255).astype(np.uint8)) for m in p[:2]] if include_maps else [None, None]
                r, info = self._cl_result(cli, centerline_rule.profile_page(heat, tt, lt, cli.knots), *detect_boxes(heat, tt, lt),
                                          [heat.shape[1], heat.shape[0]], s, *imgs)
            return r, (None if sk is None else self._skew_host(sk, r, p[0], s, (p[0].shape[1], p[0].shape[0]))), info

        if len(images) >= settings.DETECTOR_MIN_PARALLEL_THRESH:
            with ThreadPoolExecutor(max_workers=workers) as ex:
                for preds, sizes in gen:
                    futures.extend(ex.submit(one, p, s) for p, s in zip(preds, sizes))
            out = [f.result() for f in futures]
        else:
            out = []
            for preds, sizes in gen:
                out.extend(one(p, s) for p, s in zip(preds, sizes))
        if sk is not None:
            self.last_skew = [info for _, info, _ in out]
        if cli is not None:
            self.last_centerlines = [info for _, _, info in out]
        return [r for r, _, _ in out]

    def _detect_device(self, images, batch_size=None, include_maps=False) -> List[TextDetectionResult]:
        return [r for batch in self._iter_detect_device(images, batch_size, include_maps) for r in batch]

    def iter_detect(self, images: List[Image.Image], batch_size=None) -> Generator[List[TextDetectionResult], None, None]:
        """The results of `__call__(images, batch_size)` handed over batch by batch, in page order, each as soon as ITS boxes have
        left the device (the next batch is already launched by then). What RecognitionPredictor's streamed detect -> recognise
        call consumes (recognition/predictor.py `_call_streamed`): lines of the first pages are admitted to the continuous-batching
        loop while the detector still works on the later ones. Single process, device post-processing only."""
        if not self.device_postprocess or self.shard_pages:
            raise RuntimeError("iter_detect needs the device post-processing path of one process (no DETECTOR_POSTPROCESS_HOST, no page sharding)")
        return self._iter_detect_device(images, batch_size, False, eager_first=True)

    def _iter_detect_device(self, images, batch_size=None, include_maps=False, eager_first=False):
        """eager_first: hand the FIRST batch over as soon as its boxes exist instead of after the second batch has been prepared and
        launched -- a consumer that starts other device work from it (the streamed recognise call) gets going one host preparation
        (~10 ms per 16 pages) earlier, at the price of that much overlap inside the detector."""
        if self.tiling is not None:
            check_tiling(self.tiling, self.processor.size["height"])
        sk = self._check_skew(images)
        cli = self._check_centerlines()
        if getattr(self, "_post", None) is None:
            self._post = HipDetPost(self.model.device)
        tt, lt = settings.DETECTOR_TEXT_THRESHOLD, settings.DETECTOR_BLANK_THRESHOLD
        if self.tiling is not None:
            yield from self._iter_detect_tiled(images, batch_size, include_maps, eager_first, sk, cli)
            return

        def finish(job):
            """Results of one launched batch (waits for ITS event only)."""
            out: List[TextDetectionResult] = []
            jobs, n_pages, tiles_of, split_heights, sizes, heat, pw = job
            res, skews = {}, {}
            for pages_, pending, psizes, spending, cpending in jobs:
                got = self._post.collect(pending)
                for pg, (bx, cf), psize, prof in zip(pages_, got, psizes, self._cl_collect(cpending, got)):
                    res[pg] = (bx, cf, psize, prof)
                if spending is not None:
                    for pg, sc, nt in zip(pages_, *self._skew_op.collect(spending)):
                        skews[pg] = (sc, nt)
            maps = heat.cpu().numpy() if include_maps else None      # callers that want the maps pay for their D2H
            for pg in range(n_pages):
                bx, cf, psize, prof = res[pg]
                hi = ai = None
                if include_maps:
                    # the reference keeps a page's FIRST tile whole -- an unsplit page shorter than the processor height still gets
                    # its full map -- and trims only the later strips of a split page to their valid rows (detection/__init__.py:134-151)
                    rows = [maps.shape[2] if k == 0 else split_heights[t] for k, t in enumerate(tiles_of[pg])]
                    hm = np.vstack([maps[t, 0, :r] for t, r in zip(tiles_of[pg], rows)])
                    am = np.vstack([maps[t, 1, :r] for t, r in zip(tiles_of[pg], rows)])
                    hi, ai = Image.fromarray((hm * 255).astype(np.uint8)), Image.fromarray((am * 255).astype(np.uint8))
                r, info = self._cl_result(cli, prof, bx, cf, list(psize), sizes[pg], hi, ai)
                out.append(r)
                if cli is not None:
                    self.last_centerlines.append(info)
                if sk is not None:
                    self.last_skew.append(self._skew_set(sk, out[-1], *skews[pg], psize))
            return out

        def launched():
            for heat, split_index, split_heights, sizes in self.batch_heatmaps(images, batch_size):
                ph, pw = heat.shape[2], heat.shape[3]
                n_pages = split_index[-1] + 1
                tiles_of = [[i for i, k in enumerate(split_index) if k == page] for page in range(n_pages)]
                whole = [page for page in range(n_pages) if len(tiles_of[page]) == 1]
                jobs = []
                if whole:
                    sel = heat if len(whole) == heat.shape[0] else heat[[tiles_of[pg][0] for pg in whole]].contiguous()
                    jobs.append((whole, self._post.launch(sel, tt, lt), [(pw, ph)] * len(whole),
                                 None if sk is None else self._skew_launch(sk, sel, [sizes[pg] for pg in whole], (pw, ph)),
                                 self._cl_launch(cli, sel)))
                # tall pages: strips re-assembled on the device (:134-151); pages of equal height share ONE post-processing call (a call per
                # page was 17 launches + a D2H each: 16 letter pages spent 40 of their 77 ms there, tools/hostbench/det_letter_profile.py)
                by_height = {}
                for pg in range(n_pages):
                    if len(tiles_of[pg]) > 1:
                        by_height.setdefault(sum(split_heights[t] for t in tiles_of[pg]), []).append(pg)
                for hf, pgs in by_height.items():
                    full = torch.empty((len(pgs), hf, pw), dtype=heat.dtype, device=heat.device)
                    for i, pg in enumerate(pgs):
                        r0 = 0
                        for t in tiles_of[pg]:
                            full[i, r0: r0 + split_heights[t]] = heat[t, 0, : split_heights[t]]
                            r0 += split_heights[t]
                    jobs.append((pgs, self._post.launch(full, tt, lt), [(pw, hf)] * len(pgs),
                                 None if sk is None else self._skew_launch(sk, full, [sizes[pg] for pg in pgs], (pw, hf)),
                                 self._cl_launch(cli, full)))
                yield (jobs, n_pages, tiles_of, split_heights, sizes, heat, pw)

        yield from _one_batch_ahead(launched(), finish, eager_first)

    # ------------------------------------------------------------------------------------------------------------ tiled detection
    def _iter_detect_tiled(self, images, batch_size, include_maps, eager_first, sk=None, cli=None):
        """_iter_detect_device under `tiling`: the same one-batch-ahead hand-over, a page's boxes from its stitched map."""
        tt, lt = settings.DETECTOR_TEXT_THRESHOLD, settings.DETECTOR_BLANK_THRESHOLD

        def finish(job):
            groups, sizes, pendings, spendings, cpendings = job
            out = [None] * len(sizes)
            infos = [None] * len(sizes)
            cinfos = [None] * len(sizes)
            for (ks, maps, (mw, mh)), pending, spending, cpending in zip(groups, pendings, spendings, cpendings):
                host = maps.cpu().numpy() if include_maps else None      # callers that want the maps pay for their D2H
                got = self._post.collect(pending)
                for i, (k, (bx, cf), prof) in enumerate(zip(ks, got, self._cl_collect(cpending, got))):
                    out[k], cinfos[k] = self._cl_result(cli, prof, bx, cf, [mw, mh], sizes[k], *self._map_images(host, i, mw, mh))
                if spending is not None:
                    for k, sc, nt in zip(ks, *self._skew_op.collect(spending)):
                        infos[k] = self._skew_set(sk, out[k], sc, nt, (mw, mh))
            if sk is not None:
                self.last_skew.extend(infos)
            if cli is not None:
                self.last_centerlines.extend(cinfos)
            return out

        def launched():
            for groups, sizes in self._tiled_batches(images, batch_size, 2 if include_maps else 1):
                # pages of equal map size share ONE post-processing call, as tall pages of equal height do; what reads a call's workspace
                # (the centre lines) goes right behind it, before the next call rewrites it
                pendings, spendings, cpendings = [], [], []
                for ks, maps, ms in groups:
                    pendings.append(self._post.launch(maps, tt, lt))
                    cpendings.append(self._cl_launch(cli, maps))
                    spendings.append(None if sk is None else self._skew_launch(sk, maps, [sizes[k] for k in ks], ms))
                yield groups, sizes, pendings, spendings, cpendings

        yield from _one_batch_ahead(launched(), finish, eager_first)

    def _detect_tiled_host(self, images, batch_size, include_maps, sk=None, cli=None):
        """The checker arm under `tiling` (DETECTOR_POSTPROCESS_HOST): the stitched maps D2H, heatmap.py on them."""
        tt, lt = settings.DETECTOR_TEXT_THRESHOLD, settings.DETECTOR_BLANK_THRESHOLD
        out = []
        for groups, sizes in self._tiled_batches(images, batch_size, 2 if include_maps else 1):
            res, infos, cinfos = [None] * len(sizes), [None] * len(sizes), [None] * len(sizes)
            for ks, maps, (mw, mh) in groups:
                host = maps.cpu().numpy()
                for i, k in enumerate(ks):
                    boxes, confs = detect_boxes(host[i, 0], tt, lt)
                    prof = None if cli is None else centerline_rule.profile_page(host[i, 0], tt, lt, cli.knots)
                    res[k], cinfos[k] = self._cl_result(cli, prof, boxes, confs, [mw, mh], sizes[k],
                                                        *self._map_images(host if include_maps else None, i, mw, mh))
                    if sk is not None:
                        infos[k] = self._skew_host(sk, res[k], host[i, 0], sizes[k], (mw, mh))
            if sk is not None:
                self.last_skew.extend(infos)
            if cli is not None:
                self.last_centerlines.extend(cinfos)
            out.extend(res)
        return out

    @staticmethod
    def _map_images(host, i, mw, mh):
        """include_maps under `tiling`: the stitched valid region (mh x mw) of both planes, as the reference's images."""
        if host is None:
            return None, None
        return tuple(Image.fromarray((host[i, pl, :mh, :mw] * 255).astype(np.uint8)) for pl in (0, 1))

    def _tiled_batches(self, images, batch_size, planes):
        """Upload -> [scale] -> per forward: cut, model, stitch (detection/tiling.py). Yields per batch of pages (groups, page sizes), groups =
        [(pages of the batch, their maps cuda fp32 [n, planes, mh, round_up(mw, 4)], (mw, mh))]: pages of equal map size lie in one tensor.
        Everything is enqueued and nothing waited for."""
        assert all(isinstance(im, Image.Image) for im in images)
        P = self.processor.size["height"]
        assert self.processor.size["width"] == P
        tiling = check_tiling(self.tiling, P)
        if batch_size is None:
            batch_size = self.get_batch_size()
        mb = self.model.max_batch
        batch_size = min(batch_size, mb)
        plans = [page_plan(im.size[0], im.size[1], P, tiling) for im in images]
        self.last_tiling = [{"size": pl.map_size, "grid": pl.grid, "tiles": pl.n_tiles} for pl in plans]
        batches, cur, cur_n = [], [], 0
        for i, pl in enumerate(plans):                             # greedy packing by tile count, as strips are packed
            if cur_n + pl.n_tiles > batch_size:
                if cur:
                    batches.append(cur)
                cur, cur_n = [], 0
            cur.append(i)
            cur_n += pl.n_tiles
        if cur:
            batches.append(cur)
        paths = self.last_resize_paths = {"device": 0, "host": 0, "ready": 0}
        if getattr(self, "_tiler", None) is None:
            self._tiler = HipDetTiler(self.model.device)
        dev = self.model.device
        for idxs in batches:
            pages = [images[j] if images[j].mode == "RGB" else images[j].convert("RGB") for j in idxs]
            bplans = [plans[j] for j in idxs]
            # how a page becomes its scaled page S: [] = it is S, a list of steps = on the device, None = Pillow on the host
            chains = [[] if pl.map_size == pl.size else (plan_resize(pl.size[0], pl.size[1], pl.map_size) if self.device_resize else None)
                      for pl in bplans]
            for ch in chains:
                paths["device" if ch else "ready" if ch is not None else "host"] += 1

            def pixels(k):
                return self.resize_image(pages[k], bplans[k].map_size) if chains[k] is None else page_pixels(pages[k])
            px = list(copy_pool().map(pixels, range(len(pages)))) if len(pages) > 1 else [pixels(0)]
            # ONE pinned staging buffer and ONE H2D copy per batch: the pages whole, then the two descriptor tables
            n_tiles = sum(pl.n_tiles for pl in bplans)
            sizes_b = [int(a.nbytes) for a in px]
            offs = np.concatenate([[0], np.cumsum([(b + 255) & ~255 for b in sizes_b])]).astype(np.int64)
            cut_off = int(offs[-1])
            stitch_off = cut_off + n_tiles * CUT_DESC.itemsize
            stage = torch.empty(stitch_off + n_tiles * STITCH_DESC.itemsize, dtype=torch.uint8, pin_memory=True)
            sv = stage.numpy()
            parallel_copy([sv[int(o): int(o) + b].reshape(a.shape) for a, o, b in zip(px, offs[:-1], sizes_b)], px)
            dev_stage = torch.empty(stage.numel(), dtype=torch.uint8, device=dev)
            scaled = [torch.empty((pl.map_size[1], pl.map_size[0], 4), dtype=torch.uint8, device=dev) if ch else None
                      for pl, ch in zip(bplans, chains)]
            by_size = {}
            for k, pl in enumerate(bplans):
                by_size.setdefault(pl.map_size, []).append(k)
            groups, map_of = [], {}
            for (mw, mh), ks in by_size.items():
                maps = torch.empty((len(ks), planes, mh, (mw + 3) & ~3), dtype=torch.float32, device=dev)
                groups.append((ks, maps, (mw, mh)))
                for i, k in enumerate(ks):
                    map_of[k] = maps[i].data_ptr()
            # the tiles of the batch in page order, row-major inside a page; a tile's index is its place in ITS forward
            cut, st = np.zeros(n_tiles, CUT_DESC), np.zeros(n_tiles, STITCH_DESC)
            t = 0
            for k, pl in enumerate(bplans):
                mw, mh = pl.map_size
                src = ((scaled[k].data_ptr(), mw, mh, 4) if scaled[k] is not None
                       else (dev_stage.data_ptr() + int(offs[k]), px[k].shape[1], px[k].shape[0], px[k].shape[2]))
                for x0, y0, (ox0, ox1), (oy0, oy1) in pl.tiles():
                    cut[t] = (*src, x0, y0, t % mb)
                    st[t] = (map_of[k], pl.pitch, mh * pl.pitch, t % mb, ox0 - x0, oy0 - y0, ox1 - ox0, oy1 - oy0, ox0, oy0, planes,
                             pl.pitch - mw if ox1 == mw else 0, 0)
                    t += 1
            sv[cut_off: stitch_off] = cut.view(np.uint8)
            sv[stitch_off:] = st.view(np.uint8)
            dev_stage.copy_(stage, non_blocking=True)
            for k, ch in enumerate(chains):
                if ch:
                    if getattr(self, "_resampler", None) is None:
                        self._resampler = DeviceResampler(dev)
                    img = dev_stage[int(offs[k]): int(offs[k]) + sizes_b[k]].view(px[k].shape)
                    for i, step in enumerate(ch):              # [thumbnail's box reduction,] thumbnail's size, then the scaled size
                        if step[0] == "reduce":
                            img = self._resampler.reduce(img, step[1], step[2])
                        else:
                            img = self._resampler.resize(img, step[1], out=scaled[k] if i == len(ch) - 1 else None, box=step[2])
            for s in range(0, n_tiles, mb):                        # a page with more tiles than the batch: chunks of max_batch, stitched as they come
                n = min(mb, n_tiles - s)
                tiles = torch.empty((n, P, P, 4), dtype=torch.uint8, device=dev)
                self._tiler.cut(dev_stage[cut_off + s * CUT_DESC.itemsize:], n, tiles)
                heat = self.model.forward_u8(tiles, self.processor.image_mean, self.processor.image_std)
                self._tiler.stitch(heat, dev_stage[stitch_off + s * STITCH_DESC.itemsize:], n)
            yield groups, [images[j].size for j in idxs]

    def resize_image(self, img: Image.Image, size=None) -> np.ndarray:
        """The reference's double LANCZOS resize to the processor size (surya/detection/__init__.py:50-57), or to `size` (a tiled page's
        scaled size), uint8 HWC."""
        new_size = size or (self.processor.size["width"], self.processor.size["height"])
        if img.size != new_size:
            img = img.copy()                                          # thumbnail() works in place; the page may be the caller's
            img.thumbnail(new_size, Image.Resampling.LANCZOS)
            img = img.resize(new_size, Image.Resampling.LANCZOS)
        return page_pixels(img)

    def prepare_image(self, img: Image.Image) -> torch.Tensor:
        new_size = (self.processor.size["width"], self.processor.size["height"])
        img.thumbnail(new_size, Image.Resampling.LANCZOS)          # the reference's double resize (:50-57)
        img = img.resize(new_size, Image.Resampling.LANCZOS)
        arr = np.asarray(img, dtype=np.uint8)
        return torch.from_numpy(self.processor(arr)["pixel_values"][0])

    def batch_heatmaps(self, images: List, batch_size=None):
        """Split -> prepare_image -> model, like batch_detection (surya/detection/__init__.py:64-132), but the heat maps stay
        on the device: yields (heat cuda fp32 [tiles, labels, H, W], page index of each tile, valid rows of each tile, sizes)."""
        assert all(isinstance(im, Image.Image) for im in images)
        if batch_size is None:
            batch_size = self.get_batch_size()
        batch_size = min(batch_size, self.model.max_batch)
        ph = self.processor.size["height"]
        orig_sizes = [im.size for im in images]
        splits = [get_total_splits(s, ph) for s in orig_sizes]
        batches, cur, cur_n = [], [], 0
        for i in range(len(images)):                               # greedy packing by tile count (:77-90)
            if cur_n + splits[i] > batch_size:
                if cur:
                    batches.append(cur)
                cur, cur_n = [], 0
            cur.append(i)
            cur_n += splits[i]
        if cur:
            batches.append(cur)
        paths = self.last_resize_paths = {"device": 0, "host": 0, "ready": 0}
        for idxs in batches:
            # the device path only READS the pages (zero-copy pixel views, resize on the device): no defensive copies of pages that
            # already are RGB (convert() and split_image() each copied 4 MB per 1024^2 page under the GIL; the Pillow resize of
            # the host path, which works in place, copies for itself in resize_image)
            batch_images = [images[j] if images[j].mode == "RGB" else images[j].convert("RGB") for j in idxs]
            split_index, split_heights, parts = [], [], []
            tall = sum(im.size[1] > settings.DETECTOR_IMAGE_CHUNK_HEIGHT for im in batch_images)
            cut = (list(copy_pool().map(lambda im: split_image(im, ph, copy=False), batch_images)) if tall > 1     # PIL crop / pad release the GIL
                   else [split_image(im, ph, copy=False) for im in batch_images])
            for k, (ps, hs) in enumerate(cut):
                parts.extend(ps)
                split_index.extend([k] * len(ps))
                split_heights.extend(hs)
            # pages go to the device as uint8; the reference's double LANCZOS resize to the processor size runs there too
            # (surya_reduce_u8 for the box reduction of >= 4x shrinks, surya_resample_lanczos_u8; bit-identical to Pillow) unless
            # Pillow would take a path the kernels do not restate (images > 100 x as tall as wide: common/pil_resample.plan_chain)
            # or DETECTOR_RESIZE_HOST=1 asks for the host path; rescale + normalise happen in the model's first kernel
            pw = self.processor.size["width"]
            plans = [None if not self.device_resize else plan_resize(p_.size[0], p_.size[1], (pw, ph)) for p_ in parts]
            pool = copy_pool()
            # pixels of every part: Pillow's own memory where it can export it (page_pixels), the Pillow double resize for the parts the
            # device path does not take; both release the GIL in their C loops, so the parts of a batch are prepared side by side
            if len(parts) > 1:
                px = list(pool.map(lambda k: self.resize_image(parts[k]) if plans[k] is None else page_pixels(parts[k]), range(len(parts))))
            else:
                px = [self.resize_image(parts[k]) if plans[k] is None else page_pixels(parts[k]) for k in range(len(parts))]
            # RGBX views of PIL's own memory where it can export them (page_pixels), else repacked RGB; one stride per batch
            ready = [k for k, pl in enumerate(plans) if pl is None or not pl]          # already at the processor size
            for k, pl in enumerate(plans):
                paths["device" if pl else "ready" if (pl is not None or parts[k].size == (pw, ph)) else "host"] += 1
            pix = 4 if all(px[k].shape[2] == 4 for k in ready) else 3
            host = torch.empty((len(parts), ph, pw, pix), dtype=torch.uint8, pin_memory=True)   # caching host allocator
            hv = host.numpy()
            parallel_copy([hv[k] for k in ready], [px[k] if px[k].shape[2] == pix else px[k][..., :3] for k in ready])
            dev_batch = host.to(self.model.device, non_blocking=True)
            todo = [k for k, pl in enumerate(plans) if pl]
            if todo:
                # the parts that need the double LANCZOS resize: ONE pinned staging buffer and ONE H2D copy for the batch (a pinned
                # allocation + copy + transfer per page cost ~4.7 ms of host time each: 210 pages/s on letter pages), then the resize
                # passes part by part on the device
                if getattr(self, "_resampler", None) is None:
                    self._resampler = DeviceResampler(self.model.device)
                sizes_b = [int(px[k].nbytes) for k in todo]
                offs_b = np.concatenate([[0], np.cumsum([(b + 255) & ~255 for b in sizes_b])]).astype(np.int64)
                stage = torch.empty(int(offs_b[-1]), dtype=torch.uint8, pin_memory=True)
                sv = stage.numpy()
                parallel_copy([sv[int(o): int(o) + b].reshape(px[k].shape) for k, o, b in zip(todo, offs_b[:-1], sizes_b)],
                              [px[k] for k in todo])
                dev_stage = stage.to(self.model.device, non_blocking=True)
                for k, o, b in zip(todo, offs_b[:-1], sizes_b):
                    cur = dev_stage[int(o): int(o) + b].view(px[k].shape)
                    pl = plans[k]
                    for i, st in enumerate(pl):                # [thumbnail's box reduction,] thumbnail's size, then the processor size
                        if st[0] == "reduce":
                            cur = self._resampler.reduce(cur, st[1], st[2])
                        else:
                            cur = self._resampler.resize(cur, st[1], out=dev_batch[k] if i == len(pl) - 1 else None, box=st[2])
            heat_parts = []
            for s in range(0, len(parts), self.model.max_batch):            # a single page may exceed max_batch tiles
                heat_parts.append(self.model.forward_u8(dev_batch[s: s + self.model.max_batch], self.processor.image_mean,
                                                        self.processor.image_std))
            heat = heat_parts[0] if len(heat_parts) == 1 else torch.cat(heat_parts, 0)
            yield heat, split_index, [min(h, ph) for h in split_heights], [orig_sizes[j] for j in idxs]

    def batch_detection(self, images: List, batch_size=None) -> Generator[Tuple[List[List[np.ndarray]], List[Tuple[int, int]]], None, None]:
        assert all(isinstance(im, Image.Image) for im in images)
        if batch_size is None:
            batch_size = self.get_batch_size()
        batch_size = min(batch_size, self.model.max_batch)
        nlab = self.model.cfg.num_labels
        ph = self.processor.size["height"]
        orig_sizes = [im.size for im in images]
        splits = [get_total_splits(s, ph) for s in orig_sizes]
        batches, cur, cur_n = [], [], 0
        for i in range(len(images)):                               # greedy packing by tile count (:77-90)
            if cur_n + splits[i] > batch_size:
                if cur:
                    batches.append(cur)
                cur, cur_n = [], 0
            cur.append(i)
            cur_n += splits[i]
        if cur:
            batches.append(cur)
        for idxs in batches:
            batch_images = [images[j].convert("RGB") for j in idxs]
            split_index, split_heights, parts = [], [], []
            for k, im in enumerate(batch_images):
                ps, hs = split_image(im, ph)
                parts.extend(ps)
                split_index.extend([k] * len(ps))
                split_heights.extend(hs)
            tiles = torch.stack([self.prepare_image(p) for p in parts], 0).contiguous()
            heat_parts = []
            for s in range(0, tiles.shape[0], self.model.max_batch):        # a single page may exceed max_batch tiles
                chunk = tiles[s: s + self.model.max_batch]
                if torch.device(self.model.device).type == "cuda":           # (a stand-in model on the CPU in the live cross-check)
                    chunk = chunk.pin_memory().to(self.model.device, non_blocking=True)
                heat_parts.append(self.model.forward(chunk))
            logits = torch.cat(heat_parts, 0).cpu().numpy()                 # fp32, one D2H per batch (:132)
            preds: List[List[np.ndarray]] = []
            for i, (idx, height) in enumerate(zip(split_index, split_heights)):
                maps = [logits[i][k] for k in range(nlab)]
                if len(preds) <= idx:
                    preds.append(maps)
                else:
                    if height < ph:
                        maps = [m[:height, :] for m in maps]               # cut the white padding of the last strip
                    preds[idx] = [np.vstack([preds[idx][k], maps[k]]) for k in range(nlab)]
            yield preds, [orig_sizes[j] for j in idxs]
