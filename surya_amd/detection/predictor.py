"""DetectionPredictor: drop-in for surya.detection.DetectionPredictor on MI355X.

Same call signature / result schema (surya/detection/__init__.py:22-48, detection/schema.py:12-17). The model forward,
sigmoid and x4 upsample run in libsurya_amd.so (HipDetModel). This file holds the sources of page maps (`batch_heatmaps`, `_tiled_batches`,
and `batch_detection`, the reference layout of the checker arm); what turns a page map into a result is detection/pagepost.py. No CPU
fallback for the model.
"""
from __future__ import annotations

import math
import os
from itertools import accumulate
from typing import Generator, List, Tuple

import numpy as np
import torch
from PIL import Image, ImageOps

from ..common.imageops import copy_pool, page_pixels, parallel_copy
from ..common.predictor import BasePredictor, ModelLoader, gc_paused
from ..config import DetConfig, det_config
from ..settings import settings
from .heatmap import TextDetectionResult
from ..common.pil_resample import plan_chain as plan_resize
from .model import CUT_DESC, STITCH_DESC, DeviceResampler, HipDetModel, HipDetTiler
from .pagepost import PageGroup, PagePost, stitched_map_images, strip_groups, strip_map_images
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


def pack_greedy(counts, batch_size):
    """The reference's greedy packing by tile count (surya/detection/__init__.py:77-90): page indices per batch, in order; a new batch
    starts when the next page would overflow it, none is empty, and a page with more tiles than the batch goes alone."""
    batches, filled = [], 0
    for i, n in enumerate(counts):
        if not batches or filled + n > batch_size:
            batches.append([])
            filled = 0
        batches[-1].append(i)
        filled += n
    return batches


def stage_pixels(px, tail=0):
    """ONE pinned staging buffer for the pixel arrays of a batch, hence ONE H2D copy (a pinned allocation + copy + transfer per page cost
    ~4.7 ms of host time each: 210 pages/s on letter pages): every array at a 256-byte aligned offset, `tail` more bytes behind them for
    what else travels with the batch. Returns (buffer, offsets; the last one is where the tail starts)."""
    offs = [0, *accumulate((int(a.nbytes) + 255) & ~255 for a in px)]
    stage = torch.empty(offs[-1] + tail, dtype=torch.uint8, pin_memory=True)
    sv = stage.numpy()
    parallel_copy([sv[o: o + a.nbytes].reshape(a.shape) for a, o in zip(px, offs)], px)
    return stage, offs


def run_chain(resampler, src, steps, out):
    """The steps of common/pil_resample.plan_chain on the device: [thumbnail's box reduction,] thumbnail's size, then the final size into `out`."""
    for i, st in enumerate(steps):
        if st[0] == "reduce":
            src = resampler.reduce(src, st[1], st[2])
        else:
            src = resampler.resize(src, st[1], out=out if i == len(steps) - 1 else None, box=st[2])


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

    def _op(self, name, cls):
        """The device op kept under `name`, created at its first use: a call that never needs it allocates nothing for it."""
        op = getattr(self, name, None)
        if op is None:
            op = cls(self.model.device)
            setattr(self, name, op)
        return op

    def _map_geometry(self, images):
        """(page size, size of the map its boxes come from) of every page: stitched under `tiling`, else the processor's square or a tall page's strips."""
        P, pw = self.processor.size["height"], self.processor.size["width"]
        if self.tiling is not None:
            return [(im.size, page_plan(im.size[0], im.size[1], P, self.tiling).map_size) for im in images]
        return [(im.size, (pw, im.size[1] if get_total_splits(im.size, P) > 1 else P)) for im in images]

    def _detect(self, images: List[Image.Image], batch_size=None, include_maps=False) -> List[TextDetectionResult]:
        return (self._detect_device if self.device_postprocess else self._detect_host)(images, batch_size, include_maps)

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
        post = PagePost(self, images)                      # every refusal of the call, before any device work

        def launched():
            if self.tiling is not None:
                for groups, sizes in self._tiled_batches(images, batch_size, 2 if include_maps else 1):
                    yield post.launch(groups, sizes, stitched_map_images(groups) if include_maps else None)
            else:
                for heat, split_index, split_heights, sizes in self.batch_heatmaps(images, batch_size):
                    yield post.launch(strip_groups(heat, split_index, split_heights), sizes,
                                      strip_map_images(heat, split_index, split_heights) if include_maps else None)

        yield from _one_batch_ahead(launched(), post.finish, eager_first)

    def _detect_host(self, images, batch_size=None, include_maps=False) -> List[TextDetectionResult]:
        """The checker arm (DETECTOR_POSTPROCESS_HOST): the page maps D2H, heatmap.py and the numpy references of the extras on them. Without
        `tiling` the maps come from `batch_detection`, the reference-layout path that shares nothing with `batch_heatmaps`."""
        post = PagePost(self, images)                      # every refusal of the call, before any device work

        def pages():
            if self.tiling is None:
                for preds, sizes in self.batch_detection(images, batch_size=batch_size):
                    for p, size in zip(preds, sizes):
                        yield p[0], p[1] if include_maps else None, (p[0].shape[1], p[0].shape[0]), size
                return
            for groups, sizes in self._tiled_batches(images, batch_size, 2 if include_maps else 1):
                batch = [None] * len(sizes)
                for ks, maps, map_size in groups:
                    host = maps.cpu().numpy()
                    for i, k in enumerate(ks):
                        batch[k] = (host[i, 0], host[i, 1] if include_maps else None, map_size, sizes[k])
                yield from batch

        return post.host(pages(), len(images))

    # ------------------------------------------------------------------------------------------------------------ the sources of page maps
    def _tiled_batches(self, images, batch_size, planes):
        """Upload -> [scale] -> per forward: cut, model, stitch (detection/tiling.py). Yields per batch of pages (groups, page sizes), groups =
        [(pages of the batch, their maps cuda fp32 [n, planes, mh, round_up(mw, 4)], (mw, mh))]: pages of equal map size lie in one tensor.
        Everything is enqueued and nothing waited for."""
        assert all(isinstance(im, Image.Image) for im in images)
        P = self.processor.size["height"]
        assert self.processor.size["width"] == P
        tiling = check_tiling(self.tiling, P)
        mb = self.model.max_batch
        batch_size = min(self.get_batch_size() if batch_size is None else batch_size, mb)
        plans = [page_plan(im.size[0], im.size[1], P, tiling) for im in images]
        self.last_tiling = [{"size": pl.map_size, "grid": pl.grid, "tiles": pl.n_tiles} for pl in plans]
        paths = self.last_resize_paths = {"device": 0, "host": 0, "ready": 0}
        tiler = self._op("_tiler", HipDetTiler)
        dev = self.model.device
        for idxs in pack_greedy([pl.n_tiles for pl in plans], batch_size):      # by tile count, as strips are packed
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
            stage, offs = stage_pixels(px, n_tiles * (CUT_DESC.itemsize + STITCH_DESC.itemsize))
            cut_off = offs[-1]
            stitch_off = cut_off + n_tiles * CUT_DESC.itemsize
            sv = stage.numpy()
            dev_stage = torch.empty(stage.numel(), dtype=torch.uint8, device=dev)
            scaled = [torch.empty((pl.map_size[1], pl.map_size[0], 4), dtype=torch.uint8, device=dev) if ch else None
                      for pl, ch in zip(bplans, chains)]
            by_size = {}
            for k, pl in enumerate(bplans):
                by_size.setdefault(pl.map_size, []).append(k)
            groups, map_of = [], {}
            for (mw, mh), ks in by_size.items():
                maps = torch.empty((len(ks), planes, mh, (mw + 3) & ~3), dtype=torch.float32, device=dev)
                groups.append(PageGroup(ks, maps, (mw, mh)))
                for i, k in enumerate(ks):
                    map_of[k] = maps[i].data_ptr()
            # the tiles of the batch in page order, row-major inside a page; a tile's index is its place in ITS forward
            cut, st = np.zeros(n_tiles, CUT_DESC), np.zeros(n_tiles, STITCH_DESC)
            t = 0
            for k, pl in enumerate(bplans):
                mw, mh = pl.map_size
                src = ((scaled[k].data_ptr(), mw, mh, 4) if scaled[k] is not None
                       else (dev_stage.data_ptr() + offs[k], px[k].shape[1], px[k].shape[0], px[k].shape[2]))
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
                    run_chain(self._op("_resampler", DeviceResampler), dev_stage[offs[k]: offs[k] + px[k].nbytes].view(px[k].shape), ch, scaled[k])
            for s in range(0, n_tiles, mb):                        # a page with more tiles than the batch: chunks of max_batch, stitched as they come
                n = min(mb, n_tiles - s)
                tiles = torch.empty((n, P, P, 4), dtype=torch.uint8, device=dev)
                tiler.cut(dev_stage[cut_off + s * CUT_DESC.itemsize:], n, tiles)
                heat = self.model.forward_u8(tiles, self.processor.image_mean, self.processor.image_std)
                tiler.stitch(heat, dev_stage[stitch_off + s * STITCH_DESC.itemsize:], n)
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
        batch_size = min(self.get_batch_size() if batch_size is None else batch_size, self.model.max_batch)
        ph = self.processor.size["height"]
        orig_sizes = [im.size for im in images]
        paths = self.last_resize_paths = {"device": 0, "host": 0, "ready": 0}
        for idxs in pack_greedy([get_total_splits(s, ph) for s in orig_sizes], batch_size):
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
            # pixels of every part: Pillow's own memory where it can export it (page_pixels), the Pillow double resize for the parts the
            # device path does not take; both release the GIL in their C loops, so the parts of a batch are prepared side by side

            def pixels(k):
                return self.resize_image(parts[k]) if plans[k] is None else page_pixels(parts[k])
            px = list(copy_pool().map(pixels, range(len(parts)))) if len(parts) > 1 else [pixels(0)]
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
                # the parts that need the double LANCZOS resize: staged together, then the resize passes part by part on the device
                stage, offs = stage_pixels([px[k] for k in todo])
                dev_stage = stage.to(self.model.device, non_blocking=True)
                for k, o in zip(todo, offs):
                    run_chain(self._op("_resampler", DeviceResampler), dev_stage[o: o + px[k].nbytes].view(px[k].shape), plans[k], dev_batch[k])
            heat_parts = [self.model.forward_u8(dev_batch[s: s + self.model.max_batch], self.processor.image_mean, self.processor.image_std)
                          for s in range(0, len(parts), self.model.max_batch)]      # a single page may exceed max_batch tiles
            heat = heat_parts[0] if len(heat_parts) == 1 else torch.cat(heat_parts, 0)
            yield heat, split_index, [min(h, ph) for h in split_heights], [orig_sizes[j] for j in idxs]

    def batch_detection(self, images: List, batch_size=None) -> Generator[Tuple[List[List[np.ndarray]], List[Tuple[int, int]]], None, None]:
        assert all(isinstance(im, Image.Image) for im in images)
        batch_size = min(self.get_batch_size() if batch_size is None else batch_size, self.model.max_batch)
        nlab = self.model.cfg.num_labels
        ph = self.processor.size["height"]
        orig_sizes = [im.size for im in images]
        for idxs in pack_greedy([get_total_splits(s, ph) for s in orig_sizes], batch_size):
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
