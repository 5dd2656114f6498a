"""DetectionPredictor with and without `tiling` on A4 scans at 300 dpi: what tiled detection costs.

    python tools/microbench/det_tile_bench.py [--repeats 3] [--arms plain,tile0.5,tile1.0] [--pages 16] [--out FILE]     # one JSON line
    SURYA_AMD_LIB=/path/to/another/libsurya_amd.so python tools/microbench/det_tile_bench.py --arms plain               # the plain arm on another build

One process, DET-DEFAULT synthetic weights, bf16, processor size 1024. Pages (seeded): 16 of 2480 x 3508. Arms: `plain` (tiling = None:
four 1024-row strips per page, each squeezed onto the square), `tile0.5` and `tile1.0` (DetTiling(scale, overlap 128)). `pred(pages)`
is timed per arm, the arms alternating, all warmed, a device synchronise before each clock read; reported per arm: pages / s of the best
and of every repeat (the spread of identical repeats is the margin any comparison of two arms or two builds has), tiles per page, boxes.
For the tiled arms one more call runs with a device event around every cut and every stitch launch: their share of the call's device
time, and the bytes they must move (from the grid alone: window pixels inside the page read + the tile written; owned rectangle read +
written, pad columns written) over that time, against what a float4 copy reaches on this HBM.

Synthetic weights: nothing here says what tiling does to recall on real scans -- there is no trained checkpoint to measure it with."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

HBM_COPY_TBS = 6.29                              # MI355X: what a float4 copy reaches of the 8 TB/s HBM3E peak
PAGE_SIZE, SIZE, OVERLAP = (2480, 3508), 1024, 128


def make_scans(n, seed=7):
    import numpy as np
    from PIL import Image
    from surya_amd.synth import make_pages
    rng = np.random.default_rng(seed)
    return [Image.fromarray(make_pages(1, SIZE, seed=int(rng.integers(1 << 30)))[0]).resize(PAGE_SIZE, Image.Resampling.BILINEAR)
            for _ in range(n)]


def copy_bytes(pages, tiling, src_pix_of):
    """(cut bytes, stitch bytes) one call must move, from the grid alone."""
    from surya_amd.detection.tiling import page_plan
    cut = stitch = 0
    for k, im in enumerate(pages):
        pl = page_plan(im.size[0], im.size[1], SIZE, tiling)
        mw, mh = pl.map_size
        spix = 4 if pl.map_size != pl.size else src_pix_of[k]          # a scaled page is RGBX
        for x0, y0, (xa, xb), (ya, yb) in pl.tiles():
            cut += (min(x0 + SIZE, mw) - x0) * (min(y0 + SIZE, mh) - y0) * spix + SIZE * SIZE * 4
            stitch += (xb - xa) * (yb - ya) * 4 * 2 + (pl.pitch - mw if xb == mw else 0) * (yb - ya) * 4
    return cut, stitch


def run(args):
    import torch
    from surya_amd.common.imageops import page_pixels
    from surya_amd.config import det_config
    from surya_amd.detection.predictor import DetectionPredictor, DetTiling
    from surya_amd.synth import make_det_weights
    if not torch.cuda.is_available():
        raise SystemExit("det_tile_bench: needs a GPU; nothing is measured without one")
    cfg = det_config("DET-DEFAULT")
    pred = DetectionPredictor(checkpoint={"config": cfg, "state_dict": make_det_weights(cfg, 0), "size": SIZE}, dtype=torch.bfloat16)
    pages = make_scans(args.pages)
    arms = args.arms.split(",")
    tilings = {a: None if a == "plain" else DetTiling(scale=float(a[len("tile"):]), overlap=OVERLAP) for a in arms}

    def call(arm):
        pred.tiling = tilings[arm]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = pred(pages)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    times, info = {a: [] for a in arms}, {}
    for arm in arms:                                                    # warm-up of every arm (pinned buffers, tables, code objects)
        _, r = call(arm)
        info[arm] = {"boxes": sum(len(x.bboxes) for x in r),
                     "tiles_per_page": (sum(t["tiles"] for t in pred.last_tiling) / len(pages)) if tilings[arm] else None,
                     "resize_paths": dict(pred.last_resize_paths)}
    for _ in range(args.repeats):                                       # alternating
        for arm in arms:
            times[arm].append(call(arm)[0])
    line = {"tool": "det_tile_bench", "lib": os.environ.get("SURYA_AMD_LIB", "in-tree"), "config": "DET-DEFAULT bf16", "processor_size": SIZE,
            "pages": args.pages, "page_size": list(PAGE_SIZE), "overlap": OVERLAP, "repeats": args.repeats, "batch_size": pred.get_batch_size(),
            "arms": {a: {"pages_per_s_best": round(len(pages) / min(t), 2), "pages_per_s_all": [round(len(pages) / x, 2) for x in t],
                         "ms_per_call_best": round(min(t) * 1e3, 1), **info[a]} for a, t in times.items()}}
    src_pix_of = [int(page_pixels(im).shape[2]) for im in pages]
    for arm in arms:                                                    # the two copies under device events, one extra call per tiled arm
        if tilings[arm] is None:
            continue
        pred.tiling = tilings[arm]
        pred(pages)
        tiler, spans = pred._tiler, {"cut": [], "stitch": []}

        def timed(name, fn):
            def wrapped(*a, **k):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(*a, **k)
                e1.record()
                spans[name].append((e0, e1))
            return wrapped
        tiler.cut, tiler.stitch = timed("cut", tiler.cut), timed("stitch", tiler.stitch)
        try:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            pred(pages)
            b.record()
            b.synchronize()
        finally:
            del tiler.cut, tiler.stitch
        ms = {k: sum(e0.elapsed_time(e1) for e0, e1 in v) for k, v in spans.items()}
        call_ms = a.elapsed_time(b)
        cb, sb = copy_bytes(pages, tilings[arm], src_pix_of)
        line["arms"][arm]["copies"] = {
            "call_device_ms": round(call_ms, 2), "cut_ms": round(ms["cut"], 3), "stitch_ms": round(ms["stitch"], 3),
            "launches": {k: len(v) for k, v in spans.items()}, "share_of_call": round((ms["cut"] + ms["stitch"]) / call_ms, 4),
            "cut_bytes": cb, "stitch_bytes": sb, "cut_GB_per_s": round(cb / ms["cut"] / 1e6, 1), "stitch_GB_per_s": round(sb / ms["stitch"] / 1e6, 1),
            "cut_of_hbm_copy_rate": round(cb / ms["cut"] / 1e9 / HBM_COPY_TBS, 3), "stitch_of_hbm_copy_rate": round(sb / ms["stitch"] / 1e9 / HBM_COPY_TBS, 3)}
    pred.tiling = None
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--arms", default="plain,tile0.5,tile1.0")
    ap.add_argument("--pages", type=int, default=16)
    ap.add_argument("--out")
    args = ap.parse_args()
    line = json.dumps(run(args))
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
