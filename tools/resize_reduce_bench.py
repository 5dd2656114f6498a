"""DetectionPredictor on pages whose thumbnail needs Pillow's box reduction (>= 4x shrinks): device resize against host resize.

    python tools/resize_reduce_bench.py [--repeats 5] [--arms device,host] [--out FILE]        # timing, one JSON line
    rocprofv3 --kernel-trace --stats --output-format rocpd -d DIR -- python tools/resize_reduce_bench.py --arms device --repeats 2 --out RUN.json
    python tools/resize_reduce_bench.py --trace-db DIR/.../*.db --trace-run RUN.json             # the reduce kernels of that trace
    python tools/resize_reduce_bench.py --arms kernel                                            # the reduce kernel alone

One process, DET-DEFAULT synthetic weights at 1024. Pages (seeded): four 5100 x 6600 (600-dpi letter scans, seven 5100 x 1024 strips
each) and four 6000 x 4000 (24-MP photos, four strips each). `pred(pages)` is timed with `device_resize` True and False, the two arms
alternating, both warmed, a device synchronise before each clock read; on these pages the False arm is what the predictor did before
the reduction ran on the device. Reported: ms per page per arm (median, min, max over the repeats), the parts that took each path,
whether the two arms returned the same boxes. `reduce_kernel`: `DeviceResampler.reduce` alone on the strips' shapes at both pixel
strides, device events, over a ring of source buffers larger than the 256 MiB Infinity Cache, with bytes (source read once +
destination written once, from the shapes) over time against the HBM rates. With --trace-db: the same bytes over the reduce
kernels' time in a kernel trace of the device arm."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_SPEC_TBS, HBM_COPY_TBS = 8.0, 6.29          # MI355X: HBM3E peak, and what a float4 copy reaches of it
PAGE_SIZES = [(5100, 6600)] * 4 + [(6000, 4000)] * 4
SIZE = 1024


def make_big_pages(seed=7):
    import numpy as np
    from PIL import Image
    from surya_amd.synth import make_pages
    rng = np.random.default_rng(seed)
    return [Image.fromarray(make_pages(1, SIZE, seed=int(rng.integers(1 << 30)))[0]).resize(wh, Image.Resampling.BILINEAR)
            for wh in PAGE_SIZES]


def reduce_bytes_per_call(pages):
    """(bytes the reduce kernels of one pred(pages) call read + write, their launches' shapes) from the shapes alone."""
    from surya_amd.common.imageops import page_pixels
    from surya_amd.common.pil_resample import plan_chain
    from surya_amd.detection.predictor import split_image
    total, shapes = 0, {}
    for im in pages:
        for part in split_image(im, SIZE, copy=False)[0]:
            w, h = part.size
            st = plan_chain(w, h, (SIZE, SIZE))
            if st and st[0][0] == "reduce":
                spix = int(page_pixels(part).shape[2])
                _, fx, fy = st[0]
                b = w * h * spix + -(-w // fx) * -(-h // fy) * 4
                total += b
                key = f"{w}x{h}x{spix} / ({fx},{fy})"
                shapes[key] = shapes.get(key, 0) + 1
    return total, shapes


def kernel_alone(device):
    """DeviceResampler.reduce on the strips' shapes, both strides: us per call and bytes / time."""
    import torch
    from surya_amd.detection.model import DeviceResampler
    rs = DeviceResampler(device)
    out = []
    for w, h, spix, fx, fy in [(5100, 1024, 3, 2, 2), (5100, 1024, 4, 2, 2), (6000, 1024, 3, 2, 2), (6000, 1024, 4, 2, 2),
                               (7680, 1024, 4, 3, 3), (5101, 1024, 3, 2, 2)]:
        nbuf = (600 << 20) // (w * h * spix) + 1                         # the ring outgrows the Infinity Cache
        src = torch.randint(0, 256, (nbuf, h, w, spix), dtype=torch.uint8, device=device)
        dst = torch.empty((-(-h // fy), -(-w // fx), 4), dtype=torch.uint8, device=device)
        for i in range(nbuf):
            rs.reduce(src[i], fx, fy, out=dst)
        torch.cuda.synchronize()
        reps = 3 * nbuf
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(reps):
            rs.reduce(src[i % nbuf], fx, fy, out=dst)
        b.record()
        b.synchronize()
        us = a.elapsed_time(b) * 1e3 / reps
        nbytes = w * h * spix + dst.numel()
        path = "generic" if (w * spix) % 4 else "span"
        out.append({"shape": f"{w}x{h}x{spix} / ({fx},{fy})", "kernel": path, "us_per_call_back_to_back": round(us, 2), "bytes": nbytes,
                    "TB_per_s": round(nbytes / us / 1e6, 3), "of_hbm_copy_rate": round(nbytes / us / 1e6 / HBM_COPY_TBS, 3),
                    "of_hbm_spec": round(nbytes / us / 1e6 / HBM_SPEC_TBS, 3)})
        del src
    return out


def same_results(a, b):
    return len(a) == len(b) and all(
        x.image_bbox == y.image_bbox and len(x.bboxes) == len(y.bboxes)
        and all(p.polygon == q.polygon and p.confidence == q.confidence for p, q in zip(x.bboxes, y.bboxes)) for x, y in zip(a, b))


def run(args):
    import torch
    from surya_amd.config import det_config
    from surya_amd.detection.predictor import DetectionPredictor
    from surya_amd.synth import make_det_weights
    if not torch.cuda.is_available():
        raise SystemExit("resize_reduce_bench: needs a GPU; nothing is measured without one")
    if args.arms == "kernel":                           # the reduce kernel alone (under a kernel trace: its time per template)
        return {"tool": "resize_reduce_bench", "reduce_kernel": kernel_alone("cuda:0")}
    cfg = det_config("DET-DEFAULT")
    pred = DetectionPredictor(checkpoint={"config": cfg, "state_dict": make_det_weights(cfg, 0), "size": SIZE})
    pages = make_big_pages()
    arms = args.arms.split(",")
    times = {a: [] for a in arms}
    paths, results = {}, {}

    def call(arm):
        pred.device_resize = arm == "device"
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = pred(pages)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    calls = 0
    for arm in arms:                                    # warm-up of both arms (pinned buffers, tables, code objects)
        _, results[arm] = call(arm)
        paths[arm] = dict(pred.last_resize_paths)
        calls += arm == "device"
    for _ in range(args.repeats):                       # alternating
        for arm in arms:
            ms, _ = call(arm)
            times[arm].append(ms)
            calls += arm == "device"
    nbytes, shapes = reduce_bytes_per_call(pages)
    line = {"tool": "resize_reduce_bench", "pages": [list(s) for s in PAGE_SIZES], "processor_size": SIZE, "repeats": args.repeats,
            "ms_per_page": {a: {"median": round(statistics.median(t) / len(pages), 2), "min": round(min(t) / len(pages), 2),
                                "max": round(max(t) / len(pages), 2), "all_calls_ms": [round(x, 1) for x in t]} for a, t in times.items()},
            "resize_paths": paths, "device_arm_calls": calls, "reduce_bytes_per_call": nbytes, "reduce_launch_shapes_per_call": shapes}
    if len(arms) == 2:
        line["same_boxes_both_arms"] = same_results(results[arms[0]], results[arms[1]])
    if not args.no_kernel:
        line["reduce_kernel"] = kernel_alone(pred.model.device)
    return line


def trace(args):
    import sqlite3
    with open(args.trace_run) as f:
        runline = json.loads(f.read().strip().splitlines()[-1])
    c = sqlite3.connect(args.trace_db)
    sym_cols = [r[1] for r in c.execute("pragma table_info(rocpd_info_kernel_symbol)")]
    name_col = "kernel_name" if "kernel_name" in sym_cols else ("display_name" if "display_name" in sym_cols else sym_cols[-1])
    rows = list(c.execute(f"""select s.{name_col}, count(*), sum(d.end - d.start) from rocpd_kernel_dispatch d
                              join rocpd_info_kernel_symbol s on d.kernel_id = s.id where s.{name_col} like '%reduce_span_kernel%'
                              or s.{name_col} like '%reduce_generic_kernel%' group by s.{name_col} order by 3 desc"""))
    ns = sum(r[2] for r in rows)
    nbytes = runline["reduce_bytes_per_call"] * runline["device_arm_calls"]
    return {"tool": "resize_reduce_bench --trace-db", "device_arm_calls": runline["device_arm_calls"],
            "reduce_kernels": [{"kernel": r[0][:120], "dispatches": r[1], "total_ms": round(r[2] / 1e6, 3), "avg_us": round(r[2] / r[1] / 1e3, 2)}
                               for r in rows],
            "reduce_bytes_from_shapes": nbytes, "reduce_kernel_time_ms": round(ns / 1e6, 3),
            "TB_per_s": round(nbytes / ns / 1e3, 3) if ns else None,
            "of_hbm_copy_rate": round(nbytes / ns / 1e3 / HBM_COPY_TBS, 3) if ns else None,
            "of_hbm_spec": round(nbytes / ns / 1e3 / HBM_SPEC_TBS, 3) if ns else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--arms", default="device,host")
    ap.add_argument("--no-kernel", action="store_true", help="skip the timing of the reduce kernel alone")
    ap.add_argument("--out")
    ap.add_argument("--trace-db")
    ap.add_argument("--trace-run", help="the JSON line the traced run wrote (--out)")
    args = ap.parse_args()
    line = json.dumps(trace(args) if args.trace_db else run(args))
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
