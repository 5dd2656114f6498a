"""Line pre-processing with every line rectified against the same call with none (RecognitionPredictor.rectify, csrc/rec_rectify.h).

The pages and line boxes are the end-to-end leg's (bench.py: synth.make_pages_with_lines(pages, 1024, seed=4321), ~22 rows per page).
Arm "off": every row as poly_ref of its rectangle -- today's path. Arm "on": the same rows as quads, each turned by --tilt degrees about
its centre, so every line goes through surya_rec_rectify in front of surya_rec_preprocess. One DevicePreprocessor call per arm, the arms
alternated in one process, best of 3 each. Reported: the device time of surya_rec_rectify alone (events around the call) and the wall
time of the whole pre-processing call (host descriptors, upload, kernels, synchronised) per arm. One JSON object; --out writes it too.

    python tools/microbench/rectify_bench.py --out profiles/r22_a_rectify_microbench.json
"""
import argparse, json, math, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np, torch
from surya_amd.recognition.preprocess_gpu import DevicePreprocessor, poly_ref, quad_ref
from surya_amd.synth import make_pages_with_lines

ap = argparse.ArgumentParser()
ap.add_argument("--pages", type=int, default=128)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--tilt", type=float, default=5.0, help="degrees every row's quad is turned by in the arm with rectification on")
ap.add_argument("--rgbx", type=int, default=1, help="1: 4-byte pixels, the layout page_pixels hands over; 0: RGB")
ap.add_argument("--out", default=None)
args = ap.parse_args()

pages, rows = make_pages_with_lines(args.pages, args.size, seed=4321)
if args.rgbx:
    pages = [np.concatenate([p, np.zeros(p.shape[:2] + (1,), np.uint8)], axis=2) for p in pages]
c, s = math.cos(math.radians(args.tilt)), math.sin(math.radians(args.tilt))


def turned(x0, y0, x1, y1):
    cx, cy, w, h = (x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0
    return [(cx + c * x - s * y, cy + s * x + c * y) for x, y in ((-w / 2, -h / 2), (w / 2, -h / 2), (w / 2, h / 2), (-w / 2, h / 2))]


off = [poly_ref(i, args.size, args.size, [[b[0], b[1]], [b[2], b[1]], [b[2], b[3]], [b[0], b[3]]]) for i, rr in enumerate(rows) for b in rr]
on = [quad_ref(i, args.size, args.size, turned(*b)) for i, rr in enumerate(rows) for b in rr]
sizes = [(1024, 256)] * len(on)


class TimedLib:
    """The library with events around surya_rec_rectify."""

    def __init__(self, lib):
        self._lib, self.events = lib, None

    def __getattr__(self, key):
        fn = getattr(self._lib, key)
        if key != "surya_rec_rectify":
            return fn

        def timed(*a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*a)
            e1.record()
            self.events = (e0, e1)
            return rc
        return timed


pre = DevicePreprocessor("cuda:0")
pre.lib = TimedLib(pre.lib)


def run(lines):
    pre.lib.events = None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tiles, offs, grids = pre(pages, lines, sizes)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    ev = pre.lib.events
    return wall, (ev[0].elapsed_time(ev[1]) if ev else 0.0), int(offs[-1])


run(off); run(on)                                           # warm-up: allocator, pinned staging, code objects
best = {"off": None, "on": None}
for _ in range(3):
    for arm, lines in (("off", off), ("on", on)):
        r = run(lines)
        best[arm] = r if best[arm] is None else (min(best[arm][0], r[0]), min(best[arm][1], r[1]), r[2])      # each figure's own best
px = sum(ln.shape[0] * ln.shape[1] for ln in on)
res = {"pages": args.pages, "page_size": args.size, "pixel_stride": 4 if args.rgbx else 3, "lines": len(on), "tilt_deg": args.tilt,
       "rectified_pixels": px, "rectify_kernels_ms": round(best["on"][1], 3),
       "rectify_gpix_per_s": round(px / (best["on"][1] * 1e-3) / 1e9, 2) if best["on"][1] else None,
       "preprocess_call_ms": {"rectify_off": round(best["off"][0], 2), "rectify_on": round(best["on"][0], 2)},
       "patch_rows": {"rectify_off": best["off"][2], "rectify_on": best["on"][2]},
       "method": "one DevicePreprocessor call per arm, arms alternated in one process, best of 3; wall time synchronised at both ends"}
print(json.dumps(res))
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
