"""The contrast adjustment alone, and a 256-line call with `reread` off against the same call with about a tenth of its lines re-read
(RecognitionPredictor.reread, csrc/rec_adjust.h).

Leg 1: the end-to-end leg's pages and line boxes (bench.py: synth.make_pages_with_lines(pages, 1024, seed=4321), ~22 rows per page), every
row with `adjust` set: the device time of surya_rec_adjust_contrast (events around the call) and the bytes it moves per second -- each crop
is read twice (histogram, apply) and written once. Arm "off" is the same DevicePreprocessor call without `adjust`.
Leg 2: REC-FULL, bf16, synthetic weights, the headline leg's 256 ragged crops as PIL images with one box each through
RecognitionPredictor.__call__: `reread` off, then Reread(below=q, contrast=2) and Reread(below=q, contrast=2, rotations=(180,)) with q the
confidence under which a tenth of the plain call's lines lie. Arms alternated in one process, best of 3, wall clock of the call.

    python tools/microbench/reread_bench.py --out profiles/r27_a_reread.json
"""
import argparse, dataclasses, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np, torch
from PIL import Image

ap = argparse.ArgumentParser()
ap.add_argument("--pages", type=int, default=128)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--cutoff", type=int, default=2)
ap.add_argument("--rgbx", type=int, default=1, help="1: 4-byte pixels, the layout page_pixels hands over; 0: RGB")
ap.add_argument("--lines", type=int, default=256)
ap.add_argument("--config", default="REC-FULL")
ap.add_argument("--max-tokens", type=int, default=48)
ap.add_argument("--share", type=float, default=0.10, help="share of the call's lines the gate makes doubtful")
ap.add_argument("--no-call", action="store_true", help="leg 1 only")
ap.add_argument("--out", default=None)
args = ap.parse_args()
res = {"method": "arms alternated in one process, best of 3, wall time synchronised at both ends; 1 GPU"}


# ------------------------------------------------------------------------------------------------ leg 1: the entry point
def adjust_leg():
    from surya_amd.recognition.preprocess_gpu import DevicePreprocessor, poly_ref
    from surya_amd.synth import make_pages_with_lines
    pages, rows = make_pages_with_lines(args.pages, args.size, seed=4321)
    if args.rgbx:
        pages = [np.concatenate([p, np.zeros(p.shape[:2] + (1,), np.uint8)], axis=2) for p in pages]
    pix = 4 if args.rgbx else 3
    off = [poly_ref(i, args.size, args.size, [[b[0], b[1]], [b[2], b[1]], [b[2], b[3]], [b[0], b[3]]]) for i, rr in enumerate(rows) for b in rr]
    on = [dataclasses.replace(ln, adjust=args.cutoff) for ln in off]
    sizes = [(1024, 256)] * len(on)

    class TimedLib:
        """The library with events around surya_rec_adjust_contrast."""

        def __init__(self, lib):
            self._lib, self.events = lib, None

        def __getattr__(self, key):
            fn = getattr(self._lib, key)
            if key != "surya_rec_adjust_contrast":
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
        return wall, (ev[0].elapsed_time(ev[1]) if ev else 0.0)

    run(off); run(on)                                       # warm-up: allocator, pinned staging, code objects
    best = {"off": None, "on": None}
    for _ in range(3):
        for arm, lines in (("off", off), ("on", on)):
            r = run(lines)
            best[arm] = r if best[arm] is None else (min(best[arm][0], r[0]), min(best[arm][1], r[1]))
    px = sum(ln.shape[0] * ln.shape[1] for ln in on)
    moved = 3 * px * pix
    ms = best["on"][1]
    return {"pages": args.pages, "page_size": args.size, "pixel_stride": pix, "lines": len(on), "cutoff": args.cutoff, "adjusted_pixels": px,
            "adjust_contrast_ms": round(ms, 3), "bytes_moved": moved, "gb_per_s": round(moved / (ms * 1e-3) / 1e9, 1) if ms else None,
            "launches": 1 + 5 * ((len(on) + 31) // 32), "masked_lines": len(on),
            "preprocess_call_ms": {"adjust_off": round(best["off"][0], 2), "adjust_on": round(best["on"][0], 2)}}


# -------------------------------------------------------------------------------------------------- leg 2: the whole call
def call_leg():
    from surya_amd.config import rec_config
    from surya_amd.recognition.predictor import RecognitionModelLoader, RecognitionPredictor
    from surya_amd.recognition.reread import Reread
    from surya_amd.settings import settings
    from surya_amd.synth import make_line_crops, make_rec_weights
    settings.reload()
    settings.RECOGNITION_MAX_TOKENS = args.max_tokens
    cfg = rec_config(args.config)
    sd = make_rec_weights(cfg, 0, recipe="conditioned")

    class Loader(RecognitionModelLoader):
        def model(self, device=None, dtype=None, **caps):
            return super().model("cuda:0", dtype, max_slots=args.lines, max_kv_len=64 + args.max_tokens + 32, max_patches=65536,
                                 max_prefill_tokens=args.lines * 72)

    class Pred(RecognitionPredictor):
        model_loader_cls = Loader
        batch_size = args.lines

    pred = Pred(checkpoint={"config": cfg, "state_dict": sd})
    crops = make_line_crops(args.lines, seed=1234)
    imgs = [Image.fromarray(np.ascontiguousarray(c).astype(np.uint8)) for c in crops]
    boxes = [[[0, 0, im.size[0], im.size[1]]] for im in imgs]
    plain = pred(imgs, bboxes=boxes)
    conf = sorted(r.text_lines[0].confidence for r in plain if r.text_lines[0].text != "")
    q = float(conf[max(0, int(len(conf) * args.share) - 1)]) + 1e-9 if conf else 0.0
    arms = {"off": None, "contrast": Reread(below=q, contrast=args.cutoff), "contrast_rot180": Reread(below=q, contrast=args.cutoff, rotations=(180,))}
    best, info = {}, {}
    for rep in range(4):                                    # the first round is the warm-up
        for arm, setting in arms.items():
            pred.reread = setting
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = pred(imgs, bboxes=boxes)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            if rep:
                best[arm] = min(best.get(arm, ms), ms)
            t = pred.last_timing
            info[arm] = {"reread_lines": t.get("reread_lines"), "reread_variants": t.get("reread_variants"), "reread_ms": round(t.get("reread_ms", 0.0), 2),
                         "winners": {v: sum(r.text_lines[0].variant == v for r in out) for v in ("contrast", "rot180")} if setting else None}
    pred.reread = None
    return {"config": args.config, "dtype": str(pred.model.dtype), "lines": args.lines, "max_tokens": args.max_tokens, "below": q,
            "nonempty_lines": len(conf), "call_ms": {k: round(v, 2) for k, v in best.items()}, "second_pass": info}


res["adjust_entry"] = adjust_leg()
if not args.no_call:
    res["call_256_lines"] = call_leg()
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
