"""Times LayoutPredictor.__call__ and TableRecPredictor.__call__ on pages as a user hands them (bf16, synthetic LAYOUT-DEFAULT /
TABLE-DEFAULT weights), with a per-call breakdown.

It uses the public API only, so it runs on any tree of this project (`--root`): on one without the device pre-processing it prints the
call and engine times only. Per call:
  call_ms      wall time of the predictor call (device synchronised before and after);
  engine_ms    wall time spent inside the model's methods (encode, prefill, select, set_feedback, decode_steps, wait_steps, ...): the
               first wait of a batch also covers what was queued before it, i.e. the upload and, on the device path, the pre-processing
               kernel;
  staging_ms   (device path) host time of the pre-processing: descriptors and copies into the pinned staging buffer;
  prep_gpu_ms  (device path) the pre-processing kernels by hipEvent;
  ratio        call_ms / engine_ms.
Sets: 128 pages of 816 x 1056, 128 of 1632 x 2112 (sliced: above 1500 px), 128 of 768 x 768, and 32 table crops of mixed sizes
(16 per batch, box loop capped at 40 tokens: see TABLE_MAX_BOXES). --profile SET adds a cProfile of one more call of that set.

    python tools/layout_call_bench.py [--root TREE] [--sets a,b] [--label NAME] [--out FILE.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

LAYOUT_SETS = {"letter96": (816, 1056), "letter192": (1632, 2112), "square768": (768, 768)}
TABLE_SIZES = [(500, 300), (320, 200), (900, 600), (1200, 400), (250, 700), (640, 480), (1000, 1000), (1400, 900)]
# Synthetic table weights seldom emit the end token, so every table runs its box loop to the cap: at the reference's 150 (a 32-crop call
# then decodes ~84 k cells in ~37 s, and the engine's run-to-run noise of a few seconds hides any pre-processing). The table set caps the
# loop at TABLE_MAX_BOXES tokens (the 21-token prompt included) through the predictor module's own constant, and 16 tables per batch
# keep the second pass's prompts (every row prompt carries all the columns of its batch) inside the engine's 512 prompt positions.
TABLE_MAX_BOXES = 40
TABLE_BATCH = 16
ENGINE_METHODS = ("encode", "encode_host", "prefill", "select", "set_feedback", "decode_step", "decode_steps", "wait_steps")


def _pages(size, n, seed):
    import numpy as np
    from PIL import Image
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        w, h = size(k) if callable(size) else size
        # a few flat blocks on a light page: deterministic, cheap to make, not all noise
        a = np.full((h, w, 3), 235, np.uint8)
        for _ in range(6):
            x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
            a[y0:y0 + max(1, h // 10), x0:x0 + max(1, w // 3)] = rng.integers(0, 120, size=3, dtype=np.uint8)
        out.append(Image.fromarray(a))
    return out


class EngineTimer:
    """Wraps the model's methods on the instance; counts only the outermost call (encode_host calls encode)."""

    def __init__(self, model):
        self.ms, self._depth = 0.0, 0
        for name in ENGINE_METHODS:
            fn = getattr(model, name, None)
            if fn is not None:
                setattr(model, name, self._wrap(fn))

    def _wrap(self, fn):
        def timed(*a, **k):
            self._depth += 1
            t0 = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                self._depth -= 1
                if self._depth == 0:
                    self.ms += (time.perf_counter() - t0) * 1e3
        return timed


def _timed_call(pred, images, timer, **kw):
    import torch
    prep = getattr(pred, "device_prep", None)
    if prep is not None:
        prep.timing, prep.timings = True, []
    torch.cuda.synchronize()
    timer.ms = 0.0
    t0 = time.perf_counter()
    out = pred(images, **kw)
    torch.cuda.synchronize()
    rec = {"call_ms": (time.perf_counter() - t0) * 1e3, "engine_ms": timer.ms}
    prep = getattr(pred, "device_prep", None)
    if prep is not None and prep.timings:
        rec["staging_ms"] = sum(t[0] for t in prep.timings)
        rec["prep_gpu_ms"] = sum(t[1].elapsed_time(t[2]) for t in prep.timings)
        rec["prep_calls"] = len(prep.timings)
    rec["ratio"] = rec["call_ms"] / rec["engine_ms"] if rec["engine_ms"] > 0 else None
    return out, rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="tree whose surya_amd is timed")
    ap.add_argument("--sets", default="letter96,letter192,square768,table")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None, help="append one JSON line per set here")
    ap.add_argument("--profile", default=None, help="after the timed calls, profile one more call of this set (top functions)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import surya_amd
    from surya_amd.layout.predictor import LayoutPredictor
    from surya_amd.table_rec import predictor as table_module
    from surya_amd.table_rec.predictor import TableRecPredictor
    print(f"timing the tree at {os.path.dirname(os.path.dirname(os.path.abspath(surya_amd.__file__)))}", flush=True)

    sets = args.sets.split(",")
    results = []
    lay = tab = None
    for name in sets:
        if name == "table":
            if tab is None:
                table_module.TABLE_REC_MAX_BOXES = TABLE_MAX_BOXES
                tab = TableRecPredictor(checkpoint="TABLE-DEFAULT", dtype=torch.bfloat16)
                tab_timer = EngineTimer(tab.model)
                tab(_pages(lambda k: TABLE_SIZES[k], 4, 1), batch_size=TABLE_BATCH)       # warm-up
            images = _pages(lambda k: TABLE_SIZES[k % len(TABLE_SIZES)], 32, 2)
            pred = tab
            out, rec = _timed_call(tab, images, tab_timer, batch_size=TABLE_BATCH)
            rec["pages"], rec["cells"] = len(images), sum(len(r.cells) for r in out)
        else:
            if lay is None:
                lay = LayoutPredictor(checkpoint="LAYOUT-DEFAULT", dtype=torch.bfloat16)
                lay_timer = EngineTimer(lay.model)
                lay(_pages((816, 1056), 4, 1))                                    # warm-up
            images = _pages(LAYOUT_SETS[name], 128, 3)
            pred = lay
            out, rec = _timed_call(lay, images, lay_timer)
            rec["pages"], rec["boxes"] = len(images), sum(len(r.bboxes) for r in out)
        rec.update(set=name, label=args.label, device_path=getattr(pred, "device_prep", None) is not None)
        results.append(rec)
        print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in rec.items()}), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(rec) + "\n")
    if args.profile:
        import cProfile
        import pstats
        pred = tab if args.profile == "table" else lay
        images = (_pages(lambda k: TABLE_SIZES[k % len(TABLE_SIZES)], 32, 2) if args.profile == "table"
                  else _pages(LAYOUT_SETS[args.profile], 128, 3))
        kw = {"batch_size": TABLE_BATCH} if args.profile == "table" else {}
        prof = cProfile.Profile()
        prof.enable()
        pred(images, **kw)
        torch.cuda.synchronize()
        prof.disable()
        print(f"-- cProfile of one {args.profile} call (cumulative)")
        pstats.Stats(prof).sort_stats("cumulative").print_stats(25)
    print(f"{'set':<10} {'call ms':>9} {'engine ms':>10} {'staging ms':>11} {'prep gpu ms':>12} {'call/engine':>12}")
    for r in results:
        st = f"{r['staging_ms']:.1f}" if "staging_ms" in r else "-"
        pg = f"{r['prep_gpu_ms']:.2f}" if "prep_gpu_ms" in r else "-"
        print(f"{r['set']:<10} {r['call_ms']:>9.1f} {r['engine_ms']:>10.1f} {st:>11} {pg:>12} {r['ratio']:>12.2f}")


if __name__ == "__main__":
    main()
