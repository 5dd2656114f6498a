"""bf16 against fp16 on the layout / table-recognition engine, in ONE process, the two dtypes alternating.

    python tools/layout_dtype_ab.py [--rounds 4] [--reps 3] [--pages 32] [--tables 16] [--arms bf16,fp16] [--out FILE.json]

Two workloads, synthetic LAYOUT-DEFAULT / TABLE-DEFAULT weights:
  layout  LayoutPredictor.__call__ on `--pages` pages of 816 x 1056 (one engine batch: device pre-processing, encoder, the greedy box loop
          on device-fed runs, host token rule and result assembly -- the call a user makes);
  table   the first pass of table recognition on the engine: `--tables` crops encoded, the 3-token prompt in one pass
          (surya_layout_prefill), then device-fed decode runs up to 40 positions (the cap of tools/layout_call_bench.py; synthetic weights
          seldom emit the end token, so the length is the same in both dtypes).
Per round every arm runs `--reps` calls back to back (device synchronised before and after each; wall clock) and contributes their median;
the rounds alternate bf16, fp16, bf16, ... so drift of the shared host hits both. Reported: the median of the round medians per arm, the
spread of the bf16 rounds (max / min: what a ratio below it cannot tell), fp16 / bf16 of those medians and of the fastest rounds (the layout
call has host work in it, and a neighbour on the shared host shows as slow rounds of either arm) -- against the other dtype in this
process, never against a number from another run. One JSON line on stdout (and in --out). For kernel times run it under a kernel-trace profiler in a run
of its own, one dtype per trace: --arms bf16 --rounds 1 --reps 1, then --arms fp16 (no ratio is reported for a single arm)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TABLE_POSITIONS = 40
TABLE_SIZES = [(500, 300), (320, 200), (900, 600), (1200, 400), (250, 700), (640, 480), (1000, 1000), (1400, 900)]


def _pages(size, n, seed):
    import numpy as np
    from PIL import Image
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        w, h = size(k) if callable(size) else size
        a = np.full((h, w, 3), 235, np.uint8)
        for _ in range(6):
            x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
            a[y0:y0 + max(1, h // 10), x0:x0 + max(1, w // 3)] = rng.integers(0, 120, size=3, dtype=np.uint8)
        out.append(Image.fromarray(a))
    return out


def _timed(fn, reps):
    import torch
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms)


def _table_first_pass(model, px, prompt):
    """Engine calls of TableRecPredictor.inference_loop for one batch, the fed-back tokens left on the device."""
    from surya_amd.layout.model import RING_STEPS
    n, T = prompt.shape[:2]
    model.encode(px)
    model.select(list(range(n)))
    cls, box = model.prefill(prompt)
    model.set_feedback()
    first = prompt[:, -1].copy()                                 # any valid token: the run's own tokens follow on the device
    pos, ring, pending = T, 0, []
    while pos < TABLE_POSITIONS:
        k = min(RING_STEPS, TABLE_POSITIONS - pos)
        model.decode_steps(first if pos == T else None, pos, k, ring)
        pending.append((k, ring))
        if len(pending) == 2:
            model.wait_steps(*pending.pop(0))
        pos += k
        ring ^= 1
    out = None
    for p in pending:
        out = model.wait_steps(*p)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pages", type=int, default=32)
    ap.add_argument("--tables", type=int, default=16)
    ap.add_argument("--arms", default="bf16,fp16", help="the dtypes to run, in this order within a round")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("layout_dtype_ab needs a GPU: a time taken anywhere else says nothing")
    from surya_amd.layout.predictor import LayoutPredictor
    from surya_amd.layout.preprocess_gpu import device_preprocessor
    from surya_amd.table_rec.predictor import TableRecPredictor

    dtypes = {"bf16": torch.bfloat16, "fp16": torch.float16}
    arms = tuple((tag, dtypes[tag]) for tag in args.arms.split(","))
    lay = {tag: LayoutPredictor(checkpoint="LAYOUT-DEFAULT", dtype=dt) for tag, dt in arms}
    tab = {tag: TableRecPredictor(checkpoint="TABLE-DEFAULT", dtype=dt) for tag, dt in arms}
    pages = _pages((816, 1056), args.pages, 3)
    crops = [im.convert("RGB") for im in _pages(lambda k: TABLE_SIZES[k % len(TABLE_SIZES)], args.tables, 2)]
    d = tab[arms[0][0]].model.config.decoder
    rng = np.random.default_rng(7)
    prompt = np.concatenate([rng.integers(0, 1025, (args.tables, 3, 6)), rng.integers(5, 10, (args.tables, 3, 1)),
                             rng.integers(5, 9, (args.tables, 3, 1)), rng.integers(1, 4, (args.tables, 3, 1)),
                             rng.integers(5, 7, (args.tables, 3, 1))], -1).astype(np.int32)
    prompt[:, 0], prompt[:, 2] = d.bos_token_id, d.query_end_token_id
    tab_px = {}
    for tag, p in tab.items():                                   # the crops pre-processed once per arm: the timed part is the engine's
        prep = device_preprocessor(p, p.processor.image_processor)
        if prep is not None:
            tab_px[tag] = prep([(im, (0, 0, im.width, im.height)) for im in crops], p.processor.image_processor).contiguous()
        else:
            tab_px[tag] = torch.from_numpy(np.stack(p.processor.image_processor(crops)["pixel_values"])).cuda().contiguous()
    work = {"layout": {tag: (lambda p=p: p(pages)) for tag, p in lay.items()},
            "table": {tag: (lambda p=p, tag=tag: _table_first_pass(p.model, tab_px[tag], prompt)) for tag, p in tab.items()}}
    res = {"workload": "layout_dtype_ab", "layout": {"config": "LAYOUT-DEFAULT", "pages": args.pages, "page_size": [816, 1056]},
           "table": {"config": "TABLE-DEFAULT", "tables": args.tables, "positions": TABLE_POSITIONS}, "rounds": args.rounds, "reps": args.reps}
    for name, fns in work.items():
        for fn in fns.values():
            fn()                                                  # warm-up: code objects, LDS attributes, every shape of the timed call
        med = {tag: [] for tag in fns}
        for _ in range(args.rounds):
            for tag, fn in fns.items():
                med[tag].append(round(_timed(fn, args.reps), 3))
        call = {tag: statistics.median(v) for tag, v in med.items()}
        res[name].update(round_medians_ms=med, call_ms=call)
        if "bf16" in med and "fp16" in med:
            res[name].update(bf16_spread=round(max(med["bf16"]) / min(med["bf16"]), 4), fp16_over_bf16=round(call["fp16"] / call["bf16"], 4),
                             fp16_over_bf16_fastest_round=round(min(med["fp16"]) / min(med["bf16"]), 4))
    res["layout"]["boxes"] = {tag: sum(len(r.bboxes) for r in p(pages)) for tag, p in lay.items()}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
