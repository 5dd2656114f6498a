"""Recogniser, bf16 against fp16, inside ONE process on one GPU: REC-FULL (conditioned weights) on bench.py's 256 line crops.

    python tools/microbench/rec_dtype_ab.py [--arms bf16,fp16] [--reps 5] [--tokens 48]

Builds one HipRecModel per arm on the same weights and inputs and times, interleaved (bf16, fp16, bf16, ...): a PASS = prefill (vision encoder +
prompt) + the device loop up to `--tokens` tokens per line, in calls of 8 steps with the next call enqueued before the previous one is read
(the predictor's pipelined form), and inside it the DECODE STEPS alone. HIP events on the stream; the minimum and the median over `--reps` per
arm, then fp16 / bf16 of the medians. Prints one JSON line last. For a kernel trace run one arm per process under the profiler
(`--arms fp16 --reps 1`: tracing only, no counters) and summarise the database with tools/rocpd_stats.py."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", default="bf16,fp16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=48)
    args = ap.parse_args()
    from surya_amd.config import rec_config
    from surya_amd.recognition.model import HipRecModel
    from surya_amd.synth import make_rec_weights
    from util import bench_line_inputs

    cfg = rec_config("REC-FULL")
    sd = make_rec_weights(cfg, 0, recipe="conditioned")
    tiles, grids, seqs = bench_line_inputs(cfg, 256, seed=1234)
    tiles = tiles.cuda().contiguous()
    n = len(seqs)
    slots = list(range(n))
    arms = [a for a in args.arms.split(",") if a]
    models = {a: HipRecModel(cfg, sd, image_token_id=cfg.image_token_id, pad_token_id=cfg.pad_token_id, eos_token_id=cfg.eos_token_id,
                             dtype=DTYPES[a], max_slots=n, max_kv_len=64 + args.tokens + 40, max_patches=65536, max_prefill_tokens=n * 72)
              for a in arms}
    steps = args.tokens - 1                                  # the prefill yields the first token

    def run(m):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        calls = [(min(8, steps - i), (i // 8) & 1) for i in range(0, steps, 8)]
        torch.cuda.synchronize()
        ev[0].record()
        m.prefill(tiles, grids, seqs, slots)
        m.set_active(slots)
        ev[1].record()
        toks = []
        m.decode_async(*calls[0])
        for i, call in enumerate(calls):
            if i + 1 < len(calls):
                m.decode_async(*calls[i + 1])
            t, _, _ = m.wait_outputs(*call)
            toks.append(t[: call[0], :n].copy())
        ev[2].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[2]), ev[1].elapsed_time(ev[2]) * 1e3 / steps, np.concatenate(toks)

    for a in arms:                                           # warm-up: LDS opt-ins, allocator, clocks
        run(models[a]); run(models[a])
    times = {a: [] for a in arms}
    toks = {}
    for _ in range(args.reps):
        for a in arms:
            p, d, t = run(models[a])
            times[a].append((p, d))
            toks[a] = t
    out = {"config": "REC-FULL conditioned", "lines": n, "tokens": args.tokens, "reps": args.reps}
    for a in arms:
        ps, ds = [x[0] for x in times[a]], [x[1] for x in times[a]]
        out[a] = {"pass_ms_median": statistics.median(ps), "pass_ms_min": min(ps), "pass_ms_max": max(ps),
                  "decode_step_us_median": statistics.median(ds), "decode_step_us_min": min(ds), "decode_step_us_max": max(ds)}
        print(f"{a}: pass {out[a]['pass_ms_median']:.2f} ms (min {min(ps):.2f}, max {max(ps):.2f}); decode step {out[a]['decode_step_us_median']:.1f} us "
              f"(min {min(ds):.1f}, max {max(ds):.1f}) over {args.reps} passes of {n} lines x {args.tokens} tokens", flush=True)
    if "bf16" in out and "fp16" in out:
        out["fp16_over_bf16"] = {"pass": out["fp16"]["pass_ms_median"] / out["bf16"]["pass_ms_median"],
                                 "decode_step": out["fp16"]["decode_step_us_median"] / out["bf16"]["decode_step_us_median"]}
        out["lines_with_identical_tokens"] = int((toks["bf16"] == toks["fp16"]).all(0).sum())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
