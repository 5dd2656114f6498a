"""Record the recogniser's fp16 fixture from the REAL reference modules (build container only; minutes on the CPU).

    python tools/make_golden_rec_fp16.py [cond8] [cond256]

Imports VikParuchuri/surya @ v0.14.6's SuryaModel through oracle/ref_shim and the builders of oracle/make_golden_full.py, loads the
conditioned synthetic REC-FULL weights into it and runs it in fp32 and in fp16 (the dtype RecognitionPredictor(dtype=torch.float16)
hands to SuryaModel.from_pretrained) on the inputs of the existing fixtures:

  cond8    the 8 bench crops x 48 tokens of tests/golden/rec_full_cond8.pt (eager attention, whole logits in memory)
  cond256  the 256 bench crops x 48 tokens of tests/golden/rec_full_cond256.pt (sdpa, reduced step by step with RefStepper)

The fp32 run must reproduce the existing fixture (tokens and top logits: asserted). Recorded per set, TEACHER-FORCED with the fixture's
tokens: fp16_dev [steps, lines] = max over the vocabulary of |fp16 logits - fp32 logits| (cond8 also fp16_dev_top, over the fixture's
top-32 columns), and the reference's own FREE-RUNNING fp16 greedy stream. cond256 also carries `sure_share`: the share of positions whose
fp32 top-2 margin exceeds 2 x the tolerance tests/test_gpu_rec_fp16.py builds from fp16_dev -- what its argmax check can cover at all.
Anchors (pick, tiles_sum, tokens) tie the numbers to the fp32 fixtures. No weights and no logits rows: numbers only.
-> tests/golden/rec_fp16.pt"""
from __future__ import annotations

import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch

GOLD = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLD, "rec_fp16.pt")
FLOOR = 5e-3 / 8            # the bf16 tests' 5e-3 x max|logit| floor, divided by 8 for fp16's three more significand bits


def sure_share(g, dev):
    """Share of positions whose reference top-2 margin exceeds 2 x tol, tol = 2 x dev (worst line of the step) + FLOOR x max|logit|."""
    scale = g["logits_absmax"].amax(-1)
    tol = 2 * dev.amax(-1) + FLOOR * scale
    val = g["logits_top"]["values"]
    return float(((val[..., 0] - val[..., 1]) > 2 * tol[:, None]).float().mean())


def cond8(MF):
    from surya_amd.config import rec_config
    from surya_amd.synth import make_rec_weights
    from util import bench_line_inputs
    g = torch.load(os.path.join(GOLD, "rec_full_cond8.pt"))
    cfg = rec_config("REC-FULL")
    sd = make_rec_weights(cfg, 0, recipe="conditioned")
    tiles, grids, seqs = bench_line_inputs(cfg, 256, seed=1234, pick=g["pick"])
    steps = g["tokens"].shape[0]
    ref = MF.build_reference_rec(cfg, sd, "eager")
    t0 = time.time()
    lg, _, tk = MF.run_reference(ref, cfg, tiles, grids, seqs, steps)
    print(f"cond8 fp32 reference: {time.time() - t0:.1f}s", flush=True)
    assert torch.equal(tk, g["tokens"]), "fp32 run != fixture (tokens)"
    idx = g["logits_top"]["indices"]
    assert torch.allclose(torch.gather(lg, -1, idx), g["logits_top"]["values"], atol=1e-4), "fp32 run != fixture (top-32 logits)"
    refh = ref.half()
    t0 = time.time()
    lgh, _, _ = MF.run_reference(refh, cfg, tiles, grids, seqs, steps, forced=g["tokens"])
    print(f"cond8 fp16 reference, teacher forced: {time.time() - t0:.1f}s", flush=True)
    assert torch.isfinite(lgh).all()
    _, _, tkh = MF.run_reference(refh, cfg, tiles, grids, seqs, steps)
    out = {"pick": list(g["pick"]), "tiles_sum": float(tiles.double().sum()), "tokens": g["tokens"].clone(),
           "fp16_dev": (lgh - lg).abs().amax(-1), "fp16_dev_top": (torch.gather(lgh, -1, idx) - g["logits_top"]["values"]).abs().amax(-1),
           "fp16_free_tokens": tkh, "fp16_forced_argmax_equal": int((lgh.argmax(-1) == g["tokens"]).sum())}
    out["sure_share"] = sure_share(g, out["fp16_dev"])
    rel = float((out["fp16_dev"].amax(-1) / g["logits_absmax"].amax(-1)).max())
    print(f"cond8: fp16 dev / max = {rel:.4f} (bf16 {float((g['bf16_dev'].amax(-1) / g['logits_absmax'].amax(-1)).max()):.4f}); free-running fp16 == "
          f"fp32 on {int((tkh == g['tokens']).all(0).sum())}/{tkh.shape[1]} lines; teacher-forced argmax equal at "
          f"{out['fp16_forced_argmax_equal']}/{tk.numel()}; sure share {out['sure_share']:.4f}", flush=True)
    return out


def cond256(MF):
    import copy
    from surya_amd.config import rec_config
    from surya_amd.synth import make_rec_weights
    from util import bench_line_inputs
    g = torch.load(os.path.join(GOLD, "rec_full_cond256.pt"))
    cfg = rec_config("REC-FULL")
    sd = make_rec_weights(cfg, 0, recipe="conditioned")
    tiles, grids, seqs = bench_line_inputs(cfg, 256, seed=1234)
    steps = g["tokens"].shape[0]
    ref = MF.build_reference_rec(cfg, sd, "sdpa")
    refh = copy.deepcopy(ref).half()
    t0 = time.time()
    a, b = MF.RefStepper(ref, cfg, tiles, grids, seqs), MF.RefStepper(refh, cfg, tiles, grids, seqs)
    print(f"cond256 prefill fp32 + fp16: {time.time() - t0:.1f}s", flush=True)
    dev = []
    for step in range(steps):
        lg, tk = a.lm, g["tokens"][step]
        assert torch.equal(lg.argmax(-1), tk), f"fp32 run != fixture (tokens, step {step})"
        assert torch.allclose(torch.gather(lg, -1, g["logits_top"]["indices"][step]), g["logits_top"]["values"][step], atol=1e-4), \
            f"fp32 run != fixture (top logits, step {step})"
        assert torch.isfinite(b.lm).all()
        dev.append((b.lm - lg).abs().amax(-1))
        if step + 1 < steps:
            a.advance(tk); b.advance(tk)
        if step % 8 == 7:
            print(f"cond256 step {step + 1}/{steps}: {time.time() - t0:.1f}s", flush=True)
    del a, b
    t0 = time.time()
    c = MF.RefStepper(refh, cfg, tiles, grids, seqs)
    free = []
    for step in range(steps):
        tk = c.lm.argmax(-1)
        free.append(tk.clone())
        if step + 1 < steps:
            c.advance(tk)
    out = {"tiles_sum": float(tiles.double().sum()), "tokens": g["tokens"].clone(), "fp16_dev": torch.stack(dev),
           "fp16_free_tokens": torch.stack(free)}
    out["sure_share"] = sure_share(g, out["fp16_dev"])
    rel = float((out["fp16_dev"].amax(-1) / g["logits_absmax"].amax(-1)).max())
    print(f"cond256 fp16 free-running: {time.time() - t0:.1f}s; fp16 == fp32 on {int((out['fp16_free_tokens'] == g['tokens']).all(0).sum())}/256 lines "
          f"(bf16: {int((g['bf16_free_tokens'] == g['tokens']).all(0).sum())}/256); fp16 dev / max = {rel:.4f}; sure share {out['sure_share']:.4f}", flush=True)
    return out


def main():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle import make_golden_full as MF           # installs oracle/ref_shim on import
    which = sys.argv[1:] or ["cond8", "cond256"]
    g = torch.load(OUT) if os.path.exists(OUT) else {}
    for w in which:
        g[w] = {"cond8": cond8, "cond256": cond256}[w](MF)
        torch.save(g, OUT)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
