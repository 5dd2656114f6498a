"""Beam search against greedy decoding on the bench crops: 256 synthetic line crops (seed 1234, widest first), REC-FULL bf16 synthetic
weights, 256 KV slots, max_tokens 48; beam width off / 2 / 4, the arms alternated in one process, best of 3 rounds each.

Per arm: lines/s of RecognitionPredictor.generate over the 256 lines (a beam of width B keeps 256 / B lines in flight); microseconds per
decode step of one surya_rec_decode(8) call on 256 active slots (wall clock around a synchronised call); the event-timed share of the two
beam launches in that step (surya_prof buckets 4 = beam_select_kernel, 5 = kv_fork_kernel); and, from the parents the call reported, the
mean number of beams that moved to another slot per step and group and the KV rows (tokens) copied for them per step.

    python tools/microbench/beam_sweep.py [--out FILE]
"""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ.setdefault("RECOGNITION_MAX_TOKENS", "48")
import numpy as np, torch
from surya_amd import _lib as L
from surya_amd.config import rec_config
from surya_amd.settings import settings
from surya_amd.synth import make_line_crops, make_rec_weights
from surya_amd.recognition.predictor import RecognitionModelLoader, RecognitionPredictor
from surya_amd.recognition.schema import TaskNames

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()
N, T, STEPS = 256, 48, 8
settings.reload()
cfg = rec_config("REC-FULL"); sd = make_rec_weights(cfg, 0)
class Loader(RecognitionModelLoader):
    def model(self, device=None, dtype_=None, **caps):
        return super().model("cuda:0", torch.bfloat16, max_slots=N, max_kv_len=64 + T + 32, max_patches=65536, max_prefill_tokens=N * 72)
class Pred(RecognitionPredictor):
    model_loader_cls = Loader
    batch_size = N
pred = Pred(checkpoint={"config": cfg, "state_dict": sd})
m, lib, nop = pred.model, L.lib(), pred.processor.no_output_token
crops = make_line_crops(N, seed=1234); crops.sort(key=lambda c: -c.shape[1])
flat = {"slices": [c.astype(np.float32) for c in crops], "input_text": [None] * N, "task_names": [TaskNames.ocr_with_boxes] * N}
prep = pred.prepare_lines(flat, math_mode=True)
torch.cuda.synchronize()

def lines_per_s(B):
    pred._beam = B
    try:
        torch.cuda.synchronize(); t0 = time.perf_counter()
        pred.generate(prep, N)
        torch.cuda.synchronize(); return N / (time.perf_counter() - t0)
    finally:
        pred._beam = None

def step_us(B):
    """(microseconds per decode step, ms of select + fork per step, moved beams per group and step, KV rows copied per step)"""
    G = N // (B or 1)
    offs = prep["tile_offs"]
    m.set_beam(B, nop)
    try:
        lead = [g * (B or 1) for g in range(G)]
        m.prefill(prep["tiles"][: int(offs[G])], prep["grids"][:G], prep["prompt_ids"][:G], lead)
        m.set_active(list(range(G * (B or 1))))
        m.decode(STEPS); torch.cuda.synchronize()                       # warm: one-time attributes, allocator
        t0 = time.perf_counter(); m.decode(STEPS); torch.cuda.synchronize(); us = (time.perf_counter() - t0) / STEPS * 1e6
        if not B:
            return us, 0.0, 0.0, 0.0
        par = m.read_beam(STEPS)[1][:, : G * B].reshape(STEPS, G, B).copy()
        moved = (par >= 0) & (par != np.arange(B)[None, None, :])
        rows = (moved.sum(axis=(1, 2)) * (STEPS + 1 + np.arange(STEPS))).mean()      # rows behind the prompt at that step: warm-up steps + this call's
        lib.surya_prof_enable(1)
        m.decode(STEPS)
        n = 6
        la = (C.c_int * n)(); ms = (C.c_double * n)(); fl = (C.c_double * n)(); by = (C.c_double * n)()
        L.check(lib.surya_prof_read(n, la, ms, fl, by), "surya_prof_read")
        lib.surya_prof_enable(0)
        return us, (ms[4] + ms[5]) / STEPS, float(moved.sum()) / (STEPS * G), float(rows)
    finally:
        m.set_beam(None)

arms = [None, 2, 4]
best = {B: dict(lines_per_s=0.0, step_us=1e30) for B in arms}
for B in arms:                                                          # warm every arm once
    lines_per_s(B); step_us(B)
for _ in range(args.rounds):
    for B in arms:
        r = best[B]
        r["lines_per_s"] = max(r["lines_per_s"], lines_per_s(B))
        us, bms, mv, rows = step_us(B)
        if us < r["step_us"]:
            r.update(step_us=us, select_fork_ms_per_step=bms, moved_beams_per_group_step=mv, forked_kv_rows_per_step=rows)
out = []
for B in arms:
    r = best[B]
    rec = {"beam_width": B or 0, "lines_in_flight": N // (B or 1), "lines_per_s": round(r["lines_per_s"], 1), "decode_step_us": round(r["step_us"], 1)}
    if B:
        rec.update(select_fork_us_per_step=round(r["select_fork_ms_per_step"] * 1e3, 1),
                   select_fork_share=round(r["select_fork_ms_per_step"] * 1e3 / r["step_us"], 4),
                   moved_beams_per_group_step=round(r["moved_beams_per_group_step"], 3), forked_kv_rows_per_step=round(r["forked_kv_rows_per_step"], 1))
    out.append(rec)
    print(json.dumps(rec))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"workload": f"{N} bench crops (seed 1234), REC-FULL bf16 synthetic weights, {N} slots, max_tokens {T}, decode({STEPS}) calls, "
                               f"best of {args.rounds} alternated rounds", "arms": out}, f, indent=1)
