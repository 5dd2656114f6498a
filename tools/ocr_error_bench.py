"""Timing of the HIP OCR-error classifier (OCRERR-DEFAULT, bf16 or fp16) -> one JSON line.

    python tools/ocr_error_bench.py [--dtype bf16|fp16] [--texts 256] [--steps 20] [--warmup 5] [--out FILE]
    python tools/ocr_error_bench.py --dtype-ab ROUNDS [--texts 256] [--steps 20] [--warmup 5] [--out FILE]

Cases: `mixed` = texts with seeded token lengths uniform in 32..512, `full` = every text at 512 tokens. Per case: the median forward
time from device events (after warmup), texts/s and tokens/s, the executed FLOPs counted from shapes (the [CLS]-only last layer counted
as run) and their share of the 16-bit MFMA peak (bf16 and fp16 share it), the same-process A/B of the last layer (`ocrerr_cls_only` 1 vs
0), and the baseline: the plain-PyTorch padded restatement of tests/ocr_error_util.py in the same dtype on the same ids. `tokenize_ms`:
host WordPiece tokenisation of the same number of page-like texts with a fresh (cold-memo) tokenizer and again warm.

`--dtype-ab ROUNDS`: a bf16 and an fp16 engine in ONE process on the same ids, timed alternately (bf16, fp16, fp16 with the one-query
[CLS] kernel = `ocrerr_cls_only` 2; ROUNDS times round the three): per arm every round's median, so the spread of repeated bf16 runs is
there to judge the fp16 / bf16 ratio against. No PyTorch baseline in this mode (a kernel trace of it holds the engines' kernels only)."""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from surya_amd import _lib as L  # noqa: E402
from surya_amd.ocr_error.config import ocr_error_config  # noqa: E402
from surya_amd.ocr_error.model import HipOCRErrorModel, pack_ids  # noqa: E402
from surya_amd.ocr_error.tokenizer import WordPieceTokenizer, vocab_from_list  # noqa: E402
from surya_amd.synth import make_ocr_error_weights, make_wordpiece_vocab  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0     # MI355X dense bf16 MFMA peak (fp16: the same rate)
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def flops(cfg, lens, cls_only=True):
    d, h, nl = cfg.dim, cfg.hidden_dim, cfg.n_layers
    T, n = sum(lens), len(lens)
    per_tok = 2 * d * 3 * d + 2 * d * d + 4 * d * h                  # qkv, out_lin, lin1 + lin2
    attn_full = sum(4 * L * L * d for L in lens)                       # QK^T and PV over all heads
    f = (nl - 1) * (T * per_tok + attn_full)
    if cls_only:
        f += T * 2 * d * 3 * d + sum(4 * L * d for L in lens) + n * (2 * d * d + 4 * d * h)
    else:
        f += T * per_tok + attn_full
    return f + n * (2 * d * d + 2 * d * cfg.num_labels)


def time_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def set_cls_only(v):
    L.check(L.lib().surya_set_tuning(b"ocrerr_cls_only", int(v)), "surya_set_tuning")


def make_cases(cfg, n):
    rng = random.Random(1234)
    cases = {"mixed": [rng.randint(32, 512) for _ in range(n)], "full": [512] * n}
    return rng, {name: [[101] + [rng.randrange(104, cfg.vocab_size) for _ in range(L_ - 2)] + [102] for L_ in lens] for name, lens in cases.items()}


def dtype_ab(a, cfg, sd):
    n = a.texts
    eng = {name: HipOCRErrorModel(cfg, sd, dtype=dt, device="cuda:0", max_texts=n, max_tokens=n * 512) for name, dt in DTYPES.items()}
    arms = [("bf16", "bf16", 1), ("fp16", "fp16", 1), ("fp16_one_query_cls", "fp16", 2)]
    res = {"workload": "ocr_error_dtype_ab", "config": "OCRERR-DEFAULT", "texts": n, "steps": a.steps, "warmup": a.warmup, "rounds": a.dtype_ab,
           "cases": {}}
    _, cases = make_cases(cfg, n)
    for name, seqs in cases.items():
        ids, lns = pack_ids(seqs)
        ids_dev = ids.cuda()
        ms = {arm: [] for arm, _, _ in arms}
        for _ in range(a.dtype_ab):
            for arm, dt, knob in arms:
                set_cls_only(knob)
                ms[arm].append(time_ms(lambda: eng[dt].enqueue(ids_dev, lns), a.steps, a.warmup))
        set_cls_only(1)
        med = {arm: statistics.median(v) for arm, v in ms.items()}
        res["cases"][name] = {"tokens": sum(lns), "round_medians_ms": {arm: [round(x, 3) for x in v] for arm, v in ms.items()},
                              "forward_ms": {arm: round(x, 3) for arm, x in med.items()},
                              "bf16_spread": round(max(ms["bf16"]) / min(ms["bf16"]), 4),
                              "fp16_over_bf16": round(med["fp16"] / med["bf16"], 4),
                              "fp16_one_query_cls_over_fp16": round(med["fp16_one_query_cls"] / med["fp16"], 4)}
    return res


def emit(res, out):
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=sorted(DTYPES), default="bf16")
    ap.add_argument("--dtype-ab", type=int, default=0, metavar="ROUNDS", help="time a bf16 and an fp16 engine alternately, ROUNDS times each")
    ap.add_argument("--texts", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cfg = ocr_error_config("OCRERR-DEFAULT")
    sd = make_ocr_error_weights(cfg, 0, "conditioned")
    if a.dtype_ab > 0:
        emit(dtype_ab(a, cfg, sd), a.out)
        return
    n = a.texts
    dt = DTYPES[a.dtype]
    m = HipOCRErrorModel(cfg, sd, dtype=dt, device="cuda:0", max_texts=n, max_tokens=n * 512)
    from ocr_error_util import TorchOCRError, pad_batch
    base = TorchOCRError(cfg, sd, dt, "cuda:0")
    rng, cases = make_cases(cfg, n)
    res = {"workload": "ocr_error", "config": "OCRERR-DEFAULT", "dtype": a.dtype, "texts": n, "steps": a.steps, "warmup": a.warmup,
           "peak_tflops": PEAK_BF16_TFLOPS, "cases": {}}
    for name, seqs in cases.items():
        ids, lns = pack_ids(seqs)
        ids_dev = ids.cuda()
        fwd = lambda: m.enqueue(ids_dev, lns)
        ab = {}
        for v in (1, 0):
            set_cls_only(v)
            ab[v] = time_ms(fwd, a.steps, a.warmup)
        set_cls_only(1)
        ms = ab[1]
        f = flops(cfg, lns, True)
        pid, pmask = pad_batch(seqs, cfg.pad_token_id)
        pid, pmask = pid.cuda(), pmask.cuda()
        base_ms = time_ms(lambda: base(pid, pmask), max(3, a.steps // 4), 2)
        T = sum(lns)
        res["cases"][name] = {"tokens": T, "forward_ms": round(ms, 3), "texts_per_s": round(n / ms * 1e3, 1),
                              "tokens_per_s": round(T / ms * 1e3, 1), "tflop": round(f / 1e12, 4),
                              "tflops": round(f / ms / 1e9, 1), "frac_of_peak": round(f / ms / 1e9 / PEAK_BF16_TFLOPS, 4),
                              "cls_only_ab_ms": {"1": round(ab[1], 3), "0": round(ab[0], 3)},
                              f"baseline_padded_torch_{a.dtype}_ms": round(base_ms, 3), "speedup_vs_baseline": round(base_ms / ms, 2)}
    words = ["the", "model", "page", "text", "error", "and", "of", "in", "is", "résumé", "naïve", "3.14", "don't", "U.S.A.", "qzx",
             "Table", "line", "Word", "(see", "p.", "12)", "—", "x^2", "ocr"]
    texts = [" ".join(rng.choice(words) for _ in range(rng.randint(20, 300))) for _ in range(n)]
    vocab = vocab_from_list(make_wordpiece_vocab(0))
    tk = WordPieceTokenizer(vocab, max_positions=cfg.max_position_embeddings)
    t0 = time.perf_counter()
    tk(texts)
    cold = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    tk(texts)
    warm = (time.perf_counter() - t0) * 1e3
    res["tokenize_ms"] = {"cold": round(cold, 2), "warm": round(warm, 2), "texts": n}
    emit(res, a.out)


if __name__ == "__main__":
    main()
