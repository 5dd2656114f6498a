"""RecognitionPredictor.align on 256 bench-style lines (64 x {128..512} crops, 31 characters + eos each, REC-FULL bf16 synthetic weights) against
the slow host route that exists without forced decoding: prefill, then per token set_next_tokens + decode(1) + copy_last_logits + log_softmax.
Best of 3 each, lines per second, the phases of both, and the largest difference between the two routes' line log-probabilities.

    python tools/microbench/align_bench.py
"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
from PIL import Image
from surya_amd.config import rec_config
from surya_amd.synth import make_line_crops, make_rec_weights
from surya_amd.recognition.predictor import RecognitionModelLoader, RecognitionPredictor

N, CH = 256, 31
cfg = rec_config("REC-FULL"); sd = make_rec_weights(cfg, 0)
class Loader(RecognitionModelLoader):
    def model(self, device=None, dtype_=None, **caps):
        return super().model("cuda:0", torch.bfloat16, max_slots=N, max_kv_len=256, max_patches=65536, max_prefill_tokens=N * 72)
class Pred(RecognitionPredictor):
    model_loader_cls = Loader
    batch_size = N
pred = Pred(checkpoint={"config": cfg, "state_dict": sd})
imgs = [Image.fromarray(c) for c in make_line_crops(N)]
boxes = [[[0, 0, im.size[0], im.size[1]]] for im in imgs]
rng = np.random.default_rng(5)
alpha = list("abcdefghijklmnopqrstuvwxyz ABCDEFGHIJ0123456789.,-")
texts = [["".join(rng.choice(alpha, size=CH))] for _ in range(N)]
def t_align():
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = pred.align(imgs, texts, bboxes=boxes)
    torch.cuda.synchronize(); return time.perf_counter() - t0, out, dict(pred.last_timing)
def t_slow():
    m = pred.model
    torch.cuda.synchronize(); t0 = time.perf_counter()
    flat = pred.slice_bboxes(imgs, ["ocr_with_boxes"] * N, bboxes=boxes)
    ids = [pred.forced_ids(t[0], "ocr_with_boxes") for t in texts]
    prep = pred.prepare_lines(flat)
    torch.cuda.synchronize(); t1 = time.perf_counter()
    slots = list(range(N))
    m.prefill(prep["tiles"], prep["grids"], prep["prompt_ids"], slots)
    m.read_outputs(1)
    rows = torch.arange(N, device="cuda")
    lp = [torch.log_softmax(m.last_logits(), 1)[rows, torch.tensor([s[0] for s in ids], device="cuda")]]
    m.set_active(slots)
    for k in range(1, CH + 1):
        m.set_next_tokens(slots, [s[k - 1] for s in ids])
        m.decode(1); m.read_outputs(1)
        lp.append(torch.log_softmax(m.last_logits(), 1)[rows, torch.tensor([s[k] for s in ids], device="cuda")])
    total = torch.stack(lp).sum(0).cpu().numpy()
    torch.cuda.synchronize(); return time.perf_counter() - t0, total, time.perf_counter() - t1
t_align(); t_slow()
a = min((t_align() for _ in range(3)), key=lambda r: r[0]); s = min((t_slow() for _ in range(3)), key=lambda r: r[0])
got = np.asarray([r.text_lines[0].log_prob for r in a[1]])
print(f"align: {a[0] * 1e3:.1f} ms for {N} lines of {CH + 1} tokens = {N / a[0]:.0f} lines/s")
print(f"slow host route: {s[0] * 1e3:.1f} ms = {N / s[0]:.0f} lines/s; ratio {s[0] / a[0]:.1f}x")
print(f"max |log_prob(align) - log_prob(slow route)| over the lines: {np.abs(got - s[1]).max():.3e} (mean |log_prob| {np.abs(s[1]).mean():.1f})")
print("align phases (ms):", {k: round(v, 1) for k, v in a[2].items()})
print(f"slow route: slicing + prepare {(s[0] - s[2]) * 1e3:.1f} ms, prefill + {CH} x (set_next_tokens, decode(1), read, logits, log_softmax) {s[2] * 1e3:.1f} ms")
