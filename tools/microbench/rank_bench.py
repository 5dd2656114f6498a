"""RecognitionPredictor.rank of 64 lines x 16 candidates of about 12 characters (REC-FULL bf16, synthetic weights, recognition_batch_size
1024) against what exists without it: align on the same 64 bboxes, each repeated 16 times. The arms alternate in one process, best of 3
each; then the fan-out launch by itself (surya_op_rec_kv_fanout on buffers of the engine's cache shape, 64 prompts to 15 slots each),
timed with events, beside kv_fork_kernel moving the same rows.

    python tools/microbench/rank_bench.py
"""
import ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np, torch
from PIL import Image
from surya_amd import _lib as L
from surya_amd.config import rec_config
from surya_amd.synth import make_line_crops, make_rec_weights
from surya_amd.recognition.predictor import RecognitionModelLoader, RecognitionPredictor

N, K, CH, SLOTS, TMAX = 64, 16, 12, 1024, 256
cfg = rec_config("REC-FULL"); sd = make_rec_weights(cfg, 0)
class Loader(RecognitionModelLoader):
    def model(self, device=None, dtype_=None, **caps):
        return super().model("cuda:0", torch.bfloat16, max_slots=SLOTS, max_kv_len=TMAX, max_patches=65536 * 4, max_prefill_tokens=SLOTS * 72)
class Pred(RecognitionPredictor):
    model_loader_cls = Loader
    batch_size = SLOTS
pred = Pred(checkpoint={"config": cfg, "state_dict": sd})
imgs = [Image.fromarray(c) for c in make_line_crops(N)]
box = lambda im: [0, 0, im.size[0], im.size[1]]
rng = np.random.default_rng(5)
alpha = list("abcdefghijklmnopqrstuvwxyz ABCDEFGHIJ0123456789.,-")
def texts_of():
    out = set()
    while len(out) < K:
        out.add("".join(rng.choice(alpha, size=int(rng.integers(CH - 2, CH + 3)))))
    return sorted(out)
cands = [[texts_of()] for _ in range(N)]
def t_rank():
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = pred.rank(imgs, cands, bboxes=[[box(im)] for im in imgs], recognition_batch_size=SLOTS)
    torch.cuda.synchronize(); return time.perf_counter() - t0, out, dict(pred.last_timing)
def t_align():
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = pred.align(imgs, [c[0] for c in cands], bboxes=[[box(im)] * K for im in imgs], recognition_batch_size=SLOTS)
    torch.cuda.synchronize(); return time.perf_counter() - t0, out, dict(pred.last_timing)
t_rank(); t_align()
runs = {"rank": [], "align": []}
for _ in range(3):
    runs["rank"].append(t_rank()); runs["align"].append(t_align())
r, a = (min(runs[k], key=lambda x: x[0]) for k in ("rank", "align"))
diff = max(abs(c.log_prob - a[1][i].text_lines[c.index].log_prob) for i, res in enumerate(r[1]) for c in res.lines[0].candidates)
res = {"lines": N, "candidates": K, "rank_ms": [round(x[0] * 1e3, 1) for x in runs["rank"]], "align_ms": [round(x[0] * 1e3, 1) for x in runs["align"]],
       "rank_best_ms": round(r[0] * 1e3, 1), "align_best_ms": round(a[0] * 1e3, 1), "align_over_rank": round(a[0] / r[0], 2),
       "max_abs_log_prob_difference": diff, "rank_phases_ms": {k: round(v, 1) for k, v in r[2].items()},
       "align_phases_ms": {k: round(v, 1) for k, v in a[2].items()}}
# the fan-out launch alone, on buffers of the engine's cache shape
d = cfg.decoder
layers, nkv, D = d.num_hidden_layers, d.num_key_value_heads, d.head_dim
plen = int(np.mean([len(p) for p in pred.prepare_lines(pred.slice_bboxes(imgs, ["ocr_with_boxes"] * N, bboxes=[[box(im)] for im in imgs]))["prompt_ids"]]))
del pred; torch.cuda.empty_cache()
k = torch.randn((layers, SLOTS, nkv, TMAX, D), device="cuda").to(torch.bfloat16); v = k.clone()
dev = lambda x: torch.tensor(x, dtype=torch.int32, device="cuda")
src, off = dev([i * K for i in range(N)]), dev([i * (K - 1) for i in range(N + 1)])
dst, ln = dev([i * K + j for i in range(N) for j in range(1, K)]), dev([plen] * N)
fsrc = dev([-1 if s % K == 0 else s - s % K for s in range(SLOTS)]); base = dev([0] * SLOTS); flen = dev([plen] * SLOTS)
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
fan = lambda: L.lib().surya_op_rec_kv_fanout(L.DTYPE_BF16, L.ptr(k), L.ptr(v), L.ptr(src), L.ptr(off), L.ptr(dst), L.ptr(ln), N, N * (K - 1), layers, SLOTS,
                                             nkv, TMAX, D, st)
fork = lambda: L.lib().surya_op_rec_kv_fork(L.DTYPE_BF16, L.ptr(k), L.ptr(v), L.ptr(fsrc), L.ptr(base), L.ptr(flen), SLOTS, layers, SLOTS, nkv, TMAX, D, st)
def timed(fn, n=10):
    assert fn() == 0; torch.cuda.synchronize()
    best = 1e9
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); assert fn() == 0; e1.record(); torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return best
moved = 2 * layers * nkv * plen * D * 2 * N            # bytes of the 64 prompts, K and V
res.update(prompt_rows=plen, fanout_ms=round(timed(fan), 4), fork_same_rows_ms=round(timed(fork), 4),
           read_mib=round(moved / 2 ** 20, 1), written_mib=round(moved * (K - 1) / 2 ** 20, 1))
res["fanout_written_gb_per_s"] = round(moved * (K - 1) / res["fanout_ms"] / 1e6, 1)
print(json.dumps(res))
