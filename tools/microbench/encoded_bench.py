"""Lines kept on the device (RecognitionPredictor.encode / EncodedLines) against the calls that encode every time: REC-FULL bf16,
synthetic weights, the 64 crops and 16 candidates of rank_bench.py. Arms alternate in one process, one warm-up each, best of 3:

  (a) pred(...) then pred.rank(...)                      against  pred.encode(...) + enc.read() + enc.rank(...)
  (b) 256 lines read, then all re-read under a pattern   fresh (two calls)  against  restored (encode + two reads)
  (c) surya_rec_restore alone, event-timed: 64 entries into 16 slots each, bytes moved and TB/s written

    python tools/microbench/encoded_bench.py
"""
import ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np, torch
from PIL import Image
from surya_amd import _lib as L
from surya_amd.config import rec_config
from surya_amd.settings import settings
from surya_amd.synth import make_line_crops, make_rec_weights
from surya_amd.recognition.predictor import RecognitionModelLoader, RecognitionPredictor

N, K, CH, SLOTS, TMAX, NB = 64, 16, 12, 1024, 256, 256
cfg = rec_config("REC-FULL"); sd = make_rec_weights(cfg, 0)
class Loader(RecognitionModelLoader):
    def model(self, device=None, dtype_=None, **caps):
        return super().model("cuda:0", torch.bfloat16, max_slots=SLOTS, max_kv_len=TMAX, max_patches=65536 * 4, max_prefill_tokens=SLOTS * 72)
class Pred(RecognitionPredictor):
    model_loader_cls = Loader
    batch_size = SLOTS
pred = Pred(checkpoint={"config": cfg, "state_dict": sd})
box = lambda im: [0, 0, im.size[0], im.size[1]]
imgs = [Image.fromarray(c) for c in make_line_crops(N)]
boxes = [[box(im)] for im in imgs]
rng = np.random.default_rng(5)
alpha = list("abcdefghijklmnopqrstuvwxyz ABCDEFGHIJ0123456789.,-")
def texts_of():
    out = set()
    while len(out) < K:
        out.add("".join(rng.choice(alpha, size=int(rng.integers(CH - 2, CH + 3)))))
    return sorted(out)
cands = [[texts_of()] for _ in range(N)]
def wall(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(); return (time.perf_counter() - t0) * 1e3, out
def best(runs):
    return round(min(r[0] for r in runs), 1)
dump = lambda rs: [r.model_dump() for r in rs]

# (a) read, then rank
settings.RECOGNITION_MAX_TOKENS = 48
def a_fresh():
    return pred(imgs, bboxes=boxes, recognition_batch_size=SLOTS), pred.rank(imgs, cands, bboxes=boxes, recognition_batch_size=SLOTS)
def a_kept():
    with pred.encode(imgs, bboxes=boxes, recognition_batch_size=SLOTS) as enc:
        return enc.read(recognition_batch_size=SLOTS), enc.rank(cands, recognition_batch_size=SLOTS)
def a_parts():                                               # the kept arm, call by call
    t_enc, enc = wall(lambda: pred.encode(imgs, bboxes=boxes, recognition_batch_size=SLOTS))
    t_read, _ = wall(lambda: enc.read(recognition_batch_size=SLOTS))
    t_rank, _ = wall(lambda: enc.rank(cands, recognition_batch_size=SLOTS)); loop = pred.last_timing.get("device_loop_ms")
    enc.release()
    return {"encode_ms": round(t_enc, 1), "read_ms": round(t_read, 1), "rank_ms": round(t_rank, 1), "rank_device_loop_ms": round(loop, 1)}
def a_fresh_parts():
    t_read, _ = wall(lambda: pred(imgs, bboxes=boxes, recognition_batch_size=SLOTS))
    t_rank, _ = wall(lambda: pred.rank(imgs, cands, bboxes=boxes, recognition_batch_size=SLOTS)); loop = pred.last_timing.get("device_loop_ms")
    return {"read_ms": round(t_read, 1), "rank_ms": round(t_rank, 1), "rank_device_loop_ms": round(loop, 1)}
wall(a_fresh); wall(a_kept)
runs = {"fresh": [], "kept": []}
for _ in range(3):
    runs["fresh"].append(wall(a_fresh)); runs["kept"].append(wall(a_kept))
f, k = runs["fresh"][0][1], runs["kept"][0][1]
res = {"a_lines": N, "a_candidates": K, "a_fresh_ms": [round(r[0], 1) for r in runs["fresh"]], "a_kept_ms": [round(r[0], 1) for r in runs["kept"]],
       "a_fresh_best_ms": best(runs["fresh"]), "a_kept_best_ms": best(runs["kept"]), "a_equal": dump(f[0]) == dump(k[0]) and dump(f[1]) == dump(k[1]),
       "a_fresh_parts": a_fresh_parts(), "a_kept_parts": a_parts()}
res["a_fresh_over_kept"] = round(res["a_fresh_best_ms"] / res["a_kept_best_ms"], 2)

# (b) 256 lines: a free read, then a pattern re-read of all of them
imgs_b = [Image.fromarray(c) for c in make_line_crops(NB)]
boxes_b = [[box(im)] for im in imgs_b]
DATE = r"\d{2}/\d{2}/\d{4}"
def b_fresh():
    first = pred(imgs_b, bboxes=boxes_b, recognition_batch_size=NB)
    pred.pattern = DATE
    try:
        return first, pred(imgs_b, bboxes=boxes_b, recognition_batch_size=NB)
    finally:
        pred.pattern = None
def b_kept():
    with pred.encode(imgs_b, bboxes=boxes_b, recognition_batch_size=NB) as enc:
        first = enc.read(recognition_batch_size=NB)
        pred.pattern = DATE
        try:
            return first, enc.read(recognition_batch_size=NB)
        finally:
            pred.pattern = None
def b_reread():                                              # the re-read alone, fresh against restored
    enc = pred.encode(imgs_b, bboxes=boxes_b, recognition_batch_size=NB)
    pred.pattern = DATE
    try:
        t_f = min(wall(lambda: pred(imgs_b, bboxes=boxes_b, recognition_batch_size=NB))[0] for _ in range(3))
        t_k = min(wall(lambda: enc.read(recognition_batch_size=NB))[0] for _ in range(3))
    finally:
        pred.pattern = None
        enc.release()
    return {"pattern_reread_fresh_ms": round(t_f, 1), "pattern_reread_restored_ms": round(t_k, 1)}
wall(b_fresh); wall(b_kept)
runs = {"fresh": [], "kept": []}
for _ in range(3):
    runs["fresh"].append(wall(b_fresh)); runs["kept"].append(wall(b_kept))
f, k = runs["fresh"][0][1], runs["kept"][0][1]
res.update(b_lines=NB, b_fresh_ms=[round(r[0], 1) for r in runs["fresh"]], b_kept_ms=[round(r[0], 1) for r in runs["kept"]],
           b_fresh_best_ms=best(runs["fresh"]), b_kept_best_ms=best(runs["kept"]), b_equal=dump(f[0]) == dump(k[0]) and dump(f[1]) == dump(k[1]),
           **b_reread())
res["b_fresh_over_kept"] = round(res["b_fresh_best_ms"] / res["b_kept_best_ms"], 2)

# (c) surya_rec_restore alone on the engine: 64 entries into 16 slots each (the whole call: staging copy, slot state, copy, head pass),
# and the copy kernel alone through its op hook on buffers of the engine's shape
m = pred.model
enc = pred.encode(imgs, bboxes=boxes, recognition_batch_size=SLOTS)
first = [enc._first[i] for i in range(N)]
rows = [len(enc._prompt_ids[i]) for i in range(N)]
fans = [[i * K + j for j in range(K)] for i in range(N)]
def timed(fn, n=10):
    fn(); torch.cuda.synchronize()
    t = 1e9
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        t = min(t, e0.elapsed_time(e1))
    return t
d = cfg.decoder
layers, nkv, D = d.num_hidden_layers, d.num_key_value_heads, d.head_dim
moved = 2 * layers * nkv * sum(rows) * D * 2                 # bytes of the 64 prompts, K and V
t_call = timed(lambda: m.restore(first, fans))
cap = m.prompt_store_info()[0]
enc.release(); del pred, enc; torch.cuda.empty_cache()
kc = torch.randn((layers, SLOTS, nkv, TMAX, D), device="cuda").to(torch.bfloat16); vc = kc.clone()
sk = torch.randn((layers, nkv, cap, D), device="cuda").to(torch.bfloat16); sv = sk.clone()
dev = lambda x: torch.tensor(x, dtype=torch.int32, device="cuda")
d_first, d_len, d_off, d_dst = dev(first), dev(rows), dev([i * K for i in range(N + 1)]), dev([s for f_ in fans for s in f_])
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
def copy():
    assert L.lib().surya_op_rec_kv_restore(L.DTYPE_BF16, L.ptr(kc), L.ptr(vc), L.ptr(sk), L.ptr(sv), L.ptr(d_first), L.ptr(d_len), L.ptr(d_off),
                                           L.ptr(d_dst), N, N * K, layers, SLOTS, nkv, TMAX, D, cap, st) == 0
t_copy = timed(copy)
d_slot = dev([i * K for i in range(N)])
def keep():
    assert L.lib().surya_op_rec_kv_keep(L.DTYPE_BF16, L.ptr(kc), L.ptr(vc), L.ptr(sk), L.ptr(sv), L.ptr(d_slot), L.ptr(d_first), L.ptr(d_len), N,
                                        layers, SLOTS, nkv, TMAX, D, cap, None, None, None, 0, 0, st) == 0
t_keep = timed(keep)
res.update(c_entries=N, c_fan=K, c_prompt_rows_mean=round(float(np.mean(rows)), 1), c_store_rows=cap, c_read_mib=round(moved / 2 ** 20, 1),
           c_written_mib=round(moved * K / 2 ** 20, 1), c_restore_call_ms=round(t_call, 4), c_restore_kernel_ms=round(t_copy, 4),
           c_restore_written_gb_per_s=round(moved * K / t_copy / 1e6, 1), c_keep_kernel_ms=round(t_keep, 4),
           c_keep_moved_gb_per_s=round(2 * moved / t_keep / 1e6, 1), c_bytes_per_line_mb=round(moved / N / 1e6, 3))
print(json.dumps(res))
