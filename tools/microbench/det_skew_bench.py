"""What page-skew estimation and straightening cost (surya_det_skew, DetectionPredictor.skew, detection.skew.straighten).

    python tools/microbench/det_skew_bench.py --mode entry [--ab-lib OTHER.so[,OTHER2.so]] [--repeats 3] [--out FILE]      # one JSON line per run
    python tools/microbench/det_skew_bench.py --mode predictor [--arms none,skew] [--repeats 3]
    SURYA_AMD_LIB=/path/to/another/libsurya_amd.so python tools/microbench/det_skew_bench.py --mode predictor --arms none
    python tools/microbench/det_skew_bench.py --mode straighten

One process per run, every arm warmed, arms alternated, best of `repeats` and every repeat listed.

entry      surya_det_skew at 121 angles (the default grid) on 16 text-like 1024^2 maps (synth.text_like_map, 40 lines: the family
           surya_det_boxes is timed on) beside surya_det_boxes on the same maps, under device events, with the time of an empty event pair.
           The call at ONE angle is listed too: 16 workgroups walk the lists alone, so it shows the latency of one workgroup's walk, not
           a 121st of the profile pass. The split between the two passes is not taken here but from a kernel trace of this mode
           (rocprofv3 --kernel-trace, a run of its own: `skew_compact_kernel` / `skew_score_kernel`). --ab-lib: the same call through other
           builds of the library in the same process (SURYA_AMD_CXXFLAGS=-DSA_DET_SKEW_COMBINE=0: one LDS add per pixel instead of one
           per run of equal bins; -DSA_DET_SKEW_WALK=1: one list entry per lane in flight instead of four), scores held equal.
predictor  DetectionPredictor.__call__ on 16 pages of 1024^2, DET-DEFAULT synthetic weights, bf16, with `skew` set and with None, wall
           clock synchronised at both ends. Random weights give a text-free map, so plane 0 of every map is overwritten after the
           forward with the text rows drawn on the page (bench.py's e2e mechanism), in both arms alike.
straighten `straighten` of 16 RGBX pages of 1024^2 by 3 degrees on the device (upload, ONE surya_rec_rectify call, download, PIL images),
           and one host call for scale.

Synthetic weights: nothing here says how accurate the estimate is on real scans -- there is no trained checkpoint to measure it with."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
SIZE, PAGES, THR = 1024, 16, 0.35


def _event_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def run_entry(args):
    import numpy as np
    import torch
    from surya_amd import _lib as L
    from surya_amd.detection import skew as sk
    from surya_amd.synth import text_like_map
    lib = L.bind_det_skew(L.lib())
    maps = np.stack([text_like_map(SIZE, SIZE, 40, seed=100 + i) for i in range(PAGES)]).astype(np.float32)
    heat = torch.from_numpy(maps).cuda()
    angles = sk.candidate_angles(sk.SkewEstimate())
    tab = np.stack([sk.coeffs(angles)] * PAGES)
    cs, cs1 = torch.from_numpy(tab).cuda(), torch.from_numpy(np.ascontiguousarray(tab[:, 60:61])).cuda()
    scores = torch.empty((PAGES, len(angles)), dtype=torch.int64, device="cuda")
    n_text = torch.empty((PAGES,), dtype=torch.int32, device="cuda")
    ws = torch.empty(int(lib.surya_det_skew_workspace_bytes(PAGES, SIZE, SIZE)), dtype=torch.uint8, device="cuda")
    max_boxes = 4096
    bws = torch.empty(int(lib.surya_det_boxes_workspace_bytes(PAGES, SIZE, SIZE, max_boxes)), dtype=torch.uint8, device="cuda")
    boxes = torch.empty((PAGES, max_boxes, 4, 2), dtype=torch.float32, device="cuda")
    conf = torch.empty((PAGES, max_boxes), dtype=torch.float32, device="cuda")
    count = torch.empty((PAGES,), dtype=torch.int32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def skew(lb, table, n):
        def go():
            L.check(lb.surya_det_skew(L.ptr(heat), SIZE * SIZE, PAGES, SIZE, SIZE, THR, L.ptr(table), n, L.ptr(scores), L.ptr(n_text), L.ptr(ws),
                                      ws.numel(), stream), "surya_det_skew")
        return go

    def det_boxes():
        L.check(lib.surya_det_boxes(L.ptr(heat), C.c_long(SIZE * SIZE), PAGES, SIZE, SIZE, C.c_float(0.6), C.c_float(THR), max_boxes, L.ptr(boxes),
                                    L.ptr(conf), L.ptr(count), L.ptr(bws), C.c_size_t(bws.numel()), stream), "surya_det_boxes")

    arms = {"empty_event_pair": lambda: None, "det_boxes": det_boxes, "skew_121": skew(lib, cs, len(angles)), "skew_1": skew(lib, cs1, 1)}
    ab = [p for p in (args.ab_lib or "").split(",") if p]               # other builds of the library, same process
    for p in ab:
        other = L.bind_det_skew(C.CDLL(p))
        arms[f"skew_121@{os.path.basename(p)}"], arms[f"skew_1@{os.path.basename(p)}"] = skew(other, cs, len(angles)), skew(other, cs1, 1)
    ms = {k: [] for k in arms}
    check = {}
    for k, fn in arms.items():                                          # warm-up; the two builds must agree on the scores
        fn()
        torch.cuda.synchronize()
        if k.startswith("skew_121"):
            check[k] = (scores.cpu().numpy().copy(), n_text.cpu().numpy().copy())
    for k, v in check.items():
        assert all(np.array_equal(a, b) for a, b in zip(check["skew_121"], v)), f"{k}: the builds disagree"
    want, n0 = sk.skew_scores(maps[0], THR, tab[0])
    assert np.array_equal(check["skew_121"][0][0].view(np.uint64), want) and check["skew_121"][1][0] == n0
    for _ in range(args.repeats):
        for k, fn in arms.items():
            ms[k].append(_event_ms(torch, fn))
    best = {k: min(v) for k, v in ms.items()}
    line = {"tool": "det_skew_bench", "mode": "entry", "maps": [PAGES, SIZE, SIZE], "n_angles": len(angles), "repeats": args.repeats,
            "text_pixels_per_page": [int(v) for v in check["skew_121"][1]],
            "ms_best": {k: round(v, 4) for k, v in best.items()}, "ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
            "skew_over_det_boxes": round(best["skew_121"] / best["det_boxes"], 3)}
    for p in ab:
        line.setdefault("other_build_over_in_tree_121", {})[os.path.basename(p)] = round(best[f"skew_121@{os.path.basename(p)}"] / best["skew_121"], 3)
    return line


def run_predictor(args):
    import numpy as np
    import torch
    from PIL import Image
    from surya_amd.config import det_config
    from surya_amd.detection.predictor import DetectionPredictor
    from surya_amd.synth import make_det_weights, make_pages_with_lines
    pages, rows = make_pages_with_lines(PAGES, SIZE, seed=4321)
    imgs = [Image.fromarray(p) for p in pages]
    masks = np.zeros((PAGES, SIZE, SIZE), np.uint8)
    for i, rs in enumerate(rows):
        for x0, y0, x1, y1 in rs:
            masks[i, y0 + 4: y1 - 4, x0 + 4: x1 - 4] = 1
    masks_d = torch.from_numpy(masks).cuda()
    page_of = {id(im): i for i, im in enumerate(imgs)}

    class Det(DetectionPredictor):
        batch_size = 16

        def batch_heatmaps(self, images, batch_size=None):
            off = 0
            for heat, split_index, split_heights, sizes in super().batch_heatmaps(images, batch_size):
                n = split_index[-1] + 1
                idx = torch.tensor([page_of[id(im)] for im in images[off: off + n]], device=heat.device)
                heat[:, 0] = masks_d[idx].float() * 0.9 + 0.03
                off += n
                yield heat, split_index, split_heights, sizes

    cfg = det_config("DET-DEFAULT")
    pred = Det(checkpoint={"config": cfg, "state_dict": make_det_weights(cfg, 0), "size": SIZE}, dtype=torch.bfloat16)
    arms = args.arms.split(",")
    est = None
    if "skew" in arms:
        from surya_amd.detection.skew import SkewEstimate
        est = SkewEstimate()

    def call(arm):
        pred.skew = est if arm == "skew" else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = pred(imgs)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    times, info = {a: [] for a in arms}, {}
    for arm in arms:
        _, r = call(arm)
        info[arm] = {"boxes": sum(len(x.bboxes) for x in r), "angles": [getattr(x, "skew", None) for x in r][:4]}
    for _ in range(args.repeats):
        for arm in arms:
            times[arm].append(call(arm)[0])
    pred.skew = None
    return {"tool": "det_skew_bench", "mode": "predictor", "lib": os.environ.get("SURYA_AMD_LIB", "in-tree"), "config": "DET-DEFAULT bf16",
            "pages": PAGES, "size": SIZE, "repeats": args.repeats,
            "arms": {a: {"pages_per_s_best": round(PAGES / min(t), 2), "pages_per_s_all": [round(PAGES / x, 2) for x in t],
                         "ms_per_call_best": round(min(t) * 1e3, 2), **info[a]} for a, t in times.items()}}


def run_straighten(args):
    import numpy as np
    import torch
    from surya_amd.detection.skew import straighten, straighten_size
    from surya_amd.synth import make_pages
    pages = [np.ascontiguousarray(np.dstack([p, np.zeros(p.shape[:2], np.uint8)])) for p in make_pages(PAGES, SIZE, seed=3)]
    angles = [3.0] * PAGES

    def dev():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = straighten(pages, angles, device="cuda:0")
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r
    dev()
    t = [dev()[0] for _ in range(args.repeats)]
    t0 = time.perf_counter()
    host = straighten(pages[:1], angles[:1])
    t_host = time.perf_counter() - t0
    assert np.array_equal(np.asarray(host[0].image), np.asarray(dev()[1][0].image))
    return {"tool": "det_skew_bench", "mode": "straighten", "pages": PAGES, "size": SIZE, "pix": 4, "angle": 3.0,
            "out_size": list(straighten_size(SIZE, SIZE, 3.0)), "device_ms_per_call_best": round(min(t) * 1e3, 2),
            "device_ms_all": [round(x * 1e3, 2) for x in t], "device_pages_per_s_best": round(PAGES / min(t), 1),
            "host_ms_one_page": round(t_host * 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["entry", "predictor", "straighten"], required=True)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--arms", default="none,skew")
    ap.add_argument("--ab-lib")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("det_skew_bench: needs a GPU; nothing is measured without one")
    line = json.dumps({"entry": run_entry, "predictor": run_predictor, "straighten": run_straighten}[args.mode](args))
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
