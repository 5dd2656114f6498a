"""What centre lines and unrolling cost (surya_det_centerlines, surya_rec_unroll, DetectionPredictor.centerlines).

    python tools/microbench/det_centerline_bench.py --mode entry [--ab-lib OTHER.so[,OTHER2.so]] [--repeats 5] [--out FILE]   # one JSON line per run
    python tools/microbench/det_centerline_bench.py --mode unroll
    python tools/microbench/det_centerline_bench.py --mode predictor [--arms none,centerlines] [--repeats 5]
    SURYA_AMD_LIB=/path/to/another/libsurya_amd.so python tools/microbench/det_centerline_bench.py --mode predictor --arms none

One process per run, every arm warmed, arms alternated, best of `repeats` and every repeat listed.

entry      surya_det_centerlines at 16 knots behind surya_det_boxes, on 16 text-like 1024^2 maps (synth.text_like_map, 40 lines: the family
           surya_det_boxes is timed on) AND on 16 noise-like maps (uniform noise smoothed over 3 x 3: one component holds a large part of
           the page -- the contention case), beside surya_det_boxes on the same maps, under device events, with the time of an empty event
           pair. --ab-lib: the same call through other builds of the library in the same process (SURYA_AMD_CXXFLAGS=-DSA_DET_CL_LDS=0:
           every add goes to memory; -DSA_DET_CL_RUNS=0: every lane adds for its own four pixels), outputs held equal.
unroll     surya_rec_unroll on 256 bent crops of about 512 x 40 from 16 RGBX pages of 1024^2 beside surya_rec_rectify on as many quads of
           that size.
predictor  DetectionPredictor.__call__ on 16 pages of 1024^2, DET-DEFAULT synthetic weights, bf16, with `centerlines` set and with None,
           wall clock synchronised at both ends; plane 0 of every map is overwritten after the forward with the text rows drawn on the page
           (bench.py's e2e mechanism), in both arms alike.

Synthetic weights: nothing here says how accurate the centre lines are on real scans -- there is no trained checkpoint to measure it with."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
SIZE, PAGES, KNOTS, MAX_BOXES = 1024, 16, 16, 4096


def _event_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def noise_like_map(size, seed):
    import numpy as np
    from scipy import ndimage
    f = ndimage.uniform_filter(np.random.default_rng(seed).random((size, size)), size=3, mode="constant")
    return np.where(f > np.quantile(f, 0.45), 0.9, 0.02).astype(np.float32)


def run_entry(args):
    import numpy as np
    import torch
    from surya_amd import _lib as L
    from surya_amd.detection import centerline as cl
    from surya_amd.synth import text_like_map
    lib = L.bind_det_centerlines(L.lib())
    families = {"text": np.stack([text_like_map(SIZE, SIZE, 40, seed=100 + i) for i in range(PAGES)]).astype(np.float32),
                "noise": np.stack([noise_like_map(SIZE, 200 + i) for i in range(PAGES)])}
    bws = torch.empty(int(lib.surya_det_boxes_workspace_bytes(PAGES, SIZE, SIZE, MAX_BOXES)), dtype=torch.uint8, device="cuda")
    boxes = torch.empty((PAGES, MAX_BOXES, 4, 2), dtype=torch.float32, device="cuda")
    conf = torch.empty((PAGES, MAX_BOXES), dtype=torch.float32, device="cuda")
    count = torch.empty((PAGES,), dtype=torch.int32, device="cuda")
    n = PAGES * MAX_BOXES * KNOTS
    cnt, lo, hi = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3))
    sm = torch.empty(n, dtype=torch.int64, device="cuda")
    axis = torch.empty(PAGES * MAX_BOXES, dtype=torch.int32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ab = [p for p in (args.ab_lib or "").split(",") if p]
    libs = {"in_tree": lib, **{os.path.basename(p): L.bind_det_centerlines(C.CDLL(p)) for p in ab}}
    line = {"tool": "det_centerline_bench", "mode": "entry", "maps": [PAGES, SIZE, SIZE], "knots": KNOTS, "max_boxes": MAX_BOXES,
            "repeats": args.repeats, "families": {}}
    for fam, maps in families.items():
        heat = torch.from_numpy(maps).cuda()

        def det_boxes():
            L.check(lib.surya_det_boxes(L.ptr(heat), C.c_long(SIZE * SIZE), PAGES, SIZE, SIZE, C.c_float(0.6), C.c_float(0.35), MAX_BOXES, L.ptr(boxes),
                                        L.ptr(conf), L.ptr(count), L.ptr(bws), C.c_size_t(bws.numel()), stream), "surya_det_boxes")

        def centerlines(lb):
            def go():
                L.check(lb.surya_det_centerlines(PAGES, SIZE, SIZE, MAX_BOXES, KNOTS, L.ptr(bws), bws.numel(), L.ptr(cnt), L.ptr(sm), L.ptr(lo), L.ptr(hi),
                                                 L.ptr(axis), stream), "surya_det_centerlines")
            return go
        arms = {"empty_event_pair": lambda: None, "det_boxes": det_boxes, **{f"centerlines@{k}": centerlines(v) for k, v in libs.items()}}
        det_boxes()
        torch.cuda.synchronize()
        counts = count.cpu().numpy()
        check = {}
        for k, fn in arms.items():
            fn()
            torch.cuda.synchronize()
            if k.startswith("centerlines"):
                check[k] = [t.cpu().numpy().copy() for t in (cnt, sm, lo, hi, axis)]
        for k, v in check.items():
            assert all(np.array_equal(a, b) for a, b in zip(check["centerlines@in_tree"], v)), f"{k}: the builds disagree"
        want = cl.profile_page(maps[0], 0.6, 0.35, KNOTS)                # page 0 against the numpy statement
        n0 = len(want["axis"])
        got = check["centerlines@in_tree"]
        assert counts[0] == n0 and np.array_equal(got[0].view(np.uint32).reshape(PAGES, MAX_BOXES, KNOTS)[0, :n0], want["cnt"])
        assert np.array_equal(got[1].view(np.uint64).reshape(PAGES, MAX_BOXES, KNOTS)[0, :n0], want["sum"])
        ms = {k: [] for k in arms}
        for _ in range(args.repeats):
            for k, fn in arms.items():
                ms[k].append(_event_ms(torch, fn))
        best = {k: min(v) for k, v in ms.items()}
        biggest = int(got[0].view(np.uint32).reshape(PAGES, MAX_BOXES, KNOTS).sum(2).max())
        line["families"][fam] = {"components_per_page": [int(c) for c in counts], "largest_component_pixels": biggest,
                                 "ms_best": {k: round(v, 4) for k, v in best.items()}, "ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                                 "centerlines_over_det_boxes": round(best["centerlines@in_tree"] / best["det_boxes"], 3)}
    return line


def run_unroll(args):
    import numpy as np
    import torch
    from surya_amd import _lib as L
    from surya_amd.common.imageops import curve_table, quad_homographies
    from surya_amd.recognition.preprocess_gpu import RECTIFY_DESC, UNROLL_DESC
    from surya_amd.synth import make_pages
    lib = L.lib()
    pages = [np.ascontiguousarray(np.dstack([p, np.zeros(p.shape[:2], np.uint8)])) for p in make_pages(PAGES, SIZE, seed=3)]
    d_pages = torch.from_numpy(np.concatenate([p.reshape(-1) for p in pages])).cuda()
    n, W, H = 256, 512, 40
    ud, rd, tables, t_at = np.zeros(n, UNROLL_DESC), np.zeros(n, RECTIFY_DESC), [], 0
    quads = []
    for k in range(n):
        pg, row = k % PAGES, k // PAGES
        x0, y0 = 100.0 + 7 * (k % 11), 60.0 + 55.0 * row
        xs = np.linspace(0.0, 505.0, 17)
        table, w, h = curve_table(np.stack([x0 + xs, y0 + 30.0 * np.sin(np.pi * xs / 505.0)], 1), float(H))
        ud[k] = (pg * SIZE * SIZE * 4, SIZE, SIZE, w, h, k * W * 2 * H * 4, t_at)
        tables.append(table.reshape(-1))
        t_at += table.size
        c, s = np.cos(np.radians(6.0)), np.sin(np.radians(6.0))
        quads.append([(x0, y0), (x0 + W * c, y0 + W * s), (x0 + W * c - H * s, y0 + W * s + H * c), (x0 - H * s, y0 + H * c)])
        rd[k] = (pg * SIZE * SIZE * 4, SIZE, SIZE, W, H, k * W * 2 * H * 4, np.zeros(9))
    rd["h"] = quad_homographies(quads, rd["out_w"], rd["out_h"])
    d_tab = torch.from_numpy(np.concatenate(tables)).cuda()
    out = torch.empty(n * W * 2 * H * 4, dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    arms = {"empty_event_pair": lambda: None,
            "unroll": lambda: L.check(lib.surya_rec_unroll(L.ptr(d_pages), ud.ctypes.data_as(C.c_void_p), n, L.ptr(d_tab), L.ptr(out), 4,
                                                           int(ud["out_w"].max()), int(ud["out_h"].max()), stream), "surya_rec_unroll"),
            "rectify": lambda: L.check(lib.surya_rec_rectify(L.ptr(d_pages), rd.ctypes.data_as(C.c_void_p), n, L.ptr(out), 4, W, H, stream),
                                       "surya_rec_rectify")}
    ms = {k: [] for k in arms}
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        for k, fn in arms.items():
            ms[k].append(_event_ms(torch, fn))
    best = {k: min(v) for k, v in ms.items()}
    return {"tool": "det_centerline_bench", "mode": "unroll", "crops": n, "unrolled_size": [int(ud["out_w"][0]), int(ud["out_h"][0])],
            "rectified_size": [W, H], "pix": 4, "repeats": args.repeats, "ms_best": {k: round(v, 4) for k, v in best.items()},
            "ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "unroll_over_rectify": round(best["unroll"] / best["rectify"], 3)}


def run_predictor(args):
    import numpy as np
    import torch
    from PIL import Image
    from surya_amd.config import det_config
    from surya_amd.detection.centerline import Centerlines
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

    def call(arm):
        pred.centerlines = Centerlines() if arm == "centerlines" else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = pred(imgs)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    times, info = {a: [] for a in arms}, {}
    for arm in arms:
        _, r = call(arm)
        info[arm] = {"boxes": sum(len(x.bboxes) for x in r), "curved": sum(getattr(b, "centerline", None) is not None for x in r for b in x.bboxes)}
    for _ in range(args.repeats):
        for arm in arms:
            times[arm].append(call(arm)[0])
    pred.centerlines = None
    return {"tool": "det_centerline_bench", "mode": "predictor", "lib": os.environ.get("SURYA_AMD_LIB", "in-tree"), "config": "DET-DEFAULT bf16",
            "pages": PAGES, "size": SIZE, "repeats": args.repeats,
            "arms": {a: {"ms_per_call_best": round(min(t) * 1e3, 2), "ms_per_call_all": [round(x * 1e3, 2) for x in t],
                         "pages_per_s_best": round(PAGES / min(t), 2), **info[a]} for a, t in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["entry", "unroll", "predictor"], required=True)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--arms", default="none,centerlines")
    ap.add_argument("--ab-lib")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("det_centerline_bench: needs a GPU; nothing is measured without one")
    line = json.dumps({"entry": run_entry, "unroll": run_unroll, "predictor": run_predictor}[args.mode](args))
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
