"""What flattening curled pages costs (surya_warp_mesh, detection.dewarp.dewarp).

    python tools/microbench/dewarp_bench.py --mode entry [--pix 3|4] [--ab-lib OTHER.so[,OTHER2.so]] [--repeats 7] [--out FILE]   # one JSON line per run
    python tools/microbench/dewarp_bench.py --mode call [--repeats 5]
    python tools/microbench/dewarp_bench.py --mode host

One process per run, every arm warmed, arms alternated, best of `repeats` and every repeat listed.

entry   surya_warp_mesh on 16 RGB (--pix 4: RGBX) pages of 2550 x 3300 (letter at 300 dpi) under the mesh fitted (cell 64) from the lines of a page curled by
        field B -- dy = A exp(-x / (0.25 W)) (1 + 0.3 y / H), A = 40 W / 1024: the gutter of a bound volume at the left edge -- beside
        surya_rec_rectify straightening the same pages by 1 degree (the parent's page-sized warp: the same taps per pixel), under device
        events, with the time of an empty event pair. --ab-lib: the same call through other builds of the library in the same process
        (SURYA_AMD_LIB_OUT: how the LDS-staged form of the kernel was measured before it was dropped), outputs held equal.
call    `dewarp(pages, meshes=..., device="cuda")` on the same 16 pages as PIL images: upload, one call, download, PIL images; wall clock,
        synchronised at both ends.
host    imageops.warp_mesh on ONE of those pages, wall clock.

Synthetic pages: nothing here says how well a fitted mesh flattens a real scan -- there is no trained checkpoint to detect its lines with."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
W, H, PAGES, CELL = 2550, 3300, 16, 64


def _event_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def field_b_mesh():
    """The mesh fit_mesh gives for the lines of a W x H page curled by field B (lines 45 W / 1024 apart, every third one short)."""
    import numpy as np
    from surya_amd.detection.dewarp import Dewarp, fit_mesh
    k = W / 1024.0
    lines, y0, n = [], 60.0 * k, 0
    while y0 <= H - 70.0 * k:
        xs = np.linspace(0.05 * W, (0.55 if n % 3 == 2 else 0.95) * W, 18)
        lines.append(np.stack([xs, y0 + 40.0 * k * np.exp(-xs / (0.25 * W)) * (1.0 + 0.3 * y0 / H)], 1))
        y0 += 45.0 * k
        n += 1
    mesh = fit_mesh(lines, (W, H), Dewarp(cell=CELL))
    assert mesh is not None
    return mesh


def make_pages(n):
    """Light, textured pages with dark rows: seeded bytes, nothing a cache could compress away."""
    import numpy as np
    out = []
    for i in range(n):
        pg = np.random.default_rng(900 + i).integers(180, 256, size=(H, W, 3), dtype=np.uint8)
        for y in range(150, H - 150, 110):
            pg[y: y + 36, 140: W - 140] //= 5
        out.append(pg)
    return out


def _bind(lib):
    i, p = C.c_int, C.c_void_p
    lib.surya_warp_mesh.argtypes, lib.surya_warp_mesh.restype = [p, p, i, p, p, i, i, i, p], C.c_int
    return lib


def run_entry(args):
    import numpy as np
    import torch
    from surya_amd import _lib as L
    from surya_amd.detection.skew import straighten_matrix, straighten_size
    from surya_amd.recognition.preprocess_gpu import MESH_DESC, RECTIFY_DESC
    lib = L.lib()
    mesh = field_b_mesh()
    pix = args.pix
    pages = [pg if pix == 3 else np.ascontiguousarray(np.dstack([pg, np.zeros(pg.shape[:2], np.uint8)])) for pg in make_pages(PAGES)]
    nbytes = W * H * pix
    al = lambda n: (n + 255) & ~255                                     # noqa: E731
    d_pages = torch.empty(PAGES * al(nbytes), dtype=torch.uint8, device="cuda")
    for k, pg in enumerate(pages):
        d_pages[k * al(nbytes): k * al(nbytes) + nbytes] = torch.from_numpy(pg.reshape(-1)).cuda()
    d_mesh = torch.from_numpy(mesh.reshape(-1)).cuda()
    md = np.zeros(PAGES, MESH_DESC)
    for k in range(PAGES):
        md[k] = (k * al(nbytes), W, H, CELL, 0, k * al(nbytes), 0)
    RW, RH = straighten_size(W, H, 1.0)
    rd = np.zeros(PAGES, RECTIFY_DESC)
    for k in range(PAGES):
        rd[k] = (k * al(nbytes), W, H, RW, RH, k * al(RW * RH * pix), straighten_matrix(W, H, 1.0))
    out = torch.empty(PAGES * al(RW * RH * pix), dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ab = [p for p in (args.ab_lib or "").split(",") if p]
    libs = {"in_tree": lib, **{os.path.basename(p): _bind(C.CDLL(p)) for p in ab}}

    def warp(lb):
        def go():
            L.check(lb.surya_warp_mesh(L.ptr(d_pages), md.ctypes.data_as(C.c_void_p), PAGES, L.ptr(d_mesh), L.ptr(out), pix, W, H, stream), "surya_warp_mesh")
        return go

    def rectify():
        L.check(lib.surya_rec_rectify(L.ptr(d_pages), rd.ctypes.data_as(C.c_void_p), PAGES, L.ptr(out), pix, RW, RH, stream), "surya_rec_rectify")
    arms = {"empty_event_pair": lambda: None, "rectify_1deg": rectify, **{f"warp_mesh@{k}": warp(v) for k, v in libs.items()}}
    seen = {}
    for k, fn in arms.items():
        out.zero_()
        fn()
        torch.cuda.synchronize()
        if k.startswith("warp_mesh"):
            seen[k] = out[: PAGES * al(nbytes)].clone()
    for k, v in seen.items():
        assert torch.equal(seen["warp_mesh@in_tree"], v), f"{k}: the builds disagree"
    ms = {k: [] for k in arms}
    for _ in range(args.repeats):
        for k, fn in arms.items():
            ms[k].append(_event_ms(torch, fn))
    best = {k: min(v) for k, v in ms.items()}
    px = PAGES * W * H
    return {"tool": "dewarp_bench", "mode": "entry", "pages": PAGES, "size": [W, H], "pix": pix, "cell": CELL, "mesh_shape": list(mesh.shape),
            "max_shift_px": round(float(abs(mesh[..., 1]).max()), 2), "rectified_size": [RW, RH], "repeats": args.repeats,
            "ms_best": {k: round(v, 4) for k, v in best.items()}, "ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
            "warp_mesh_gpix_per_s": round(px / best["warp_mesh@in_tree"] / 1e6, 2),
            "rectify_gpix_per_s": round(PAGES * RW * RH / best["rectify_1deg"] / 1e6, 2),
            "warp_mesh_over_rectify_per_pixel": round((best["warp_mesh@in_tree"] / px) / (best["rectify_1deg"] / (PAGES * RW * RH)), 3),
            "warp_mesh_over_rectify": round(best["warp_mesh@in_tree"] / best["rectify_1deg"], 3)}


def run_call(args):
    import numpy as np
    import torch
    from PIL import Image
    from surya_amd.detection.dewarp import Dewarp, dewarp
    mesh = field_b_mesh()
    imgs = [Image.fromarray(p) for p in make_pages(PAGES)]
    meshes = [mesh] * PAGES

    def call():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = dewarp(imgs, meshes=meshes, options=Dewarp(cell=CELL), device="cuda:0")
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r
    _, r = call()
    assert all(x.mesh is mesh and x.image.size == (W, H) for x in r) and not np.array_equal(np.asarray(r[0].image), np.asarray(imgs[0]))
    t = [call()[0] for _ in range(args.repeats)]
    return {"tool": "dewarp_bench", "mode": "call", "pages": PAGES, "size": [W, H], "cell": CELL, "repeats": args.repeats,
            "ms_per_call_best": round(min(t) * 1e3, 1), "ms_per_call_all": [round(x * 1e3, 1) for x in t], "pages_per_s_best": round(PAGES / min(t), 2)}


def run_host(args):
    from surya_amd.common.imageops import warp_mesh
    mesh = field_b_mesh()
    (pg,) = make_pages(1)
    t0 = time.perf_counter()
    out = warp_mesh(pg, mesh, CELL)
    dt = time.perf_counter() - t0
    assert out.shape == pg.shape
    return {"tool": "dewarp_bench", "mode": "host", "pages": 1, "size": [W, H], "cell": CELL, "s_per_page": round(dt, 2),
            "s_per_16_pages_extrapolated": round(16 * dt, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["entry", "call", "host"], required=True)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--pix", type=int, choices=[3, 4], default=3, help="entry: RGB or RGBX pages")
    ap.add_argument("--ab-lib")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.mode != "host":
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("dewarp_bench: needs a GPU; nothing is measured without one")
    line = json.dumps({"entry": run_entry, "call": run_call, "host": run_host}[args.mode](args))
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
