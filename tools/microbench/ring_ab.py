"""Decode gate|up and down projections, loader / consumer ring (sa::Tuning dring = 1 / 2) against the gemm_nt_kernel tiles (dring = 0).

Each arm is timed as back-to-back launches (the replayed state the decode loop runs in), arms interleaved round by round so a lease's
drift hits all of them alike; prints the median device time per launch and the per-CU intake it implies (bytes a workgroup stages
into LDS / time, one workgroup per CU on the ring tiles).

  python tools/microbench/ring_ab.py [--rounds 5] [--iters 200]
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from surya_amd import _lib as L  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--M", type=int, default=256)
    args = ap.parse_args()
    lib = L.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    M = args.M
    g = torch.Generator(device="cuda").manual_seed(0)
    xg = torch.randn(M, 1280, device="cuda", generator=g).to(torch.bfloat16)
    wg = (torch.randn(10240, 1280, device="cuda", generator=g) / 36).to(torch.bfloat16)
    cg = torch.empty(M, 5120, device="cuda", dtype=torch.bfloat16)
    xd = torch.randn(M, 5120, device="cuda", generator=g).to(torch.bfloat16)
    wd = (torch.randn(1280, 5120, device="cuda", generator=g) / 72).to(torch.bfloat16)
    part = torch.empty(8, M, 1280, device="cuda", dtype=torch.float32)
    s = C.c_int(0)

    def gateup():
        return lib.surya_op_gemm(L.DTYPE_BF16, 0, L.EPI_SWIGLU, L.ptr(xg), C.c_long(1280), L.ptr(wg), C.c_long(1280), L.ptr(cg), C.c_long(5120),
                                 None, None, C.c_long(0), M, 10240, 1280, st)

    def down():
        return lib.surya_op_gemm_splitk_bf16(L.ptr(xd), C.c_long(5120), L.ptr(wd), C.c_long(5120), L.ptr(part), M, 1280, 5120, C.byref(s), st)

    # bytes one workgroup stages per launch (gate|up: 20 K-tiles; down: 26-27 K-tiles of its slice), by tile
    stage = {("gateup", 0): 20 * 128 * 128, ("gateup", 1): 20 * 224 * 128, ("down", 0): 80 / 3 * 128 * 128, ("down", 1): 80 / 3 * 128 * 128}
    res = {}
    L.check(lib.surya_set_tuning(b"dring_min_kt", C.c_int(16)), "dring_min_kt")       # the down projection on the ring in arms 1 / 2
    for _ in range(args.rounds):
        for name, fn in (("gateup", gateup), ("down", down)):
            for arm in (0, 1, 2):
                L.check(lib.surya_set_tuning(b"dring", C.c_int(arm)), "dring")
                for _ in range(10):
                    assert fn() == 0
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                res.setdefault((name, arm), []).append(e0.elapsed_time(e1) * 1000.0 / args.iters)
    L.check(lib.surya_set_tuning(b"dring", C.c_int(1)), "dring")
    L.check(lib.surya_set_tuning(b"dring_min_kt", C.c_int(0)), "dring_min_kt")
    assert lib.surya_gemm_ring_status(1) == 0, "a ring wait gave up"
    out = {}
    for (name, arm), v in sorted(res.items()):
        v = sorted(v)
        med = v[len(v) // 2]
        gbps = stage[(name, min(arm, 1))] / (med * 1e-6) / 1e9
        out[f"{name}_dring{arm}"] = dict(us_median=round(med, 2), us_all=[round(x, 2) for x in v], per_wg_intake_GBps=round(gbps, 1))
        print(f"{name:7s} dring={arm}: {med:7.2f} us  (runs {', '.join(f'{x:.2f}' for x in v)})  staged per workgroup / time: {gbps:5.1f} GB/s", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
