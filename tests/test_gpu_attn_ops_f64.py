"""GPU: every attention kernel alone, through its op-level hook and therefore through launch_attn / launch_decode_attn / launch_decode_attn_kv8
as the engines call them, against float64 under a per-element bound derived from the kernels' code (tests/attn_ops_ref.py: the cases, the
references, the bounds; tests/test_attn_ops_cpu.py proves on the CPU that the bounds hold for an fp32 evaluation in the kernel's order and
that every listed mutant leaves them). tests/test_gpu_attn_ops.py, test_gpu_kv8.py and the fp16 op tests hold the same kernels to one number
per test (2e-2 x max|ref| on unit-variance data): a key dropped at a chunk edge, a forbidden key let through, a record combined without its
shift or a scale byte in the wrong K-tile fits inside that.

Every output buffer is pre-filled with NaN (scale bytes and the KV8 arrays with a sentinel) and sits between two guard bands; caches are
uploaded with their poison. Afterwards the guards are intact, EVERY element is held to its bound, and every byte the launch does not own --
the pad between output rows, rows between segments, all other cache rows, spare slots, scale rows >= rows, the inputs -- is unchanged.
The worst error / bound per kernel and dtype is printed (`ATTNOPS` lines)."""
import collections
import ctypes as C

import numpy as np
import pytest
import torch

import attn_ops_ref as R
from surya_amd import _lib as L
from test_gpu_lay_ops import Bufs

pytestmark = pytest.mark.gpu

CASES = R.all_cases()
DT = {torch.float32: L.DTYPE_F32, torch.bfloat16: L.DTYPE_BF16, torch.float16: L.DTYPE_F16}
U8, F32 = torch.uint8, torch.float32
SENT8, SENTF = 0xAA, -7.0
WORST = collections.defaultdict(float)

SEG = [c for c in CASES if c.family == "seg"]
DEC = [(c, v) for c in CASES if c.family == "dec" and not c.p["kv8"] for v in R.DEC_VARIANTS[c.dtype]]
KV8 = [c for c in CASES if c.family == "dec" and c.p["kv8"]]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t):
    return t.cuda().contiguous()


def _same(dev, host):
    """Bitwise (NaN poison included)."""
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[host.element_size()]
    return torch.equal(dev.cpu().contiguous().view(view), host.contiguous().view(view))


@pytest.fixture
def tune(hip_lib):
    """Set decode-attention tuning for one test; the defaults are back afterwards."""
    def set_(**kw):
        for k, v in kw.items():
            L.check(hip_lib.surya_set_tuning(k.encode(), C.c_int(v)), "surya_set_tuning")
    yield set_
    set_(dattn=4, dattn_db=0)


def _report(c, kernel, rep):
    worst = max(r for _, r, _, _ in rep)
    WORST[(kernel, R.DT_NAME[c.dtype])] = max(WORST[(kernel, R.DT_NAME[c.dtype])], worst if worst != float("inf") else 1e30)
    print(f"ATTNOPS {c.id} [{kernel}]: " + ", ".join(f"{k} {r:.3f}" for k, r, _, _ in rep))
    assert all(over == 0 and finite for _, _, over, finite in rep), (c.id, kernel, rep)


@pytest.mark.parametrize("case", SEG, ids=[c.id for c in SEG])
def test_segment_attention(hip_lib, case):
    c, p, b = case, case.p, Bufs()
    q = _dev(c.t["q"])
    k, v = (q, q) if c.t["k"] is c.t["q"] else (_dev(c.t["k"]), _dev(c.t["v"]))
    out = b.out((p["out_rows"], p["o_row"]), c.dtype)
    i64 = lambda key: np.ascontiguousarray([sg[key] for sg in p["segs"]], dtype=np.int64)
    sl = np.ascontiguousarray([sg["L"] for sg in p["segs"]], dtype=np.int32)
    offs = [i64(key) for key in ("q_off", "k_off", "v_off", "o_off")]
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    rc = hip_lib.surya_op_attn(DT[c.dtype], p["D"], L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(out), sl.ctypes.data_as(C.POINTER(C.c_int32)),
                               ip(offs[0]), ip(offs[1]), ip(offs[2]), ip(offs[3]), len(sl), p["heads"], p["group"], int(p["causal"]),
                               C.c_float(p["scale"]), C.c_long(p["q_row"]), C.c_long(p["q_head"]), C.c_long(p["k_row"]), C.c_long(p["k_head"]),
                               C.c_long(p["o_row"]), C.c_long(p["o_head"]), _stream())
    assert rc == 0, rc
    b.check_guards()
    assert _same(q, c.t["q"]) and _same(k, c.t["k"]) and _same(v, c.t["v"]), "an input was written"
    _report(c, c.kernel.split("<")[0], R.check(c, {"out": out.cpu()}))


def _run_decode(lib, c, b, mx):
    p, t = c.p, c.t
    dev = {k: _dev(t[k]) for k in ("part", "bias", "slots", "lens", "rope")}
    out = b.out((p["M"], p["nq"] * p["d"]), c.dtype)
    kc, vc = b.out(tuple(t["kc"].shape), c.dtype, init=t["kc"].cuda()), b.out(tuple(t["vc"].shape), c.dtype, init=t["vc"].cuda())
    outs = {"out": out, "kc": kc, "vc": vc}
    head = (L.ptr(dev["part"]), p["S"], L.ptr(dev["bias"]), L.ptr(out), L.ptr(kc), L.ptr(vc), L.ptr(dev["slots"]), L.ptr(dev["lens"]), L.ptr(dev["rope"]),
            p["M"], p["nq"], p["nkv"], p["Tmax"], C.c_float(p["scale"]), _stream())
    if mx:
        outs["out8"] = b.out((p["M"], p["nq"] * p["d"]), U8, fill=R.SENT_B)
        outs["sout"] = b.out((p["nq"] * p["d"] // 128, p["srows"], 4), U8, fill=R.SENT_B)
        rc = lib.surya_op_decode_attn_mx(DT[c.dtype], p["d"], *head, L.ptr(outs["out8"]), L.ptr(outs["sout"]), p["srows"])
    else:
        rc = lib.surya_op_decode_attn(DT[c.dtype], p["d"], *head)
    torch.cuda.synchronize()
    b.check_guards()
    for k in dev:
        assert _same(dev[k], t[k]), f"input {k} was written"
    return rc, {k: v.cpu() for k, v in outs.items()}


@pytest.mark.parametrize("case,variant", DEC, ids=[f"{c.id}-{v[0]}" for c, v in DEC])
def test_decode_attention(hip_lib, tune, case, variant):
    name, knobs, pinned = variant
    tune(**knobs)
    rc, outs = _run_decode(hip_lib, case, Bufs(), case.p["mx"])
    assert rc == 0, rc
    kern = {"flash2": "decode_attn_flash2_kernel", "flash2db": "decode_attn_flash2_kernel<DB>", "flash": "decode_attn_flash_kernel",
            "mfma": "decode_attn_mfma_kernel"}[name]
    _report(case, kern + ("+mx" if case.p["mx"] else ""), R.check(case, outs, pinned=pinned))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_decode_attention_without_a_copy_refuses_and_writes_nothing(hip_lib, dtype):
    c = next(c for c in CASES if c.family == "dec" and not c.p["kv8"] and c.dtype == dtype and c.p["family"] == "poison" and c.p["d"] == 128)
    rc, outs = _run_decode(hip_lib, c, Bufs(), True)
    assert rc == L.SA_ERR_UNSUPPORTED, rc
    assert bool(torch.isnan(outs["out"].float()).all()) and bool((outs["out8"] == R.SENT_B).all()) and bool((outs["sout"] == R.SENT_B).all())
    assert _same(outs["kc"], c.t["kc"]) and _same(outs["vc"], c.t["vc"])


@pytest.mark.parametrize("case", KV8, ids=[c.id for c in KV8])
def test_kv8_quant_rows_and_decode_attention(hip_lib, case):
    c, p, t = case, case.p, case.t
    names = ("k8", "v8t", "ksc", "vsc")
    # 1. surya_op_kv8_quant_rows: the tokens of every context, bit for bit the oracle's arrays; every other byte keeps its sentinel
    b = Bufs()
    kc, vc, ts, tp = (_dev(t[k]) for k in ("kc", "vc", "tok_slot", "tok_pos"))
    arr = {k: b.out(tuple(t[k].shape), t[k].dtype, fill=SENT8 if t[k].dtype == U8 else SENTF) for k in names}
    rc = hip_lib.surya_op_kv8_quant_rows(p["d"], L.ptr(kc), L.ptr(vc), L.ptr(ts), L.ptr(tp), int(ts.numel()), L.ptr(arr["k8"]), L.ptr(arr["v8t"]),
                                         L.ptr(arr["ksc"]), L.ptr(arr["vsc"]), p["nkv"], p["Tmax"], _stream())
    assert rc == 0, rc
    b.check_guards()
    sl, ps = t["tok_slot"].long(), t["tok_pos"].long()
    want = {k: torch.full(tuple(t[k].shape), SENT8 if t[k].dtype == U8 else SENTF, dtype=t[k].dtype) for k in names}
    for k in ("k8", "ksc", "vsc"):
        want[k][sl, :, ps] = t[k][sl, :, ps]
    want["v8t"][sl, :, ps >> 7, :, ps & 127] = t["v8t"][sl, :, ps >> 7, :, ps & 127]
    for k in names:
        assert _same(arr[k], want[k]), f"kv8_quant_rows: {k} differs from oracle.mx_oracle.kv8_quantize, or a byte outside the tokens was written"
    assert _same(kc, t["kc"]) and _same(vc, t["vc"])
    # 2. the decode step over the oracle's arrays (with their poison)
    b = Bufs()
    dev = {k: _dev(t[k]) for k in ("part", "bias", "slots", "lens", "rope")}
    arr = {k: b.out(tuple(t[k].shape), t[k].dtype, init=t[k].cuda()) for k in names}
    outs = dict(arr, out=b.out((p["M"], p["nq"] * p["d"]), c.dtype))
    head = (p["d"], L.ptr(dev["part"]), p["S"], L.ptr(dev["bias"]), L.ptr(outs["out"]), L.ptr(arr["k8"]), L.ptr(arr["v8t"]), L.ptr(arr["ksc"]), L.ptr(arr["vsc"]),
            L.ptr(dev["slots"]), L.ptr(dev["lens"]), L.ptr(dev["rope"]), p["M"], p["nq"], p["nkv"], p["Tmax"], C.c_float(p["scale"]), _stream())
    if p["mx"]:
        outs["out8"] = b.out((p["M"], p["nq"] * p["d"]), U8, fill=R.SENT_B)
        outs["sout"] = b.out((p["nq"] * p["d"] // 128, p["srows"], 4), U8, fill=R.SENT_B)
        rc = hip_lib.surya_op_decode_attn_kv8_mx(*head, L.ptr(outs["out8"]), L.ptr(outs["sout"]), p["srows"])
    else:
        rc = hip_lib.surya_op_decode_attn_kv8(*head)
    assert rc == 0, rc
    torch.cuda.synchronize()
    b.check_guards()
    for k in dev:
        assert _same(dev[k], t[k]), f"input {k} was written"
    _report(c, "decode_attn_kv8_kernel" + ("+mx" if p["mx"] else ""), R.check(c, {k: v.cpu() for k, v in outs.items()}))


def test_worst_ratio_per_kernel():
    """Printed after the tests above ran (file order): the worst error / bound per kernel and dtype, for DESIGN.md."""
    for (kern, dt), w in sorted(WORST.items()):
        print(f"ATTNOPS-WORST {kern} {dt}: {w:.3f}")
        assert w <= 1.0
