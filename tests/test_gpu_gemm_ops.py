"""GPU: the GEMM itself, one launch per case, through its op-level hooks and therefore through launch_gemm / launch_gemm_splitk as the engines
call them, against float64 under a per-element bound derived from the kernels' code (tests/gemm_ops_ref.py: the cases, the references, the
bounds, the knob row of every arm; tests/test_gemm_ops_cpu.py proves on the CPU that the bounds hold for an fp32 evaluation and that every
listed mutant leaves them). tests/test_gpu_ops.py, test_gpu_round4.py and the fp16 op tests hold the same kernels to one number per test
(2e-2 x max|ref| in bf16) or to another launch's bits, and none of their shapes sets the tuning knobs that select the 4-wave tile, the
3-stage rings or the big_m_* paths: a dropped K-chunk, a K-tile skipped in an odd tail, a slice boundary off by one tile or a residual added
before the rounding fits inside that.

Every case sets its arm's knobs through a fixture that restores the defaults. Outputs are pre-filled with NaN, the pad columns of C and the
slabs past the returned slice count with a sentinel, and every output sits between two guard bands. After the launch the guards are
intact, the inputs are bitwise unchanged and EVERY element meets its bound. Two arms are confirmed by what the launch reports: split-K by
its slice count, the ring by surya_gemm_ring_status. The table's four cases above 4000 rows evaluate their float64 reference with torch on the
device (code independent of the kernel), every other reference is evaluated on the host. A `GEMMOPS` line per case, a `GEMMOPS-WORST`
line per arm and dtype (informative: the assertion is ratio <= 1)."""
import collections
import ctypes as C

import pytest
import torch

import gemm_ops_ref as R
from surya_amd import _lib as L
from test_gpu_lay_ops import Bufs

pytestmark = pytest.mark.gpu

CASES = R.all_cases()
DT = {torch.float32: L.DTYPE_F32, torch.bfloat16: L.DTYPE_BF16, torch.float16: L.DTYPE_F16}
WORST = collections.defaultdict(float)
NAN = float("nan")
GEMM = [c for c in CASES if c.family == "gemm"]
SPLITK = [c for c in CASES if c.family == "splitk"]
ROPE = [c for c in CASES if c.family == "rope"]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _same(dev, host):
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[host.element_size()]
    return torch.equal(dev.cpu().contiguous().view(view), host.contiguous().view(view))


@pytest.fixture
def tune(hip_lib):
    """Set the GEMM tuning of one case; the defaults are back afterwards, and the ring's status word is clean before and after."""
    def set_(**kw):
        for k, v in kw.items():
            L.check(hip_lib.surya_set_tuning(k.encode(), C.c_int(v)), f"surya_set_tuning({k})")
    assert hip_lib.surya_gemm_ring_status(1) == 0
    yield set_
    set_(**R.DEFAULTS)


def _report(c, rep, hip_lib):
    torch.cuda.synchronize()
    if "ring" in c.kernel:
        assert hip_lib.surya_gemm_ring_status(1) == 0, "a ring wait gave up"
    worst = max(r for _, r, _, _ in rep)
    k = (c.arm, R.DT_NAME[c.dtype])
    WORST[k] = max(WORST[k], worst if worst != float("inf") else 1e30)
    print(f"GEMMOPS {c.id} [{c.kernel}]: " + ", ".join(f"{w} {r:.3f}" for w, r, _, _ in rep))
    assert all(over == 0 and finite for _, _, over, finite in rep), (c.id, c.kernel, rep)


@pytest.mark.parametrize("case", GEMM, ids=[c.id for c in GEMM])
def test_gemm(hip_lib, tune, case):
    c, p, b = case, case.p, Bufs()
    TO = R.out_dtype(c)
    n_out = p["N"] // 2 if p["epi"] == R.EPI_SWIGLU else p["N"]
    dev = {k: v.cuda() for k, v in c.t.items() if v is not None and not (k == "r" and p["inplace"])}
    if p["inplace"]:
        out = b.out((p["M"], p["ldc"]), TO, init=c.t["r"].cuda())           # C aliases R: the pad columns hold R's values and must keep them
    else:
        out = b.out((p["M"], p["ldc"]), TO, fill=R.SENT)
        out[:, :n_out] = NAN
    r = out if p["inplace"] else dev.get("r")
    tune(**c.knobs)
    args = (L.ptr(dev["x"]), C.c_long(p["ldx"]), L.ptr(dev["w"]), C.c_long(p["ldw"]), L.ptr(out), C.c_long(p["ldc"]), L.ptr(dev.get("b")), L.ptr(r),
            C.c_long(p["ldr"] if r is not None else 0), p["M"], p["N"], p["K"])
    if p["hook"] == "rec_f16":
        rc = hip_lib.surya_op_rec_gemm_f16(1 if p["out_f32"] else 0, p["epi"], *args, None, None, _stream())
    else:
        rc = hip_lib.surya_op_gemm(DT[c.dtype], int(p["out_f32"]), p["epi"], *args, _stream())
    assert rc == 0, rc
    b.check_guards()
    for k, v in dev.items():
        assert _same(v, c.t[k]), f"input {k} was written"
    if p["inplace"]:
        assert _same(out[:, n_out:], c.t["r"][:, n_out:]), "a pad column of C was written"
        got = {"out": out[:, :n_out]}
    else:
        got = {"out": out}
    if p["device_ref"]:
        rep = R.check(c, got, device="cuda", keep=False)
    else:
        rep = R.check(c, {k: v.cpu() for k, v in got.items()}, keep=False)
    _report(c, rep, hip_lib)


@pytest.mark.parametrize("case", SPLITK, ids=[c.id for c in SPLITK])
def test_splitk_slabs(hip_lib, tune, case):
    c, p, b = case, case.p, Bufs()
    dev = {k: v.cuda() for k, v in c.t.items()}
    part = b.out((R.SLAB_CAP, p["M"], p["N"]), torch.float32, fill=R.SENT)
    part[:p["S"]] = NAN
    tune(**c.knobs)
    s = C.c_int(0)
    f = hip_lib.surya_op_gemm_splitk_bf16 if c.dtype == torch.bfloat16 else hip_lib.surya_op_gemm_splitk_f16
    rc = f(L.ptr(dev["x"]), C.c_long(p["ldx"]), L.ptr(dev["w"]), C.c_long(p["ldw"]), L.ptr(part), p["M"], p["N"], p["K"], C.byref(s), _stream())
    assert rc == 0, rc
    assert s.value == p["S"], (s.value, p["S"])                              # the arm is confirmed by the slice count the launch returns
    b.check_guards()
    for k, v in dev.items():
        assert _same(v, c.t[k]), f"input {k} was written"
    _report(c, R.check(c, {"part": part.cpu()}, keep=False), hip_lib)


@pytest.mark.parametrize("case", ROPE, ids=[c.id for c in ROPE])
def test_rope_epilogue(hip_lib, tune, case):
    c, p, b = case, case.p, Bufs()
    dev = {k: v.cuda() for k, v in c.t.items()}
    out = b.out((p["M"], p["N"]), c.dtype)
    tune(**c.knobs)
    rc = hip_lib.surya_op_gemm_rope(DT[c.dtype], L.ptr(dev["x"]), C.c_long(p["ldx"]), L.ptr(dev["w"]), C.c_long(p["ldw"]), L.ptr(out), C.c_long(p["ldc"]),
                                    L.ptr(dev["b"]), L.ptr(dev["rope"]), p["rope_cols"], p["D"], p["M"], p["N"], p["K"], _stream())
    assert rc == 0, rc
    b.check_guards()
    for k, v in dev.items():
        assert _same(v, c.t[k]), f"input {k} was written"
    _report(c, R.check(c, {"out": out.cpu()}, keep=False), hip_lib)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
def test_launch_gemm_refuses_and_writes_nothing(hip_lib, dtype):
    """K = 0, an odd ldx, ldr off the 16-byte chunks: SA_ERR_SHAPE from the host, and C keeps its NaN fill (the checks stand in launch_gemm,
    before any launch; tests/test_gemm_ops_cpu.py asks the same of made-up pointers)."""
    M, N, K = 300, 136, 2 * R.ke(dtype)
    chunk = 16 // torch.tensor([], dtype=dtype).element_size()
    b = Bufs()
    x = torch.ones(M, K + 16, dtype=dtype, device="cuda")
    w = torch.ones(N, K, dtype=dtype, device="cuda")
    r = torch.ones(M, N + 16, dtype=dtype, device="cuda")
    out = b.out((M, N), dtype)
    g = lambda epi, ldx, ldr, k, rr: hip_lib.surya_op_gemm(DT[dtype], 0, epi, L.ptr(x), C.c_long(ldx), L.ptr(w), C.c_long(K), L.ptr(out), C.c_long(N), None,
                                                           L.ptr(rr), C.c_long(ldr), M, N, k, _stream())
    assert g(L.EPI_BIAS, K, 0, 0, None) == L.SA_ERR_SHAPE
    assert g(L.EPI_BIAS, K + 1, 0, K, None) == L.SA_ERR_SHAPE
    assert g(L.EPI_RESIDUAL, K, N + chunk // 2, K, r) == L.SA_ERR_SHAPE
    b.check_guards()
    assert bool(torch.isnan(out.float()).all()), "a refused call wrote C"


def test_worst_ratio_per_arm():
    """Printed after the tests above ran (file order): the worst error / bound per arm and dtype, for DESIGN.md."""
    for (arm, dt), w in sorted(WORST.items()):
        print(f"GEMMOPS-WORST {arm} {dt}: {w:.3f}")
        assert w <= 1.0
