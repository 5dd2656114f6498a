"""GPU: every kernel of the layout / table-recognition engine alone, through its op-level entry point (surya_op_lay_*, surya_op_gemm's
GEGLU code: the launch code LayoutModel itself uses), against float64 under a bound that follows from the arithmetic
(tests/lay_ops_ref.py: the cases, the references, the bounds). The model-level tests hold these kernels to 3e-2 .. 4e-2 x max in bf16 through
whole networks: a dropped tail key, a wrong shift region in one corner window, a mistaken kv head map or an unsummed split-K slab fits
inside that.

Every output buffer is filled with NaN before the call and sits between two guard bands of a known value; afterwards the guards must be
untouched, no NaN may be left where the kernel has to write, and EVERY element is held to the bound. The worst error / bound ratio of
every output is printed (`LAYOPS` lines)."""
import ctypes as C

import numpy as np
import pytest
import torch

import lay_ops_ref as R
from surya_amd import _lib as L

pytestmark = pytest.mark.gpu

CASES = R.all_cases()
GUARD, GUARD_VALUE = 64, 7.0


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Bufs:
    """Device buffers of one call; every output between two guard bands."""

    def __init__(self):
        self.guarded = []

    def out(self, shape, dtype, fill=float("nan"), init=None):
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * GUARD,), GUARD_VALUE, dtype=dtype, device="cuda")
        mid = buf[GUARD:GUARD + n].view(shape)
        if init is not None:
            mid.copy_(init)
        else:
            mid.fill_(fill)
        self.guarded.append((buf, n))
        return mid

    def check_guards(self):
        torch.cuda.synchronize()
        for buf, n in self.guarded:
            assert bool((buf[:GUARD] == GUARD_VALUE).all()) and bool((buf[GUARD + n:] == GUARD_VALUE).all()), "a guard band was written"


def _dev(t):
    return None if t is None else t.cuda().contiguous()


def _p(t):
    return None if t is None else t.data_ptr()


def _dt(c):
    return L.DTYPE_F32 if c.dtype == torch.float32 else L.DTYPE_BF16


def run_window(lib, c, b):
    p = c.p
    nW = p["images"] * p["nwx"] * p["nwy"]
    qkv, bias = _dev(c.t["qkv"]), _dev(c.t["bias"])
    out = b.out((nW * 64, p["nh"] * 32), c.dtype)
    rc = lib.surya_op_lay_window_attn(_dt(c), _p(qkv), _p(bias), _p(out), nW, p["nh"], p["nkv"], p["nwx"], p["nwy"], p["shift"], 8, _stream())
    return rc, {"out": out}


def run_ln(lib, c, b):
    p = c.p
    x, w, bb, perm = (_dev(c.t[k]) for k in ("x", "w", "b", "perm"))
    n_out = (p["rows"] // p["rpi"]) * p["rpo"] if perm is not None else p["rows"]
    y = b.out((n_out, p["C"]), c.dtype)
    L.check(lib.surya_set_tuning(b"lay_ln", C.c_int(p["lay_ln"])), "surya_set_tuning")
    try:
        rc = lib.surya_op_lay_layernorm(_dt(c), _p(x), _p(w), _p(bb), _p(y), _p(perm), p["rows"], p["rpi"], p["C"], p["eps"], p["rpo"], _stream())
        torch.cuda.synchronize()
    finally:
        L.check(lib.surya_set_tuning(b"lay_ln", C.c_int(1)), "surya_set_tuning")
    r = torch.arange(p["rows"])
    dst = r if perm is None else (r // p["rpi"]) * p["rpo"] + c.t["perm"].long()[r % p["rpi"]]
    yc = y.cpu()
    untouched = torch.ones(n_out, dtype=torch.bool)
    untouched[dst] = False
    assert bool(torch.isnan(yc[untouched].float()).all()), "a row no token maps to was written"
    return rc, {"y": yc[dst]}


def run_merge(lib, c, b):
    p = c.p
    x, w, bb = (_dev(c.t[k]) for k in ("x", "w", "b"))
    y = b.out((p["B"] * (p["H"] // 2) * (p["W"] // 2), 4 * p["C"]), c.dtype)
    return lib.surya_op_lay_merge_ln(_dt(c), _p(x), _p(w), _p(bb), _p(y), p["B"], p["H"], p["W"], p["C"], p["eps"], _stream()), {"y": y}


def run_rms(lib, c, b):
    p = c.p
    x, w = _dev(c.t["x"]), _dev(c.t["w"])
    y = b.out((p["rows"], p["C"]), c.dtype)
    return lib.surya_op_lay_rmsnorm(_dt(c), _p(x), _p(w), _p(y), p["rows"], p["C"], p["eps"], _stream()), {"y": y}


def run_cross(lib, c, b):
    p = c.p
    chunk, ranges, lkp = R.cross_plan(p["Lk"])
    q = _dev(c.t["q"] if p["S"] == 0 else c.t["qpart"])
    kv, im = _dev(c.t["kv"]), _dev(c.t["item_map"])
    out = b.out((p["M"], p["nq"] * p["D"]), c.dtype)
    scratch = b.out((p["M"] * p["nq"] * ranges * (p["D"] + 2),), torch.float32) if c.dtype == torch.float32 else None
    vT = b.out((p["images"] * p["nkv"] * p["D"] * lkp,), c.dtype) if c.dtype == torch.bfloat16 else None
    rc = lib.surya_op_lay_cross_attn(_dt(c), p["D"], _p(q), p["S"], p["M"], _p(kv), p["images"], _p(im), _p(out), _p(scratch), _p(vT), p["nq"],
                                     p["nkv"], p["Lk"], p["scale"], _stream())
    if vT is not None:                                           # the transpose fills every element, the padding keys with zeros
        torch.cuda.synchronize()
        want = torch.zeros(p["images"], p["nkv"], p["D"], lkp, dtype=c.dtype)
        want[..., :p["Lk"]] = c.t["kv"].view(p["images"], p["Lk"], 2, p["nkv"], p["D"])[:, :, 1].permute(0, 2, 3, 1)
        assert torch.equal(vT.cpu().view(want.shape), want), "transpose_cross_v_kernel"
    return rc, {"out": out}


def run_prompt(lib, c, b):
    p = c.p
    qkv, rope = _dev(c.t["qkv"]), _dev(c.t["rope"])
    out = b.out((p["B"] * p["Tn"], p["nq"] * p["D"]), c.dtype)
    kc = b.out((p["B"], p["nkv"], p["Tmax"], p["D"]), c.dtype, fill=5.0)
    vc = b.out((p["B"], p["nkv"], p["Tmax"], p["D"]), c.dtype, fill=5.0)
    rc = lib.surya_op_lay_prefill_attn(_dt(c), p["D"], _p(qkv), _p(out), _p(kc), _p(vc), _p(rope), p["B"], p["Tn"], p["nq"], p["nkv"], p["Tmax"],
                                       p["scale"], _stream())
    torch.cuda.synchronize()
    assert bool((kc[:, :, p["Tn"]:] == 5.0).all()) and bool((vc[:, :, p["Tn"]:] == 5.0).all()), "a cache row >= Tn lost its sentinel"
    return rc, {"out": out, "k_rows": kc[:, :, :p["Tn"]], "v_rows": vc[:, :, :p["Tn"]]}


def run_reduce(lib, c, b):
    p = c.p
    part, bias, w = (_dev(c.t[k]) for k in ("part", "bias", "w"))
    if p["alias"]:
        res = xo = b.out((p["M"], p["H"]), c.dtype, init=c.t["res"].cuda())
    else:
        res, xo = _dev(c.t["res"]), b.out((p["M"], p["H"]), c.dtype)
    y = b.out((p["M"], p["H"]), c.dtype) if w is not None else None
    rc = lib.surya_op_lay_reduce_norm(_dt(c), _p(part), p["S"], p["M"], _p(res), _p(bias), _p(xo), _p(w), _p(y), p["H"], p["eps"], _stream())
    outs = {"x_out": xo}
    if y is not None:
        outs["y"] = y
    return rc, outs


def run_embed(lib, c, b):
    p = c.p
    fam = L.FAMILY_LAYOUT if p["family"] == "layout" else L.FAMILY_TABLE
    names = R.EMBED_NAMES[:15] if p["family"] == "layout" else R.EMBED_NAMES[:14] + R.EMBED_NAMES[15:]
    tabs = [_dev(c.t["tables"][nm]) for nm in names]
    ptrs = torch.tensor([t.data_ptr() for t in tabs] + [0] * (17 - len(tabs)), dtype=torch.int64).cuda()
    tok = _dev(c.t["tokens"])
    x = b.out((tok.shape[0], p["Hd"]), c.dtype)
    rc = lib.surya_op_lay_embed(_dt(c), fam, _p(tok), _p(ptrs), _p(x), tok.shape[0], p["Hd"], p["box_embed"], p["bbox_size"], p["vocab"],
                                p["label_count"], p["category_count"], p["merge_count"], _stream())
    torch.cuda.synchronize()
    return rc, {"x": x}


def run_rows(lib, c, b):
    p, k = c.p, c.p["kind"]
    src, idx = _dev(c.t["src"]), _dev(c.t["index"])
    if k == "patchify":
        dst = b.out((p["B"] * (p["H"] // p["P"]) * (p["W"] // p["P"]), p["Kpad"]), c.dtype)
        kind, dims = L.LAY_PATCHIFY, [p["B"], p["C"], p["H"], p["W"], p["P"], p["Kpad"]]
    else:
        dst = b.out(tuple(c.t["dst"].shape), c.dtype, init=c.t["dst"].cuda())
        if k == "add_rows":
            kind, dims = L.LAY_ADD_ROWS, [p["rows"], p["rpi"], p["C"]]
        elif k == "zero_rows":
            kind, dims = L.LAY_ZERO_ROWS, [p["B"], p["n_pad"], p["rpi"], p["C"]]
        else:
            kind, dims = L.LAY_GATHER_ADD, [p["rows"], p["rpi"], p["C"], p["rpi_src"]]
    d = np.asarray(dims, dtype=np.int32)
    return lib.surya_op_lay_rows(_dt(c), kind, _p(dst), _p(src), _p(idx), L.np_ptr(d), _stream()), {"dst": dst}


def run_heads(lib, c, b):
    p = c.p
    t = {k: _dev(v) for k, v in c.t.items()}
    cls, box = b.out((p["B"], p["label_count"]), torch.float32), b.out((p["B"], 6), torch.float32)
    rc = lib.surya_op_lay_heads(_dt(c), _p(t["x"]), p["ldx"], _p(t["fnorm_w"]), _p(t["ln_w"]), _p(t["ln_b"]), _p(t["lm_w"]), _p(t["bb_w"]),
                                _p(t["bb_b"]), _p(cls), _p(box), p["B"], p["Hd"], p["label_count"], p["rms_eps"], p["ln_eps"], _stream())
    torch.cuda.synchronize()
    return rc, {"cls": cls, "box": box}


def run_geglu(lib, c, b):
    p = c.p
    x, w = _dev(c.t["x"]), _dev(c.t["w"])
    out = b.out((p["M"], p["N"] // 2), c.dtype)
    rc = lib.surya_op_gemm(_dt(c), 0, L.EPI_GEGLU, L.ptr(x), C.c_long(p["K"]), L.ptr(w), C.c_long(p["K"]), L.ptr(out), C.c_long(p["N"] // 2), None, None,
                           C.c_long(0), p["M"], p["N"], p["K"], C.c_void_p(_stream()))
    return rc, {"out": out}


RUN = {"window": run_window, "ln": run_ln, "merge_ln": run_merge, "rms": run_rms, "cross": run_cross, "prompt": run_prompt, "reduce": run_reduce,
       "embed": run_embed, "rows": run_rows, "heads": run_heads, "geglu": run_geglu}


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_kernel_alone_vs_float64(hip_lib, case):
    b = Bufs()
    rc, outs = RUN[case.family](hip_lib, case, b)
    assert rc == 0, rc
    b.check_guards()
    rep = R.check(case, {k: v.cpu() if v.is_cuda else v for k, v in outs.items()})
    for what, ratio, over, finite in rep:
        print(f"LAYOPS {case.kernel} | {'fp32' if case.dtype == torch.float32 else 'bf16'} | {case.name} | {what} | {ratio:.3g}")
    bad = [(what, ratio, over, finite) for what, ratio, over, finite in rep if over or not finite]
    assert not bad, f"{case.id} [{case.kernel}]: (output, worst error / bound, elements over the bound, finite): {bad}"


def test_unsupported_dtype_and_shapes_are_refused(hip_lib):
    """fp32 and bf16 only, as the engine; the shape limits of the launch code come back as error codes before anything is launched."""
    x = torch.zeros(4096, device="cuda")
    p, s = x.data_ptr(), _stream()
    U_ = L.SA_ERR_UNSUPPORTED
    assert hip_lib.surya_op_lay_layernorm(L.DTYPE_F16, p, p, p, p, None, 1, 1, 64, 1e-5, 0, s) == U_
    assert hip_lib.surya_op_lay_window_attn(L.DTYPE_F16, p, p, p, 1, 1, 1, 1, 1, 0, 8, s) == U_
    assert hip_lib.surya_op_lay_window_attn(L.DTYPE_F32, p, p, p, 1, 1, 1, 1, 1, 0, 7, s) == U_
    assert hip_lib.surya_op_lay_merge_ln(L.DTYPE_F16, p, p, p, p, 1, 2, 2, 4, 1e-5, s) == U_
    assert hip_lib.surya_op_lay_rmsnorm(L.DTYPE_F16, p, p, p, 1, 64, 1e-5, s) == U_
    assert hip_lib.surya_op_lay_reduce_norm(L.DTYPE_F16, p, 1, 1, p, None, p, None, None, 64, 1e-5, s) == U_
    assert hip_lib.surya_op_lay_reduce_norm(L.DTYPE_F32, p, 9, 1, p, None, p, None, None, 64, 1e-5, s) == U_
    assert hip_lib.surya_op_lay_reduce_norm(L.DTYPE_F32, p, 1, 1, p, None, p, None, None, 4100, 1e-5, s) == U_
    assert hip_lib.surya_op_lay_cross_attn(L.DTYPE_F16, 64, p, 1, 1, p, 1, p, p, p, p, 2, 2, 64, 0.125, s) == U_
    assert hip_lib.surya_op_lay_cross_attn(L.DTYPE_F32, 48, p, 1, 1, p, 1, p, p, p, p, 2, 2, 64, 0.125, s) == U_
    assert hip_lib.surya_op_lay_cross_attn(L.DTYPE_F32, 64, p, 1, 1, p, 1, p, p, p, p, 32, 2, 64, 0.125, s) == U_
    assert hip_lib.surya_op_lay_prefill_attn(L.DTYPE_F16, 64, p, p, p, p, p, 1, 1, 2, 2, 8, 0.125, s) == U_
    assert hip_lib.surya_op_lay_prefill_attn(L.DTYPE_F32, 64, p, p, p, p, p, 1, 9, 2, 2, 8, 0.125, s) == U_
    assert hip_lib.surya_op_lay_embed(L.DTYPE_F16, L.FAMILY_LAYOUT, p, p, p, 1, 64, 0, 64, 70, 9, 0, 0, s) == U_
    assert hip_lib.surya_op_lay_embed(L.DTYPE_F32, L.FAMILY_LAYOUT, p, p, p, 1, 64, 0, 64, 64, 9, 0, 0, s) == L.SA_ERR_SHAPE
    assert hip_lib.surya_op_lay_heads(L.DTYPE_F16, p, 64, p, p, p, p, p, p, p, p, 1, 64, 20, 1e-5, 1e-5, s) == U_
    d = np.asarray([1, 1, 4], dtype=np.int32)
    assert hip_lib.surya_op_lay_rows(L.DTYPE_F16, L.LAY_ADD_ROWS, p, p, None, L.np_ptr(d), s) == U_
    assert hip_lib.surya_op_gemm(L.DTYPE_F16, 0, L.EPI_GEGLU, L.ptr(x), C.c_long(64), L.ptr(x), C.c_long(64), L.ptr(x), C.c_long(4), None, None,
                                 C.c_long(0), 1, 8, 64, C.c_void_p(s)) == U_
    torch.cuda.synchronize()
