"""GPU: every kernel of the OCR-error classifier alone, through its op-level entry point (surya_op_ocrerr_*: the launch code OcrErrModel
itself uses), against float64 under a bound that follows from the arithmetic (tests/ocr_ops_ref.py: the cases, the references, the
bounds). The model-level tests hold these kernels to 3e-2 x max in bf16 through whole networks: a dropped tail key, a lost chunk factor of
the [CLS] attention's running-max softmax, a wrong head at head_dim 80 or a wrapped id fits inside that.

Every output buffer is filled with NaN (labels: -1) before the call and sits between two guard bands of a known value; afterwards the
guards must be untouched, no NaN may be left where the kernel has to write, and EVERY element is held to the bound. The worst error / bound
ratio of every output is printed (`OCROPS` lines)."""
import numpy as np
import pytest
import torch

import ocr_ops_ref as R
from surya_amd import _lib as L

pytestmark = pytest.mark.gpu

CASES = R.all_cases()
GUARD, GUARD_VALUE = 64, 7.0
DT = {torch.float32: L.DTYPE_F32, torch.bfloat16: L.DTYPE_BF16, torch.float16: L.DTYPE_F16}


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Bufs:
    """Device buffers of one call; every output between two guard bands."""

    def __init__(self):
        self.guarded = []

    def out(self, shape, dtype, fill=float("nan")):
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * GUARD,), GUARD_VALUE, dtype=dtype, device="cuda")
        mid = buf[GUARD:GUARD + n].view(shape)
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


def run_embed(lib, c, b):
    p = c.p
    t = {k: _dev(v) for k, v in c.t.items()}
    y = b.out((p["rows"], p["C"]), c.dtype)
    rc = lib.surya_op_ocrerr_embed_ln(DT[c.dtype], _p(t["ids"]), _p(t["tok_pos"]), _p(t["word"]), _p(t["pos"]), _p(t["w"]), _p(t["b"]), _p(y),
                                      p["rows"], p["C"], p["vocab"], p["eps"], _stream())
    torch.cuda.synchronize()
    return rc, {"y": y}


def run_ln(lib, c, b):
    p = c.p
    x, w, bb = (_dev(c.t[k]) for k in ("x", "w", "b"))
    y = b.out((p["rows"], p["C"]), c.dtype)
    rc = lib.surya_op_ocrerr_layernorm(DT[c.dtype], _p(x), _p(w), _p(bb), _p(y), p["rows"], p["C"], p["eps"], _stream())
    torch.cuda.synchronize()
    return rc, {"y": y}


def run_gather(lib, c, b):
    p = c.p
    x, idx = _dev(c.t["x"]), _dev(c.t["idx"])
    out = b.out((p["n"], p["C"]), c.dtype)
    rc = lib.surya_op_ocrerr_gather_rows(DT[c.dtype], _p(x), _p(idx), _p(out), p["n"], p["C"], _stream())
    torch.cuda.synchronize()
    return rc, {"out": out}


def run_attn(lib, c, b):
    p = c.p
    qkv = _dev(c.t["qkv"])
    n = len(p["lens"])
    out = b.out((n, p["dim"]), c.dtype)
    starts, lens = np.asarray(p["starts"], dtype=np.int32), np.asarray(p["lens"], dtype=np.int32)
    rc = lib.surya_op_ocrerr_cls_attn(DT[c.dtype], p["D"], _p(qkv), L.np_ptr(starts), L.np_ptr(lens), n, _p(out), p["dim"], p["heads"],
                                      p["max_len"], p["scale"], _stream())
    return rc, {"out": out}


def run_head(lib, c, b):
    p = c.p
    pre, w, bb = (_dev(c.t[k]) for k in ("pre", "w", "b"))
    logits = b.out((p["n"], p["num_labels"]), torch.float32)
    labels = b.out((p["n"],), torch.int32, fill=-1)
    rc = lib.surya_op_ocrerr_cls_head(DT[c.dtype], _p(pre), _p(w), _p(bb), _p(logits), _p(labels), p["n"], p["dim"], p["num_labels"], _stream())
    torch.cuda.synchronize()
    lab = labels.cpu()
    assert bool(((lab >= 0) & (lab < p["num_labels"])).all()), "a label was not written, or lies outside the label set"
    return rc, {"logits": logits, "labels": lab}


def run_gemm(lib, c, b):
    """X rows ldx elements apart; everything between them (and nothing after row M - 1's K elements) is NaN: a row read at another stride
    poisons its outputs."""
    p = c.p
    M, N, K, ldx = p["M"], p["N"], p["K"], p["ldx"]
    X = torch.full(((M - 1) * ldx + K,), float("nan"), dtype=c.dtype, device="cuda")
    torch.as_strided(X, (M, K), (ldx, 1)).copy_(c.t["x"].cuda())
    w, bias, r = _dev(c.t["w"]), _dev(c.t["b"]), _dev(c.t["r"])
    out = b.out((M, N), c.dtype)
    rc = lib.surya_op_ocrerr_gemm(DT[c.dtype], p["epi"], p["pinned"], _p(X), ldx, _p(w), _p(bias), _p(out), _p(r), M, N, K, _stream())
    torch.cuda.synchronize()
    return rc, {"out": out}


RUN = {"embed_ln": run_embed, "ln": run_ln, "gather": run_gather, "cls_attn": run_attn, "cls_head": run_head, "gemm": run_gemm}


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_kernel_alone_vs_float64(hip_lib, case):
    b = Bufs()
    rc, outs = RUN[case.family](hip_lib, case, b)
    assert rc == 0, rc
    b.check_guards()
    rep = R.check(case, {k: v.cpu() for k, v in outs.items()})
    for what, ratio, over, finite in rep:
        print(f"OCROPS {case.kernel} | {R.DT_NAME[case.dtype]} | {case.name} | {what} | {ratio:.3g}")
    bad = [(what, ratio, over, finite) for what, ratio, over, finite in rep if over or not finite]
    assert not bad, f"{case.id} [{case.kernel}]: (output, worst error / bound, elements over the bound, finite): {bad}"


def test_refusals_launch_nothing(hip_lib):
    """fp32, a text longer than max_len and an LDS over 64 KB are refused by surya_op_ocrerr_cls_attn, shapes the vector accesses cannot take
    by every hook: an error code comes back and the NaN-filled output stays NaN."""
    b = Bufs()
    x = torch.zeros(1 << 16, dtype=torch.bfloat16, device="cuda")
    out = b.out((4096,), torch.bfloat16)
    p, s = x.data_ptr(), _stream()
    one, five, big = (np.asarray([v], dtype=np.int32) for v in (3, 5, 513))
    f = hip_lib.surya_op_ocrerr_cls_attn
    assert f(L.DTYPE_F32, 64, p, L.np_ptr(one), L.np_ptr(five), 1, _p(out), 768, 12, 512, 0.125, s) == L.SA_ERR_UNSUPPORTED
    assert f(L.DTYPE_BF16, 64, p, L.np_ptr(one), L.np_ptr(big), 1, _p(out), 768, 12, 512, 0.125, s) == L.SA_ERR_SHAPE
    assert f(L.DTYPE_F16, 64, p, L.np_ptr(one), L.np_ptr(five), 1, _p(out), 768, 12, 4096, 0.125, s) == L.SA_ERR_UNSUPPORTED
    assert f(L.DTYPE_BF16, 36, p, L.np_ptr(one), L.np_ptr(five), 1, _p(out), 72, 2, 512, 0.125, s) == L.SA_ERR_SHAPE
    assert hip_lib.surya_op_ocrerr_layernorm(L.DTYPE_BF16, p, p, p, _p(out), 1, 62, 1e-12, s) == L.SA_ERR_SHAPE
    assert hip_lib.surya_op_ocrerr_embed_ln(L.DTYPE_BF16, p, p, p, p, p, p, _p(out), 1, 62, 8, 1e-12, s) == L.SA_ERR_SHAPE
    assert hip_lib.surya_op_ocrerr_gather_rows(L.DTYPE_BF16, p, p, _p(out), 1, 62, s) == L.SA_ERR_SHAPE
    assert hip_lib.surya_op_ocrerr_gemm(L.DTYPE_BF16, R.EPI_BIAS, 1, p, 64, p, p, _p(out), None, 1, 64, 48, s) == L.SA_ERR_SHAPE
    assert hip_lib.surya_op_ocrerr_gemm(L.DTYPE_BF16, L.EPI_SWIGLU, 1, p, 64, p, p, _p(out), None, 1, 64, 64, s) == L.SA_ERR_UNSUPPORTED
    b.check_guards()
    assert bool(torch.isnan(out.float()).all()), "a refused call wrote its output"
