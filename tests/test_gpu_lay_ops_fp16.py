"""GPU: every kernel of the layout / table-recognition engine alone in float16, through its op-level entry point
(surya_op_lay_<op>_f16, surya_op_gemm_geglu_f16: the launch code LayoutModel<fp16_t> itself uses) against float64 --
tests/test_gpu_lay_ops.py for the engine's third compute dtype. (surya_op_lay_<op>(dtype, ...) and surya_op_gemm's GEGLU code keep
their two dtypes and refuse SA_DTYPE_F16, as that file checks; the fp16 entries take the same arguments without `dtype`.)

The cases, the float64 references and the bounds are tests/lay_ops_fp16.py's: lay_ops_ref's case list and bound formulas with u = 2^-10
and r_P = 2^-11, the LayerNorm widths 128 ... 1024 on both kernels, and the cases only fp16 can fail (P entries that are fp16 subnormals,
the RMSNorm's clamp at 65504 and its NaN -> 0 on a row holding +inf through all three kernels that carry the norm, GEGLU over every
finite fp16 gate). The launchers and the guard bands are tests/test_gpu_lay_ops.py's, handed the fp16 entries under the names they call: outputs are pre-filled with NaN and sit between
guard bands, every element is held to the bound, the worst error / bound ratio of every output is printed (`LAYOPS` lines).

On top: a GEMM output above 65504 rounds to +inf (torch's .half()) while its neighbours stay finite, for the plain, the residual and the
GEGLU epilogue."""
import ctypes as C

import numpy as np
import pytest
import torch

import lay_ops_fp16 as H
import test_gpu_lay_ops as G
from surya_amd import _lib as L

pytestmark = pytest.mark.gpu

F16 = torch.float16
CASES = H.all_cases()


def run_cross(lib, c, b):
    """test_gpu_lay_ops.run_cross with the transposed values allocated for fp16 (there: for bf16 only)."""
    p = c.p
    _, _, lkp = H.R.cross_plan(p["Lk"])
    q = G._dev(c.t["q"] if p["S"] == 0 else c.t["qpart"])
    kv, im = G._dev(c.t["kv"]), G._dev(c.t["item_map"])
    out = b.out((p["M"], p["nq"] * p["D"]), F16)
    vT = b.out((p["images"] * p["nkv"] * p["D"] * lkp,), F16)
    rc = lib.surya_op_lay_cross_attn_f16(p["D"], G._p(q), p["S"], p["M"], G._p(kv), p["images"], G._p(im), G._p(out), None, G._p(vT), p["nq"],
                                     p["nkv"], p["Lk"], p["scale"], G._stream())
    torch.cuda.synchronize()
    want = torch.zeros(p["images"], p["nkv"], p["D"], lkp, dtype=F16)      # the transpose fills every element, the padding keys with zeros
    want[..., :p["Lk"]] = c.t["kv"].view(p["images"], p["Lk"], 2, p["nkv"], p["D"])[:, :, 1].permute(0, 2, 3, 1)
    assert torch.equal(vT.cpu().view(want.shape), want), "transpose_cross_v_kernel"
    return rc, {"out": out}


RUN = dict(G.RUN, cross=run_cross)


class Fp16Entries:
    """The library as tests/test_gpu_lay_ops.py's launchers call it, every call routed to the fp16 entry of the same op: surya_op_lay_<op>
    (dtype, ...) -> surya_op_lay_<op>_f16(...), surya_op_gemm(dtype, 0, EPI_GEGLU, X, ldx, W, ldw, C, ldc, NULL, NULL, 0, M, N, K, stream) ->
    surya_op_gemm_geglu_f16(X, ldx, W, ldw, C, ldc, M, N, K, stream). The dtype code those launchers pass is dropped."""

    def __init__(self, lib):
        self.lib = lib

    def __getattr__(self, name):
        if name.startswith("surya_op_lay_"):
            fn = getattr(self.lib, name + "_f16")
            return lambda dtype, *a: fn(*a)
        return getattr(self.lib, name)

    def surya_op_gemm(self, dtype, out_f32, epi, X, ldx, W, ldw, Cp, ldc, bias, R, ldr, M, N, K, stream):
        assert epi == L.EPI_GEGLU and not out_f32 and bias is None and R is None
        return self.lib.surya_op_gemm_geglu_f16(X, ldx, W, ldw, Cp, ldc, M, N, K, stream)


@pytest.mark.parametrize("case", CASES, ids=[H.case_id(c) for c in CASES])
def test_kernel_alone_vs_float64_fp16(hip_lib, case):
    b = G.Bufs()
    rc, outs = RUN[case.family](hip_lib if case.family == "cross" else Fp16Entries(hip_lib), case, b)
    assert rc == 0, rc
    b.check_guards()
    outs = {k: v.cpu() if v.is_cuda else v for k, v in outs.items()}
    rep = H.check(case, outs)
    for what, ratio, over, finite in rep:
        print(f"LAYOPS {case.kernel} | fp16 | {case.name} | {what} | {ratio:.3g}")
    bad = [(what, ratio, over, finite) for what, ratio, over, finite in rep if over or not finite]
    assert not bad, f"{H.case_id(case)} [{case.kernel}]: (output, worst error / bound, elements over the bound, finite): {bad}"
    if "exact_rows" in case.p:                                   # the norm's clamp and NaN -> 0, against the reference module in fp16
        n = H.exact_norm_rows(case, outs["y"])
        print(f"LAYOPS {case.kernel} | fp16 | {case.name} | {n} elements clamped to +-65504 exactly, the +inf row all zeros")


def _gemm(lib, epi, x, w, out, bias=None, res=None):
    M, K = x.shape
    N = w.shape[0]
    if epi == L.EPI_GEGLU:
        rc = lib.surya_op_gemm_geglu_f16(L.ptr(x), K, L.ptr(w), K, L.ptr(out), out.shape[1], M, N, K, C.c_void_p(G._stream()))
        assert rc == 0, rc
        torch.cuda.synchronize()
        return
    rc = lib.surya_op_gemm(L.DTYPE_F16, 0, epi, L.ptr(x), C.c_long(K), L.ptr(w), C.c_long(K), L.ptr(out), C.c_long(out.shape[1]), L.ptr(bias) if bias is not None
                           else None, L.ptr(res) if res is not None else None, C.c_long(res.shape[1] if res is not None else 0), M, N, K,
                           C.c_void_p(G._stream()))
    assert rc == 0, rc
    torch.cuda.synchronize()


def _half64(t):
    """float64 -> fp16 in ONE correctly rounded step (numpy converts directly; torch may go through fp32 and round twice), as float64."""
    with np.errstate(over="ignore"):
        return torch.from_numpy(t.numpy().astype(np.float16).astype(np.float64))


def _grid(shape, g, lim, den):
    return (torch.randint(-lim, lim + 1, shape, generator=g).float() / den).to(F16)


@pytest.mark.parametrize("epi", ["bias", "residual", "geglu"])
def test_gemm_output_above_65504_is_inf_and_its_neighbours_finite(hip_lib, epi):
    """Operands on a binary grid (every product a multiple of 2^-10, sums far below 2^24: the fp32 accumulation is exact in any order), one
    row of x and one row of W at 32: that dot product is 64 * 32 * 32 = 65536, which rounds to +inf in fp16 as torch's .half() does."""
    M, N, K = 65, 64, 64
    g = torch.Generator().manual_seed(9)
    x, w = _grid((M, K), g, 32, 16), _grid((N, K), g, 16, 64)
    x[3], w[6 if epi == "geglu" else 5] = 32.0, 32.0                         # geglu: row 6 = gate 3, row 7 = up 3
    b = G.Bufs()
    if epi == "geglu":
        w[7] = _grid((K,), g, 16, 64).abs() + 2.0 ** -6                      # a positive up: sign(gelu(inf) * up) = +
        out = b.out((M, N // 2), F16)
        _gemm(hip_lib, L.EPI_GEGLU, x.cuda(), w.cuda(), out)
        y = x.double() @ w.double().t()
        gate, up = _half64(y[:, 0::2]), _half64(y[:, 1::2])
        want = _half64(H.R._gelu_tanh(gate)) * up
        hot = (3, 3)
    else:
        bias = _grid((N,), g, 64, 64)
        res = _grid((M, N), g, 64, 64) if epi == "residual" else None
        out = b.out((M, N), F16)
        _gemm(hip_lib, L.EPI_RESIDUAL if res is not None else L.EPI_BIAS, x.cuda(), w.cuda(), out, bias.cuda(), res.cuda() if res is not None else None)
        want = _half64(x.double() @ w.double().t() + bias.double())           # T(x W^T + b): the sum is exact, one rounding
        if res is not None:
            want = want + res.double()                                                       # T(res + T(...)): rounded below
        hot = (3, 5)
    b.check_guards()
    got = out.cpu().double()
    want = _half64(want)
    assert torch.isinf(want[hot]) and want[hot] > 0 and int(torch.isinf(want).sum()) == 1
    assert torch.isinf(got[hot]) and got[hot] > 0, got[hot]
    fin = torch.isfinite(want)
    assert torch.isfinite(got[fin]).all() and not torch.isnan(got).any()
    if epi != "geglu":
        assert torch.equal(got[fin], want[fin])                              # exact sums: bit for bit
    else:                                                                    # tanhf: the GEGLU bound of lay_ops_ref with exact dot products
        gq, uq = _half64(H.R._gelu_tanh(gate)), up
        tol = H.U16 * want.abs() + (8 * H.E * gq.abs() + 4 * H.E * gate.abs() + H.U16 * gq.abs()) * uq.abs()
        assert bool(((got - want).abs()[fin] <= tol[fin]).all())


def test_fp16_cross_attention_refuses_what_bf16_refuses(hip_lib):
    """The fp16 matrix-core cross attention needs its transposed-value buffer and a head dim it has, like bf16."""
    x = torch.zeros(4096, device="cuda")
    p, s = x.data_ptr(), G._stream()
    assert hip_lib.surya_op_lay_cross_attn_f16(64, p, 1, 1, p, 1, p, p, None, None, 2, 2, 64, 0.125, s) == L.SA_ERR_ARG
    assert hip_lib.surya_op_lay_cross_attn_f16(48, p, 1, 1, p, 1, p, p, None, p, 2, 2, 64, 0.125, s) == L.SA_ERR_UNSUPPORTED
    torch.cuda.synchronize()
