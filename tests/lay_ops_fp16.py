"""Test infrastructure: tests/lay_ops_ref.py for float16, the third compute dtype of the layout / table-recognition engine.

Everything that does not depend on the dtype IS lay_ops_ref's: the case shapes and seeds, the float64 references, the bound formulas, the
mutants, check() and emulate(). This module executes that file a second time as a private module instance (`R`) and restates in the
instance only what the file keys on torch.bfloat16:

  DTYPES        (float16,): the case builders round their float64 inputs to fp16;
  U             u = 2^-10, the fp16 unit in the last place relative to the value;
  r_P           2^-11 where the kernel rounds P to storage before P V (both MFMA kernels and the prompt kernel, as in bf16);
  emulation     the fp32 "reference alone" rounds P to fp16 for those kernels;
  kernel names  fp16 takes the matrix-core kernels bf16 takes (layout_model.hip selects them by sizeof(T) == 2);
  LayerNorm     the widths 128 / 256 / 512 / 1024 on BOTH kernels (lay_ln = 1 and 0), which the file lists for bf16 only.

Nothing in a bound is measured. On top of the bf16 case list, cases only fp16 can fail (fp16_only_cases):

  * subnormal P: cross attention at Lk = 576 and window attention with one key whose score exceeds all others by 11 -- every other entry
    of P lies in (2^-24, 2^-14), an fp16 SUBNORMAL; those keys carry positive V, the spike -1. 575 (63) such entries hold ~1e-2 (~1e-3) of
    the row's weight: a matrix core or a conversion that flushed them would miss the bound several times over. A second query uses a gap of
    24: every other entry rounds to zero. (The construction of tests/test_gpu_ocr_error_fp16.py.)
  * RMSNorm overflow, through all three kernels that hold the norm: rows whose x rstd (1 + w) exceeds 65504 in both signs (weight 60000,
    normalised values of about +-2.8) and a row holding one +inf (the reference returns zeros: variance inf, rstd 0, inf * 0 = NaN -> 0).
    rms_f16() restates the reference module (surya/common/adetr/decoder.py:29-47) in torch fp16 arithmetic for the exact checks.
  * GEGLU over every finite fp16 gate (up = 1).
Not a conftest; never imported by the product."""
from __future__ import annotations

import dataclasses
import importlib.util
import math
import sys

import torch

import lay_ops_ref as _BASE

F16 = torch.float16
U16, RP16 = 2.0 ** -10, 2.0 ** -11
F64 = torch.float64


def _instance():
    spec = importlib.util.spec_from_file_location("lay_ops_ref_fp16", _BASE.__file__)
    m = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = m                                   # dataclasses resolve the module by name
    spec.loader.exec_module(m)
    return m


R = _instance()
R.DTYPES = (F16,)
R.U[F16] = U16
Case, E = R.Case, R.E

_softmax_pv_base = R._softmax_pv
R._softmax_pv = lambda s, v, c, dt, round_p: _softmax_pv_base(s, v, c, dt, dt == torch.float32)     # every case here is fp16: P is rounded


def _with_rp(f):
    def g(c, dt, mutant=None):
        outs, aux = f(c, dt, mutant)
        if aux is not None:
            aux["rp"] = RP16
        return outs, aux
    return g


for _fam in ("window", "cross", "prompt"):
    R.FAMILIES[_fam] = _with_rp(R.FAMILIES[_fam])

LN_ROWS_WIDTHS = (128, 256, 512, 1024)
KERNELS = {"window": "swin_window_attn_mfma_kernel<fp16>", "cross": "transpose_cross_v_kernel + cross_attn_mfma_kernel<fp16>"}


def case_id(c) -> str:
    return f"{c.name}-fp16"


def rms_f16(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    """SuryaADETRDecoderRMSNorm.forward (surya/common/adetr/decoder.py:29-47) on fp16 tensors, statement by statement."""
    assert x.dtype == F16 and w.dtype == F16
    xf = x.float()
    variance = torch.clamp(xf.pow(2).mean(-1, keepdim=True), min=eps)
    output = xf * torch.rsqrt(variance)
    output = output * (1.0 + w.float())
    info = torch.finfo(x.dtype)
    output = output.clamp(min=info.min, max=info.max)
    output = torch.where(torch.isnan(output), torch.tensor(0.0), output)
    return output.type_as(x)


# ------------------------------------------------------------------------------------------------------------- the bf16 list in fp16
def _base_cases():
    out = []
    for c in R.all_cases():
        assert c.dtype == F16
        kern = KERNELS.get(c.family, c.kernel)
        if c.family == "ln" and c.p["C"] in LN_ROWS_WIDTHS:
            out.append(dataclasses.replace(c, kernel="layernorm_rows_bf16_kernel<fp16>"))
            out.append(dataclasses.replace(c, name=c.name[:-1] + "0", p={**c.p, "lay_ln": 0}, kernel="layernorm_kernel<fp16>"))
            continue
        out.append(dataclasses.replace(c, kernel=kern))
    return out


# ------------------------------------------------------------------------------------------------------------- fp16 only
SPIKE_KEY, GAPS = 100, (11.0, 24.0)


def _spike_scores_ok(c):
    """The construction holds: gap 11 -> every other P entry is an fp16 subnormal, gap 24 -> below 2^-25 (rounds to zero)."""
    _, aux = R.FAMILIES[c.family](c, F64, None)
    s = aux["s"]
    d = s.amax(-1, keepdim=True) - s
    d = d.reshape(-1, d.shape[-1]) if c.family == "cross" else d[0, 0]                 # cross: [rows * heads, Lk]; window: head 0 [64, 64]
    rows = {"cross": lambda g: slice(g * c.p["nq"], (g + 1) * c.p["nq"]), "window": lambda g: slice(g * 32, (g + 1) * 32)}[c.family]
    key = c.p["spike_key"]
    for gi, gap in enumerate(GAPS):
        dd = d[rows(gi)]
        others = torch.cat([dd[:, :key], dd[:, key + 1:]], -1)
        assert float(dd[:, key].abs().max()) == 0.0
        if gap < 20:
            p = torch.exp(-others)
            assert float(p.max()) < 2.0 ** -14 and float(p.min()) > 2.0 ** -24, "the other entries must be fp16 subnormals"
        else:
            assert float(others.min()) >= 20.0


def spike_cases():
    out = []
    # cross attention: 2 rows (gap 11, gap 24) over one image of 576 keys, D = 64, 4 query heads on 2 kv heads, q a plain matrix (S = 0)
    g = R._gen(4242)
    D, nq, nkv, Lk = 64, 4, 2, 576
    q = 1.0 + 0.01 * R._rand(g, 2, nq * D)
    q[1] *= GAPS[1] / GAPS[0]
    kv = torch.empty(1, Lk, 2 * nkv * D, dtype=F64)
    kv[..., :nkv * D] = 0.02 * R._rand(g, 1, Lk, nkv * D)
    kv[:, SPIKE_KEY, :nkv * D] = GAPS[0] / math.sqrt(D)           # score = scale * D * (gap / sqrt D) * ~1 = ~gap
    kv[..., nkv * D:] = 1.0 + R._rand(g, 1, Lk, nkv * D).abs()
    kv[:, SPIKE_KEY, nkv * D:] = -1.0
    chunk, _, _ = R.cross_plan(Lk)
    c = Case("cross", "cross-subnormalP-Lk576", F16, dict(M=2, nq=nq, nkv=nkv, D=D, Lk=Lk, S=0, images=1, scale=D ** -0.5, chunk=chunk,
                                                           spike_key=SPIKE_KEY),
             dict(kv=kv.to(F16), item_map=torch.zeros(2, dtype=torch.int32), q=q.to(F16), qpart=None), (), KERNELS["cross"])
    _spike_scores_ok(c)
    out.append(c)
    # window attention: one window, 2 heads; queries 0 .. 31 gap 11, queries 32 .. 63 gap 24; no bias, no shift
    g = R._gen(4343)
    nh = nkv = 2
    key = 37
    qkv = torch.empty(64, (nh + 2 * nkv) * 32, dtype=F64)
    qkv[:, :nh * 32] = 1.0 + 0.01 * R._rand(g, 64, nh * 32)
    qkv[32:, :nh * 32] *= GAPS[1] / GAPS[0]
    qkv[:, nh * 32:(nh + nkv) * 32] = 0.02 * R._rand(g, 64, nkv * 32)
    qkv[key, nh * 32:(nh + nkv) * 32] = GAPS[0] / math.sqrt(32)
    qkv[:, (nh + nkv) * 32:] = 8.0 + R._rand(g, 64, nkv * 32).abs()
    qkv[key, (nh + nkv) * 32:] = -1.0
    c = Case("window", "win-subnormalP", F16, dict(nh=nh, nkv=nkv, nwx=1, nwy=1, images=1, shift=0, spike_key=key),
             dict(qkv=qkv.to(F16), bias=torch.zeros(nh, 64, 64)), (), KERNELS["window"])
    _spike_scores_ok(c)
    out.append(c)
    return out


OVERFLOW_W = 60000.0             # representable in fp16 (a multiple of 32)


def _overflow_rows(g, C):
    """Row 0: one eighth of the entries at about +-3, the rest at about +-0.1 -> normalised +-2.8 and +-0.09: with 1 + w = 60001 the former
    leave the fp16 range in both signs, the latter stay finite. Row 1: ordinary values and one +inf. Row 2: ordinary."""
    x = R._rand(g, 3, C)
    sign = torch.where(R._rand(g, C) < 0, -1.0, 1.0)
    big = torch.arange(C) % 8 == 3
    x[0] = sign * torch.where(big, 3.0 + 0.05 * R._rand(g, C), 0.1 + 0.005 * R._rand(g, C))
    assert (x[0][big] > 0).any() and (x[0][big] < 0).any()
    x[1, C // 3] = math.inf
    return x.to(F16)


def overflow_cases():
    out = []
    g = R._gen(65504)
    C = 256
    x = _overflow_rows(g, C)
    w = torch.full((C,), OVERFLOW_W, dtype=F16)
    out.append(Case("rms", "rms-f16-overflow-inf", F16, dict(rows=3, C=C, eps=1e-5, exact_rows=(0, 1)), dict(x=x, w=w), (), "adetr_rmsnorm_kernel<fp16>"))
    # reduce-norm: x_out = T(res + T(bias + part)) must BE those rows: res = 0, no bias, one slab holding the rows (70000 where the +inf goes:
    # the Linear output above 65504 rounds to +inf, as .half() does)
    part = x.float()[None].clone()
    part[0, 1, C // 3] = 70000.0
    out.append(Case("reduce", "reduce-f16-overflow-inf", F16, dict(M=3, H=C, S=1, eps=1e-5, alias=False, dyadic=True, exact_rows=(0, 1), inf_at=(1, C // 3)),
                    dict(part=part, res=torch.zeros(3, C, dtype=F16), bias=None, w=w), (), "splitk_residual_adetr_norm_kernel<fp16>"))
    # heads: the final norm with that weight; everything after it stays finite
    Hd, lc = C, 20
    t = dict(x=x, fnorm_w=w, ln_w=(1 + 0.2 * R._rand(g, Hd)).to(F16), ln_b=(0.3 * R._rand(g, Hd)).to(F16), lm_w=(R._rand(g, lc, Hd) / Hd ** 0.5).to(F16),
             bb_w=(R._rand(g, 6, Hd) / Hd ** 0.5).to(F16), bb_b=R._rand(g, 6).to(F16))
    out.append(Case("heads", "heads-f16-overflow-inf", F16, dict(B=3, Hd=Hd, label_count=lc, ldx=Hd, rms_eps=1e-5, ln_eps=1e-5), t, (),
                    "layout_heads_kernel<fp16, false>"))
    return out


def geglu_sweep_case():
    """Every finite fp16 value as the gate, up = 1: x = (v, 1, 0, ...), gate rows (1, 0, ...), up rows (0, 1, 0, ...). 63488 rows x 64 outputs."""
    vals = torch.arange(0, 0x7C00, dtype=torch.int32).to(torch.int16).view(F16)
    vals = torch.cat([vals, -vals])
    M, K, I = vals.numel(), 64, 64
    x = torch.zeros(M, K, dtype=F16)
    x[:, 0], x[:, 1] = vals, 1.0
    w = torch.zeros(2 * I, K, dtype=F16)
    w[0::2, 0], w[1::2, 1] = 1.0, 1.0
    return Case("geglu", "geglu-every-finite-gate", F16, dict(M=M, N=2 * I, K=K), dict(x=x, w=w), (), "gemm EPI_GEGLU <fp16>")


def fp16_only_cases():
    return spike_cases() + overflow_cases() + [geglu_sweep_case()]


_CASES = None


def all_cases():
    """The bf16 case list in fp16, then the fp16-only cases. Built once per process and shared: never modified."""
    global _CASES
    if _CASES is None:
        _CASES = _base_cases() + fp16_only_cases()
    return _CASES


emulate, evaluate, reference, MUTANTS = R.emulate, R.evaluate, R.reference, R.MUTANTS


def check(c, outs):
    """lay_ops_ref.check. Every buffer must be finite -- except x_out of the reduce-norm overflow case, which must hold its one +inf (the
    Linear output above 65504, as .half() rounds it; held bit for bit like the rest of x_out) and nothing else that is not finite."""
    rep = R.check(c, outs)
    if "inf_at" in c.p:
        xo = outs["x_out"].reshape(c.p["M"], c.p["H"]).float()
        want = torch.zeros_like(xo, dtype=torch.bool)
        want[c.p["inf_at"]] = True
        ok = torch.equal(~torch.isfinite(xo), want) and float(xo[c.p["inf_at"]]) == math.inf
        rep = [(w, r, o, ok if w == "x_out" else f) for w, r, o, f in rep]
    return rep


def exact_norm_rows(c, y: torch.Tensor):
    """The fp16-only norm cases: where the reference module's fp16 result is +-65504 the kernel's must be exactly that, and the row holding
    +inf must be exactly zero. `y`: the kernel's norm output (fp16, CPU) for the case's rows. Returns the number of clamped elements checked."""
    x = c.t["x"] if c.family == "rms" else (c.t["res"].float() + c.t["part"][0]).to(F16)
    want = rms_f16(x, c.t["w"], c.p["eps"])
    clamped = want[0].abs() == 65504.0
    assert int((want[0][clamped] > 0).sum()) > 0 and int((want[0][clamped] < 0).sum()) > 0 and int((~clamped).sum()) > 0
    assert torch.isinf(x[1]).sum() == 1 and bool((want[1] == 0).all())
    got = y.reshape(want.shape)
    assert torch.equal(got[0][clamped], want[0][clamped]), "a value beyond the fp16 range must clamp to +-65504 exactly"
    assert bool((got[1] == 0).all()), "a row holding +inf must come out as zeros (clamp keeps NaN, then NaN -> 0)"
    return int(clamped.sum())
