"""Test infrastructure: the OCR-error classifier's kernels one at a time (surya_op_ocrerr_*: the launchers OcrErrModel itself uses) -- the
cases, float64 references of every op in plain torch, and the per-element error bound each family is held to. Built like lay_ops_ref.py.

A Case holds the inputs exactly as the device gets them (already rounded to the storage type T) and the parameters of ONE call.
evaluate(case, dt, mutant) computes the op:
  dt = float64              the reference. It rounds to storage only where the bound below says so;
  dt = float32              "the reference alone": fp32 arithmetic that rounds where the kernel rounds, outputs rounded to storage;
  mutant = a name           a deliberately wrong evaluation (float64): what the bound has to catch (MUTANTS).
check(case, outs) holds EVERY element of every output to the bound and wants every buffer finite. Nothing in a bound is measured.

Symbols: u = one unit in the last place relative to the value (fp32 2^-23, bf16 2^-7, fp16 2^-10): half of it the rounding to storage, the
other half a rounding that flips because the fp32 value differs in its last bits. E = 2^-24, the unit roundoff of fp32.

layernorm, embed_ln (C channels, two reductions; lay_ops_ref.py has the derivation):
    tol = u |ref| + (C + 8) E (|x - mean| + mean|x|) rstd |w| + (C + 8) E |b|
    embed_ln: x = T(word[clamp(id)] + pos[p]) is ONE correctly rounded add of two T values: torch arithmetic in the storage dtype on the
    CPU, in the reference as in the kernel. Rows whose ids clamp to the same table row at the same position must come out bit-equal.
cls_attn (one query per text, N = L keys in NC = ceil(L / 64) chunks, head dim D, p = softmax(s), A = sum_j p_j |v_j|):
    tol = u |ref| + (2 e_s + 2 e_exp + (N + NC + 4) E + r_P) A + sub
    e_s   = max_j (D + 4) E scale sum_c |q_c| |k_jc| + 2 E |s_j|         (a D-term fp32 dot product, the scale)
    e_exp = (max_j |s_j - m| + 4 (NC + 1)) 2^-23. The single-pass form of lay_ops_ref.py is (max |s - m| + 4) 2^-23 for ONE exp2 per entry
            (product with log2 e, exp2, the subtraction). cls_attn_kernel walks the keys in chunks with a running max: an entry's weight is
            the product of up to NC + 1 exp2 factors -- exp(s_j - m_c), then exp(m_c - m) in the numerator, or the chain of rescalings
            exp(m_c - m_c+1) ... of the denominator -- whose exponents have one sign and add up to s_j - m. The |x| 2^-24-per-unit part of the
            error therefore adds up to the single-pass one; the fixed 4 x 2^-23 is paid once per factor. Inputs keep |s - m| <= 40.
    (N + NC + 4) E: the fp32 sums over the keys of the numerator and the denominator, one product and one addition per chunk, the division.
    r_P   = half a storage step of the un-normalised P the kernel rounds to T before P V: 2^-8 (bf16), 2^-11 (fp16).
    sub   = fp16 only: an entry below 2^-14 is rounded to a SUBNORMAL, an absolute error of up to 2^-25 instead of a relative one:
            sum over the entries with exp(s_j - m) < 2^-14 of 2^-25 |v_j|, over l = sum_j exp(s_j - m). (The kernel rounds exp(s_j - m_c) with
            m_c <= m: an entry subnormal there is below 2^-14 here too, and its error is scaled down by exp(m_c - m) <= 1 afterwards.)
    No "P left unrounded" mutant: the float64 reference does not round P, so that mutant IS the reference; r_P is the room the bound leaves
    for the kernel's rounding, not something an output can be caught lacking.
cls_head (K = dim): logits tol = u |ref| + 2 (K + 4) E (|x| |W|^T) + E |b| against the UNROUNDED float64 value; every logit must be a value
    of T (the kernel rounds them: the reference's logits are T tensors); the label must equal the first argmax of the candidate's OWN
    logits, and the reference's argmax wherever the reference's margin exceeds 2 tol. A row whose input holds a NaN: all its logits NaN,
    label 0, the other rows unaffected.
gather_rows: bit for bit.
gemm (OcrErrModel's GEMM, pinned 64 x 64 tile or launch_gemm's choice): operands on the binary grid of test_gpu_ocr_error_fp16.py section 3
    (x in 2^-4 steps within [-2, 2], W in 2^-6 steps within [-1/4, 1/4], bias in 2^-6 steps within [-1, 1], the residual on x's grid):
    every product is a multiple of 2^-10 and every partial sum stays below 2^11, so the fp32 accumulation is exact in ANY order up to K =
    3072 and x W^T + b is the same 21-bit number in the kernel and in float64. bias, ReLU: T(.) of it, bit for bit. residual: T(T(x W^T + b)
    + R) -- the second sum is exact in fp32 too -- bit for bit. GELU: got = T(g + d) against want = T(g) differ by at most ONE STORAGE STEP
    of want plus |d|, d = the absolute error of the epilogue's erf GELU before its store:
      fp16  d = 0: gelu_epi<fp16_t> rounds the projection to fp16 first (so does the reference) and its erfc has a RELATIVE error below
            1.2e-7, far inside half a step for every finite input (common.h): one step, as test_gpu_ocr_error_fp16.py has it;
      bf16  d = 0.5 |x| 1.5e-7 + 2^-21 |g|: gelu_epi's Abramowitz-Stegun erfc is good to 1.5e-7 ABSOLUTE (common.h), which 0.5 |x|
            multiplies; rcp, exp and the polynomial's roundings are relative to erfc <= 1 <= 2 - erfc: 2^-21 |g| covers them and the two
            products. In the negative tail (x = -5: g = -1.4e-6, a bf16 step of 7e-9) the absolute term is most of the bound: the grid's
            projections reach |x| = 30 at K = 3072, where one step alone does not describe that code;
      fp32  d = 2^-23 |x| + 2^-22 |g|: 0.5 x (1 + erff(x / sqrt 2)): erff to 2 ulp of a value <= 1 (2^-23), the rounded argument moves erf
            by at most erf'(z) z 2^-23 <= 2^-24, the sum 1 + erf rounds by 2^-24: 2^-22 absolute on the bracket, times 0.5 |x|; the two
            products 2^-22 |g|.
Not a conftest; never imported by the product."""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

E = 2.0 ** -24
U = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}
RP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
MANT = {torch.float32: 23, torch.bfloat16: 7, torch.float16: 10}
MIN_EXP = {torch.float32: -126, torch.bfloat16: -126, torch.float16: -14}
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
DTYPES16 = (torch.bfloat16, torch.float16)
DT_NAME = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}
F64, F32 = torch.float64, torch.float32
EPI_BIAS, EPI_RESIDUAL, EPI_GELU, EPI_RELU = 0, 1, 2, 5
EPI_NAME = {EPI_BIAS: "bias", EPI_RESIDUAL: "residual", EPI_GELU: "gelu", EPI_RELU: "relu"}


@dataclass
class Case:
    family: str
    name: str
    dtype: torch.dtype
    p: dict
    t: Dict[str, Optional[torch.Tensor]]
    kills: Tuple[str, ...] = ()          # the mutants this case is meant to catch
    kernel: str = ""
    _ref: Optional[tuple] = field(default=None, repr=False)

    @property
    def id(self):
        return f"{self.name}-{DT_NAME[self.dtype]}"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F64)


def _rk(c, dt):
    """Rounding the KERNEL makes (only the fp32 emulation repeats it) and rounding the REFERENCE makes too."""
    rr = lambda x: x.to(F32).to(c.dtype).to(dt)
    return (rr if dt == F32 else (lambda x: x)), rr


# ------------------------------------------------------------------------------------------------------------- layernorm, embed_ln
def _ln(x, w, b, eps, mutant=None):
    C = x.shape[-1]
    mean = x[..., :C - 4].mean(-1, keepdim=True) if mutant == "mean_c_minus_4" else x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = 1.0 / (torch.sqrt(var) + eps) if mutant == "eps_outside_sqrt" else torch.rsqrt(var + eps)
    return d * rstd * w + b, d, rstd


def _ln_tol(c, ref, x, d, rstd, w, b):
    C = x.shape[-1]
    return U[c.dtype] * ref.abs() + (C + 8) * E * ((d.abs() + x.abs().mean(-1, keepdim=True)) * rstd * w.abs() + b.abs())


def f_ln(c, dt, mutant=None):
    rk, _ = _rk(c, dt)
    x, w, b = (c.t[k].to(dt) for k in ("x", "w", "b"))
    y, d, rstd = _ln(x, w, b, c.p["eps"], mutant)
    return {"y": rk(y)}, dict(x=x, d=d, rstd=rstd, w=w, b=b)


def f_embed(c, dt, mutant=None):
    rk, _ = _rk(c, dt)
    V = c.p["vocab"]
    ids, tp = c.t["ids"].long(), c.t["tok_pos"].long()
    idc = torch.remainder(ids, V) if mutant == "id_wrapped" else ids.clamp(0, V - 1)
    if mutant == "sum_unrounded":
        x = c.t["word"].to(F64)[idc] + c.t["pos"].to(F64)[tp]
    else:
        x = (c.t["word"][idc] + c.t["pos"][tp]).to(dt)           # one correctly rounded add in the storage dtype
    w, b = c.t["w"].to(dt), c.t["b"].to(dt)
    y, d, rstd = _ln(x, w, b, c.p["eps"], mutant)
    return {"y": rk(y)}, dict(x=x, d=d, rstd=rstd, w=w, b=b)


# ------------------------------------------------------------------------------------------------------------- gather_rows
def f_gather(c, dt, mutant=None):
    idx = c.t["idx"].long()
    if mutant == "index_ignored":
        idx = torch.arange(idx.numel())
    if mutant == "rows_sorted":
        idx = idx.sort().values
    return {"out": c.t["x"][idx].to(dt)}, None


# ------------------------------------------------------------------------------------------------------------- cls_attn
def _text_views(c, dt, i):
    p = c.p
    H, D, dim = p["heads"], p["D"], p["dim"]
    s0, L = p["starts"][i], p["lens"][i]
    rows = c.t["qkv"][s0:s0 + L].to(dt)
    return rows[0, :dim].reshape(H, D), rows[:, dim:2 * dim].reshape(L, H, D), rows[:, 2 * dim:].reshape(L, H, D), L


def _chunk_max(sc):
    """The running max after every 64-key chunk, per key: [H, L]."""
    H, L = sc.shape
    NC = (L + 63) // 64
    pad = torch.full((H, NC * 64 - L), -math.inf, dtype=sc.dtype)
    cm = torch.cat([sc, pad], -1).view(H, NC, 64).amax(-1).cummax(-1).values
    return cm.repeat_interleave(64, dim=-1)[:, :L]


def _attn_emulate(c, q, k, v, L):
    """cls_attn_kernel in fp32: chunks of 64 keys, the running max, P rounded to T against the chunk's max, the chunk factors."""
    p = c.p
    H, D = p["heads"], p["D"]
    sc = torch.einsum("hd,lhd->hl", q, k)
    m = torch.full((H, 1), -math.inf, dtype=F32)
    l = torch.zeros(H, 1, dtype=F32)
    parts, maxes = [], []
    for c0 in range(0, L, 64):
        s = sc[:, c0:c0 + 64]
        mn = torch.maximum(m, s.amax(-1, keepdim=True))
        alpha = torch.exp((m - mn) * p["scale"])
        e = torch.exp((s - mn) * p["scale"])
        l = l * alpha + e.sum(-1, keepdim=True)
        parts.append(torch.einsum("hl,lhd->hd", e.to(c.dtype).to(F32), v[c0:c0 + 64]))
        maxes.append(mn)
        m = mn
    out = torch.zeros(H, D, dtype=F32)
    for part, mc in zip(parts, maxes):
        out = out + part * (torch.exp((mc - m) * p["scale"]) / l)
    return out


def f_attn(c, dt, mutant=None):
    p = c.p
    H, D, dim, scale = p["heads"], p["D"], p["dim"], p["scale"]
    rk, _ = _rk(c, dt)
    outs, tols = [], []
    want_aux = dt == F64 and mutant is None
    for i in range(len(p["lens"])):
        q, k, v, L = _text_views(c, dt, i)
        if dt == F32:
            outs.append(_attn_emulate(c, q, k, v, L).reshape(dim))
            continue
        sc = torch.einsum("hd,lhd->hl", q, k) * scale
        if mutant == "tail_dropped":
            sc = sc.clone()
            sc[:, L - 1] = -math.inf
        m = sc.amax(-1, keepdim=True)
        e = torch.exp(sc - m)
        l = e.sum(-1, keepdim=True)
        if mutant == "chunk_factor_lost":
            e = torch.exp(sc - _chunk_max(sc))                    # every chunk's P against its own running max, never rescaled
        pr = e / l
        if mutant == "head_o_div_64":                            # the head of output column o taken as o / 64
            hh = (torch.arange(dim) // 64).clamp(max=H - 1)
            o = torch.einsum("ol,lo->o", pr[hh], v.reshape(L, dim))
        else:
            o = torch.einsum("hl,lhd->hd", pr, v).reshape(dim)
        outs.append(o)
        if want_aux:
            NC = (L + 63) // 64
            qk = torch.einsum("hd,lhd->hl", q.abs(), k.abs()) * scale
            A = torch.einsum("hl,lhd->hd", pr, v.abs())
            e_s = ((D + 4) * E * qk + 2 * E * sc.abs()).amax(-1, keepdim=True)
            dmax = (sc - m).abs().amax(-1, keepdim=True)
            assert float(dmax.max()) <= 40.0, "inputs must keep |s - m| <= 40"
            e_exp = (dmax + 4 * (NC + 1)) * 2.0 ** -23
            sub = torch.zeros_like(A)
            if c.dtype == torch.float16:
                sub = torch.einsum("hl,lhd->hd", (e < 2.0 ** -14).to(F64) * 2.0 ** -25, v.abs()) / l
            tols.append((U[c.dtype] * o.abs().view(H, D) + (2 * e_s + 2 * e_exp + (L + NC + 4) * E + RP[c.dtype]) * A + sub).reshape(dim))
    return {"out": rk(torch.stack(outs))}, (torch.stack(tols) if want_aux else None)


# ------------------------------------------------------------------------------------------------------------- cls_head
def first_argmax(lg):
    """The first of equal maxima; a NaN never wins (an all-NaN row: 0) -- the kernel's rule, written with a strict comparison as there."""
    n, Lb = lg.shape
    best = torch.full((n,), -math.inf, dtype=lg.dtype)
    arg = torch.zeros(n, dtype=torch.int64)
    for j in range(Lb):
        better = lg[:, j] > best
        best = torch.where(better, lg[:, j], best)
        arg = torch.where(better, torch.full_like(arg, j), arg)
    return arg


def f_head(c, dt, mutant=None):
    rk, _ = _rk(c, dt)
    x, w, b = (c.t[k].to(dt) for k in ("pre", "w", "b"))
    lg = (x[:, None, :] * w[None]).sum(-1) + b                    # every label's sum in one order: identical rows tie exactly
    aux = None
    if dt == F64 and mutant is None:
        K = x.shape[1]
        xa = torch.where(torch.isnan(x), torch.zeros_like(x), x).abs()
        aux = U[c.dtype] * lg.abs() + 2 * (K + 4) * E * (xa @ w.abs().T) + E * b.abs()
    if dt == F32:
        lg = rk(lg)
    elif mutant != "logits_unrounded" and mutant is not None:
        lg = lg.to(F32).to(c.dtype).to(F64)                       # a mutant rounds its logits as the kernel does
    labels = first_argmax(lg)
    if mutant == "last_of_equal_maxima":
        Lb = lg.shape[1]
        labels = Lb - 1 - first_argmax(lg.flip(-1))
    return {"logits": lg, "labels": labels.to(torch.int32)}, aux


# ------------------------------------------------------------------------------------------------------------- gemm
def _round64(x, dtype):
    """float64 -> T -> float64 in ONE correctly rounded step where it matters: numpy converts to fp16 directly (torch goes through fp32)."""
    if dtype == torch.float16:
        with np.errstate(over="ignore"):
            return torch.from_numpy(x.numpy().astype(np.float16).astype(np.float64))
    return x.to(F32).to(dtype).to(F64)


def _step(x, dtype):
    """The spacing of T at |x| (float64)."""
    a = x.abs().clamp_min(2.0 ** MIN_EXP[dtype])
    return torch.pow(2.0, torch.floor(torch.log2(a)) - MANT[dtype])


def _gelu(x, erfc_form):
    if erfc_form:
        return 0.5 * x * torch.special.erfc(-x * math.sqrt(0.5))       # no cancellation in the negative tail
    return 0.5 * x * (1.0 + torch.erf(x * math.sqrt(0.5)))


def f_gemm(c, dt, mutant=None):
    p = c.p
    _, rr = _rk(c, dt)
    x, w, b = (c.t[k].to(dt) for k in ("x", "w", "b"))
    if mutant == "row_stride_ignored" and p["ldx"] != p["K"]:
        x = x.clone()
        x[1:] = 0.0                                              # rows read K apart land in the gap between the real rows (zeros here)
    pre = x @ w.T + b                                            # exact in fp32 and in float64: the grid
    epi = p["epi"]
    tol = None
    if epi == EPI_BIAS:
        out = rr(pre)
    elif epi == EPI_RELU:
        out = rr(pre.clamp(min=0.0))
    elif epi == EPI_RESIDUAL:
        r = c.t["r"].to(dt)
        out = rr(pre + r) if mutant == "residual_before_rounding" else rr(rr(pre) + r)
    else:
        xin = rr(pre) if c.dtype == torch.float16 else pre
        if dt == F64:
            g = _gelu(xin, True)
            out = _round64(g, c.dtype)
            d = {torch.float16: 0.0 * g, torch.bfloat16: 0.5 * xin.abs() * 1.5e-7 + 2.0 ** -21 * g.abs(),
                 torch.float32: 2.0 ** -23 * xin.abs() + 2.0 ** -22 * g.abs()}[c.dtype]
            tol = _step(out, c.dtype) + d
        else:
            out = rr(_gelu(xin, c.dtype != torch.float32))
    return {"out": out}, tol


FAMILIES = {"embed_ln": f_embed, "ln": f_ln, "gather": f_gather, "cls_attn": f_attn, "cls_head": f_head, "gemm": f_gemm}
MUTANTS = {"embed_ln": ("id_wrapped", "sum_unrounded", "mean_c_minus_4", "eps_outside_sqrt"), "ln": ("mean_c_minus_4", "eps_outside_sqrt"),
           "gather": ("index_ignored", "rows_sorted"), "cls_attn": ("tail_dropped", "chunk_factor_lost", "head_o_div_64"),
           "cls_head": ("last_of_equal_maxima", "logits_unrounded"), "gemm": ("residual_before_rounding", "row_stride_ignored")}


def evaluate(c: Case, dt=F64, mutant=None):
    return FAMILIES[c.family](c, dt, mutant)[0]


def reference(c: Case):
    """(outputs, tolerances) in float64, computed once per case and never modified. A tolerance of None = bit for bit."""
    if c._ref is None:
        outs, aux = FAMILIES[c.family](c, F64, None)
        f = c.family
        if f in ("ln", "embed_ln"):
            tol = {"y": _ln_tol(c, outs["y"], aux["x"], aux["d"], aux["rstd"], aux["w"], aux["b"])}
        elif f == "gather":
            tol = {"out": None}
        elif f == "cls_attn":
            tol = {"out": aux}
        elif f == "cls_head":
            tol = {"logits": aux}
        else:
            tol = {"out": aux}
        c._ref = (outs, tol)
    return c._ref


def _cmp(what, got, ref, tol):
    got = got.to(F64)
    finite = bool(torch.isfinite(got).all())
    if tol is None:
        bad = int((got != ref).sum())
        return (what, float("inf") if bad else 0.0, bad, finite)
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol.clamp(min=1e-300))
    return (what, float(ratio.max()), int((err > tol).sum()), finite)


def _count(what, bad):
    bad = int(bad)
    return (what, float("inf") if bad else 0.0, bad, True)


def check(c: Case, outs: Dict[str, torch.Tensor]):
    """[(output, worst error / bound, elements over the bound, all finite)] of a candidate's outputs (storage-dtype or float tensors on
    the CPU, shaped like the reference's). Exact properties (labels, representable logits, clamped ids) report their misses as elements
    over the bound."""
    ref, tol = reference(c)
    if c.family == "cls_head":
        lg = outs["logits"].to(F64).reshape(ref["logits"].shape)
        nan_rows = torch.isnan(c.t["pre"].to(F64)).any(-1)
        rep = [_count("nan_rows", (~torch.isnan(lg[nan_rows])).sum())]
        ok = ~nan_rows
        rep.append(_cmp("logits", lg[ok], ref["logits"][ok], tol["logits"][ok]))
        rep.append(_count("logits_in_T", (lg[ok] != lg[ok].to(F32).to(c.dtype).to(F64)).sum()))
        lab = outs["labels"].long().reshape(-1)
        miss = lab != first_argmax(lg)
        srt = torch.sort(ref["logits"][ok], -1, descending=True).values
        margin = srt[:, 0] - srt[:, 1] if srt.shape[1] > 1 else torch.full((int(ok.sum()),), math.inf, dtype=F64)
        clear = margin > 2 * tol["logits"][ok].amax(-1)
        miss[ok.nonzero().flatten()[clear]] |= (lab[ok] != ref["labels"].long()[ok])[clear]
        rep.append(_count("labels", miss.sum()))
        return rep
    rep = [_cmp(k, outs[k].reshape(ref[k].shape), ref[k], tol[k]) for k in ref]
    if c.family == "embed_ln":
        y = outs["y"].to(F64).reshape(ref["y"].shape)
        rep.append(_count("clamped_ids", sum(int((y[a] != y[b]).sum()) for a, b in c.p["same_rows"])))
    return rep


def emulate(c: Case):
    """The reference alone: fp32 arithmetic, rounded where the kernel rounds."""
    return {k: v.to(c.dtype) if v.is_floating_point() else v for k, v in evaluate(c, F32).items()}


# ------------------------------------------------------------------------------------------------------------- the cases
LN_C = (64, 256, 320, 768)            # a quarter of the wave's lanes, one pass of 256 channels, a ragged second pass, the model's width
LN_ROWS = (1, 4, 5, 130)              # four rows per workgroup: one, a full one, one row into the second, 33 workgroups with two dead rows
VOCAB, MAX_POS = 64, 520


def _ln_wb(g, C, dtype):
    return (1 + 0.2 * _rand(g, C)).to(dtype), (0.3 * _rand(g, C)).to(dtype)


def ln_cases() -> List[Case]:
    """C x rows as above at the model's eps 1e-12; `bigmean`: a row 4 + 0.1 n, its mean 40 times its spread (the mean|x| term of the bound);
    `eps`: eps = 0.25 beside variances around 1, where eps inside and outside the square root differ by a tenth."""
    out = []
    for dtype in DTYPES:
        for C in LN_C:
            for rows in LN_ROWS:
                g = _gen(1000 + C + rows)
                x = _rand(g, rows, C) * (0.5 + _rand(g, rows, 1).abs()) + 0.5 * _rand(g, rows, 1)
                w, b = _ln_wb(g, C, dtype)
                out.append(Case("ln", f"ln-C{C}-r{rows}", dtype, dict(rows=rows, C=C, eps=1e-12), dict(x=x.to(dtype), w=w, b=b),
                                ("mean_c_minus_4",), "layernorm_kernel"))
        g = _gen(1)
        x = _rand(g, 5, 256)
        x[0] = 4.0 + 0.1 * x[0]
        w, b = _ln_wb(g, 256, dtype)
        out.append(Case("ln", "ln-bigmean", dtype, dict(rows=5, C=256, eps=1e-12), dict(x=x.to(dtype), w=w, b=b), ("mean_c_minus_4",),
                        "layernorm_kernel"))
        g = _gen(2)
        w, b = _ln_wb(g, 64, dtype)
        out.append(Case("ln", "ln-eps", dtype, dict(rows=4, C=64, eps=0.25), dict(x=_rand(g, 4, 64).to(dtype), w=w, b=b),
                        ("mean_c_minus_4", "eps_outside_sqrt"), "layernorm_kernel"))
    return out


def _embed_ids(g, rows):
    """ids -5, 0 (one position) and vocab - 1, vocab + 3 (the table's last position) first, then a repeated id at a repeated position, then
    random ones (130 rows over 64 ids: repeats); rows (0, 1) and (2, 3) clamp to the same table rows."""
    ids = [-5, 0, VOCAB - 1, VOCAB + 3, VOCAB - 1] + torch.randint(0, VOCAB, (rows,), generator=g).tolist()
    tp = [7, 7, MAX_POS - 1, MAX_POS - 1, 7] + torch.randint(0, MAX_POS, (rows,), generator=g).tolist()
    same = [(a, b) for a, b in ((0, 1), (2, 3)) if b < rows]
    return torch.tensor(ids[:rows], dtype=torch.int32), torch.tensor(tp[:rows], dtype=torch.int32), same


def embed_cases() -> List[Case]:
    """The LayerNorm matrix over word [64][C] + pos [520][C] tables. `bigmean`: word rows around 3, position rows around 1, spread 0.1: the
    sum sits near 4, where a 16-bit step is a fifth (bf16) or a fortieth (fp16) of the spread -- an unrounded sum leaves the bound."""
    out = []
    for dtype in DTYPES:
        for C in LN_C:
            for rows in LN_ROWS:
                g = _gen(2000 + C + rows)
                ids, tp, same = _embed_ids(g, rows)
                w, b = _ln_wb(g, C, dtype)
                t = dict(ids=ids, tok_pos=tp, word=_rand(g, VOCAB, C).to(dtype), pos=(0.5 * _rand(g, MAX_POS, C)).to(dtype), w=w, b=b)
                out.append(Case("embed_ln", f"embed-C{C}-r{rows}", dtype, dict(rows=rows, C=C, vocab=VOCAB, eps=1e-12, same_rows=same), t,
                                ("id_wrapped", "mean_c_minus_4"), "embed_ln_kernel"))
        g = _gen(3)
        ids, tp, same = _embed_ids(g, 5)
        w, b = _ln_wb(g, 256, dtype)
        t = dict(ids=ids, tok_pos=tp, word=(3.0 + 0.1 * _rand(g, VOCAB, 256)).to(dtype), pos=(1.0 + 0.1 * _rand(g, MAX_POS, 256)).to(dtype), w=w, b=b)
        out.append(Case("embed_ln", "embed-bigmean", dtype, dict(rows=5, C=256, vocab=VOCAB, eps=1e-12, same_rows=same), t,
                        ("id_wrapped", "mean_c_minus_4") + (("sum_unrounded",) if dtype != torch.float32 else ()), "embed_ln_kernel"))
        g = _gen(4)
        ids, tp, same = _embed_ids(g, 4)
        w, b = _ln_wb(g, 64, dtype)
        t = dict(ids=ids, tok_pos=tp, word=_rand(g, VOCAB, 64).to(dtype), pos=(0.5 * _rand(g, MAX_POS, 64)).to(dtype), w=w, b=b)
        out.append(Case("embed_ln", "embed-eps", dtype, dict(rows=4, C=64, vocab=VOCAB, eps=0.25, same_rows=same), t,
                        ("id_wrapped", "eps_outside_sqrt"), "embed_ln_kernel"))
    return out


def gather_cases() -> List[Case]:
    out = []
    for dtype in DTYPES:
        for C in (64, 768):
            for n, idx in ((1, [3]), (7, [5, 2, 9, 2, 0, 11, 5])):
                g = _gen(3000 + C + n)
                out.append(Case("gather", f"gather-C{C}-n{n}", dtype, dict(n=n, C=C, src_rows=12),
                                dict(x=_rand(g, 12, C).to(dtype), idx=torch.tensor(idx, dtype=torch.int32)),
                                ("index_ignored",) + (("rows_sorted",) if n > 1 else ()), "gather_rows_kernel"))
    return out


ATTN_CFG = ((1, 32), (3, 80), (12, 64), (2, 128))          # (heads, D): one head; heads % 4 != 0 and D no power of two; the model; two wide heads
ATTN_LENS = (1, 2, 63, 64, 65, 128, 129, 512)
ATTN_KINDS = ("asc", "desc", "spike24", "spike11")          # 512 keys each
SPIKE_KEY = 100
ATTN_MAX_LEN = 512


def attn_cases() -> List[Case]:
    """Per (heads, D) one launch over twelve texts, 3 to 9 unused rows between them so that no start is a multiple of 64:
      random texts of every length in ATTN_LENS (a lone key, the chunk edges, eight chunks), the last key's value four times the others';
      asc / desc: scores rising (falling) from -12 to 12 over 512 keys: every chunk raises the running max (chunk 0 sets it for good);
      spike24 / spike11: the spike rows of test_attn_fp16_segments_vs_fp32: key 100 above every other by 24 (all other P round to zero in
      fp16) and by 11 (the 511 other P are fp16 subnormals holding 1.4e-2 of the weight; their V is positive, the spike's -1)."""
    out = []
    for dtype in DTYPES16:
        for H, D in ATTN_CFG:
            dim = H * D
            g = _gen(4000 + H * 1000 + D)
            scale = D ** -0.5
            texts = [(L, "rand") for L in ATTN_LENS] + [(512, k) for k in ATTN_KINDS]
            starts, lens, row = [], [], 5
            for i, (L, _) in enumerate(texts):
                while row % 64 == 0:
                    row += 1
                starts.append(row)
                lens.append(L)
                row += L + 3 + i % 7
            qkv = _rand(g, row, 3 * dim)
            for (L, kind), s0 in zip(texts, starts):
                blk = qkv[s0:s0 + L]
                if kind == "rand":
                    blk[L - 1, 2 * dim:] *= 4.0
                elif kind in ("asc", "desc"):
                    qs = blk[0, :dim].to(dtype).to(F64).view(H, D)                 # the query as the device holds it
                    a = torch.linspace(-12.0, 12.0, L, dtype=F64)
                    a = a if kind == "asc" else a.flip(0)
                    unit = qs / (qs * qs).sum(-1, keepdim=True) / scale            # scale q . unit = 1
                    blk[:, dim:2 * dim] = (a[:, None, None] * unit[None] + 0.05 * _rand(g, L, H, D)).view(L, dim)
                    blk[L - 1, 2 * dim:] *= 4.0
                else:
                    gap = 24.0 if kind == "spike24" else 11.0
                    blk[:, :dim] = 1.0 + 0.01 * _rand(g, L, dim)
                    blk[:, dim:2 * dim] = 0.02 * _rand(g, L, dim)
                    blk[SPIKE_KEY, dim:2 * dim] = gap / math.sqrt(D)
                    blk[:, 2 * dim:] = 1.0 + _rand(g, L, dim).abs()
                    blk[SPIKE_KEY, 2 * dim:] = -1.0
            assert all(s % 64 for s in starts)
            kills = ("tail_dropped", "chunk_factor_lost") + (("head_o_div_64",) if D == 80 else ())
            out.append(Case("cls_attn", f"attn-h{H}-D{D}", dtype,
                            dict(heads=H, D=D, dim=dim, scale=scale, starts=starts, lens=lens, max_len=ATTN_MAX_LEN, kinds=[k for _, k in texts]),
                            dict(qkv=qkv.to(dtype)), kills, f"cls_attn_kernel<{DT_NAME[dtype]}, {D}>"))
    return out


def head_cases() -> List[Case]:
    """dim x num_labels x n; `tie`: weight rows 1 and 3 and their biases identical and the largest (bias 8): the label is 1; `nan`: row 4 of 9
    holds one NaN."""
    out = []
    for dtype in DTYPES:
        for dim in (64, 768):
            for Lb in (1, 2, 5):
                for n in (1, 9):
                    g = _gen(5000 + dim + 10 * Lb + n)
                    t = dict(pre=_rand(g, n, dim).clamp(min=0.0).to(dtype), w=(_rand(g, Lb, dim) / dim ** 0.5).to(dtype), b=(0.5 * _rand(g, Lb)).to(dtype))
                    out.append(Case("cls_head", f"head-d{dim}-L{Lb}-n{n}", dtype, dict(n=n, dim=dim, num_labels=Lb), t, ("logits_unrounded",), "cls_head_kernel"))
        g = _gen(6)
        w, b = _rand(g, 5, 64) / 8.0, 0.5 * _rand(g, 5)
        w[3], b[1], b[3] = w[1], 8.0, 8.0
        t = dict(pre=_rand(g, 9, 64).clamp(min=0.0).to(dtype), w=w.to(dtype), b=b.to(dtype))
        out.append(Case("cls_head", "head-tie", dtype, dict(n=9, dim=64, num_labels=5), t, ("last_of_equal_maxima", "logits_unrounded"), "cls_head_kernel"))
        g = _gen(7)
        pre = _rand(g, 9, 768).clamp(min=0.0)
        pre[4, 17] = math.nan
        t = dict(pre=pre.to(dtype), w=(_rand(g, 5, 768) / 768 ** 0.5).to(dtype), b=(0.5 * _rand(g, 5)).to(dtype))
        out.append(Case("cls_head", "head-nan", dtype, dict(n=9, dim=768, num_labels=5), t, ("logits_unrounded",), "cls_head_kernel"))
    return out


_GRID = {}


def _grid(key, shape, lim, den, dtype):
    """Shared among the cases (never modified): integers in [-lim, lim] over den."""
    k = (key, tuple(shape), dtype)
    if k not in _GRID:
        g = _gen(zlib.crc32(repr((key, tuple(shape))).encode()))
        _GRID[k] = (torch.randint(-lim, lim + 1, shape, generator=g).to(F64) / den).to(dtype)
    return _GRID[k]


GEMM_M = (1, 63, 65)
GEMM_NK = ((64, 64), (768, 768), (768, 3072))
GEMM_EPIS = (EPI_BIAS, EPI_RESIDUAL, EPI_GELU, EPI_RELU)


def gemm_cases() -> List[Case]:
    """The pinned 64 x 64 tile: M in {1, 63, 65} (one row, a ragged tile, a second row tile) x (N, K) (one tile; out_lin and
    pre_classifier; lin2) x ldx in {K, 64 K} (the [CLS] rows of a text's 64-row attention block) x the four epilogues; launch_gemm's
    own choice at M = 300, once per epilogue."""
    out = []
    for dtype in DTYPES:
        combos = [(M, N, K, mul, epi, 1) for M in GEMM_M for N, K in GEMM_NK for mul in (1, 64) for epi in GEMM_EPIS]
        combos += [(300, 768, 768, 1, epi, 0) for epi in GEMM_EPIS]
        for M, N, K, mul, epi, pinned in combos:
            t = dict(x=_grid("x", (M, K), 32, 16, dtype), w=_grid("w", (N, K), 16, 64, dtype), b=_grid("b", (N,), 64, 64, dtype),
                     r=_grid("r", (M, N), 32, 16, dtype) if epi == EPI_RESIDUAL else None)
            kills = (("residual_before_rounding",) if epi == EPI_RESIDUAL and dtype != torch.float32 else ()) + \
                    (("row_stride_ignored",) if mul != 1 and M > 1 else ())
            out.append(Case("gemm", f"gemm-{'pin' if pinned else 'auto'}-M{M}-N{N}-K{K}-ldx{mul}K-{EPI_NAME[epi]}", dtype,
                            dict(M=M, N=N, K=K, ldx=mul * K, epi=epi, pinned=pinned), t, kills,
                            "gemm_nt_kernel 64x64" if pinned else "launch_gemm"))
    return out


_CASES = None


def all_cases() -> List[Case]:
    """Built once per process and shared: the cases and their inputs are never modified."""
    global _CASES
    if _CASES is None:
        _CASES = ln_cases() + embed_cases() + gather_cases() + attn_cases() + head_cases() + gemm_cases()
    return _CASES
