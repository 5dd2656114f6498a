"""Test infrastructure: the layout / table-recognition engine's kernels one at a time (surya_op_lay_*, surya_op_gemm's GEGLU code) --
the cases, float64 references of every op in plain torch, and the per-element error bound each family is held to.

A Case holds the inputs exactly as the device gets them (already rounded to the storage type) and the parameters of ONE call.
evaluate(case, dt, mutant) computes the op:
  dt = float64              the reference. It rounds to storage only where the bound below says so;
  dt = float32              "the reference alone": fp32 arithmetic that rounds where the kernel rounds, outputs rounded to storage;
  mutant = a name           a deliberately wrong evaluation (float64): what the bound has to catch (MUTANTS).
check(case, outs) holds EVERY element of every output to the bound and wants every buffer finite. Nothing in a bound is measured.

Symbols: u = one unit in the last place relative to the value (fp32 2^-23, bf16 2^-7): half of it the rounding to storage, the other half
a rounding that flips because the fp32 value differs in its last bits. E = 2^-24, the unit roundoff of fp32.

Softmax attention (window, cross, prompt): N keys, head dim D, scores s (scale, bias and mask included), p = softmax(s), A = sum_j p_j |v_j|
    tol = u |ref| + (2 e_s + 2 e_exp + (N + 4) E + r_P) A
    e_s   = max over the query's live keys of (D + 4) E scale sum_c |q_c| |k_jc| + 2 E (|s_j| + |bias_j|)
            (a D-term fp32 dot product, the scale, the two additions). A live key is one the mask leaves (p_j > 1e-30).
    e_exp = (max_j |s_j - m| + 4) 2^-23: the kernels compute exp(x) as a hardware exp2 of x log2(e). The product is rounded to fp32, an
            ABSOLUTE error of |x| 2^-24 in the exponent = a relative error |x| 2^-24 ln 2 of the result; exp2 itself is good to one ulp
            (2^-23); the subtraction s - m adds 2^-24 (|s| + |m|) before that. (max |s - m| + 4) 2^-23 covers the three for |s - m| <= 40,
            which the inputs keep for every live key. An error of d in every p_j moves the normalised output by at most 2 d A: the
            factors 2 of e_s and e_exp.
    (N + 4) E: the fp32 sums over keys of the numerator and of the denominator, the reciprocal, the final product.
    r_P = 2^-8 where the kernel rounds P to bf16 before P V (both MFMA kernels, and the prompt kernel in bf16), else 0.
    The prompt kernel also rounds the rotated q, the rotated k and q scale to storage: the reference does the same roundings, and
    u scale sum |q| |k| is added to e_s for their flips. Its cache rows: k = u |ref| + 4 E (|x1 cos| + |x2 sin|), v bit for bit.
    Where the q row is a sum of split-K slabs the slabs sit on a dyadic grid (multiples of 2^-5, |sum| <= 4): the sum is exact in fp32 and
    representable in bf16, so the rounding to storage is the identity and cannot flip.
LayerNorm, merge_ln (C channels, two reductions):
    tol = u |ref| + (C + 8) E (|x - mean| + mean|x|) rstd |w| + (C + 8) E |b|
    The variance sum has relative error (C + 2) E, so rstd (C / 2 + 4) E with the rsqrt; centring, two products and the add are 4 E more:
    c = 1 on the (C + 8) E |x - mean| rstd |w| form. The first reduction enters differently: the mean is off by up to (C + 1) E mean|x|, an
    ABSOLUTE shift of x - mean that does not shrink where x is close to the mean -- the mean|x| term. (Its effect on the variance is
    second order: sum (x - mean) = 0.)
ADETR RMSNorm, the norm half of reduce-norm (one reduction, variance CLAMPED at eps, not added):
    tol = u |ref| + (C + 8) E |x| rstd |1 + w|
Sum half of reduce-norm: x_out = T(res + T(bias + sum_s part_s)). Slabs, bias and res on the dyadic grid: every fp32 sum is exact, so x_out
    equals the same two roundings done in float64 bit for bit. Otherwise tol = u |ref| + (S + 2) E sum |terms|.
Row movers, both embeddings: exact. Every `+` is one correctly rounded operation of the storage type; the reference is torch arithmetic
    in that dtype on the CPU in the kernel's order of additions (oracle/layout_oracle.py for the embeddings). Bit for bit.
Heads: the reference rounds to storage where the kernel (and the reference module) materialises a tensor: h1 = T(rmsnorm(x)), h2 =
    T(layernorm(h1)), logits = T(h2 W^T), z = T(h2 Wb^T + b), box = T(sigmoid(z)). Errors are pushed through per element:
    e_h1 = rms bound + u |h1| (flip); e_h2 = the LayerNorm's derivative applied to e_h1, rstd |w| (e + mean e + |yhat| mean(|yhat| e)),
    + the LayerNorm bound + u |h2|; logits: u |ref| + 2 (K + 4) E |h2| |W|^T + e_h2 |W|^T (the linear-op bound of det_microplan.py);
    box: u |ref| + tol_z / 4 + 2^-20 (sigma' <= 1/4; exp, add, reciprocal).
GEGLU (surya_op_gemm code 8): gate and up are K-term dot products, e_lin = 2 (K + 4) E A with A = |x| |W|^T; the epilogue rounds gate, up and
    gelu_tanh(gate) to storage (u |.| each for the flips); |gelu_tanh'| <= 1.13, and tanhf with the 1 + tanh cancellation costs 8 E |g| + 4 E |gate|:
    e_g = 1.13 (e_lin + u |gate|) + 8 E |g| + 4 E |gate| + u |g|, e_up = e_lin + u |up|, tol = u |ref| + e_g |up| + |g| e_up + e_g e_up.
Not a conftest; never imported by the product."""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

from oracle import layout_oracle as LO

E = 2.0 ** -24
U = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -7}
DTYPES = (torch.float32, torch.bfloat16)
F64 = torch.float64
EMBED_NAMES = ["w", "h", "cx", "cy", "xskew", "yskew", "x1", "y1", "x2", "y2", "x3", "y3", "x4", "y4", "label", "category", "merge", "colspan"]


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
        return f"{self.name}-{'fp32' if self.dtype == torch.float32 else 'bf16'}"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, dtype=F64) * scale


def _st(x, dtype):
    return x.to(dtype)


def _dyadic(g, *shape, lim=128, step=2.0 ** -5):
    """Multiples of `step` in [-lim, lim] * step as float64."""
    return torch.randint(-lim, lim + 1, shape, generator=g).to(F64) * step


# ------------------------------------------------------------------------------------------------------------- window tables
def oracle_window_tables(h, w, ws, shift):
    """The window-order row of every token, the padding rows and the padded grid, from the reference's own steps on an index tensor:
    F.pad to whole windows, torch.roll(-shift), window_partition (oracle/layout_oracle.py:swin_layer). No shift when min(h, w) <= ws."""
    if min(h, w) <= ws:
        shift = 0
    idx = torch.arange(h * w, dtype=torch.int64).view(1, h, w, 1)
    pr, pb = (ws - w % ws) % ws, (ws - h % ws) % ws
    x = F.pad(idx, (0, 0, 0, pr, 0, pb), value=-1)
    if shift > 0:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
    flat = LO.window_partition(x, ws).reshape(-1)
    perm = torch.empty(h * w, dtype=torch.int64)
    tok = flat >= 0
    perm[flat[tok]] = torch.nonzero(tok).flatten()
    pads = torch.nonzero(~tok).flatten()
    return perm.to(torch.int32), pads.to(torch.int32), (h + pb, w + pr), shift


# ------------------------------------------------------------------------------------------------------------- families
def _rk(c, dt):
    """Rounding the KERNEL makes (only the fp32 emulation repeats it) and rounding the REFERENCE makes too."""
    rr = lambda x: x.to(c.dtype).to(dt)
    return (rr if dt == torch.float32 else (lambda x: x)), rr


def _region_mask(nwx, nwy, images, shift, dt, mutant):
    ws = 8
    m = torch.zeros(images * nwx * nwy, 64, 64, dtype=dt)
    if shift <= 0:
        return m
    n = torch.arange(64)
    for wi in range(images * nwx * nwy):
        wimg = wi % (nwx * nwy)
        if mutant == "mask_image0_only" and wi >= nwx * nwy:
            continue                                             # the window index not taken modulo nwx * nwy: no later window is "last"
        ly = (wimg // nwx) == nwy - 1
        lx = (wimg % nwx) == nwx - 1 and mutant != "mask_lastcol_missing"
        r = (2 * (ly & (n // ws >= ws - shift))) + (1 * (lx & (n % ws >= ws - shift)))
        m[wi] = (r[:, None] != r[None, :]).to(dt) * -100.0
    return m


def _softmax_pv(s, v, c, dt, round_p):
    """softmax(s) v. round_p (the fp32 emulation of a kernel that rounds P to bf16): the un-normalised exp is rounded, the sum is not."""
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    if round_p:
        return (e.to(c.dtype).to(dt) @ v) / l, e / l
    p = e / l
    return p @ v, p


def f_window(c, dt, mutant=None):
    p = c.p
    nh, nkv, nW = p["nh"], p["nkv"], p["images"] * p["nwx"] * p["nwy"]
    rk, _ = _rk(c, dt)
    qkv = c.t["qkv"].to(dt).view(nW, 64, nh + 2 * nkv, 32).permute(0, 2, 1, 3)
    q, k, v = qkv[:, :nh], qkv[:, nh:nh + nkv], qkv[:, nh + nkv:]
    idx = torch.arange(nh) // (nh // nkv) if mutant == "kv_head_div" else torch.arange(nh) % nkv
    bias = c.t["bias"].to(dt)
    if mutant == "bias_transposed":
        bias = bias.transpose(-1, -2)
    if mutant is None and dt == F64:                             # the reference's own mask builder
        m1 = LO.shift_mask(p["nwy"] * 8, p["nwx"] * 8, 8, p["shift"], dt)
        mask = torch.zeros(nW, 64, 64, dtype=dt) if m1 is None else m1.repeat(p["images"], 1, 1)
    else:
        mask = _region_mask(p["nwx"], p["nwy"], p["images"], p["shift"], dt, mutant)
    scale = 32 ** -0.5
    kk, vv = k[:, idx], v[:, idx]
    s = (q @ kk.transpose(-1, -2)) * scale + bias[None] + mask[:, None]
    o, pr = _softmax_pv(s, vv, c, dt, dt == torch.float32 and c.dtype == torch.bfloat16)
    out = rk(o.permute(0, 2, 1, 3).reshape(nW * 64, nh * 32))
    aux = None
    if dt == F64 and mutant is None:
        aux = dict(s=s, bias=bias[None].abs().expand_as(s), qk=(q.abs() @ kk.abs().transpose(-1, -2)) * scale, p=pr, A=pr @ vv.abs(),
                   live=pr > 1e-30, N=64, D=32, rp=2.0 ** -8 if c.dtype == torch.bfloat16 else 0.0,
                   back=lambda x: x.permute(0, 2, 1, 3).reshape(nW * 64, nh * 32))
    return {"out": out}, aux


def f_cross(c, dt, mutant=None):
    p = c.p
    M, nq, nkv, D, Lk, S, NI = p["M"], p["nq"], p["nkv"], p["D"], p["Lk"], p["S"], p["images"]
    G = nq // nkv
    rk, rr = _rk(c, dt)
    q = c.t["q"].to(dt) if S == 0 else rr(c.t["qpart"].to(dt).sum(0))
    q = q.view(M, nq, D)
    kv = c.t["kv"].to(dt).view(NI, Lk, 2, nkv, D)
    im = c.t["item_map"].long()
    if mutant == "item_map_ignored":
        im = torch.arange(M).clamp(max=NI - 1)
    hmap = torch.arange(nq) % nkv if mutant == "kv_head_mod" else torch.arange(nq) // G
    k = kv[im, :, 0][:, :, hmap].permute(0, 2, 1, 3)            # [M, nq, Lk, D]
    v = kv[im, :, 1][:, :, hmap].permute(0, 2, 1, 3)
    s = (q[:, :, None, :] @ k.transpose(-1, -2)) * p["scale"]   # [M, nq, 1, Lk]
    if mutant == "last_key_dropped":
        s[..., -1] = -math.inf
    if mutant == "range_skipped":
        s[..., p["chunk"]:2 * p["chunk"]] = -math.inf
    o, pr = _softmax_pv(s, v, c, dt, dt == torch.float32 and c.dtype == torch.bfloat16)
    out = rk(o.reshape(M, nq * D))
    aux = None
    if dt == F64 and mutant is None:
        aux = dict(s=s, bias=torch.zeros_like(s), qk=(q.abs()[:, :, None, :] @ k.abs().transpose(-1, -2)) * p["scale"], p=pr, A=pr @ v.abs(),
                   live=torch.ones_like(s, dtype=torch.bool), N=Lk, D=D, rp=2.0 ** -8 if c.dtype == torch.bfloat16 else 0.0,
                   back=lambda x: x.reshape(M, nq * D))
    return {"out": out}, aux


def f_prompt(c, dt, mutant=None):
    p = c.p
    B, Tn, nq, nkv, D = p["B"], p["Tn"], p["nq"], p["nkv"], p["D"]
    G, half = nq // nkv, D // 2
    rk, rr = _rk(c, dt)
    x = c.t["qkv"].to(dt).view(B, Tn, nq + 2 * nkv, D).permute(0, 2, 1, 3)          # [B, heads, Tn, D]
    pos = torch.arange(Tn) + (1 if mutant == "rope_pos_off1" else 0)
    cs = c.t["rope"].to(dt)[pos]                                                       # [Tn, half, 2]
    cos, sin = torch.cat([cs[..., 0]] * 2, -1), torch.cat([cs[..., 1]] * 2, -1)
    rot = lambda t: t * cos + LO.rotate_half(t) * sin
    qx, kx, vx = x[:, :nq], x[:, nq:nq + nkv], x[:, nq + nkv:]
    k_exact = rot(kx)
    kr = rr(k_exact)
    qr = rr(rr(rot(qx)) * p["scale"])
    hmap = torch.arange(nq) // G
    kk, vv = kr[:, hmap], vx[:, hmap]
    s = qr @ kk.transpose(-1, -2)                                                      # [B, nq, Tn, Tn]
    t = torch.arange(Tn)
    live = t[None, :] <= t[:, None]
    if mutant == "causal_off1":
        live = (t[None, :] < t[:, None]) | (t[None, :] == 0)
    s = s.masked_fill(~live, -math.inf)
    o, pr = _softmax_pv(s, vv, c, dt, dt == torch.float32 and c.dtype == torch.bfloat16)
    back = lambda y: y.permute(0, 2, 1, 3).reshape(B * Tn, nq * D)
    outs = {"out": rk(back(o)), "k_rows": rk(k_exact) if dt == torch.float32 else k_exact, "v_rows": vx}
    aux = None
    if dt == F64 and mutant is None:
        qk = qr.abs() @ kk.abs().transpose(-1, -2)
        aux = dict(s=s, bias=torch.zeros_like(s), qk=qk, p=pr, A=pr @ vv.abs(), live=live.expand_as(s), N=Tn, D=D, extra=U[c.dtype] * qk,
                   rp=2.0 ** -8 if c.dtype == torch.bfloat16 else 0.0, back=back,
                   k_mag=kx.abs() * cos.abs() + LO.rotate_half(kx).abs() * sin.abs())
    return outs, aux


def _attn_tol(c, ref, aux):
    u = U[c.dtype]
    live, s = aux["live"], aux["s"]
    sa = torch.where(live, s.abs(), torch.zeros_like(s))
    e_s = (aux["D"] + 4) * E * aux["qk"] + 2 * E * (sa + aux["bias"]) + aux.get("extra", 0.0)
    e_s = torch.where(live, e_s, torch.zeros_like(e_s)).amax(-1, keepdim=True)
    m = s.amax(-1, keepdim=True)
    d = torch.where(live, (s - m).abs(), torch.zeros_like(s))
    assert d.max().item() <= 40.0, "inputs must keep |s - m| <= 40 on the live keys"
    e_exp = (d.amax(-1, keepdim=True) + 4) * 2.0 ** -23
    return u * ref.abs() + aux["back"]((2 * e_s + 2 * e_exp + (aux["N"] + 4) * E + aux["rp"]) * aux["A"])


def _ln(x, w, b, eps, mutant=None):
    mean = x.mean(-1, keepdim=True)
    if mutant == "no_mean":
        mean = torch.zeros_like(mean)
    d = x - mean
    rstd = torch.rsqrt((d * d).mean(-1, keepdim=True) + eps)
    return d * rstd * w + b, d, rstd


def _ln_tol(c, ref, x, d, rstd, w, b, C):
    return U[c.dtype] * ref.abs() + (C + 8) * E * ((d.abs() + x.abs().mean(-1, keepdim=True)) * rstd * w.abs() + b.abs())


def _rms(x, w, eps, dtype, mutant=None):
    var = (x * x).mean(-1, keepdim=True)
    var = var + eps if mutant == "eps_added" else var.clamp(min=eps)
    rstd = torch.rsqrt(var)
    lim = torch.finfo(dtype).max
    y = (x * rstd * (1.0 + w)).clamp(min=-lim, max=lim)
    return torch.where(torch.isnan(y), torch.zeros_like(y), y), rstd


def _rms_tol(c, ref, x, rstd, w, C):
    return U[c.dtype] * ref.abs() + (C + 8) * E * x.abs() * rstd * (1.0 + w).abs()


def f_ln(c, dt, mutant=None):
    rk, _ = _rk(c, dt)
    x, w, b = (c.t[k].to(dt) for k in ("x", "w", "b"))
    y, d, rstd = _ln(x, w, b, c.p["eps"], mutant)
    return {"y": rk(y)}, dict(x=x, d=d, rstd=rstd, w=w, b=b)


def _merge_cat(x, mutant=None):
    parts = [x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]]
    if mutant == "merge_order":
        parts[1], parts[2] = parts[2], parts[1]
    return torch.cat(parts, -1).reshape(-1, 4 * x.shape[-1])


def f_merge(c, dt, mutant=None):
    rk, _ = _rk(c, dt)
    p = c.p
    x, w, b = (c.t[k].to(dt) for k in ("x", "w", "b"))
    cat = _merge_cat(x, mutant)
    if mutant is None and dt == F64:                             # the reference's module; its reduction Linear as the identity
        sd = {"norm.weight": w, "norm.bias": b, "reduction.weight": torch.eye(4 * p["C"], dtype=dt)}
        y = LO.patch_merging(sd, "", x.view(p["B"], p["H"] * p["W"], p["C"]), (p["H"], p["W"])).reshape(-1, 4 * p["C"])
        _, d, rstd = _ln(cat, w, b, 1e-5)
    else:
        y, d, rstd = _ln(cat, w, b, 1e-5)
    return {"y": rk(y)}, dict(x=cat, d=d, rstd=rstd, w=w, b=b)


def f_rms(c, dt, mutant=None):
    rk, _ = _rk(c, dt)
    x, w = c.t["x"].to(dt), c.t["w"].to(dt)
    y, rstd = _rms(x, w, c.p["eps"], c.dtype, mutant)
    return {"y": rk(y)}, dict(x=x, rstd=rstd, w=w)


def f_reduce(c, dt, mutant=None):
    _, rr = _rk(c, dt)
    part = c.t["part"].to(dt)
    if mutant == "slab_dropped":
        part = part[:-1]
    v = torch.zeros_like(part[0])
    for s_ in range(part.shape[0]):                               # the kernel's order
        v = v + part[s_]
    res = c.t["res"].to(dt)
    bias = c.t["bias"].to(dt) if c.t["bias"] is not None else torch.zeros_like(v[0])
    lin = rr(v + bias)
    xo = rr(res + lin)
    outs = {"x_out": xo}
    if c.t["w"] is not None:
        y, _ = _rms(lin if mutant == "residual_after_norm" else xo, c.t["w"].to(dt), c.p["eps"], c.dtype)
        outs["y"] = rr(y + res) if mutant == "residual_after_norm" else (rr(y) if dt == torch.float32 else y)
    terms = part.abs().sum(0) + bias.abs() + res.abs()
    return outs, dict(terms=terms)


def _embed_idx(tok, p, family):
    """The kernels' clamps: every number to [0, vocab - 1], the label / category / merge ids to their tables."""
    t = tok.long().clamp(0, p["vocab"] - 1)
    if family == "layout":
        t[:, 6] = tok[:, 6].long().clamp(0, p["label_count"] - 1)
    else:
        t[:, 6] = t[:, 6].clamp(max=p["category_count"] - 1)
        t[:, 7] = t[:, 7].clamp(max=p["merge_count"] - 1)
    return t


def embed_own(c, mutant=None):
    """The embedding written out once more (storage-dtype torch arithmetic, the kernel's order): carries the w / 2 mutant, and the CPU tier
    checks it against oracle/layout_oracle.py bit for bit."""
    p, fam = c.p, c.p["family"]
    tb = c.t["tables"]
    t = _embed_idx(c.t["tokens"], p, fam)
    cx, cy, w, h, xs, ys = (t[:, i] for i in range(6))
    half = (lambda a: (a + 1) // 2) if mutant == "half_rounded" else (lambda a: a // 2)
    xa = ((xs - p["bbox_size"] // 2) / 2).to(torch.long)
    ya = ((ys - p["bbox_size"] // 2) / 2).to(torch.long)
    cl = lambda a: a.clamp(0, p["bbox_size"])
    Em = lambda nm, idx: tb[nm][idx]
    size_e = Em("w", w) + Em("h", h) + Em("cx", cx) + Em("cy", cy)
    skew_e = Em("xskew", xs) + Em("yskew", ys)
    x1, y1, x3, y3 = cl(cx - half(w) - xa), cl(cy - half(h) - ya), cl(cx + half(w) + xa), cl(cy + half(h) + ya)
    if fam == "layout":
        x2, y2, x4, y4 = cl(cx + half(w) - xa), cl(cy + half(h) + ya), cl(cx - half(w) + xa), cl(cy - half(h) - ya)
        corner = Em("x1", x1) + Em("y1", y1) + Em("x2", x2) + Em("y2", y2) + Em("x3", x3) + Em("y3", y3) + Em("x4", x4) + Em("y4", y4)
        return Em("label", t[:, 6]) + size_e + skew_e + corner
    corner = Em("x1", x1) + Em("y1", y1) + Em("x3", x3) + Em("y3", y3)
    return torch.cat([size_e + skew_e + corner, Em("category", t[:, 6]) + Em("merge", t[:, 7]) + Em("colspan", t[:, 8])], -1)


def f_embed(c, dt, mutant=None):
    if mutant is not None or dt != F64:
        return {"x": embed_own(c, mutant).to(dt)}, None
    p = c.p
    sd = {f"decoder.model.embed_tokens.{nm}_embed.weight": tb for nm, tb in c.t["tables"].items()}
    d = SimpleNamespace(bbox_size=p["bbox_size"], vocab_size=p["vocab"])
    t = _embed_idx(c.t["tokens"], p, p["family"])[:, None, :]
    y = LO.embed_boxes(sd, d, t) if p["family"] == "layout" else LO.embed_table_tokens(sd, d, t)
    return {"x": y[:, 0].to(dt)}, None


def f_rows(c, dt, mutant=None):
    p, k = c.p, c.p["kind"]
    if k == "patchify":
        B, C_, H, W, P, Kp = (p[n] for n in ("B", "C", "H", "W", "P", "Kpad"))
        cols = F.unfold(c.t["src"], P, stride=P).transpose(1, 2).reshape(-1, C_ * P * P)      # K index = (c P + ky) P + kx
        y = F.pad(cols, (0, Kp - C_ * P * P)).to(c.dtype)
    elif k == "add_rows":
        x = c.t["dst"]
        y = x + c.t["src"][torch.arange(x.shape[0]) % p["rpi"]]
    elif k == "zero_rows":
        y = c.t["dst"].clone()
        rows = (torch.arange(p["B"])[:, None] * p["rpi"] + c.t["index"].long()[None]).flatten()
        y[rows] = 0
    else:
        x = c.t["dst"]
        r = torch.arange(x.shape[0])
        y = x + c.t["src"][(r // p["rpi"]) * (p["rpi_src"] or p["rpi"]) + c.t["index"].long()[r % p["rpi"]]]
    return {"dst": y.to(dt)}, None


def _sigmoid(z):
    return 1.0 / (1.0 + torch.exp(-z))


def f_heads(c, dt, mutant=None):
    _, rr = _rk(c, dt)
    p, t = c.p, c.t
    Hd = p["Hd"]
    x = t["x"].to(dt)[:, :Hd]
    g = lambda k: t[k].to(dt)
    h1u, rstd1 = _rms(x, g("fnorm_w"), p["rms_eps"], c.dtype)
    h1 = rr(h1u)
    h2u, d, rstd2 = _ln(h1, g("ln_w"), g("ln_b"), p["ln_eps"], mutant)
    h2 = rr(h2u)
    cls = rr(h2 @ g("lm_w").T)
    z = rr(h2 @ g("bb_w").T + g("bb_b"))
    box = rr(_sigmoid(z))
    aux = None
    if dt == F64 and mutant is None:
        u = U[c.dtype]
        e1 = _rms_tol(c, h1u, x, rstd1, g("fnorm_w"), Hd)
        yhat = d * rstd2
        e2 = rstd2 * g("ln_w").abs() * (e1 + e1.mean(-1, keepdim=True) + yhat.abs() * (yhat.abs() * e1).mean(-1, keepdim=True))
        e2 = e2 + _ln_tol(c, h2u, h1, d, rstd2, g("ln_w"), g("ln_b"), Hd)
        lin = lambda W: 2 * (Hd + 4) * E * (h2.abs() @ W.abs().T) + e2 @ W.abs().T
        tz = u * z.abs() + lin(g("bb_w")) + 2 * (Hd + 4) * E * g("bb_b").abs()
        aux = dict(cls=u * cls.abs() + lin(g("lm_w")), box=u * box.abs() + tz / 4 + 2.0 ** -20)
    return {"cls": cls, "box": box}, aux


def _gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x * x * x)))


def f_geglu(c, dt, mutant=None):
    rk, rr = _rk(c, dt)
    x, W = c.t["x"].to(dt), c.t["w"].to(dt)
    y = x @ W.T
    gate, up = y[:, 0::2], y[:, 1::2]
    if mutant == "gate_up_swapped":
        gate, up = up, gate
    gr, ur = rr(gate), rr(up)
    g = rr(0.5 * gr * (1.0 + torch.erf(gr / math.sqrt(2.0))) if mutant == "gelu_exact" else _gelu_tanh(gr))
    aux = None
    if dt == F64 and mutant is None:
        u, K = U[c.dtype], x.shape[1]
        A = x.abs() @ W.abs().T
        e_lin = 2 * (K + 4) * E * A
        e_g = 1.13 * (e_lin[:, 0::2] + u * gate.abs()) + 8 * E * g.abs() + 4 * E * gr.abs() + u * g.abs()
        e_u = e_lin[:, 1::2] + u * up.abs()
        aux = dict(tol=u * (g * ur).abs() + e_g * ur.abs() + g.abs() * e_u + e_g * e_u)
    return {"out": rk(g * ur)}, aux


FAMILIES = {"window": f_window, "cross": f_cross, "prompt": f_prompt, "ln": f_ln, "merge_ln": f_merge, "rms": f_rms, "reduce": f_reduce,
            "embed": f_embed, "rows": f_rows, "heads": f_heads, "geglu": f_geglu}
MUTANTS = {"window": ("mask_lastcol_missing", "mask_image0_only", "kv_head_div", "bias_transposed"),
           "cross": ("last_key_dropped", "range_skipped", "kv_head_mod", "item_map_ignored"),
           "prompt": ("causal_off1", "rope_pos_off1"), "ln": ("no_mean",), "merge_ln": ("merge_order",), "rms": ("eps_added",),
           "reduce": ("slab_dropped", "residual_after_norm"), "embed": ("half_rounded",), "rows": (), "heads": ("no_mean",),
           "geglu": ("gate_up_swapped", "gelu_exact")}


def evaluate(c: Case, dt=F64, mutant=None):
    return FAMILIES[c.family](c, dt, mutant)[0]


def reference(c: Case):
    """(outputs, tolerances) in float64, computed once per case and never modified. A tolerance of None = bit for bit."""
    if c._ref is None:
        outs, aux = FAMILIES[c.family](c, F64, None)
        f = c.family
        if f in ("window", "cross"):
            tol = {"out": _attn_tol(c, outs["out"], aux)}
        elif f == "prompt":
            tol = {"out": _attn_tol(c, outs["out"], aux), "k_rows": U[c.dtype] * outs["k_rows"].abs() + 4 * E * aux["k_mag"], "v_rows": None}
        elif f in ("ln", "merge_ln"):
            tol = {"y": _ln_tol(c, outs["y"], aux["x"], aux["d"], aux["rstd"], aux["w"], aux["b"], aux["x"].shape[-1])}
        elif f == "rms":
            tol = {"y": _rms_tol(c, outs["y"], aux["x"], aux["rstd"], aux["w"], aux["x"].shape[-1])}
        elif f == "reduce":
            if c.p["dyadic"]:
                tol = {"x_out": None}
            else:
                tol = {"x_out": U[c.dtype] * outs["x_out"].abs() + (c.p["S"] + 2) * E * aux["terms"]}
            outs.pop("y", None)                                  # y is held to the norm of the CANDIDATE's x_out: check()
        elif f in ("embed", "rows"):
            tol = {k: None for k in outs}
        elif f == "heads":
            tol = {"cls": aux["cls"], "box": aux["box"]}
        else:
            tol = {"out": aux["tol"]}
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


def check(c: Case, outs: Dict[str, torch.Tensor]):
    """[(output, worst error / bound, elements over the bound, all finite)] of a candidate's outputs (storage-dtype or float tensors on
    the CPU, shaped like the reference's)."""
    ref, tol = reference(c)
    rep = [_cmp(k, outs[k].reshape(ref[k].shape), ref[k], tol[k]) for k in ref]
    if c.family == "reduce" and c.t["w"] is not None:
        xo = outs["x_out"].to(F64)
        w = c.t["w"].to(F64)
        y, rstd = _rms(xo, w, c.p["eps"], c.dtype)
        rep.append(_cmp("y", outs["y"], y, _rms_tol(c, y, xo, rstd, w, c.p["H"])))
    return rep


def emulate(c: Case):
    """The reference alone: fp32 arithmetic, rounded where the kernel rounds."""
    return {k: v.to(c.dtype) if v.is_floating_point() else v for k, v in evaluate(c, torch.float32).items()}


# ------------------------------------------------------------------------------------------------------------- the cases
def window_cases() -> List[Case]:
    """2 images of 3 x 2 windows (so that window % (nwx nwy) matters), (nh, nkv) in {(2, 2), (4, 2), (8, 4)}, shift 0 and 4; one case whose
    bias carries +12 spikes on the keys of columns 3 and 4 -- the two sides of the cyclic-shift boundary -- so that every row's maximum sits
    on a key that is masked for some queries and not for others."""
    out = []
    for dtype in DTYPES:
        for i, (nh, nkv) in enumerate(((2, 2), (4, 2), (8, 4))):
            for shift in (0, 4):
                for spikes in ((False, True) if (nh, shift) == (4, 4) else (False,)):
                    g = _gen(100 + 10 * i + shift + spikes)
                    nW = 12
                    qkv = _rand(g, nW * 64, (nh + 2 * nkv) * 32)
                    qkv[:, :(nh + nkv) * 32] *= 1.5
                    bias = _rand(g, nh, 64, 64)
                    if spikes:
                        n = torch.arange(64)
                        bias[:, :, (n % 8 == 3) | (n % 8 == 4) | (n // 8 == 3) | (n // 8 == 4)] += 12.0
                    kills = ("kv_head_div", "bias_transposed") if nh != nkv else ("bias_transposed",)
                    if shift:
                        kills += ("mask_lastcol_missing", "mask_image0_only")
                    out.append(Case("window", f"win-h{nh}kv{nkv}-s{shift}" + ("-spikes" if spikes else ""), dtype,
                                    dict(nh=nh, nkv=nkv, nwx=3, nwy=2, images=2, shift=shift),
                                    dict(qkv=_st(qkv, dtype), bias=bias.float()), kills,
                                    "swin_window_attn_mfma_kernel" if dtype == torch.bfloat16 else "swin_window_attn_kernel"))
    return out


def real_perm(h, w, shift):
    perm, pads, (hp, wp), _ = oracle_window_tables(h, w, 8, shift)
    return perm, pads, hp * wp


def ln_cases() -> List[Case]:
    """C in {128, 256, 512, 1024}: bf16 takes layernorm_rows_bf16_kernel<LPR, NV> (lay_ln = 1) or the generic kernel (lay_ln = 0); C in {64, 192}
    generic only. rows in {1, 5, 256 / LPR + 3}: one workgroup with dead tail rows, and a second one. perm absent, or the real window
    permutation of two 12 x 20 images padded to 16 x 24 (rows_per_image_out = 384 > rows_per_image = 240), shift 4."""
    out = []
    for dtype in DTYPES:
        for C in (128, 256, 512, 1024, 64, 192):
            lpr = min(64, C // 8)
            knobs = (1, 0) if (dtype == torch.bfloat16 and C in (128, 256, 512, 1024)) else (1,)
            for lay_ln in knobs:
                for rows in (1, 5, 256 // lpr + 3, "perm"):
                    if rows == "perm" and C not in (128, 1024, 64):
                        continue
                    g = _gen(C + (7 if rows == "perm" else rows))
                    perm, rpi, rpo = None, 0, 0
                    if rows == "perm":
                        perm, _, rpo = real_perm(12, 20, 4)
                        rpi, rows = 240, 480
                    x = _rand(g, rows, C) * (0.5 + _rand(g, rows, 1).abs()) + _rand(g, rows, 1)
                    kern = "layernorm_rows_bf16_kernel" if (dtype == torch.bfloat16 and lay_ln and C in (128, 256, 512, 1024)) else "layernorm_kernel"
                    out.append(Case("ln", f"ln-C{C}-r{rows}-{'perm' if perm is not None else 'id'}-k{lay_ln}", dtype,
                                    dict(rows=rows, rpi=rpi or rows, rpo=rpo, C=C, eps=1e-5, lay_ln=lay_ln),
                                    dict(x=_st(x, dtype), w=_st(1 + 0.2 * _rand(g, C), dtype), b=_st(0.3 * _rand(g, C), dtype), perm=perm),
                                    ("no_mean",), kern))
    return out


def merge_cases() -> List[Case]:
    out = []
    for dtype in DTYPES:
        for B, H, W, C in ((2, 6, 10, 32), (1, 2, 2, 128), (2, 4, 6, 96)):
            g = _gen(B * 1000 + H * W + C)
            x = _rand(g, B, H, W, C) + _rand(g, B, H, W, 1)
            out.append(Case("merge_ln", f"merge-{B}x{H}x{W}x{C}", dtype, dict(B=B, H=H, W=W, C=C, eps=1e-5),
                            dict(x=_st(x, dtype), w=_st(1 + 0.2 * _rand(g, 4 * C), dtype), b=_st(0.3 * _rand(g, 4 * C), dtype)),
                            ("merge_order",), "merge_ln_kernel"))
    return out


def rms_cases() -> List[Case]:
    """Rows of ordinary size, rows whose mean square is around and below eps (the clamp), an all-zero row, and a row whose weight makes
    x rstd (1 + w) overflow the storage type: the clamp to its largest finite value."""
    out = []
    for dtype in DTYPES:
        for rows, C in ((1, 64), (5, 192), (7, 1024)):
            g = _gen(rows * C)
            x = _rand(g, rows, C)
            x[0] *= 3e-3                                          # mean square ~ 1e-5 = eps
            if rows > 2:
                x[1] *= 1e-4                                       # far below eps
                x[2] = 0.0
            w = 0.2 * _rand(g, C)
            p = dict(rows=rows, C=C, eps=1e-5)
            out.append(Case("rms", f"rms-{rows}x{C}", dtype, p, dict(x=_st(x, dtype), w=_st(w, dtype)), ("eps_added",), "adetr_rmsnorm_kernel"))
        g = _gen(77)
        w = 0.2 * _rand(g, 64)
        w[::3] = 3e38
        out.append(Case("rms", "rms-overflow", dtype, dict(rows=3, C=64, eps=1e-5), dict(x=_st(_rand(g, 3, 64), dtype), w=_st(w, dtype)), (),
                        "adetr_rmsnorm_kernel"))
    return out


def cross_plan(Lk):
    n = max(1, min(8, Lk // 128))
    chunk = (Lk + n - 1) // n
    return chunk, (Lk + chunk - 1) // chunk, (Lk + 31) & ~31


def cross_cases() -> List[Case]:
    """Lk in {64 (waves with no keys), 143 (ragged final step), 257 (two ranges, ragged), 576 (the default model)} x G in {1, 2, 4, 8} as a
    Latin square with S in {0, 1, 3, 8}; D in {32, 64}; 1 row, or 5 rows with item_map = [2, 0, 2, 1, 0] over 3 images. 2 kv heads.
    Lk = 1000 on top: the only size here at which a wave of the MFMA kernel walks more than one 96-key chunk (its second one ragged), and
    seven ranges of the fp32 kernel."""
    out = []
    Lks, Gs, Ss = (64, 143, 257, 576), (1, 2, 4, 8), (0, 1, 3, 8)
    for dtype in DTYPES:
        combos = [(Lk, G, Ss[(a + b) % 4], (32, 64)[(a + b // 2) % 2], (1, 5)[(a // 2 + b) % 2]) for a, Lk in enumerate(Lks) for b, G in enumerate(Gs)]
        for Lk, G, S, D, M in combos + [(1000, 4, 3, 64, 5), (1000, 8, 0, 32, 1)]:
            nkv, nq, NI = 2, 2 * G, 3
            g = _gen(Lk * 100 + G * 10 + S)
            q = _dyadic(g, M, nq * D)
            kv = _rand(g, NI, Lk, 2 * nkv * D)
            kv[:, -1, nkv * D:] *= 4.0                        # the last key's value stands out: a dropped tail must show in a single row
            t = dict(kv=_st(kv, dtype), item_map=torch.tensor([2, 0, 2, 1, 0][:M], dtype=torch.int32), q=None, qpart=None)
            if S == 0:
                t["q"] = _st(q, dtype)
            else:
                slabs = _dyadic(g, S, M, nq * D, lim=200)
                slabs[-1] = q - slabs[:-1].sum(0)
                assert torch.equal(slabs.float().sum(0).to(dtype).to(F64), q)
                t["qpart"] = slabs.float()
            chunk, ranges, _ = cross_plan(Lk)
            kills = ("last_key_dropped",) + (("kv_head_mod",) if G > 1 else ()) + (("item_map_ignored",) if M > 1 else ()) + \
                    (("range_skipped",) if ranges > 1 else ())
            out.append(Case("cross", f"cross-Lk{Lk}-D{D}-G{G}-S{S}-M{M}", dtype,
                            dict(M=M, nq=nq, nkv=nkv, D=D, Lk=Lk, S=S, images=NI, scale=D ** -0.5, chunk=chunk), t, kills,
                            "transpose_cross_v_kernel + cross_attn_mfma_kernel" if dtype == torch.bfloat16 else
                            "cross_attn_split_kernel + cross_attn_merge_kernel"))
    return out


def rope_table(Tmax, D):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=F64) / D))
    ang = (torch.arange(Tmax, dtype=F64)[:, None] * inv[None]).float()          # the engine's table is fp32 (cos, sin) of an fp32 angle
    return torch.stack([torch.cos(ang), torch.sin(ang)], -1).contiguous()


def prompt_cases() -> List[Case]:
    """Tn in {1, 3, 64} x G in {1, 2, 4}, D in {32, 64} alternating; B = 2, 2 kv heads, Tmax = 70 (cache rows >= Tn keep their sentinel).
    Tn = 64 with G = 8 on top: 512 (query, head) pairs, the one shape at which a thread of the workgroup takes a second pair."""
    out = []
    for dtype in DTYPES:
        for Tn, G, D in [(Tn, G, (32, 64)[(a + b) % 2]) for a, Tn in enumerate((1, 3, 64)) for b, G in enumerate((1, 2, 4))] + [(64, 8, 32)]:
            nkv, B, Tmax = 2, 2, 70
            nq = nkv * G
            g = _gen(Tn * 10 + G)
            qkv = _rand(g, B * Tn, (nq + 2 * nkv) * D)
            out.append(Case("prompt", f"prompt-T{Tn}-D{D}-G{G}", dtype, dict(B=B, Tn=Tn, nq=nq, nkv=nkv, D=D, Tmax=Tmax, scale=D ** -0.5),
                            dict(qkv=_st(qkv, dtype), rope=rope_table(Tmax, D)), ("rope_pos_off1",) + (("causal_off1",) if Tn > 1 else ()),
                            "adetr_prefill_attn_kernel"))
    return out


def reduce_cases() -> List[Case]:
    """H in {64, 68, 1024, 4096} x S in {1, 2, 8}; bias and w each NULL and set; res aliasing x_out or not; 5 rows. Everything on the dyadic
    grid (x_out is exact), plus one case of arbitrary fp32 slabs."""
    out = []
    for dtype in DTYPES:
        for a, H in enumerate((64, 68, 1024, 4096)):
            for b, S in enumerate((1, 2, 8)):
                has_b, has_w, alias = (a + b) % 2 == 0, (a + b // 2) % 2 == 0 or S == 2, b % 2 == a % 2
                g = _gen(H + S)
                part = _dyadic(g, S, 5, H, lim=40, step=2.0 ** -4).float()
                t = dict(part=part, res=_st(_dyadic(g, 5, H, lim=16, step=2.0 ** -4), dtype),
                         bias=_st(_dyadic(g, H, lim=16, step=2.0 ** -4), dtype) if has_b else None, w=_st(0.2 * _rand(g, H), dtype) if has_w else None)
                kills = (("slab_dropped",) if S > 1 else ()) + (("residual_after_norm",) if has_w else ())
                out.append(Case("reduce", f"reduce-H{H}-S{S}-b{int(has_b)}w{int(has_w)}a{int(alias)}", dtype,
                                dict(M=5, H=H, S=S, eps=1e-5, alias=alias, dyadic=True), t, kills, "splitk_residual_adetr_norm_kernel"))
        g = _gen(5)
        t = dict(part=_rand(g, 8, 5, 1024).float(), res=_st(_rand(g, 5, 1024), dtype), bias=_st(_rand(g, 1024), dtype), w=_st(0.2 * _rand(g, 1024), dtype))
        out.append(Case("reduce", "reduce-H1024-S8-random", dtype, dict(M=5, H=1024, S=8, eps=1e-5, alias=True, dyadic=False), t,
                        ("slab_dropped", "residual_after_norm"), "splitk_residual_adetr_norm_kernel"))
    return out


def embed_cases() -> List[Case]:
    """Tokens below 0, at vocab - 1 and above it; odd w and h; skew 0 and bbox_size; corners that clamp to 0 and to bbox_size; label /
    category / merge ids past their tables. Hd = 320 > 256 threads; table recognition: box columns 192, property columns 128."""
    out = []
    bs, vocab = 64, 70
    lay_tok = [[30, 31, 9, 7, 32, 32, 2], [5, 60, 21, 13, 0, 64, 0], [60, 3, 33, 41, 64, 0, 8], [-3, 69, 70, 200, 31, 33, 9], [0, 0, 1, 1, 40, 20, -1],
               [64, 64, 63, 63, 64, 64, 100], [10, 10, 5, 5, 32, 32, 3], [69, 1, 2, 69, 1, 69, 4]]
    tab_tok = [r[:6] + e for r, e in zip(lay_tok, ([1, 2, 3, 0], [4, 3, 69, 1], [5, 4, 70, 0], [-1, -2, -3, 1], [0, 0, 0, 0], [9, 9, 9, 9], [2, 1, 1, 1],
                                                   [69, 69, 69, 69]))]
    for dtype in DTYPES:
        for fam, Hd, BE, toks in (("layout", 320, 0, lay_tok), ("table", 320, 192, tab_tok)):
            g = _gen(len(fam))
            p = dict(family=fam, Hd=Hd, box_embed=BE, bbox_size=bs, vocab=vocab, label_count=9, category_count=5, merge_count=4)
            if fam == "layout":
                tables = {nm: _st(_rand(g, 9 if nm == "label" else vocab, Hd), dtype) for nm in EMBED_NAMES[:15]}
            else:
                tables = {nm: _st(_rand(g, vocab, BE), dtype) for nm in EMBED_NAMES[:14]}
                tables.update({nm: _st(_rand(g, n, Hd - BE), dtype) for nm, n in (("category", 5), ("merge", 4), ("colspan", vocab))})
            out.append(Case("embed", f"embed-{fam}", dtype, p, dict(tokens=torch.tensor(toks, dtype=torch.int32), tables=tables), ("half_rounded",),
                            "box_embed_kernel" if fam == "layout" else "table_embed_kernel"))
    return out


def rows_cases() -> List[Case]:
    """One padded two-image case each: 12 x 20 tokens per image in 16 x 24 window-order rows, shift 4, C = 96."""
    out = []
    perm, pads, rpw = real_perm(12, 20, 4)
    for dtype in DTYPES:
        g = _gen(11)
        C = 96
        out.append(Case("rows", "rows-patchify", dtype, dict(kind="patchify", B=2, C=3, H=8, W=12, P=4, Kpad=64),
                        dict(src=_rand(g, 2, 3, 8, 12).float(), dst=None, index=None), (), "patchify_kernel"))
        out.append(Case("rows", "rows-add", dtype, dict(kind="add_rows", rows=480, rpi=240, C=C),
                        dict(dst=_st(_rand(g, 480, C), dtype), src=_st(_rand(g, 240, C), dtype), index=None), (), "add_rows_kernel"))
        out.append(Case("rows", "rows-zero", dtype, dict(kind="zero_rows", B=2, n_pad=len(pads), rpi=rpw, C=C),
                        dict(dst=_st(_rand(g, 2 * rpw, C), dtype), src=None, index=pads), (), "zero_rows_kernel"))
        out.append(Case("rows", "rows-gather", dtype, dict(kind="gather_add", rows=480, rpi=240, C=C, rpi_src=rpw),
                        dict(dst=_st(_rand(g, 480, C), dtype), src=_st(_rand(g, 2 * rpw, C), dtype), index=perm), (), "gather_add_kernel"))
    return out


def heads_cases() -> List[Case]:
    """Hd in {64, 1024} x label_count in {20, 27} x ldx in {Hd, 3 Hd}; 3 rows."""
    out = []
    for dtype in DTYPES:
        for Hd in (64, 1024):
            for lc in (20, 27):
                for mul in (1, 3):
                    g = _gen(Hd + lc + mul)
                    t = dict(x=_st(_rand(g, 3, mul * Hd) + 1.5, dtype), fnorm_w=_st(0.2 * _rand(g, Hd), dtype), ln_w=_st(1 + 0.2 * _rand(g, Hd), dtype),
                             ln_b=_st(0.3 * _rand(g, Hd), dtype), lm_w=_st(_rand(g, lc, Hd) / Hd ** 0.5, dtype),
                             bb_w=_st(_rand(g, 6, Hd) / Hd ** 0.5, dtype), bb_b=_st(_rand(g, 6), dtype))
                    out.append(Case("heads", f"heads-Hd{Hd}-L{lc}-ldx{mul}", dtype, dict(B=3, Hd=Hd, label_count=lc, ldx=mul * Hd, rms_eps=1e-5, ln_eps=1e-5),
                                    t, ("no_mean",), "layout_heads_kernel<false>"))
    return out


def geglu_cases() -> List[Case]:
    """M in {1, 5, 130} x I in {128, 2048}, K in {64, 1024} alternating; N = 2 I weight rows, interleaved (gate_j, up_j). The exact gelu differs
    from the tanh form by up to 5e-4: above the fp32 bound at K = 64, inside the accumulation term 2 (K + 4) E A at K = 1024 and inside u in bf16."""
    out = []
    for dtype in DTYPES:
        for a, M in enumerate((1, 5, 130)):
            for b, I in enumerate((128, 2048)):
                K = (64, 1024)[(a + b) % 2]
                g = _gen(M + I + K)
                out.append(Case("geglu", f"geglu-M{M}-I{I}-K{K}", dtype, dict(M=M, N=2 * I, K=K),
                                dict(x=_st(_rand(g, M, K), dtype), w=_st(_rand(g, 2 * I, K) * (2.0 / K ** 0.5), dtype)),
                                ("gate_up_swapped",) + (("gelu_exact",) if dtype == torch.float32 and K == 64 else ()), "gemm EPI_GEGLU"))
    return out


_CASES = None


def all_cases() -> List[Case]:
    """Built once per process and shared: the cases and their inputs are never modified."""
    global _CASES
    if _CASES is None:
        _CASES = (window_cases() + ln_cases() + merge_cases() + rms_cases() + cross_cases() + prompt_cases() + reduce_cases() + embed_cases() +
                  rows_cases() + heads_cases() + geglu_cases())
    return _CASES
