"""Test infrastructure: the recognition engine's non-GEMM kernels one at a time (surya_op_rec_*) -- the cases, float64 references of every op
in plain torch / numpy, and the per-element bound each family is held to. Built like lay_ops_ref.py.

A Case holds the inputs exactly as the device gets them (already rounded to the storage type T) and the parameters of ONE call.
evaluate(case, dt, mutant):
  dt = float64              the reference; it rounds to storage only where the bound below says the result is determined bit for bit;
  dt = float32              "the reference alone": fp32 arithmetic that rounds where the kernel rounds;
  mutant = a name           a deliberately wrong evaluation (float64): what the bound has to catch (MUTANTS).
check(case, outs) holds EVERY element of every output to the bound. Nothing in a bound is measured.

Symbols: E = 2^-24 (unit roundoff of fp32), u = one unit in the last place relative to the value (fp32 2^-23, bf16 2^-7, fp16 2^-10).

Qwen2 RMSNorm (rmsnorm_rows, the norm half of reduce-norm, both embedding norms; eps ADDED to the mean square): y = T(w T(x rstd))
    tol = 2 u |ref| + (C + 8) E |x| rstd |w|          one u for the inner rounding's flip, one for the outer; the sum of C squares has relative
    error (C + 2) E, rstd half of it plus the rsqrt, and the two products are 2 E more. A row of values around sqrt(eps) tells added from
    clamped eps (rstd differs by up to sqrt 2 there). (fp16 results below 2^-14 are subnormal: a rounding there is 2^-25 absolute, more than
    u / 2 of the value. The bound has no floor for them; the cases' inputs are fixed and their handful of subnormal results stays inside
    it, the fp32 evaluation of rmsrows-C1280-r5 at 0.96 of the bound being the closest.)
Sum half of reduce-norm: x = T(x + sum_s part_s) is ONE rounding. Slabs and x on a dyadic grid (multiples of 2^-4, |sum| < 2^9): every fp32
    partial sum is exact in any order, so x is the rounding of the exact sum: bit for bit. Random data: u |ref| + (S + 2) E sum |terms|.
    y is held to the norm of the CANDIDATE's x (which the first check has already tied down).
MXFP8 copies (bf16): y8 / sy = oracle.mx_oracle.quantize of the candidate's own y rows, bit for bit; scales at [c / 128][srows][4]; scale
    bytes of rows the launch does not own keep their sentinel.
Row movers, embeddings, convert_tiles: bit for bit; torch arithmetic in the storage dtype, the kernel's order (scatter_image: T(a + T(h + w))).
    Rows nobody targets keep NaN; padding columns are zero.
rope_kv_append: q (in place) and the k cache rows u |ref| + 4 E (|x1 cos| + |x2 sin|), rotate_half pairing, table values as given; v rows,
    the v part of qkv, the k part of qkv and every other cache row bit for bit (untouched).
RoPE tables: the angle is the fp32 product the kernel forms (numpy float32 here), cos / sin in float64 of it: tol = 2^-21 + u |ref|. 2^-21 is
    four fp32 ulps of 1, twice the 2 ulp specified for sincosf, entries being at most 1; this margin is NOT derived from the kernel, and
    the CPU tier shows the table mutants exceed it by orders of magnitude.
Head, token and state: exact. token = first maximum over the tiles, the lower column among equal values; next_token pad when done;
    kv_len[slot] += len_inc for the rows' slots only; fused row_len[r] = min(kv_len + len_inc, Tmax - 1); the forced cursor advances by one;
    greedy_token is the argmax.
Head, score: tot = sum_t s_t exp(m_t - best); relative bound on 1 / tot: rel = sum_t share_t (|m_t - best| + 4) 2^-23 + 18 E (lay_ops_ref's
    e_exp weighted by each tile's share of the total, at most 16 additions, the reciprocal). greedy_prob and a forced score:
    (rel + 4 E (1 + |flogit - best|)) |ref|; logprob = (flogit - best) - log tot, an ABSOLUTE rel + 4 E (1 + |flogit - best|): a relative
    error of tot is an absolute error of its logarithm (the inputs keep tot < 64, so that logf's own ulp stays inside the 4 E).
    Where the forced id is the argmax the score has the bits of the candidate's own 1 / tot (greedy_prob).
Head, bbox: exact by construction. hidden on multiples of 2^-3 in [-1, 1], wb on 2^-6 in [-1/8, 1/8], bb on 2^-6: every product is a multiple
    of 2^-9 and every partial sum stays below 2^8, so the dot product and the bias add are exact in fp32 in any order and T(d + b) is
    determined. A row is redrawn until the float64 sigmoid is further than 2^-20 (relative) from a rounding boundary of T and
    T(sigmoid) bbox_size further than bbox_size 2^-20 from an integer. (T 16 bit: T(sigmoid) has at most 11 significant bits, the fp32
    product with bbox_size is exact and an exact integer is no ambiguity; the distance is asked of fp32 only, where the kernel's own
    sigmoid is what gets truncated.) No coordinate is exempt; at most two redraws per case (CPU tier).
Not a conftest; never imported by the product."""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from lay_ops_ref import E, F64, _dyadic, _gen, _rand
from lay_ops_ref import U as _U_LAY
from oracle import mx_oracle as MX

U = dict(_U_LAY)
U[torch.float16] = 2.0 ** -10
F32 = torch.float32
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
DT_NAME = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}
NO_COL = 0x7fffffff                     # gemm.h: the record of a tile with no allowed column is (-inf, 0x7fffffff, 0, 0)
SENT_I, SENT_F, SENT_B = -7, -7.0, 0xAA  # sentinels of partly written outputs (ints, floats, scale bytes)
HEAD_THREADS = 384                      # SA_HEAD_THREADS
SLOTS = 8


@dataclass
class Case:
    family: str
    name: str
    dtype: torch.dtype
    p: dict
    t: Dict[str, Optional[torch.Tensor]]
    kills: Tuple[str, ...] = ()
    kernel: str = ""
    redraws: int = 0
    _ref: Optional[tuple] = field(default=None, repr=False)

    @property
    def id(self):
        return f"{self.name}-{DT_NAME[self.dtype]}"


def _rk(c, dt):
    """(rounding only the KERNEL makes -- the fp32 emulation repeats it, the reference does not --, rounding both make)."""
    rr = lambda x: x.to(c.dtype).to(dt)
    return (rr if dt == F32 else (lambda x: x)), rr


def _st(x, dtype):
    return x.to(dtype)


# ------------------------------------------------------------------------------------------------------------- norm
def _qnorm(x, w, eps, rk, mutant=None, n_div=None, extra_ss=None):
    ss = (x * x).sum(-1, keepdim=True)
    if extra_ss is not None:
        ss = ss + extra_ss
    var = ss / (n_div or x.shape[-1])
    var = var.clamp(min=eps) if mutant == "eps_clamped" else var + eps
    rstd = torch.rsqrt(var)
    return rk(w * rk(x * rstd)), rstd


def _qnorm_tol(c, ref, x, rstd, w):
    return 2 * U[c.dtype] * ref.abs() + (x.shape[-1] + 8) * E * x.abs() * rstd * w.abs()


def _mx(c, y, srows, mutant=None):
    """MXFP8 copy of the rows y (any float dtype; rounded to the case's storage type first): codes [rows][H], scales [H / 128][srows][4]."""
    yq = y.to(c.dtype).to(F32).numpy()
    rows, H = yq.shape
    q, s = MX.quantize(yq)
    s = s.reshape(rows, H // 128, 4).transpose(1, 0, 2)
    if mutant == "scale_wrong_ktile":
        s = np.roll(s, 1, axis=0)
    sy = np.full((H // 128, srows, 4), SENT_B, dtype=np.uint8)
    sy[:, :rows] = s
    return torch.from_numpy(q.copy()), torch.from_numpy(sy)


def f_rms(c, dt, mutant=None):
    rk, _ = _rk(c, dt)
    x = c.t["x"].to(dt)[c.t["src_row"].long(), :c.p["C"]]
    if mutant == "src_row_ignored":
        x = c.t["x"].to(dt)[:c.p["rows"], :c.p["C"]]
    w = c.t["w"].to(dt)
    y, rstd = _qnorm(x, w, c.p["eps"], rk, mutant)
    return {"y": y}, dict(x=x, rstd=rstd, w=w)


def reduce_threads(H):
    return -(-(H // 4) // 64) * 64


def f_reduce(c, dt, mutant=None):
    rk, rr = _rk(c, dt)
    p, H = c.p, c.p["H"]
    part, x0 = c.t["part"].to(dt), c.t["x"].to(dt)
    if mutant == "slab_dropped":
        part = part[:-1]
    v = x0.clone()
    for s_ in range(part.shape[0]):                               # the kernel's order
        v = v + part[s_]
    x = rr(v)
    outs = {"x": x}
    if c.t["w"] is not None:
        xn = x0 if mutant == "norm_of_old_x" else x
        thr = reduce_threads(H)
        extra = (thr - H // 4) * (xn[:, :4] ** 2).sum(-1, keepdim=True) if mutant == "shadow_lanes_counted" else None
        y, _ = _qnorm(xn, c.t["w"].to(dt), p["eps"], rk, mutant, 4 * thr if mutant == "mean_over_threads" else None, extra)
        outs["y"] = y
        if p["mx"]:
            outs["y8"], outs["sy"] = _mx(c, y, p["srows"], mutant)
    return outs, dict(terms=c.t["part"].to(dt).abs().sum(0) + x0.abs())


def f_embed(c, dt, mutant=None):
    rk, _ = _rk(c, dt)
    p = c.p
    slot = c.t["active"].long()
    tok = c.t["next_token"].long()[torch.arange(len(slot)) if mutant == "slot_is_row" else slot]
    x = c.t["table"].to(dt)[tok]
    kl = c.t["kv_len"][slot]
    row_len = kl if mutant == "row_len_unclamped" else kl.clamp(max=p["Tmax"] - 1)
    w = c.t["w"].to(dt)
    y, rstd = _qnorm(x, w, p["eps"], rk, mutant)
    outs = {"row_len": row_len.to(torch.int32), "x": x, "y": y}
    if p["mx"]:
        outs["y8"], outs["sy"] = _mx(c, y, p["srows"], mutant)
    return outs, dict(x=x, rstd=rstd, w=w)


# ------------------------------------------------------------------------------------------------------------- head
def _bbox(c, hidden, wb, bb, dt, mutant=None):
    _, rr = _rk(c, dt)
    if mutant == "bbox_rows_shifted":
        wb = wb.roll(1, 0)
    d = hidden @ wb.T                                               # exact in fp32 and up (see the module text)
    lin = rr(d if mutant == "bbox_no_bias" else d + bb)
    sg = rr(1.0 / (1.0 + torch.exp(-lin)))
    v = sg * c.p["bbox_size"]
    return (torch.round(v) if mutant == "bbox_rounds" else torch.floor(v)).to(torch.int32), lin, sg


def f_head(c, dt, mutant=None):
    rk, rr = _rk(c, dt)
    p, t = c.p, c.t
    M, Tn, eos, pad = p["M"], p["tiles_n"], p["eos"], p["pad"]
    part = t["part"]
    m, s = part[..., 0].to(dt), part[..., 2].to(dt)
    idx = part[..., 1].contiguous().view(torch.int32).long()
    best = m.amax(-1)
    eq = m == best[:, None]
    tile = torch.arange(Tn)[None].expand(M, Tn)
    if mutant == "tie_takes_last":
        pick = torch.where(eq, tile, torch.full_like(tile, -1)).argmax(-1)
    elif mutant == "tile_order":                                   # ties go to the lower thread (tile % threads), not to the lower column
        key = (tile % HEAD_THREADS) * 8 + tile // HEAD_THREADS
        pick = torch.where(eq, key, torch.full_like(key, 1 << 40)).argmin(-1)
    else:
        pick = torch.where(eq, idx, torch.full_like(idx, 1 << 40)).argmin(-1)
    bi = idx[torch.arange(M), pick]
    ex = torch.exp(m - best[:, None])
    tot = s.sum(-1) if mutant == "sumexp_not_rescaled" else (s * ex).sum(-1)
    slot = t["row_slot"].long()
    forced = p["forced"]
    if forced:
        cur = t["cursor"].long()[slot]
        ok = (cur >= 0) & (cur < p["stride"])
        f = torch.where(ok, t["forced_table"].long()[slot, cur.clamp(0, p["stride"] - 1)], torch.full_like(cur, -1))
        dl = torch.where(f >= 0, t["flogit"].to(dt) - best, torch.zeros_like(best))
    else:
        f = torch.full_like(bi, -1)
        dl = torch.zeros_like(best)
    tok = torch.where(f >= 0, f, bi)
    done = (tok == eos) | (tok == pad)
    score = torch.where(f >= 0, torch.exp(dl) / tot, 1.0 / tot)
    if mutant != "done_score_kept":
        score = torch.where(done, torch.zeros_like(score), score)
    nxt = tok if mutant == "next_not_pad" else torch.where(done, torch.full_like(tok, pad), tok)
    kv0 = t["kv_len"].long()
    inc = 0 if mutant == "len_not_incremented" else p["len_inc"]

    def by_slot(vals, sent, dtype):
        o = torch.full((SLOTS,) + tuple(vals.shape[1:]), sent, dtype=dtype)
        o[slot] = vals.to(dtype)
        return o
    fdt = dt
    kv = kv0.clone()
    kv[slot] += inc
    box, lin, sg = _bbox(c, t["hidden"].to(dt), t["wb"].to(dt), t["bb"].to(dt), dt, mutant)
    outs = {"out_token": by_slot(tok, SENT_I, torch.int32), "out_score": by_slot(score, SENT_F, fdt), "out_bbox": by_slot(box, SENT_I, torch.int32),
            "next_token": by_slot(nxt, SENT_I, torch.int32), "kv_len": kv.to(torch.int32)}
    if p["alts"]:
        outs["best_tot"] = by_slot(torch.stack([best, tot], -1), SENT_F, fdt)
    if forced:
        outs.update(greedy_token=by_slot(bi, SENT_I, torch.int32), greedy_prob=by_slot(1.0 / tot, SENT_F, fdt),
                    logprob=by_slot(dl - torch.log(tot), SENT_F, fdt))
        cu = t["cursor"].long().clone()
        cu[slot] += 1
        outs["cursor"] = cu.to(torch.int32)
    aux = dict(m=m, s=s, best=best, tot=tot, dl=dl, f=f, bi=bi, done=done, slot=slot, lin=lin, sg=sg)
    if p["fused"]:
        rl = kv0[slot] + p["len_inc"]
        outs["row_len"] = (rl if mutant == "row_len_unclamped" else rl.clamp(max=p["Tmax"] - 1)).to(torch.int32)
        x = t["table"].to(dt)[nxt]
        w = t["wnorm"].to(dt)
        y, rstd = _qnorm(x, w, p["eps"], rk, mutant)
        outs.update(x=x, y=y)
        if p["mx"]:
            outs["y8"], outs["sy"] = _mx(c, y, p["srows"], mutant)
        aux.update(x=x, rstd=rstd, w=w)
    return outs, aux


def _head_tol(c, outs, a):
    m, s, best, tot = a["m"], a["s"], a["best"], a["tot"]
    live = s > 0
    share = torch.where(live, s * torch.exp(m - best[:, None]) / tot[:, None], torch.zeros_like(s))
    dm = torch.where(live, (m - best[:, None]).abs(), torch.zeros_like(m))
    assert float(tot.max()) < 64.0 and float(dm.max()) <= 40.0
    rel = (share * (dm + 4)).sum(-1) * 2.0 ** -23 + 18 * E
    relf = rel + 4 * E * (1 + a["dl"].abs())
    slot = a["slot"]

    def by_slot(v, width=None):
        o = torch.zeros((SLOTS,) + tuple(v.shape[1:]), dtype=F64)
        o[slot] = v
        return o
    forced_row = a["f"] >= 0
    tol = {k: None for k in outs}
    tol["out_score"] = by_slot(torch.where(forced_row, relf, rel) * outs["out_score"][slot].abs())
    if "best_tot" in outs:
        tol["best_tot"] = by_slot(torch.stack([torch.zeros_like(rel), rel * tot], -1))
    if "greedy_prob" in outs:
        tol["greedy_prob"] = by_slot(relf * outs["greedy_prob"][slot].abs())
        tol["logprob"] = by_slot(relf)
    if "y" in outs:
        tol["y"] = _qnorm_tol(c, outs["y"], a["x"], a["rstd"], a["w"])
    return tol


# ------------------------------------------------------------------------------------------------------------- rope
def f_ropekv(c, dt, mutant=None):
    rk, _ = _rk(c, dt)
    p = c.p
    D, nq, nkv, Tmax = p["D"], p["nq"], p["nkv"], p["Tmax"]
    half = D // 2
    qkv = c.t["qkv"].to(dt)
    n = qkv.shape[0]
    x = qkv.view(n, nq + 2 * nkv, D)
    slot, pos = c.t["tok_slot"].long(), c.t["tok_pos"].long()
    rpos = torch.arange(n) if mutant == "pos_is_token_index" else pos
    cs = c.t["rope"].to(dt)[rpos]                                  # [n, half, 2]
    cos, sin = cs[:, None, :, 0], cs[:, None, :, 1]
    if mutant == "sin_sign":
        sin = -sin

    def rot(v):
        if mutant == "interleaved_pairs":
            x1, x2 = v[..., 0::2], v[..., 1::2]
            o = torch.empty_like(v)
            o[..., 0::2], o[..., 1::2] = x1 * cos - x2 * sin, x2 * cos + x1 * sin
            return o
        x1, x2 = v[..., :half], v[..., half:]
        return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], -1)

    def mag(v):
        x1, x2 = v[..., :half].abs(), v[..., half:].abs()
        return torch.cat([x1 * cos.abs() + x2 * sin.abs(), x2 * cos.abs() + x1 * sin.abs()], -1)
    q, k, v = x[:, :nq], x[:, nq:nq + nkv], x[:, nq + nkv:]
    out = x.clone()
    out[:, :nq] = rk(rot(q))
    kc = torch.full((p["slots"], nkv, Tmax, D), 5.0, dtype=dt)
    vc = torch.full((p["slots"], nkv, Tmax, D), 5.0, dtype=dt)
    heads = (torch.arange(nkv) + 1) % nkv if mutant == "k_head_off_by_nq" else torch.arange(nkv)
    kc[slot[:, None], heads[None], pos[:, None]] = rk(rot(k))
    vc[slot[:, None], torch.arange(nkv)[None], pos[:, None]] = rk(rot(v)) if mutant == "v_rotated" else v
    tq = torch.zeros_like(out)
    tq[:, :nq] = mag(q)
    tk = torch.zeros_like(kc)
    tk[slot[:, None], torch.arange(nkv)[None], pos[:, None]] = mag(k)
    return {"qkv": out.reshape(n, -1), "kc": kc, "vc": vc}, dict(tq=tq.reshape(n, -1), tk=tk)


def inv_freq(n, D):
    return (1.0 / (10000.0 ** (np.arange(n, dtype=np.float64) * 2 / D))).astype(np.float32)


def f_table(c, dt, mutant=None):
    """cos / sin of the fp32 angle the kernel forms; dt float32 takes numpy's float32 cos / sin of it."""
    p = c.p
    f = c.t["inv_freq"].numpy()
    if p["kind"] == "decoder":
        pos = np.arange(p["Tmax"], dtype=np.int64) + (1 if mutant == "table_pos_off_by_one" else 0)
        ang = pos.astype(np.float32)[:, None] * f[None]
    else:
        ph = c.t["pos_hw"].numpy().astype(np.int64) + (1 if mutant == "table_pos_off_by_one" else 0)
        h, w = (ph[:, 1], ph[:, 0]) if mutant == "hw_swapped" else (ph[:, 0], ph[:, 1])
        ang = np.concatenate([h.astype(np.float32)[:, None] * f[None], w.astype(np.float32)[:, None] * f[None]], 1)
    assert ang.dtype == np.float32
    a = ang if dt == F32 else ang.astype(np.float64)
    cs, sn = np.cos(a), np.sin(a)
    if mutant == "table_cos_sin_swapped":
        cs, sn = sn, cs
    out = torch.from_numpy(np.stack([cs, sn], -1)).to(dt)
    if dt == F32 and p["kind"] == "decoder":
        out = out.to(c.dtype).to(dt)
    return {"table": out}, None


# ------------------------------------------------------------------------------------------------------------- movers
def f_rows(c, dt, mutant=None):
    p, k, t = c.p, c.p["kind"], c.t
    nan = float("nan")
    if k == "convert_tiles":
        src, idx = t["src"], t["index"].long()
        y = torch.zeros(p["P"], p["kout"], dtype=c.dtype)
        if mutant == "scatter_is_gather":
            y[idx, :p["kin"]] = src.to(c.dtype)
        else:
            y[:, :p["kin"]] = src[idx].to(c.dtype)
    elif k == "scatter_image":
        hi, wi = t["index2"].long(), t["index3"].long()
        if mutant == "hw_swapped":
            hi, wi = wi % t["src2"].shape[0], hi % t["src3"].shape[0]
        y = torch.full((p["dst_rows"], p["H"]), nan, dtype=c.dtype)
        y[t["index"].long()] = t["src"] + (t["src2"][hi] + t["src3"][wi])
    elif k == "scatter_rows":
        y = torch.full((p["dst_rows"], p["H"]), nan, dtype=c.dtype)
        if mutant == "scatter_is_gather":
            y[:len(t["index"])] = t["src"][t["index"].long() % t["src"].shape[0]]
        else:
            y[t["index"].long()] = t["src"]
    else:
        ids = t["index"].long()
        y = torch.full((len(ids), p["H"]), nan, dtype=c.dtype)
        keep = torch.ones_like(ids, dtype=torch.bool) if mutant == "negative_id_written" else ids >= 0
        y[keep] = t["src"][ids.clamp(min=0)[keep]]
    return {"dst": y.to(dt)}, None


FAMILIES = {"rms": f_rms, "reduce": f_reduce, "embed": f_embed, "head": f_head, "ropekv": f_ropekv, "table": f_table, "rows": f_rows}
MUTANTS = {"rms": ("eps_clamped", "src_row_ignored"),
           "reduce": ("slab_dropped", "norm_of_old_x", "eps_clamped", "mean_over_threads", "shadow_lanes_counted", "scale_wrong_ktile"),
           "embed": ("eps_clamped", "row_len_unclamped", "slot_is_row", "scale_wrong_ktile"),
           "head": ("tie_takes_last", "tile_order", "sumexp_not_rescaled", "done_score_kept", "next_not_pad", "len_not_incremented",
                    "row_len_unclamped", "bbox_no_bias", "bbox_rounds", "bbox_rows_shifted", "eps_clamped", "scale_wrong_ktile"),
           "ropekv": ("interleaved_pairs", "sin_sign", "pos_is_token_index", "k_head_off_by_nq", "v_rotated"),
           "table": ("hw_swapped", "table_pos_off_by_one", "table_cos_sin_swapped"),
           "rows": ("hw_swapped", "scatter_is_gather", "negative_id_written")}
TABLE_MUTANT_MARGIN = 100.0             # the CPU tier wants the table mutants this many times over the bound


def evaluate(c: Case, dt=F64, mutant=None):
    return FAMILIES[c.family](c, dt, mutant)[0]


def reference(c: Case):
    """(outputs, tolerances) in float64, computed once per case and never modified. A tolerance of None = bit for bit."""
    if c._ref is None:
        outs, aux = FAMILIES[c.family](c, F64, None)
        f, u = c.family, U[c.dtype]
        tol = {k: None for k in outs}
        if f == "rms":
            tol["y"] = _qnorm_tol(c, outs["y"], aux["x"], aux["rstd"], aux["w"])
        elif f == "reduce":
            if not c.p["dyadic"]:
                tol["x"] = u * outs["x"].abs() + (c.p["S"] + 2) * E * aux["terms"]
            for k in ("y", "y8", "sy"):                              # held to the CANDIDATE's x / y: check()
                outs.pop(k, None), tol.pop(k, None)
        elif f == "embed":
            tol["y"] = _qnorm_tol(c, outs["y"], aux["x"], aux["rstd"], aux["w"])
            for k in ("y8", "sy"):
                outs.pop(k, None), tol.pop(k, None)
        elif f == "head":
            tol = _head_tol(c, outs, aux)
            for k in ("y8", "sy"):
                outs.pop(k, None), tol.pop(k, None)
        elif f == "ropekv":
            tol["qkv"] = torch.where(aux["tq"] > 0, u * outs["qkv"].abs() + 4 * E * aux["tq"], torch.zeros_like(aux["tq"]))
            tol["kc"] = torch.where(aux["tk"] > 0, u * outs["kc"].abs() + 4 * E * aux["tk"], torch.zeros_like(aux["tk"]))
        elif f == "table":
            tol["table"] = 2.0 ** -21 + (u if c.p["kind"] == "decoder" else U[F32]) * outs["table"].abs()
        c._ref = (outs, tol)
    return c._ref


def _cmp(what, got, ref, tol):
    got, ref = got.to(F64), ref.to(F64)
    both_nan = torch.isnan(got) & torch.isnan(ref)
    finite = bool(torch.isfinite(got[~torch.isnan(ref)]).all())
    if tol is None:
        bad = int(((got != ref) & ~both_nan).sum())
        return (what, float("inf") if bad else 0.0, bad, finite)
    err = (got - ref).abs()
    err = torch.where(both_nan, torch.zeros_like(err), torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf)))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol.clamp(min=1e-300))
    return (what, float(ratio.max()), int((err > tol).sum()), finite)


def check(c: Case, outs: Dict[str, torch.Tensor]):
    """[(output, worst error / bound, elements over the bound, all finite)] of a candidate's outputs (CPU tensors shaped like the reference's)."""
    ref, tol = reference(c)
    rep = [_cmp(k, outs[k].reshape(ref[k].shape), ref[k], tol[k]) for k in ref]
    p = c.p
    if c.family == "reduce" and c.t["w"] is not None:
        xo = outs["x"].to(F64)
        w = c.t["w"].to(F64)
        y, rstd = _qnorm(xo, w, p["eps"], lambda v: v)
        rep.append(_cmp("y", outs["y"], y, _qnorm_tol(c, y, xo, rstd, w)))
    if p.get("mx"):
        y8, sy = _mx(c, outs["y"].reshape(-1, p["H"]), p["srows"])
        rep.append(_cmp("y8", outs["y8"].reshape(y8.shape), y8, None))
        rep.append(_cmp("sy", outs["sy"].reshape(sy.shape), sy, None))
    if c.family == "head" and p["forced"]:                           # forced id == argmax: the score is the candidate's own 1 / tot
        _, aux = FAMILIES["head"](c, F64, None)
        rows = (aux["f"] == aux["bi"]) & ~aux["done"]
        sl = aux["slot"][rows]
        rep.append(_cmp("score_bits", outs["out_score"].reshape(-1)[sl], outs["greedy_prob"].reshape(-1)[sl], None))
    return rep


def emulate(c: Case):
    """The reference alone: fp32 arithmetic, rounded where the kernel rounds; storage-dtype outputs where the kernel stores T."""
    outs = evaluate(c, F32)
    keep32 = {"out_score", "best_tot", "greedy_prob", "logprob", "table"}
    return {k: (v.to(c.dtype) if v.is_floating_point() and k not in keep32 else v) for k, v in outs.items()}


def representable(c: Case):
    """Every floating-point input is already a value of the dtype the device gets it in."""
    f32_inputs = {"part", "rope", "inv_freq", "flogit"}
    for k, v in c.t.items():
        if v is None or not v.is_floating_point():
            continue
        if c.family == "rows" and c.p["kind"] == "convert_tiles" and k == "src":
            want = F32
        else:
            want = F32 if k in f32_inputs else c.dtype
        if v.dtype != want:
            return False, k
    return True, None


# ------------------------------------------------------------------------------------------------------------- the cases
def _tiny_rows(x, eps, row=0):
    """Row `row` around sqrt(eps): added and clamped eps give an rstd that differs by a third."""
    x[row] = x[row] * math.sqrt(eps)
    return x


def rms_cases() -> List[Case]:
    """C in {8, 128, 1280, 5120} x rows in {1, 5}; ldx = C + 8 > C; src_row over 6 source rows with a repeat; source row 2 is tiny."""
    out = []
    for dtype in DTYPES:
        for C in (8, 128, 1280, 5120):
            for rows in (1, 5):
                g = _gen(C + rows)
                x = _tiny_rows(_rand(g, 6, C + 8), 1e-6, 2)
                src = torch.tensor([2, 0, 2, 4, 1][:rows], dtype=torch.int32)
                out.append(Case("rms", f"rmsrows-C{C}-r{rows}", dtype, dict(rows=rows, C=C, ldx=C + 8, eps=1e-6),
                                dict(x=_st(x, dtype), w=_st(1 + 0.2 * _rand(g, C), dtype), src_row=src), ("eps_clamped", "src_row_ignored"),
                                "rmsnorm_kernel"))
    return out


def reduce_cases() -> List[Case]:
    """H in {128, 320, 1280, 1288, 4096} (32 shadow lanes, 48 idle lanes, exactly five waves, a last wave with 62 idle lanes, 16 waves) x S in
    {1, 2, 3, 4, 5, 8}, each at rnorm 2 and 1; M in {1, 3, 257} as a Latin square; w = NULL once; dyadic data (x bit for bit), row 0 tiny; one
    random-data case; MXFP8 (bf16) at H in {128, 1280}, M = 3, srows = 8."""
    out = []
    Hs, Ss, Ms = (128, 320, 1280, 1288, 4096), (1, 2, 3, 4, 5, 8), (1, 3, 257)
    shared = {}
    for dtype in DTYPES:
        for a, H in enumerate(Hs):
            for b, S in enumerate(Ss):
                M = Ms[(a + b) % 3]
                if (a, b) not in shared:
                    g = _gen(1000 * a + b)
                    part = _dyadic(g, S, M, H, lim=40, step=2.0 ** -4)
                    x = _dyadic(g, M, H, lim=32, step=2.0 ** -4)
                    part[:, 0] = _dyadic(g, S, H, lim=1, step=2.0 ** -11)     # row 0: mean square around eps
                    x[0] = _dyadic(g, H, lim=1, step=2.0 ** -11)
                    shared[(a, b)] = (part.float(), x, 1 + 0.2 * _rand(g, H))
                part, x, w = shared[(a, b)]
                has_w = not (H == 320 and S == 3)
                thr = reduce_threads(H)
                for rnorm in (2, 1):
                    kills = ()
                    if S > 1:
                        kills += ("slab_dropped",)
                    if has_w:
                        kills += ("norm_of_old_x", "eps_clamped")
                        if 4 * thr != H:
                            kills += ("mean_over_threads", "shadow_lanes_counted")
                    sl = 8 if (rnorm == 1 or S > 4) else (4 if S > 2 else 2)
                    out.append(Case("reduce", f"reduce-H{H}-S{S}-M{M}-rn{rnorm}" + ("" if has_w else "-now"), dtype,
                                    dict(H=H, S=S, M=M, eps=1e-6, dyadic=True, rnorm=rnorm, mx=False, srows=0),
                                    dict(part=part, x=_st(x, dtype), w=_st(w, dtype) if has_w else None), kills,
                                    f"splitk_residual_norm_kernel<T, {sl}>"))
        g = _gen(5)
        out.append(Case("reduce", "reduce-H1280-S8-M3-random", dtype, dict(H=1280, S=8, M=3, eps=1e-6, dyadic=False, rnorm=2, mx=False, srows=0),
                        dict(part=_rand(g, 8, 3, 1280).float(), x=_st(_rand(g, 3, 1280), dtype), w=_st(1 + 0.2 * _rand(g, 1280), dtype)),
                        ("slab_dropped", "norm_of_old_x"), "splitk_residual_norm_kernel<T, 8>"))
    for H, S in ((128, 2), (1280, 4)):
        g = _gen(70 + H)
        t = dict(part=_dyadic(g, S, 3, H, lim=40, step=2.0 ** -4).float(), x=_st(_dyadic(g, 3, H, lim=32, step=2.0 ** -4), torch.bfloat16),
                 w=_st(1 + 0.2 * _rand(g, H), torch.bfloat16))
        out.append(Case("reduce", f"reduce-H{H}-S{S}-M3-mx", torch.bfloat16, dict(H=H, S=S, M=3, eps=1e-6, dyadic=True, rnorm=2, mx=True, srows=8), t,
                        ("slab_dropped",) + (("scale_wrong_ktile",) if H > 128 else ()), "splitk_residual_norm_kernel<T, .> + MXFP8 copy"))
    return out


def embed_cases() -> List[Case]:
    """8 slots, active list [5, 0, 6]; kv_len of those slots 0, Tmax - 1, Tmax + 3; their next tokens vocab - 1, 0 and a row of tiny values.
    embed_slots_norm2_kernel (ghead 2) at H in {128, 1280, 1536, 1544, 2048}; embed_slots_norm_kernel at ghead 1, H in {128, 132, 1280}, and
    at H = 2304 with ghead 2 (above the register geometry). MXFP8 (bf16) at {256, 1280} on both and at 1408 (a multiple of 128 only) on the old."""
    out = []
    V, Tmax = 11, 64
    plain = [(H, 2) for H in (128, 1280, 1536, 1544, 2048)] + [(128, 1), (132, 1), (1280, 1), (2304, 2)]
    mxs = [(256, 2), (1280, 2), (256, 1), (1280, 1), (1408, 1)]
    for dtype in DTYPES:
        for H, ghead, mx in [(H, gh, False) for H, gh in plain] + ([(H, gh, True) for H, gh in mxs] if dtype == torch.bfloat16 else []):
            g = _gen(H * 4 + ghead + mx)
            table = _tiny_rows(_rand(g, V, H), 1e-6, 4)
            nt = torch.tensor([0, 3, 2, 7, 1, V - 1, 4, 5], dtype=torch.int32)
            kv = torch.tensor([Tmax - 1, 9, 9, 9, 9, 0, Tmax + 3, 9], dtype=torch.int32)
            new = ghead == 2 and H <= 2048 and H % 8 == 0
            kills = ("eps_clamped", "row_len_unclamped", "slot_is_row") + (("scale_wrong_ktile",) if mx and H > 128 else ())
            out.append(Case("embed", f"embed-H{H}-gh{ghead}" + ("-mx" if mx else ""), dtype, dict(H=H, Tmax=Tmax, eps=1e-6, ghead=ghead, mx=mx, srows=8),
                            dict(table=_st(table, dtype), next_token=nt, active=torch.tensor([5, 0, 6], dtype=torch.int32), kv_len=kv,
                                 w=_st(1 + 0.2 * _rand(g, H), dtype)), kills, "embed_slots_norm2_kernel" if new else "embed_slots_norm_kernel"))
    return out


def _bbox_ok(c, hidden, wb, bb):
    """Every coordinate of every row unambiguous (module text)."""
    d = hidden.to(F64) @ wb.to(F64).T + bb.to(F64)
    lin = d.to(c.dtype).to(F64)
    sg = 1.0 / (1.0 + torch.exp(-lin))
    if c.dtype == F32:
        v = sg.to(F32).to(F64) * c.p["bbox_size"]
        return (v - torch.round(v)).abs() > c.p["bbox_size"] * 2.0 ** -20
    r = sg.to(c.dtype)
    return ((sg * (1 + 2.0 ** -20)).to(c.dtype) == r) & ((sg * (1 - 2.0 ** -20)).to(c.dtype) == r)


def _head_case(dtype, tiles_n, H, M, mode, ghead, seed):
    """mode: plain0 (len_inc 0), plain1, fused, fusedmx, alts (best_tot, len_inc 0), forced (+ fused where the head has it)."""
    V, Tmax, eos, pad, stride, bbox_size = 12, 64, 1, 0, 4, 1025
    head2 = ghead == 2 and tiles_n <= 4 * HEAD_THREADS
    forced = mode == "forced"
    fused = mode in ("fused", "fusedmx") or (forced and head2)
    p = dict(tiles_n=tiles_n, H=H, M=M, len_inc=0 if mode in ("plain0", "alts") else 1, eos=eos, pad=pad, bbox_size=bbox_size, Tmax=Tmax, fused=fused,
             mx=mode == "fusedmx", srows=8, alts=mode == "alts", forced=forced, ghead=ghead, stride=stride, eps=1e-6)
    g = _gen(seed)
    m = torch.rand(M, tiles_n, generator=g, dtype=F64) * -6.0 - 6.0                # every tile 6 .. 12 below the row's best, which is set below
    s = 1.0 + 7.0 * torch.rand(M, tiles_n, generator=g, dtype=F64)
    idx = 2 + (torch.arange(tiles_n)[None] * 5 + torch.arange(M)[:, None]) % (V - 2)
    ties = sorted({t_ for t_ in (3, 385, 700) if t_ < tiles_n}) if tiles_n > 3 else list(range(tiles_n))
    if len(ties) == 1 and tiles_n > 4:
        ties.append(tiles_n - 1)
    bt = torch.randint(0, tiles_n, (M,), generator=g)
    bt[0] = ties[0]
    base = torch.rand(M, generator=g, dtype=F64) * 4.0
    m += base[:, None]
    m[torch.arange(M), bt] = base
    m = m.float()
    for j, t_ in enumerate(ties):                                                    # row 0: equal maxima, columns ascending with the tile
        m[0, t_] = m[0, ties[0]]
        idx[0, t_] = 2 + 3 * j
    if M > 1:
        idx[1, bt[1]] = eos                                                          # row 1: eos argmax; row 2: pad argmax
        idx[2, bt[2]] = pad
        if tiles_n > 1:                                                              # row 3: a tile as the masked epilogue leaves it when nothing is allowed
            e = (int(bt[3]) + 1) % tiles_n
            m[3, e], s[3, e], idx[3, e] = -math.inf, 0.0, NO_COL
    part = torch.zeros(M, tiles_n, 4, dtype=F32)
    part[..., 0], part[..., 2] = m, s.float()
    part[..., 1] = idx.to(torch.int32).view(F32)
    row_slot = torch.tensor([3, 0, 6, 1, 4][:M], dtype=torch.int32)
    kv = torch.tensor([Tmax - 1, 20, 9, Tmax + 3, 0, 9, 31, 9], dtype=torch.int32)
    t = dict(part=part, row_slot=row_slot, kv_len=kv, bb=_st(_dyadic(g, 6, lim=64, step=2.0 ** -6), dtype), wb=None, hidden=None,
             table=None, wnorm=None, forced_table=None, cursor=None, flogit=None)
    if fused:
        t["table"], t["wnorm"] = _st(_tiny_rows(_rand(g, V, H), 1e-6, 2), dtype), _st(1 + 0.2 * _rand(g, H), dtype)
    c = Case("head", f"head-t{tiles_n}-H{H}-M{M}-{mode}-gh{ghead}", dtype, p, t, (), "greedy_head2_kernel" if head2 else "greedy_head_kernel<T, true>")
    t["wb"] = _st(_dyadic(g, 6, H, lim=8, step=2.0 ** -6), dtype)
    hidden = torch.zeros(M, H, dtype=F64)
    todo = torch.ones(M, dtype=torch.bool)
    while bool(todo.any()):
        hidden[todo] = _dyadic(g, int(todo.sum()), H, lim=8, step=2.0 ** -3)
        bad = ~_bbox_ok(c, _st(hidden, dtype), t["wb"], t["bb"]).all(-1)
        c.redraws += int(bad.any())
        todo = bad
    t["hidden"] = _st(hidden, dtype)
    if forced:
        best = m.amax(-1)
        ft = torch.full((SLOTS, stride), 9, dtype=torch.int32)
        cur = torch.full((SLOTS,), 1, dtype=torch.int32)
        fl = torch.zeros(M, dtype=F32)
        sl = row_slot.long()
        ft[sl[0], 0], cur[sl[0]], fl[0] = int(idx[0, ties[0]]), 0, best[0]          # the argmax itself: flogit has the bits of best
        if M > 1:
            ft[sl[1], 2], cur[sl[1]], fl[1] = 7, 2, best[1] - 1.75                   # another id (the argmax is eos)
            ft[sl[2], 3], cur[sl[2]], fl[2] = eos, 3, best[2] - 3.0                  # eos forced (the argmax is pad)
            cur[sl[3]], cur[sl[4]] = -1, stride                                       # free-running: before the table, past it
        t.update(forced_table=ft, cursor=cur, flogit=fl)
    kills = ("bbox_no_bias", "bbox_rows_shifted") + (("bbox_rounds",) if M > 1 else ()) + (("sumexp_not_rescaled",) if tiles_n > 1 else ())
    if len(ties) > 1:
        kills += ("tie_takes_last",)
        if any(t_ % HEAD_THREADS < ties[0] for t_ in ties[1:]):
            kills += ("tile_order",)
    if M > 1:
        kills += ("next_not_pad",) + (() if forced else ("done_score_kept",))
    if p["len_inc"]:
        kills += ("len_not_incremented",)
    if fused:
        kills += ("row_len_unclamped", "eps_clamped") + (("scale_wrong_ktile",) if p["mx"] else ())
    c.kills = kills
    return c


def head_cases() -> List[Case]:
    """tiles_n in {1, 2, 383, 384, 385, 1280, 1536, 1537 (the fallback head whatever ghead)} with H in {128, 1280, 2048} and M in {1, 5}; rows 3, 0,
    6, 1, 4 of 8 slots. Per shape: ghead 2 plain (len_inc 0), fused (len_inc 1), alternatives' best_tot, forced (+ fused); ghead 1 plain
    (len_inc 1) and forced. MXFP8 beside the fused embedding once (bf16, H = 1280)."""
    out = []
    shapes = [(1, 128, 1), (2, 1280, 5), (383, 2048, 5), (384, 128, 5), (385, 1280, 1), (1280, 2048, 5), (1536, 1280, 5), (1537, 128, 5)]
    for dtype in DTYPES:
        for i, (tn, H, M) in enumerate(shapes):
            modes = [("plain0", 2), ("alts", 2), ("forced", 2), ("plain1", 1), ("forced", 1)]
            if tn <= 4 * HEAD_THREADS:
                modes.insert(1, ("fused", 2))
            if dtype == torch.bfloat16 and (tn, H) == (1536, 1280):
                modes.append(("fusedmx", 2))
            for j, (mode, gh) in enumerate(modes):
                out.append(_head_case(dtype, tn, H, M, mode, gh, 9000 + 10 * i + j))
    return out


def rope_cs_table(Tmax, D, dtype):
    ang = np.arange(Tmax, dtype=np.float32)[:, None] * inv_freq(D // 2, D)[None]
    return torch.from_numpy(np.stack([np.cos(ang), np.sin(ang)], -1)).to(dtype).to(F32).contiguous()


def ropekv_cases() -> List[Case]:
    """(D, nq, nkv) in {(128, 10, 2), (32, 4, 4), (128, 5, 1)}; 7 tokens over slots [2, 0, 2, 1, 0, 2, 1], positions with 0 and Tmax - 1."""
    out = []
    Tmax = 16
    for dtype in DTYPES:
        for D, nq, nkv in ((128, 10, 2), (32, 4, 4), (128, 5, 1)):
            g = _gen(D + nq)
            t = dict(qkv=_st(_rand(g, 7, (nq + 2 * nkv) * D), dtype), tok_slot=torch.tensor([2, 0, 2, 1, 0, 2, 1], dtype=torch.int32),
                     tok_pos=torch.tensor([0, 5, Tmax - 1, 3, 0, 1, Tmax - 1], dtype=torch.int32), rope=rope_cs_table(Tmax, D, dtype))
            kills = ("interleaved_pairs", "sin_sign", "pos_is_token_index", "v_rotated") + (("k_head_off_by_nq",) if nkv > 1 else ())
            out.append(Case("ropekv", f"ropekv-D{D}-q{nq}-kv{nkv}", dtype, dict(D=D, nq=nq, nkv=nkv, Tmax=Tmax, slots=3), t, kills, "rope_kv_append_kernel"))
    return out


def table_cases() -> List[Case]:
    """Decoder: Tmax = 1024, half in {16, 64}. Vision: P = 37, D in {32, 80}, positions up to 255 with h != w."""
    out = []
    for dtype in DTYPES:
        for half in (16, 64):
            out.append(Case("table", f"ropetab-dec-h{half}", dtype, dict(kind="decoder", Tmax=1024, half=half),
                            dict(inv_freq=torch.from_numpy(inv_freq(half, 2 * half)), pos_hw=None), ("table_pos_off_by_one", "table_cos_sin_swapped"),
                            "rope_table_kernel"))
        for D in (32, 80):
            g = _gen(D)
            pos = torch.randint(0, 256, (37, 2), generator=g).to(torch.int32)
            pos[0], pos[1] = torch.tensor([0, 255]), torch.tensor([255, 0])
            out.append(Case("table", f"ropetab-vis-D{D}", dtype, dict(kind="vision", P=37, D=D),
                            dict(inv_freq=torch.from_numpy(inv_freq(D // 4, D // 2)), pos_hw=pos),
                            ("hw_swapped", "table_pos_off_by_one", "table_cos_sin_swapped"), "rope_vision_table_kernel"))
    return out


def rows_cases() -> List[Case]:
    out = []
    for dtype in DTYPES:
        for kin, kout in ((588, 640), (12, 64)):
            g = _gen(kin)
            out.append(Case("rows", f"rows-convert-{kin}-{kout}", dtype, dict(kind="convert_tiles", P=7, kin=kin, kout=kout),
                            dict(src=_rand(g, 7, kin).float(), index=torch.tensor([1, 2, 0, 3, 6, 4, 5], dtype=torch.int32)), ("scatter_is_gather",),
                            "convert_tiles_kernel"))
        for H in (128, 1280):
            g = _gen(H)
            t = dict(src=_st(_rand(g, 5, H), dtype), src2=_st(_rand(g, 4, H), dtype), src3=_st(_rand(g, 6, H), dtype),
                     index=torch.tensor([6, 0, 3, 9, 4], dtype=torch.int32), index2=torch.tensor([0, 3, 1, 2, 3], dtype=torch.int32),
                     index3=torch.tensor([5, 1, 4, 0, 2], dtype=torch.int32))
            out.append(Case("rows", f"rows-scatter-image-H{H}", dtype, dict(kind="scatter_image", H=H, dst_rows=11), t, ("hw_swapped",),
                            "scatter_image_kernel"))
        for H in (128, 1288):
            g = _gen(H + 1)
            out.append(Case("rows", f"rows-scatter-rows-H{H}", dtype, dict(kind="scatter_rows", H=H, dst_rows=11),
                            dict(src=_st(_rand(g, 5, H), dtype), index=torch.tensor([6, 0, 3, 9, 4], dtype=torch.int32)), ("scatter_is_gather",),
                            "scatter_rows_kernel"))
            out.append(Case("rows", f"rows-embed-tokens-H{H}", dtype, dict(kind="embed_tokens", H=H),
                            dict(src=_st(_rand(g, 9, H), dtype), index=torch.tensor([8, -1, 0, 3, -1, 8, 5], dtype=torch.int32)), ("negative_id_written",),
                            "embed_tokens_kernel"))
    return out


_CASES = None


def all_cases() -> List[Case]:
    """Built once per process and shared: the cases and their inputs are never modified."""
    global _CASES
    if _CASES is None:
        _CASES = rms_cases() + reduce_cases() + embed_cases() + head_cases() + ropekv_cases() + table_cases() + rows_cases()
    return _CASES
