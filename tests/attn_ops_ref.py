"""Test infrastructure: the attention kernels one at a time -- surya_op_attn (attn_mfma_kernel<bf16 | fp16, D>, attn_valu_kernel<float, D>),
surya_op_decode_attn (decode_attn_flash2_kernel in both buffer forms, decode_attn_flash_kernel, decode_attn_mfma_kernel),
surya_op_decode_attn_kv8 with surya_op_kv8_quant_rows, and the MXFP8 copy of the decode output (surya_op_decode_attn_mx / _kv8_mx) -- the cases,
float64 references in plain torch, and the per-element bound each output is held to. Built like lay_ops_ref.py / rec_ops_ref.py / ocr_ops_ref.py,
whose Case, E, U, _dyadic, _rand, _gen, _cmp, _mx and softmax bound (_attn_tol) are used here, not restated.

evaluate(case, dt, mutant):  dt = float64 the reference; dt = float32 "the reference alone": fp32 arithmetic in the kernel's order (chunks, waves,
running maxima, the combine) that rounds where the kernel rounds; mutant = a name: a deliberately wrong float64 evaluation (MUTANTS).
check(case, outs, pinned) holds EVERY element of every output to the bound; bytes the launch does not own must keep their sentinel / input bits.
No term of any bound was fitted to a measured error: each is read off the code lines named below.

Symbols: u = one unit in the last place relative to the value (fp32 2^-23, bf16 2^-7, fp16 2^-10), E = 2^-24, N visible keys of a query,
s the scores (scale included), m their maximum, p = softmax(s), A = sum_j p_j |v_j|.

Softmax output (all kernels). Start: lay_ops_ref._attn_tol,  u |ref| + (2 e_s + 2 e_exp + (N + 4) E + r_P) A, with
    e_s   = max_j (D + 4) E scale sum_c |q_c| |k_jc| + 2 E |s_j|      a D-term fp32 dot product (MFMA, or attn_valu_kernel's quad sums) and the scale;
    e_exp = (max_j |s_j - m| + 4) 2^-23                               ONE hardware exp2 of x log2 e (attn_mfma.h: exp2f((s - m) * sl2); the decode
            kernels and attn_valu_kernel: __expf); inputs keep |s - m| <= 40.
  added here, as ocr_ops_ref.py derives for cls_attn:
    chunks  every kernel walks the keys in chunks with a running maximum (attn_mfma.h `mnew / alpha`: 64 keys; attn_valu_kernel: 16; the decode
            kernels: a wave's 32 keys of every 128-key tile, decode_attn.h `mrun / alpha`; decode_attn_mfma_kernel: a 64- or 128-key tile, `hstat`;
            the KV8 kernel: 32 keys of every 256-key tile) and the decode kernels combine their waves' records with one more exp
            (`__expf(rec[D] - mx)`). An entry's weight is a product of 1 + (times its query's running maximum rose afterwards) + (1 for the
            combine) exp factors whose exponents add up to s_j - m: the |x| 2^-24 part adds up to the single-pass one, the fixed 4 x 2^-23 is paid
            per factor: + 2 x 4 n_f 2^-23 A with n_f = rises + 1, the rises counted on the float64 scores.
            Sums: one product and one addition per chunk and per record of the combine, the reciprocal, the final product: + (NC + 8) E A.
    r_P     the un-normalised P is rounded to T before P V (`H16<T>::pk`, `pack2`): 2^-8 (bf16), 2^-11 (fp16), 0 (fp32 kernels).
    sub     fp16 only (attn_mfma.h header): an entry below 2^-14 becomes a subnormal, up to 2^-25 ABSOLUTE: sum over those keys of 2^-25 |v_j| / l
            (P is taken against the running maximum, which never exceeds the final one). The OUTPUT has the same floor: an element below
            2^-14 is stored as a subnormal, spacing 2^-24 whatever its size, which u |ref| does not cover: + 2^-24 (rounding and flip).
    KV8     score = (q . k8) * sk_j: one more product, + 2 E |s_j| in e_s; P * sv_j is one more product before the bf16 pack: + E A. The
            reference is attention over the DEQUANTISED arrays (the format is the definition: oracle/mx_oracle.py::kv8_quantize).
Scores of the decode kernels: x = T(bias + slabs in order) (decode_attn.h `Ty<T>::rnd(val)`); the slabs and the bias are on a dyadic grid
    (multiples of 2^-5, |sum| <= 4), so every fp32 sum is exact in any order and T(.) is the identity: x has no error and no flip. RoPE:
    decode_attn_flash2_kernel pins `__fmaf_rn(x1, cos, -__fmul_rn(x2, sin))`; the reference computes exactly that (a float64 product of two
    short values is exact, rounded once to fp32; the sum is checked exact in float64 and rounded once), then T(.), then q_s = T(fp32(q scale)):
    the SAME values the kernel holds, bit for bit, so no flip term. The other kernels (`x1 * cs - x2 * sn`, contraction left to the compiler)
    can differ from the pinned form in the last fp32 bit and flip a rounding to T: with a REAL table (cos / sin of the model, rounded to T) their
    e_s carries 2 u scale sum |q| |k| (one flip of T(rope), one of T(q scale)) and their appended K row is held to u |ref| + 4 E (|x1 cos| +
    |x2 sin|); with a DYADIC table (cos, sin multiples of 2^-3: every product and sum exact in fp32 in any form) they have no flip either and
    the K row is held bit for bit in every kernel. Only the `random` family uses the real table.
Appended V row, every other cache row, spare slots, the KV8 arrays outside the appended token: bit for bit. KV8 appended token: bytes and scale
    equal kv8_quantize of the (exact) bf16 row, and the stored token is a fixed point of the quantiser IN VALUE: quantising its dequantised
    values gives the same values again. (Not always the same bytes: a largest element of 224.5 x 2^e is stored as 224 x 2^e, which a second
    pass writes as 448 x 2^(e - 1).)
uniform family: q = 0 (decode: the q part of bias + slabs is exactly 0 and RoPE leaves it 0), so every score is 0, every un-normalised weight
    exactly 1 (exp2f(0) = __expf(0) = 1, alpha = 1 or 0), V holds odd integers: the numerator is an exact integer in fp32 in any order and
    the denominator is N. out = T(fp32(num * fp32(1 / N))), within 2 E of num / N: bf16 / fp16 are held BIT FOR BIT to T(num / N), every
    element redrawn (its V column) until num / N lies further than 2^-20 (relative) from a rounding boundary of T; fp32 is held to 4 E |ref|
    (`1.0f / den` may be the hardware reciprocal, good to one ulp = 2 E; the product adds E).
MXFP8 copy: out8 / sout = oracle.mx_oracle.quantize of the CANDIDATE's own output rows as stored, bit for bit (rec_ops_ref._mx), scales at
    [col / 128][srows][4]; scale bytes of rows >= rows keep their sentinel.
Not mutants: "P left unrounded" and "P normalised before rounding" are inside the bound by construction -- the float64 reference does not round
    P at all, r_P is the room the bound leaves for either rounding. `q_scale_unrounded` (q scale kept in fp32) moves a score by up to
    2^-9 sum |q_s| |k|: the CPU tier shows the bf16 bound of the random d = 128 cases separates it (x 2.1), so it IS a mutant there; in fp16
    (2^-12) and fp32 it is inside and no case lists it.
Poison: what no launch may read holds NaN -- cache rows >= row_len (row row_len is overwritten, never read), other slots, slabs >= n_slabs, rows
    between segments. decode_attn.h clamps rows to len - 1; with an EMPTY cache (row_len = 0, which LayoutModel::decode_step launches at position 0)
    the three kernels used to fill rows 1 .. 15 (1 .. 7) of their first MFMA step from the stale cache row 0 and multiply it by P = 0 --
    0 x NaN = NaN: fixed in decode_attn.h (`len == 0`), and tested here with NaN in row 0. The KV8 kernel's contract differs (include/surya_amd.h):
    it fetches V^T and the v scales by whole 16-key blocks, so those of tokens row_len + 1 .. (row_len | 31) must be finite; its poison is NaN
    in the K rows and k scales past the context and finite but huge (byte 0x7e = 448, scale 2^10) in V^T and the v scales.
Not a conftest; never imported by the product."""
from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Dict, List

import numpy as np
import torch

from lay_ops_ref import E, F64, _attn_tol, _dyadic, _gen, _rand
from oracle import mx_oracle as MX
from rec_ops_ref import DT_NAME, F32, SENT_B, U, Case, _cmp, _mx, _st, rope_cs_table

BF16, F16 = torch.bfloat16, torch.float16
DTYPES = (F32, BF16, F16)
NAN = float("nan")
RP = {F32: 0.0, BF16: 2.0 ** -8, F16: 2.0 ** -11}
_C32 = SimpleNamespace(dtype=F32)          # _attn_tol's u |ref| is taken at fp32 and topped up to the case's u below
SEG_LENS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)
TMAX = 400
DEC_LENS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 143, 144, 255, 256, 257, 383, 384, TMAX - 1)
SPARE_SLOTS = 3
# kernels behind surya_op_decode_attn per dtype: (name, tuning, rotation pinned)
DEC_VARIANTS = {BF16: (("flash2", dict(dattn=4, dattn_db=-1), True), ("flash2db", dict(dattn=4, dattn_db=1), True), ("flash", dict(dattn=3, dattn_db=-1), False)),
                F16: (("flash2", dict(dattn=4, dattn_db=-1), True), ("flash2db", dict(dattn=4, dattn_db=1), True)),
                F32: (("mfma", dict(dattn=4, dattn_db=-1), False),)}


def _h16():
    h = torch.ones(1, 1, dtype=F64)
    for _ in range(4):
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return h


H16 = _h16()                                # 16 orthogonal +-1 codes; tiled over the head dim they stay orthogonal


def _code(i, D):
    return H16[i].repeat(D // 16)


def _rt(x, dtype, dt=F64):
    return x.to(dtype).to(dt)


def _f32(x):
    return x.to(F32).to(F64)


def _far(v, dtype):
    """v (float64) lies further than 2^-20 (relative) from every rounding boundary of dtype."""
    r = v.to(dtype)
    return ((v * (1 + 2.0 ** -20)).to(dtype) == r) & ((v * (1 - 2.0 ** -20)).to(dtype) == r)


# ------------------------------------------------------------------------------------------------------------- the kernels' order of operations
def _flash(s, v, groups, rnd, ex):
    """Online softmax as the kernels run it. s [B, Q, N] scores (-inf = masked), v [B, N, D]; groups = one list of key-index chunks per wave
    (one group: no combine). rnd(p, idx) = what enters P V. Returns [B, Q, D]."""
    recs = []
    zero = lambda t: torch.zeros_like(t)
    for chunks in groups:
        m = torch.full(s.shape[:2], -math.inf, dtype=s.dtype)
        l, o = zero(m), torch.zeros(s.shape[0], s.shape[1], v.shape[-1], dtype=s.dtype)
        for idx in chunks:
            sc = s[..., idx]
            mnew = torch.maximum(m, sc.amax(-1))
            safe = torch.where(torch.isinf(mnew), zero(mnew), mnew)
            alpha = torch.where(torch.isinf(m), zero(m), ex(m - safe))
            pv = ex(sc - safe[..., None])
            l = l * alpha + pv.sum(-1)
            o = o * alpha[..., None] + rnd(pv, idx) @ v[:, idx]
            m = mnew
        recs.append((m, l, o))
    if len(recs) == 1:
        return o / l[..., None]
    mx = torch.stack([r[0] for r in recs]).amax(0)
    num, den = 0.0, 0.0
    for m, l, o in recs:
        e = torch.where(torch.isinf(m), zero(m), ex(torch.where(torch.isinf(m), zero(m), m) - mx))
        num, den = num + e[..., None] * o, den + e * l
    return num / den[..., None]


def _rises(s, groups):
    """Per query: the largest number of chunks of one group in which its running maximum rises (>= 1), + 1 where waves are combined."""
    best = torch.zeros(s.shape[:2], dtype=F64)
    for chunks in groups:
        m = torch.full(s.shape[:2], -math.inf, dtype=s.dtype)
        n = torch.zeros(s.shape[:2], dtype=F64)
        for idx in chunks:
            bm = s[..., idx].amax(-1)
            n = n + (bm > m).to(F64)
            m = torch.maximum(m, bm)
        best = torch.maximum(best, n)
    return best.clamp(min=1.0) + (1.0 if len(groups) > 1 else 0.0)


def _softmax_tol(dtype, ref, s, qk, vis, vabs, D, groups, extra_es=0.0, extra_A=0.0):
    """The bound of the module text for ref [B, Q, Dv]; s [B, Q, N] float64 scores (-inf where masked), qk = scale |q| |k|^T, vabs [B, N, Dv]."""
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    p = e / l
    A = p @ vabs
    aux = dict(s=s, bias=torch.zeros_like(s), qk=qk, p=p, A=A, live=vis.expand_as(s), N=int(vis.sum(-1).max()), D=D, rp=RP[dtype],
               back=lambda x: x, extra=extra_es)
    tol = _attn_tol(_C32, ref, aux) + (U[dtype] - U[F32]) * ref.abs()
    nf = _rises(s, groups)[..., None]
    nc = sum(len(g) for g in groups) + len(groups)
    tol = tol + (8 * nf * 2.0 ** -23 + (nc + 8) * E + extra_A) * A
    if dtype == F16:
        tol = tol + (((e < 2.0 ** -14) & vis).to(F64) * 2.0 ** -25) @ vabs / l + 2.0 ** -24
    return tol


def _chunks(n, size):
    return [torch.arange(a, min(a + size, n)) for a in range(0, n, size)]


# ------------------------------------------------------------------------------------------------------------- segment attention
def _strided(buf, off, rows, rs, heads, hs, D):
    return buf.reshape(-1).as_strided((rows, heads, D), (rs, hs, 1), off)


def _seg_vis(L, Lx, causal, mutant):
    qi, j = torch.arange(L)[:, None], torch.arange(Lx)[None]
    q0 = (qi // 64) * 64
    kend = torch.clamp(q0 + 64, max=L) if causal else torch.full_like(qi, L)
    vis = j < kend
    if causal:
        if mutant == "causal_strict":
            vis = vis & ((j < qi) | ((j == 0) & (qi == 0)))
        elif mutant == "causal_plus_one":
            vis = (j <= qi + 1) & (j < L)
        elif mutant == "causal_by_tile":
            vis = vis & (j <= q0)
        else:
            vis = vis & (j <= qi)
    if mutant == "last_key_dropped":
        vis = vis & ~((j == kend - 1) & (kend % 64 != 0) & (kend > 1))
    if mutant == "segment_leak" and not causal:
        vis = j < min((L + 63) // 64 * 64, Lx)
    return vis


def _seg_groups(dtype, n):
    return [_chunks(n, 16 if dtype == F32 else 64)]


def f_seg(c, dt, mutant=None):
    p, T = c.p, c.dtype
    D, H, G, causal = p["D"], p["heads"], p["group"], p["causal"]
    Hkv = H // G
    out = torch.full((p["out_rows"] * p["o_row"],), NAN, dtype=dt)
    tol = torch.zeros_like(out) if (dt == F64 and mutant is None) else None
    scale = 1.0 if mutant == "scale_missing" else p["scale"]
    hmap = torch.arange(H) % Hkv if mutant == "kv_head_modulo" else torch.arange(H) // G
    for sg in p["segs"]:
        L, Lx = sg["L"], sg["L"] + sg["tail"]
        q = _strided(c.t["q"], sg["q_off"], L, p["q_row"], H, p["q_head"], D).to(dt).permute(1, 0, 2)
        k = _strided(c.t["k"], sg["k_off"], Lx, p["k_row"], Hkv, p["k_head"], D).to(dt).permute(1, 0, 2)[hmap]
        v = _strided(c.t["v"], sg["v_off"], Lx, p["k_row"], Hkv, p["k_head"], D).to(dt).permute(1, 0, 2)[hmap]
        vis = _seg_vis(L, Lx, causal, mutant)
        used = vis.any(0)
        v = torch.where(used[None, :, None], v, torch.zeros_like(v))            # rows nobody sees never enter a product
        k = torch.where(used[None, :, None], k, torch.zeros_like(k))
        if mutant == "pv_key_order":                                            # V fragment halves swapped: key j meets the V row of key j ^ 8
            idx = torch.arange(Lx) ^ 8
            v = torch.where((idx < L)[None, :, None], v[:, idx.clamp(max=Lx - 1)], torch.zeros_like(v))
        groups = _seg_groups(T, Lx)
        if dt == F32:                                                            # the kernel's arithmetic
            if T == F32:                                                         # attn_valu_kernel: q * scale first, __expf
                s = ((q * torch.tensor(scale, dtype=F32)) @ k.transpose(-1, -2)).masked_fill(~vis, -math.inf)
                o = _flash(s, v, groups, lambda pv, idx: pv, torch.exp)
            else:                                                                # attn_mfma_kernel: raw scores, exp2f((s - m) * scale * log2 e), P -> T
                sl2 = torch.tensor(scale, dtype=F32) * torch.tensor(1.44269504088896340736, dtype=F32)
                s = (q @ k.transpose(-1, -2)).masked_fill(~vis, -math.inf)
                o = _flash(s, v, groups, lambda pv, idx: _rt(pv, T, F32), lambda x: torch.exp2(x * sl2))
            o = _rt(o, T, dt)
        else:
            s = ((q @ k.transpose(-1, -2)) * scale).masked_fill(~vis, -math.inf)
            if mutant == "no_rescale":                                           # exp against the running chunk maximum, never rescaled
                nch = (Lx + 63) // 64
                sp = torch.nn.functional.pad(s, (0, nch * 64 - Lx), value=-math.inf).view(H, L, nch, 64)
                mk = torch.cummax(sp.amax(-1), -1).values.repeat_interleave(64, -1)[..., :Lx]
                e = torch.exp(s - mk)
            else:
                e = torch.exp(s - s.amax(-1, keepdim=True))
            o = (e @ v) / e.sum(-1, keepdim=True)
            if tol is not None:
                t = _softmax_tol(T, o, s, (q.abs() @ k.abs().transpose(-1, -2)) * scale, vis, v.abs(), D, groups)
                if p["exact"]:
                    t = 4 * E * o.abs() if T == F32 else torch.zeros_like(o)
        oi = sg["o_off"] + (torch.arange(L)[:, None, None] * p["o_row"] + torch.arange(H)[None, :, None] * p["o_head"] + torch.arange(D)[None, None, :])
        out[oi] = o.permute(1, 0, 2)
        if tol is not None:
            tol[oi] = t.permute(1, 0, 2)
        if mutant == "query_clamped_row_written":                                # rows L .. tile end get the clamped query's output
            own = p["own"].reshape(-1)
            for r in range(L, min((L + 63) // 64 * 64, p["out_rows"] - sg["o_off"] // p["o_row"])):
                ri = oi[L - 1] + (r - (L - 1)) * p["o_row"]
                free = ~own[ri]
                out[ri[free]] = o.permute(1, 0, 2)[L - 1][free]
    shape = (p["out_rows"], p["o_row"])
    return {"out": out.view(shape)}, (None if tol is None else {"out": tol.view(shape)})


# ------------------------------------------------------------------------------------------------------------- decode attention
def _rope_pinned(x, cs, interleaved=False):
    """decode_attn_flash2_kernel's rotation on float64 copies of fp32 values: fp32(x1 cos - fp32(x2 sin)) | fp32(x2 cos + fp32(x1 sin))."""
    half = x.shape[-1] // 2
    x1, x2 = (x[..., 0::2], x[..., 1::2]) if interleaved else (x[..., :half], x[..., half:])
    cos, sin = cs[:, 0], cs[:, 1]

    def add(a, b):                                                               # a + b must be exact in float64 (TwoSum error 0)
        t = a + b
        bb = t - a
        assert bool(((a - (t - bb)) + (b - bb) == 0).all()), "the rotation's sum is not exact in float64"
        return _f32(t)
    lo, hi = add(x1 * cos, -_f32(x2 * sin)), add(x2 * cos, _f32(x1 * sin))
    return torch.stack([lo, hi], -1).flatten(-2) if interleaved else torch.cat([lo, hi], -1)


def _dec_groups(c, n):
    d, T = c.p["d"], c.dtype
    if c.p["kv8"]:
        waves, kt = 8, 256
    elif T == F32:
        return [_chunks(n, 64 if d * 4 >= 512 else 128)]
    else:
        waves, kt = 4, 128
    groups = []
    for w in range(waves):
        ch = [torch.arange(t0 + 32 * w, min(t0 + 32 * w + 32, n)) for t0 in range(0, n, kt) if t0 + 32 * w < n]
        groups.append(ch)
    return groups


def _slab_sum(c, dt, mutant):
    p = c.p
    S = p["S"]
    x = torch.zeros_like(c.t["bias"].to(dt)) if mutant == "bias_missing" else c.t["bias"].to(dt)
    x = x[None].expand(p["M"], -1).clone()
    n = S
    if mutant == "slab_clamped_counted":
        n = 2 if S <= 2 else (4 if S <= 4 else 8)
    for s_ in range(n):
        x = x + c.t["part"][min(s_, S - 1)].to(dt)
    return _rt(x, c.dtype, dt)


_VIEWS = {}


def _kv8_views(c):
    """The e4m3 codes of the KV8 arrays decoded to float64, unscaled: k8 [slot][kvh][Tmax][d], v8t [slot][kvh][tile][d][128]."""
    t = c.t
    if _VIEWS.get("case") is not c or _VIEWS["v8t"] is not t["v8t"]:              # one entry: the reference and a case's mutants share the decode
        k8 = torch.from_numpy(MX.e4m3_decode(t["k8"].numpy()).astype(np.float64))
        v8 = torch.from_numpy(MX.e4m3_decode(t["v8t"].numpy()).astype(np.float64))   # [slot][kvh][tile][d][128]
        _VIEWS.update(case=c, v8t=t["v8t"], views=(k8, v8))
    return _VIEWS["views"]


def f_dec(c, dt, mutant=None, pinned=True):
    p, t, T = c.p, c.t, c.dtype
    M, nq, nkv, d, Tmax, kv8 = p["M"], p["nq"], p["nkv"], p["d"], p["Tmax"], p["kv8"]
    G, half = nq // nkv, d // 2
    scale32 = float(np.float32(p["scale"]))
    x = _slab_sum(c, F64, mutant)                                               # exact (dyadic), whatever dt
    xq, xk, xv = x[:, :nq * d].view(M, nq, d), x[:, nq * d:(nq + nkv) * d].view(M, nkv, d), x[:, (nq + nkv) * d:].view(M, nkv, d)
    out = torch.zeros(M, nq, d, dtype=dt)
    tol = torch.zeros(M, nq, d, dtype=F64) if (dt == F64 and mutant is None) else None
    k_rows, v_rows = torch.zeros(M, nkv, d, dtype=F64), torch.zeros(M, nkv, d, dtype=F64)
    k_mag = torch.zeros(M, nkv, d, dtype=F64)
    pmark = torch.full((M, nq), NAN, dtype=F64)                                   # marked family: the weight of every head's marked key
    e2 = torch.zeros(M, nq, dtype=F64)                                            # the second largest un-normalised weight of every head
    rises = torch.zeros(M, nq, dtype=F64)                                         # _rises of every head: chunks that raise one wave's maximum (+ 1: combine)
    spread = torch.zeros(M, nq, dtype=F64)                                        # largest - smallest maximum among the waves that hold keys
    if kv8:
        k8v, v8v = _kv8_views(c)
        ksc, vsc = t["ksc"].to(F64), t["vsc"].to(F64)
        new = dict(k8=t["k8"].clone(), v8t=t["v8t"].clone(), ksc=t["ksc"].clone(), vsc=t["vsc"].clone())
    else:
        new = dict(kc=t["kc"].clone(), vc=t["vc"].clone())
    hk = torch.arange(nq) // G
    for r in range(M):
        ln = int(t["lens"][r])
        slot = r if mutant == "slot_is_row" else int(t["slots"][r])
        cs = t["rope"][max(ln - 1, 0) if mutant == "rope_pos_minus_1" else ln].to(F64)
        il = mutant == "rope_interleaved"
        kn = _rt(_rope_pinned(xk[r], cs, il), T)                                 # [nkv, d]
        qr = _rt(_rope_pinned(xq[r], cs, il), T)
        qs = qr * scale32 if mutant == "q_scale_unrounded" else _rt(_f32(qr * scale32), T)
        vn = _rt(_rope_pinned(xv[r], cs), T) if mutant == "v_rotated" else xv[r]
        k_rows[r], v_rows[r] = kn, vn
        x1a, x2a = xk[r][:, :half].abs(), xk[r][:, half:].abs()                  # lower half x1 cos - x2 sin, upper half x2 cos + x1 sin
        k_mag[r] = torch.cat([x1a * cs[:, 0].abs() + x2a * cs[:, 1].abs(), x2a * cs[:, 0].abs() + x1a * cs[:, 1].abs()], -1)
        at = max(ln - 1, 0) if mutant == "append_at_len_minus_1" else ln
        extra = ln + 1 < Tmax and mutant == "reads_row_past_len"
        rows = list(range(ln)) + ([ln + 1] if extra else [])
        if kv8:
            qk8, ks_ = MX.kv8_quantize(kn.to(F32).numpy())
            qv8, vs_ = MX.kv8_quantize(vn.to(F32).numpy())
            new["k8"][slot, :, at] = torch.from_numpy(qk8)
            new["ksc"][slot, :, at], new["vsc"][slot, :, at] = torch.from_numpy(ks_), torch.from_numpy(vs_)
            new["v8t"][slot, :, at >> 7, :, at & 127] = torch.from_numpy(qv8)
            kn8, vn8 = torch.from_numpy(MX.e4m3_decode(qk8).astype(np.float64)), torch.from_numpy(MX.e4m3_decode(qv8).astype(np.float64))
            ri = torch.tensor(rows, dtype=torch.long)
            Kc = k8v[slot][:, ri]                                                # [nkv, n, d] codes
            if mutant == "v_tile_untransposed":                                  # the tile [d][128] read as [128][d]
                flat = v8v[slot].reshape(nkv, -1, d * 128)
                Vc = torch.stack([flat[:, j >> 7, (j & 127) * d + torch.arange(d)] for j in rows], 1) if rows else torch.zeros(nkv, 0, d, dtype=F64)
            else:
                Vc = v8v[slot][:, ri >> 7, :, ri & 127]                          # [n, nkv, d] -> below
                Vc = Vc.permute(1, 0, 2) if rows else torch.zeros(nkv, 0, d, dtype=F64)
            si = (ri - 1).clamp(min=0) if mutant == "scale_of_wrong_token" else ri
            sk, sv = ksc[slot][:, si], vsc[slot][:, si]
            if mutant == "k_v_scales_swapped":
                sk, sv = sv, sk
            nk_s, nv_s = torch.from_numpy(ks_.astype(np.float64))[:, None], torch.from_numpy(vs_.astype(np.float64))[:, None]
            # the new key sits at index len, a leaked row after it
            Kc, Vc = torch.cat([Kc[:, :ln], kn8[:, None], Kc[:, ln:]], 1), torch.cat([Vc[:, :ln], vn8[:, None], Vc[:, ln:]], 1)
            sk, sv = torch.cat([sk[:, :ln], nk_s, sk[:, ln:]], 1), torch.cat([sv[:, :ln], nv_s, sv[:, ln:]], 1)
            K, V = Kc * sk[..., None], Vc * sv[..., None]
        else:
            new["kc"][slot, :, at], new["vc"][slot, :, at] = kn.to(T), vn.to(T)
            ri = torch.tensor(rows, dtype=torch.long)
            Kc, Vc = t["kc"][slot][:, ri].to(F64), t["vc"][slot][:, ri].to(F64)
            K, V = torch.cat([Kc[:, :ln], kn[:, None], Kc[:, ln:]], 1), torch.cat([Vc[:, :ln], vn[:, None], Vc[:, ln:]], 1)
        n = K.shape[1]
        vis = torch.ones(n, dtype=torch.bool)
        if mutant == "new_key_unseen" and ln > 0:
            vis[ln] = False
        groups = _dec_groups(c, n)
        if dt == F32:
            q32 = qs.to(F32)[:, None, :]                                         # [nq, 1, d]
            if kv8:
                s = (q32 @ Kc[hk].to(F32).transpose(-1, -2)) * sk[hk].to(F32)[:, None, :]
                sv32 = sv[hk].to(F32)
                o = _flash(s, Vc[hk].to(F32), groups, lambda pv, idx: _rt(pv * sv32[:, None, idx], BF16, F32), torch.exp)
            else:
                s = q32 @ K[hk].to(F32).transpose(-1, -2)
                o = _flash(s, V[hk].to(F32), groups, (lambda pv, idx: pv) if T == F32 else (lambda pv, idx: _rt(pv, T, F32)), torch.exp)
            out[r] = _rt(o[:, 0], T, F32)
            continue
        s = (qs[:, None, :] @ K[hk].transpose(-1, -2)).masked_fill(~vis, -math.inf)      # [nq, 1, n]
        m = s.amax(-1, keepdim=True)
        if mutant == "wave_record_unshifted" and len(groups) > 1:
            e = torch.zeros_like(s)
            for ch in groups:
                if ch:
                    idx = torch.cat(ch)
                    e[..., idx] = torch.exp(s[..., idx] - s[..., idx].amax(-1, keepdim=True))
        else:
            e = torch.exp(s - m)
        l = e.sum(-1, keepdim=True)
        if mutant == "empty_wave_counted" and len(groups) > 1:
            kt = 256 if kv8 else 128
            nk = n - (n - 1) // kt * kt
            l = l + (len(groups) - (nk + 31) // 32) * torch.exp(-m)
        o = (e @ V[hk]) / l
        out[r] = o[:, 0]
        if tol is not None:
            qk = qs.abs()[:, None, :] @ K[hk].abs().transpose(-1, -2)
            flip = 0.0 if (pinned or p["rope"] == "dyadic") else 2 * U[T] * qk
            es_x = flip + (2 * E * s.abs() if kv8 else 0.0)
            tr = _softmax_tol(T, o, s, qk, vis[None, None], V[hk].abs(), d, groups, extra_es=es_x, extra_A=E if kv8 else 0.0)
            if p["exact"]:
                tr = 4 * E * o.abs() if T == F32 else torch.zeros_like(o)
            tol[r] = tr[:, 0]
            if n > 1:
                e2[r] = e[:, 0].sort(-1).values[:, -2]
            rises[r] = _rises(s, groups)[:, 0]
            wm = torch.stack([s[:, 0, torch.cat(ch)].amax(-1) for ch in groups if ch])
            spread[r] = wm.amax(0) - wm.amin(0)
            mk = p["marks"][r]
            pmark[r] = torch.where(mk >= 0, (e / l)[:, 0].gather(-1, mk.clamp(min=0)[:, None])[:, 0], pmark[r])
    outs = {"out": out.view(M, nq * d), **new}
    aux = None
    if tol is not None:
        aux = dict(out=tol.view(M, nq * d), k_rows=k_rows, v_rows=v_rows, k_mag=k_mag, pmark=pmark, e2=e2, rises=rises, spread=spread)
    return outs, aux


FAMILIES = {"seg": f_seg, "dec": f_dec}
MUTANTS = {"seg": ("causal_strict", "causal_plus_one", "causal_by_tile", "last_key_dropped", "segment_leak", "no_rescale", "kv_head_modulo",
                   "pv_key_order", "scale_missing", "query_clamped_row_written"),
           "dec": ("new_key_unseen", "append_at_len_minus_1", "rope_pos_minus_1", "rope_interleaved", "v_rotated", "bias_missing",
                   "slab_clamped_counted", "wave_record_unshifted", "empty_wave_counted", "reads_row_past_len", "slot_is_row", "q_scale_unrounded"),
           "kv8": ("k_v_scales_swapped", "scale_of_wrong_token", "v_tile_untransposed"),
           "mx": ("scale_wrong_ktile", "quantises_unrounded_output")}


def evaluate(c: Case, dt=F64, mutant=None):
    """Outputs as the device buffers hold them: `out` in dt (rounded to storage by the fp32 emulation only), caches in their storage types.
    With p["mx"]: out8 / sout of the MXFP8 copy as well (of T(out); the mx mutants change only these)."""
    mx_mut = mutant if mutant in MUTANTS["mx"] else None
    outs = FAMILIES[c.family](c, dt, None if mx_mut else mutant)[0]
    if c.p.get("mx"):
        y = outs["out"] if mx_mut == "quantises_unrounded_output" else _rt(outs["out"], c.dtype, F32)
        q, s = MX.quantize(y.to(F32).numpy())
        rows, H = q.shape
        s = s.reshape(rows, H // 128, 4).transpose(1, 0, 2)
        if mx_mut == "scale_wrong_ktile":
            s = np.roll(s, 1, axis=0)
        sy = np.full((H // 128, c.p["srows"], 4), SENT_B, dtype=np.uint8)
        sy[:, :rows] = s
        outs["out8"], outs["sout"] = torch.from_numpy(q.copy()), torch.from_numpy(sy)
    return outs


def reference(c: Case, pinned=True):
    """(outputs, tolerances) in float64, computed once per (case, pinned) and never modified. pinned: the kernel's rotation is the pinned fma
    form (decode_attn_flash2_kernel); it matters for the `random` decode family (real table) only."""
    if c._ref is None:
        c._ref = {}
    key = bool(pinned) or c.family == "seg" or c.p["rope"] == "dyadic"
    if key not in c._ref:
        outs, aux = FAMILIES[c.family](c, F64, None) if c.family == "seg" else f_dec(c, F64, None, pinned=key)
        ref = {"out": outs["out"]}
        if c.p["exact"] and c.dtype != F32:
            ref["out"] = _rt(ref["out"], c.dtype)
        c._ref[key] = (ref, aux)
    return c._ref[key]


def _bits(what, got, want):
    g, w = got.contiguous(), want.contiguous()
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[g.element_size()]
    bad = int((g.view(view) != w.to(g.dtype).view(view)).sum())
    return (what, float("inf") if bad else 0.0, bad, True)


def check(c: Case, outs: Dict[str, torch.Tensor], pinned=True):
    """[(output, worst error / bound, elements over the bound, all owned elements finite)] of a candidate's outputs (CPU tensors, the device
    buffers' shapes). Unowned elements of `out` must still hold their NaN sentinel; caches are compared over ALL their bytes."""
    ref, aux = reference(c, pinned)
    p, t, T = c.p, c.t, c.dtype
    exact = p["exact"] and T != F32
    rep = [_cmp("out", outs["out"].reshape(ref["out"].shape), ref["out"], None if exact else aux["out"])]
    if c.family == "dec":
        sl, ln = t["slots"].long(), t["lens"].long()
        if p["kv8"]:
            want = {k: t[k].clone() for k in ("k8", "v8t", "ksc", "vsc")}
            qk8, ks_ = MX.kv8_quantize(aux["k_rows"].to(F32).numpy())
            qv8, vs_ = MX.kv8_quantize(aux["v_rows"].to(F32).numpy())
            want["k8"][sl, :, ln] = torch.from_numpy(qk8)
            want["v8t"][sl, :, ln >> 7, :, ln & 127] = torch.from_numpy(qv8)
            want["ksc"][sl, :, ln], want["vsc"][sl, :, ln] = torch.from_numpy(ks_), torch.from_numpy(vs_)
            for k in want:
                rep.append(_bits(k, outs[k].reshape(want[k].shape), want[k]))
            shp = lambda k: outs[k].reshape(want[k].shape)
            stored = {"k8": (shp("k8")[sl, :, ln], shp("ksc")[sl, :, ln]), "v8t": (shp("v8t")[sl, :, ln >> 7, :, ln & 127], shp("vsc")[sl, :, ln])}
            for k, (got_q, got_s) in stored.items():                                  # the stored token, K and V, is a fixed point of the quantiser
                val = MX.kv8_dequantize(got_q.numpy(), got_s.numpy())
                bad = int((MX.kv8_dequantize(*MX.kv8_quantize(val)) != val).sum()) if np.isfinite(val).all() else val.size
                rep.append((k + "_fixed_point", float("inf") if bad else 0.0, bad, True))
        else:
            wk, wv = t["kc"].clone(), t["vc"].clone()
            wk[sl, :, ln], wv[sl, :, ln] = aux["k_rows"].to(T), aux["v_rows"].to(T)
            gk = outs["kc"].reshape(wk.shape)
            if not (pinned or p["rope"] == "dyadic"):                                 # unpinned rotation, real table: the K row within a flip
                rows = gk[sl, :, ln]
                rep.append(_cmp("k_rows", rows, aux["k_rows"], U[T] * aux["k_rows"].abs() + 4 * E * aux["k_mag"]))
                gk = gk.clone()
                gk[sl, :, ln] = wk[sl, :, ln]
            rep.append(_bits("kc", gk, wk))
            rep.append(_bits("vc", outs["vc"].reshape(wv.shape), wv))
    if p.get("mx"):
        y8, sy = _mx(c, outs["out"].reshape(p["M"], -1), p["srows"])
        rep.append(_cmp("out8", outs["out8"].reshape(y8.shape), y8, None))
        rep.append(_cmp("sout", outs["sout"].reshape(sy.shape), sy, None))
    return rep


def emulate(c: Case):
    """The reference alone: fp32 arithmetic in the kernel's order, outputs in the storage types."""
    outs = evaluate(c, F32)
    outs["out"] = outs["out"].to(c.dtype)
    return outs


def outside(rep):
    return any(n > 0 or not fin for _, _, n, fin in rep)


# ------------------------------------------------------------------------------------------------------------- segment cases
def _seg_layout(kind, D, heads, group, lens, gap, dtype):
    """Geometry of one case. packed: one [rows][3 heads D] buffer, segments `gap` rows apart, 64 spare rows at the end (the vision encoder's
    and the classifier's form). cache: q rows [rows][(heads + 2 kvh) D], K / V in a slot cache [slot][kvh][Tmax][D] (the prefill's form).
    Output rows are o_row = heads D + 8 apart: 8 sentinel elements after every row."""
    He, Hkv = heads * D, heads // group
    starts, a = [], 0
    for L in lens:
        starts.append(a)
        a += L + gap
    rows = a + 64
    o_row = He + 8
    p = dict(D=D, heads=heads, group=group, causal=kind == "cache", scale=float(np.float32(D ** -0.5)), kind=kind, gap=gap, out_rows=rows, o_row=o_row,
             o_head=D, rows=rows, exact=False)
    if kind == "packed":
        p.update(q_row=3 * He, q_head=D, k_row=3 * He, k_head=D)
        segs = [dict(L=L, q_off=s * 3 * He, k_off=s * 3 * He + He, v_off=s * 3 * He + 2 * He, o_off=s * o_row, tail=min((L + 63) // 64 * 64 - L, rows - s - L))
                for L, s in zip(lens, starts)]
    else:
        Tm = 208
        perm = torch.randperm(len(lens) + 2, generator=_gen(len(lens) + D)).tolist()
        p.update(q_row=(heads + 2 * Hkv) * D, q_head=D, k_row=D, k_head=Tm * D, Tmax=Tm, n_slots=len(lens) + 2, slots=perm[:len(lens)])
        segs = [dict(L=L, q_off=s * p["q_row"], k_off=sl * Hkv * Tm * D, v_off=sl * Hkv * Tm * D, o_off=s * o_row, tail=min((L + 63) // 64 * 64 - L, Tm - L))
                for L, s, sl in zip(lens, starts, perm)]
    own = torch.zeros(rows, o_row, dtype=torch.bool)
    for L, s in zip(lens, starts):
        own[s:s + L, :He] = True
    p.update(segs=segs, own=own, starts=starts, lens=list(lens))
    return p


def _seg_marks(L, causal):
    """(candidate keys, per query: the key that carries its weight, or -1 = a forbidden key's code)."""
    if causal:
        cand = sorted({j for j in (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, L - 1) if 0 <= j < L})
        mark = []
        for i in range(L):
            if i in cand and i % 5 != 1:
                mark.append(i)                                                   # the diagonal
            elif i + 1 in cand:
                mark.append(-(i + 1) - 1)                                        # forbidden: j = i + 1 (encoded as -(j) - 1)
            else:
                vis = [j for j in cand if j <= i]
                mark.append(vis[i % len(vis)])
        return cand, mark
    cand = sorted({j for j in (0, 62, 63, 64, 65, 126, 127, 128, 129, L - 2, L - 1) if 0 <= j < L})
    mark = [(-L - 1) if i % 7 == 3 else cand[i % len(cand)] for i in range(L)]       # forbidden: row L, the next segment's first key
    return cand, mark


def _seg_case(dtype, kind, family, D, heads, group, lens, seed):
    gap = 1 if family == "poison" else 0
    p = _seg_layout(kind, D, heads, group, lens, gap, dtype)
    g = _gen(seed)
    He, Hkv, rows = heads * D, heads // group, p["rows"]
    amp = {32: (2.0, 2.0), 64: (2.0, 1.25), 80: (2.0, 1.0), 128: (2.0, 1.0)}[D]
    if kind == "packed":
        buf = _rand(g, rows, 3, heads, D)
        qv, kv, vv = buf[:, 0], buf[:, 1], buf[:, 2]                             # views [rows, heads, D]
    else:
        qbuf = _rand(g, rows, heads + 2 * Hkv, D)
        kc, vc = _rand(g, p["n_slots"], Hkv, p["Tmax"], D), _rand(g, p["n_slots"], Hkv, p["Tmax"], D)
        qv = qbuf[:, :heads]
    redraws = 0
    for si, L in enumerate(lens):
        a = p["starts"][si]
        if kind == "packed":
            K, V = kv[a:a + L + p["segs"][si]["tail"]], vv[a:a + L + p["segs"][si]["tail"]]          # [Lx, heads, D]
        else:
            sl = p["slots"][si]
            K, V = kc[sl].permute(1, 0, 2), vc[sl].permute(1, 0, 2)                                  # [Tmax, Hkv, D] views
        Q = qv[a:a + L]
        if family == "uniform":
            Q.zero_()
            V[:] = (torch.randint(0, 4, V.shape, generator=g) * 2 - 3).to(F64)
        elif family in ("marked", "spike"):
            K[:] = _dyadic(g, *K.shape, lim=8, step=2.0 ** -6)
            if family == "marked":
                cand, mark = _seg_marks(L, kind == "cache")
                ids = {j: (si % 2 if j == 0 else 2 + n) for n, j in enumerate(cand)}
                for j in cand:
                    K[j] = amp[1] * _code(ids[j], D)
                if kind == "packed" and L < K.shape[0]:
                    K[L] = amp[1] * _code((si + 1) % 2, D)                       # the next segment's first key (set again, identically, by that segment)
                mk_t = torch.empty(L, heads, dtype=torch.long)
                for i in range(L):
                    for h in range(heads):
                        mk = mark[(i + h) % L] if kind == "packed" else mark[i]
                        code = ((si + 1) % 2) if (mk < 0 and kind == "packed") else ids[-mk - 1 if mk < 0 else mk]
                        Q[i, h] = amp[0] * _code(code, D)
                        mk_t[i, h] = max(mk, -1)
                p["segs"][si]["marks"] = mk_t                                     # the key that carries the query's weight; -1: a forbidden key's code
            else:
                qa, ka = {32: (2.0, 1.0), 64: (1.0, 1.375), 80: (1.0, 1.25), 128: (1.0, 1.0)}[D]
                for j, mult in ((5, 1.0), (70, 2.0), (L - 1, 3.0)):
                    if 0 <= j < L:
                        K[j] = mult * ka * _code(3, D)
                Q[:] = qa * _code(3, D)
    if kind == "packed":
        t = dict(q=buf.reshape(rows, 3 * He))
        if family == "poison":
            for si, L in enumerate(lens):
                t["q"][p["starts"][si] + L:(p["starts"][si + 1] if si + 1 < len(lens) else rows)] = NAN
        t["q"] = _st(t["q"], dtype)
        t["k"] = t["v"] = t["q"]
    else:
        if family == "poison":
            qbuf[:, heads:] = NAN
            for si, L in enumerate(lens):
                kc[p["slots"][si], :, L:], vc[p["slots"][si], :, L:] = NAN, NAN
                qbuf[p["starts"][si] + L:(p["starts"][si + 1] if si + 1 < len(lens) else rows)] = NAN
            spare = [s for s in range(p["n_slots"]) if s not in p["slots"]]
            kc[spare], vc[spare] = NAN, NAN
        t = dict(q=_st(qbuf.reshape(rows, -1), dtype), k=_st(kc, dtype), v=_st(vc, dtype))
    p["exact"] = family == "uniform"
    p["family"] = family
    causal = kind == "cache"
    kills = {"random": ("scale_missing", "pv_key_order", "query_clamped_row_written") + (("kv_head_modulo",) if group > 1 else ()),
             "uniform": ("last_key_dropped", "query_clamped_row_written") + (("causal_strict", "causal_plus_one", "causal_by_tile") if causal else ("segment_leak",)),
             "marked": ("last_key_dropped", "scale_missing") + (("causal_strict", "causal_plus_one", "causal_by_tile") if causal else ("segment_leak",)),
             "spike": ("no_rescale", "scale_missing"), "poison": ("query_clamped_row_written",) + (() if causal else ("segment_leak",))}[family]
    kern = f"attn_valu_kernel<float, {D}>" if dtype == F32 else f"attn_mfma_kernel<{DT_NAME[dtype]}, {D}>"
    c = Case("seg", f"seg-{kind}-{family}-D{D}-h{heads}g{group}", dtype, p, t, kills, kern)
    if family == "uniform" and dtype != F32:
        c.redraws = _redraw_seg(c, g)
    return c


def _redraw_seg(c, g):
    """Redraw the V column of every output element whose exact value lies within 2^-20 of a rounding boundary of T."""
    p, n = c.p, 0
    D, H, G = p["D"], p["heads"], p["group"]
    for _ in range(40):
        o = f_seg(c, F64)[0]["out"]
        bad = p["own"] & ~_far(torch.nan_to_num(o), c.dtype)
        if not bool(bad.any()):
            return n
        for si, sg in enumerate(p["segs"]):
            a, L = p["starts"][si], sg["L"]
            cols = bad[a:a + L, :H * D].any(0).view(H, D)
            cols = cols.view(H // G, G, D).any(1)                                # per kv head
            for kvh, dd in cols.nonzero().tolist():
                col = _strided(c.t["v"], sg["v_off"], L, p["k_row"], H // G, p["k_head"], D)[:, kvh, dd]
                col.copy_((torch.randint(0, 4, (L,), generator=g) * 2 - 3).to(c.dtype))
                n += 1
    raise AssertionError("uniform segment case: redraws do not converge")


def seg_cases() -> List[Case]:
    """Lengths 1 .. 200 of SEG_LENS in one buffer (the 32-query half of a wave, the 64-query tile, the 64-key chunk, four chunks at 200).
    packed (non-causal, group 1): random at every D; uniform, marked, spike, poison at D = 80 (third 32-wide block half used) and one other D.
    cache (causal GQA, D = 128, 10 query / 2 kv heads, K / V strided as a slot cache): every family."""
    out = []
    for dtype in DTYPES:
        for i, D in enumerate((32, 64, 80, 128)):
            out.append(_seg_case(dtype, "packed", "random", D, (2, 3, 4, 2)[i], 1, SEG_LENS, 10 + D))
        for fam, Ds in (("uniform", (80, 32)), ("marked", (80, 64)), ("spike", (80, 128)), ("poison", (80, 32))):
            for D in Ds:
                out.append(_seg_case(dtype, "packed", fam, D, 2, 1, SEG_LENS, 20 + D + len(fam)))
        for fam in ("random", "uniform", "marked", "spike", "poison"):
            out.append(_seg_case(dtype, "cache", fam, 128, 10, 5, SEG_LENS, 30 + len(fam)))
    return out


# ------------------------------------------------------------------------------------------------------------- decode cases
def dyadic_rope(Tmax, d, seed, identity=False):
    """[Tmax][d / 2][2] (cos, sin) on the 2^-3 grid: not a rotation, the kernels do not care; every fp32 product and sum of the rotation is exact."""
    if identity:
        return torch.stack([torch.ones(Tmax, d // 2), torch.zeros(Tmax, d // 2)], -1).float().contiguous()
    return (torch.randint(-8, 9, (Tmax, d // 2, 2), generator=_gen(seed)).float() / 8).contiguous()


def _dec_marks(ln):
    cand = sorted({j for j in (0, 31, 32, 63, 64, 95, 96, 127, 128, 255, 256, ln - 1) if 0 <= j < ln})
    return cand


_BASE = {}


def _base_cache(dtype, d, n_slots):
    """Random caches shared (read-only) by the random cases of one (dtype, d)."""
    if (dtype, d) not in _BASE:
        g = _gen(1000 + d)
        _BASE[(dtype, d)] = (_st(_rand(g, n_slots, 2, TMAX, d), dtype), _st(_rand(g, n_slots, 2, TMAX, d), dtype))
    return _BASE[(dtype, d)]


def _dec_case(dtype, family, d, G, S, seed, kv8=False, mx=False, real_rope=True):
    nkv, nq, M, Tmax = 2, 2 * G, len(DEC_LENS), TMAX
    n_slots = M + SPARE_SLOTS
    g = _gen(seed)
    qkv_d = (nq + 2 * nkv) * d
    slots = torch.randperm(n_slots, generator=g)[:M].to(torch.int32)
    lens = torch.tensor(DEC_LENS, dtype=torch.int32)
    rope_kind = "real" if (family == "random" and not kv8 and real_rope) else "dyadic"
    rope = rope_cs_table(Tmax, d, dtype) if rope_kind == "real" else dyadic_rope(Tmax, d, seed, identity=family in ("marked", "spike"))
    x = _dyadic(g, M, nq + 2 * nkv, d)                                           # |x| <= 4 on the 2^-5 grid
    if family in ("random", "poison") and not kv8:
        kc, vc = _base_cache(dtype, d, n_slots)
        if family == "poison":
            kc, vc = kc.clone(), vc.clone()
    else:
        kc, vc = _rand(g, n_slots, nkv, Tmax, d), _rand(g, n_slots, nkv, Tmax, d)
    if kv8:                                                                      # token-dependent magnitudes: the scales differ between tokens and between K and V
        j = torch.arange(Tmax)
        kc, vc = kc * (2.0 ** (j % 3 - 2))[None, None, :, None], vc * (2.0 ** ((j + 1) % 4 - 1))[None, None, :, None]
    qa, ka = {32: (2.0, 2.0), 64: (2.0, 1.25), 128: (2.0, 1.0)}[d]
    marks = torch.full((M, nq), -2, dtype=torch.long)                            # marked family: the key that carries the weight; -1: the forbidden row len + 1
    if family == "uniform":
        x[:, :nq] = 0.0
        x[:, nq + nkv:] = (torch.randint(0, 2, (M, nkv, d), generator=g) * 2 - 1).to(F64) * (1 + 2 * torch.randint(0, 2, (M, nkv, d), generator=g)).to(F64)
        vc = (torch.randint(0, 4, vc.shape, generator=g) * 2 - 3).to(F64)
    elif family in ("marked", "spike"):
        kc = _dyadic(g, n_slots, nkv, Tmax, d, lim=8, step=2.0 ** -6)
        x[:, nq:nq + nkv] = _dyadic(g, M, nkv, d, lim=4, step=2.0 ** -5)
        for r, ln in enumerate(DEC_LENS):
            sl = int(slots[r])
            if family == "marked":
                cand = _dec_marks(ln)
                ids = {j: n for n, j in enumerate(cand)}
                new_id, fb_id = len(cand), len(cand) + 1
                for j in cand:
                    kc[sl, :, j] = ka * _code(ids[j], d)
                x[r, nq:nq + nkv] = ka * _code(new_id, d)
                if ln + 1 < Tmax:
                    kc[sl, :, ln + 1] = ka * _code(fb_id, d)
                for h in range(nq):
                    sel = (h + r) % (len(cand) + 2)
                    fb = sel == len(cand) + 1 and ln + 1 < Tmax
                    code = fb_id if fb else (new_id if sel >= len(cand) else ids[cand[sel]])
                    x[r, h] = qa * _code(code, d)
                    marks[r, h] = -1 if fb else (ln if sel >= len(cand) else cand[sel])
            else:
                qs, ks = {32: (2.0, 1.0), 64: (1.0, 1.375), 128: (1.0, 1.0)}[d]
                # wave 0 rises in its second tile (key 130 of the 128-key tiles, key 260 of the KV8 kernel's 256-key tiles), the last key tops all
                for j, mult in ((5, 1.0), (40, 2.0), (130, 2.0)) + (((260, 2.0),) if kv8 else ()) + ((ln - 1, 3.0),):
                    if 0 <= j < ln:
                        kc[sl, :, j] = mult * ks * _code(3, d)
                if ln == 0:
                    x[r, nq:nq + nkv] = ks * _code(3, d)
                x[r, :nq] = qs * _code(3, d)
    kc, vc = _st(kc, BF16 if kv8 else dtype), _st(vc, BF16 if kv8 else dtype)
    if family == "poison" and not kv8:
        for r, ln in enumerate(DEC_LENS):
            kc[int(slots[r]), :, ln:], vc[int(slots[r]), :, ln:] = NAN, NAN
        spare = [s for s in range(n_slots) if s not in slots.tolist()]
        kc[spare], vc[spare] = NAN, NAN
    # bias + slabs on the dyadic grid, summing to x exactly
    bias = _dyadic(g, qkv_d, lim=64)
    slabs = _dyadic(g, 8, M, qkv_d, lim=200)
    slabs[S - 1] = x.reshape(M, qkv_d) - bias[None] - slabs[:S - 1].sum(0)
    slabs[S:] = NAN
    assert torch.equal((bias[None] + slabs[:S].float().sum(0).to(F64)).to(dtype).to(F64), x.reshape(M, qkv_d))
    p = dict(M=M, nq=nq, nkv=nkv, d=d, Tmax=Tmax, S=S, scale=float(np.float32(d ** -0.5)), n_slots=n_slots, kv8=kv8, mx=mx, srows=M + 3,
             rope=rope_kind, exact=family == "uniform", family=family, marks=marks)
    t = dict(part=slabs.float(), bias=_st(bias, BF16 if kv8 else dtype), kc=kc, vc=vc, slots=slots, lens=lens, rope=rope)
    if kv8:
        _kv8_arrays(p, t, poison=family == "poison")
    kills = {"random": ("rope_pos_minus_1", "rope_interleaved", "v_rotated", "bias_missing", "slot_is_row", "append_at_len_minus_1", "empty_wave_counted",
                        "reads_row_past_len") + (("slab_clamped_counted",) if S in (1, 3, 5, 7) else ()),
             "uniform": ("new_key_unseen", "empty_wave_counted", "reads_row_past_len", "slot_is_row"),
             "marked": ("new_key_unseen", "reads_row_past_len", "slot_is_row"),
             "spike": ("wave_record_unshifted",),
             "poison": ("reads_row_past_len", "slot_is_row", "append_at_len_minus_1")}[family]
    if family == "random" and dtype == BF16 and d == 128 and G >= 5 and not kv8:
        kills += ("q_scale_unrounded",)
    if kv8:
        if family in ("random", "poison"):
            kills += ("k_v_scales_swapped", "scale_of_wrong_token", "v_tile_untransposed")
    if mx:
        kills += ("quantises_unrounded_output",) + (("scale_wrong_ktile",) if nq * d > 128 else ())
    if dtype == F32 and not kv8:                                                 # one group of chunks: no records to combine
        kills = tuple(k for k in kills if k not in ("wave_record_unshifted", "empty_wave_counted"))
    kern = "decode_attn_kv8_kernel" if kv8 else ("decode_attn_mfma_kernel" if dtype == F32 else "decode_attn_flash2_kernel / decode_attn_flash_kernel")
    c = Case("dec", f"{'kv8' if kv8 else 'dec'}-{family}-d{d}-G{G}-S{S}" + ("-mx" if mx else "") + ("" if real_rope else "-dyadic"), dtype, p, t, kills, kern)
    if family == "uniform" and dtype != F32:
        c.redraws = _redraw_dec(c, g)
    return c


def _kv8_arrays(p, t, poison):
    """The KV8 arrays of the bf16 caches: tokens < row_len of every active slot quantised (oracle/mx_oracle.py), everything else zero (what
    RecModel allocates) or, poisoned, NaN in K / k scales and huge finite values in V^T / v scales (module text). tok_slot / tok_pos list
    the quantised tokens for surya_op_kv8_quant_rows."""
    n_slots, nkv, Tmax, d = p["n_slots"], p["nkv"], p["Tmax"], p["d"]
    T8 = (Tmax + 255) & ~255
    k8 = torch.full((n_slots, nkv, Tmax, d), 0x7f if poison else 0, dtype=torch.uint8)
    v8t = torch.full((n_slots, nkv, T8 // 128, d, 128), 0x7e if poison else 0, dtype=torch.uint8)
    ksc = torch.full((n_slots, nkv, T8), NAN if poison else 0.0, dtype=F32)
    vsc = torch.full((n_slots, nkv, T8), 1024.0 if poison else 0.0, dtype=F32)
    ts, tp = [], []
    for r, ln in enumerate(t["lens"].tolist()):
        sl = int(t["slots"][r])
        if ln == 0:
            continue
        qk, sk = MX.kv8_quantize(t["kc"][sl, :, :ln].float().numpy())
        qv, sv = MX.kv8_quantize(t["vc"][sl, :, :ln].float().numpy())
        k8[sl, :, :ln] = torch.from_numpy(qk)
        ksc[sl, :, :ln], vsc[sl, :, :ln] = torch.from_numpy(sk), torch.from_numpy(sv)
        j = torch.arange(ln)
        v8t[sl][:, j >> 7, :, j & 127] = torch.from_numpy(qv).permute(1, 0, 2)
        ts += [sl] * ln
        tp += list(range(ln))
    p["Tmax8"] = T8
    t.update(k8=k8, v8t=v8t, ksc=ksc, vsc=vsc, tok_slot=torch.tensor(ts, dtype=torch.int32), tok_pos=torch.tensor(tp, dtype=torch.int32))


def _redraw_dec(c, g):
    p, t, n = c.p, c.t, 0
    G, d, nkv = p["nq"] // p["nkv"], p["d"], p["nkv"]
    for _ in range(40):
        o = f_dec(c, F64)[0]["out"]
        bad = ~_far(o, c.dtype)
        if not bool(bad.any()):
            return n
        cols = bad.view(p["M"], nkv, G, d).any(2)
        for r, kvh, dd in cols.nonzero().tolist():
            ln, sl = int(t["lens"][r]), int(t["slots"][r])
            new = (torch.randint(0, 4, (ln,), generator=g) * 2 - 3).to(F64)
            t["vc"][sl, kvh, :ln, dd] = new.to(t["vc"].dtype)
            if p["kv8"]:
                _kv8_arrays(p, t, poison=False)
            n += 1
    raise AssertionError("uniform decode case: redraws do not converge")


HEAD_SHAPES = ((128, 5), (128, 6), (128, 8), (64, 4), (32, 2), (128, 1))


def dec_cases() -> List[Case]:
    """All 25 contexts of DEC_LENS in every case (Tmax = 400, one row per context, slots a permutation with 3 spare slots). random: every head
    shape of the ladders under the model's RoPE table, slab counts 1, 2, 3, 4, 5, 7 spread over them (8 slabs in a poison case), and two of
    them again under a dyadic table, where decode_attn_flash_kernel, decode_attn_mfma_kernel and the KV8 kernel carry no flip term. The other families at d = 128 G = 5 (the recogniser's) and at one or two smaller
    shapes."""
    out = []
    for dtype in DTYPES:
        for i, (d, G) in enumerate(HEAD_SHAPES):
            out.append(_dec_case(dtype, "random", d, G, (3, 1, 2, 4, 5, 7)[i], 100 + i, mx=dtype == BF16 and (d, G) in ((128, 5), (64, 4), (32, 2))))
        for i, (d, G) in enumerate(((128, 5), (64, 4))):                           # the same data under a dyadic table: no flip term in any kernel
            out.append(_dec_case(dtype, "random", d, G, (4, 7)[i], 150 + i, real_rope=False))
        for fam, shapes in (("uniform", ((128, 5), (64, 4), (32, 2))), ("marked", ((128, 5), (128, 8), (32, 2))), ("spike", ((128, 5), (64, 4))),
                            ("poison", ((128, 5), (128, 6), (32, 2)))):
            for i, (d, G) in enumerate(shapes):
                out.append(_dec_case(dtype, fam, d, G, (8, 2, 1)[i] if fam == "poison" else (2, 3, 1)[i], 200 + 10 * len(fam) + i))
    return out


def kv8_cases() -> List[Case]:
    """decode_attn_kv8_kernel (bf16 model path): d = 128 G = 5 and d = 64 G = 4; random (with the MXFP8 copy), uniform, marked, poison; late
    spike at d = 128 (its eight-wave combine and the rescale between its 256-key tiles)."""
    out = []
    for i, (d, G) in enumerate(((128, 5), (64, 4))):
        for j, fam in enumerate(("random", "uniform", "marked", "poison") + (("spike",) if d == 128 else ())):
            out.append(_dec_case(BF16, fam, d, G, (3, 1, 2, 5, 4)[j], 300 + 10 * i + j, kv8=True, mx=fam == "random"))
    return out


_CASES = None


def all_cases() -> List[Case]:
    """Built once per process and shared: the cases and their inputs are never modified."""
    global _CASES
    if _CASES is None:
        _CASES = seg_cases() + dec_cases() + kv8_cases()
    return _CASES
