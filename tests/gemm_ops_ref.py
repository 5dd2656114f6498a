"""Test infrastructure: the GEMM itself -- gemm_nt_kernel in every tile and staging launch_gemm / launch_gemm_splitk can pick, the persistent
8-phase loop gemm_nt_p8p_kernel and the loader / consumer ring gemm_ring_kernel (csrc/gemm.h, csrc/gemm_ring.h) -- through surya_op_gemm,
surya_op_rec_gemm_f16, surya_op_gemm_splitk_bf16 / _f16 and surya_op_gemm_rope: the cases, float64 references in plain torch, the per-element
bound each output is held to, and the mutants the bounds must catch. Built like attn_ops_ref.py / ocr_ops_ref.py (whose grid generator,
_round64, _step and _cmp are used here, not restated).

A Case carries the operands exactly as the device gets them (rounded to the storage type, row pads included), the parameters of one call,
the tuning knobs that select its arm (`knobs`; everything else at DEFAULTS), the arm's name, the kernel route() expects launch_gemm to pick
under those knobs (route() restates the launcher's choice in Python; tests/test_gemm_ops_cpu.py holds every case's kernel to its arm's
`expect`), and the mutants it must kill.
evaluate(case, dt, mutant):  dt = float64 the reference; dt = float32 "the reference alone": fp32 accumulation over K, K-tile by K-tile, in
fp32, rounded where the kernel rounds; mutant = a name: a deliberately wrong float64 evaluation (MUTANTS).
check(case, outs) holds EVERY element to its bound; the pad columns of C and the slabs past the slice count must keep their sentinel.
No term of any bound was fitted to a measured error. Symbols: T the storage type of C, u its relative step (bf16 2^-7, fp16 2^-10,
fp32 2^-23), E = 2^-24, K the reduction length, A = |x| |W|^T + |b|.

GRID data (ocr_ops_ref.py's grid: x multiples of 2^-4 in [-2, 2], W of 2^-6 in [-1/4, 1/4], bias of 2^-6 in [-1, 1], R on x's grid): every
    product is a multiple of 2^-10, every partial sum below 2^11 up to K = 3072 -- the fp32 accumulators of the MFMAs (gemm.h SA_FRAGS /
    Mfma<T>::run, `acc[j][i]`) hold the exact sum in any order, and the bias addition (`v[r] += b[r]`, gemm.h epilogue, line 1165) is exact.
    bias / no bias / ReLU (`fmaxf(v[r], 0.f)`, line 1175) / fp32 output: the store's rounding of the exact number (store4, line 1206): BIT FOR BIT.
    residual: the staged tile holds T(x W^T + b) (store4 into LDS, line 1206), the read-back adds R in fp32 and rounds once more
        (`a[e] + r[e]`, line 1296; the persistent loop: its second pass, gemm.h lines 1778 ff.): T(T(x W^T + b) + R), the second sum exact too:
        BIT FOR BIT, C aliasing R included (each thread reads its own 16 bytes of R before it stores them, lines 1271-1277).
    split-K slab ks: the exact partial product over K-tiles [ks nk / S, (ks + 1) nk / S) (gemm.h lines 417-418), raw fp32 (line 1287): BIT FOR BIT.
    GELU / SwiGLU / Hardswish: got = T(f + d') with |d'| <= d against want = T(f): one storage step of want plus d, d = the absolute error of the
        epilogue's function before the store:
        GELU      ocr_ops_ref.py's d, from common.h gelu_epi (lines 254-279): fp16 0 (the projection rounded to fp16 first, as the reference
                  does; erfc to 1.2e-7 relative); bf16 0.5 |x| 1.5e-7 + 2^-21 |g|; fp32 2^-23 |x| + 2^-22 |g|.
        SwiGLU    silu_epi (common.h lines 234-238): x * rcp(1 + __expf(-x)) (fp32: x / (1 + __expf(-x))), then `silu * v[1]` (gemm.h line
                  1201). __expf = ONE hardware exp2 of -x log2 e: relative error (|x| + 4) 2^-23 (attn_ops_ref.py's e_exp); it enters
                  sigma = 1 / (1 + e) with weight e / (1 + e) = 1 - sigma. The sum 1 + e rounds by E, v_rcp_f32 is good to 1 ulp = 2 E
                  (a correctly rounded division is within that), the two products round by E each:
                  d = |silu(g) up| ((1 - sigma(g)) (|g| + 4) 2^-23 + 5 E).
        Hardswish hardswish_f (common.h lines 287-291): t = clamp(fma(x, fl(1/6), 0.5)), x * t. fl(1/6) is off by <= E relative: |x| E / 6;
                  the fma rounds a value <= |x| / 6 + 1/2 by E; the product rounds by E |h|:  d = E (|x| (|x| / 3 + 1/2) + |h|).
RANDOM full-mantissa data (unit-variance x, W / sqrt K, unit-variance bias and R, each rounded to the storage type once): the grid's 5-6
    mantissa bits would not show an operand truncated on its way to the MFMA. e_lin = 2 (K + 4) E A, lay_ops_ref.py's linear-op bound: every
    term passes at most K roundings of relative size E in any summation order; the factor 2 and the + 4 cover the MFMA's own grouping of its
    16 (bf16 / fp16) or 2 (fp32) products, the bias addition and an fp32 store.
    bias / no bias / ReLU (1-Lipschitz): u |ref| + e_lin; fp32 output and slabs (over the slab's own K range): e_lin alone.
    residual: the inner rounding T(pre) may flip against the reference's: + u |pre|; fp32 output: the second sum rounds once more, + E |ref|.
    GELU: |gelu'| <= 1.13: u |ref| + 1.13 e_lin + d (fp16: its input rounding may flip, + 1.13 u |pre|).
    Hardswish: |h'| = |2 x + 3| / 6 <= 1.5: u |ref| + 1.5 e_lin + d.
    SwiGLU: |silu'| <= 1.1: u |ref| + 1.1 e_g |up| + |silu(g)| e_up + 1.1 e_g e_up + d.
    fp16 outputs below 2^-14 are stored as subnormals, spacing 2^-24 whatever their size: + 2^-24 (as attn_ops_ref.py has it).
ROPE (surya_op_gemm_rope, gemm.h lines 1178-1190 and 1711 ff.): grid operands, so x = T(x W^T + b) is exact and rounded once (Ty<TO>::rnd, line 1184);
    columns n < rope_cols in pairs (2j, 2j + 1) of each rope_D-wide head, (cos, sin) = rope[m][(n % D) / 2] from random angles (fp32):
    out0 = fma(x0, cos, -fl(x1 sin)), out1 = fma(x1, cos, fl(x0 sin)) (lines 1188-1189): one rounded product (E |x1 sin|) and one fused
    multiply-add (E |out| <= E (|x0 cos| + |x1 sin|)), then the store: u |ref| + 2 E (|x0 cos| + |x1 sin|) (+ 2^-24 in fp16, as above).
    Columns >= rope_cols: T(x W^T + b) BIT FOR BIT.
Pads: C is [M][ldc]; columns >= N (N / 2 after SwiGLU) keep SENT; slabs >= the returned slice count keep SENT.
Not a conftest; never imported by the product."""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch

from ocr_ops_ref import DT_NAME, E, F32, F64, U, _cmp, _gen, _grid, _round64, _step

BF16, F16 = torch.bfloat16, torch.float16
SENT = -7.0
EPI_BIAS, EPI_RESIDUAL, EPI_GELU, EPI_SWIGLU, EPI_HARDSWISH, EPI_RELU = range(6)
# epilogue names of the matrix -> (epilogue code, bias, C aliases R, fp32 output)
EPIS = {"bias": (EPI_BIAS, True, False, False), "nobias": (EPI_BIAS, False, False, False), "residual": (EPI_RESIDUAL, True, False, False),
        "residual_inplace": (EPI_RESIDUAL, True, True, False), "gelu": (EPI_GELU, True, False, False), "swiglu": (EPI_SWIGLU, False, False, False),
        "swiglu_bias": (EPI_SWIGLU, True, False, False), "hardswish": (EPI_HARDSWISH, True, False, False), "relu": (EPI_RELU, True, False, False),
        "f32out": (EPI_BIAS, True, False, True)}
ALL_EPIS = tuple(EPIS)
EPIS_16 = tuple(e for e in ALL_EPIS if e != "f32out")              # arms that exist for 16-bit outputs only
DEFAULTS = dict(bigtile=3, bigtile_any=0, persist=1, glds=2, gateup_ring=2, dring=1, dring_min_kt=0, big_m_split=-1, big_m_gateup=-1)
SPLIT_TARGET, SPLIT_MIN_KT, SPLIT_MAX = 256, 4, 8                  # sa::Tuning split_target / split_min_kt / split_max (common.h): never changed here
SLAB_CAP = 8

MUTANTS = {"gemm": ("last_k_chunk_dropped", "odd_tail_tile_skipped", "bias_shifted_4_columns", "last_column_chunk_from_clamped_address",
                    "residual_before_rounding", "row_stride_ignored", "gate_up_swapped", "tile_row_written_twice", "operand_truncated_to_10_bits"),
           "splitk": ("slice_boundary_off_by_one_tile", "last_k_chunk_dropped", "odd_tail_tile_skipped", "row_stride_ignored", "tile_row_written_twice"),
           "rope": ("half_split_pairing", "sine_sign_flipped", "projection_unrounded", "column_past_rope_cols_rotated", "row_angles_of_previous_row")}


@dataclass
class Case:
    family: str                           # gemm | splitk | rope
    name: str
    dtype: torch.dtype
    p: dict
    t: Dict[str, Optional[torch.Tensor]]
    knobs: dict
    arm: str
    kernel: str
    kills: Tuple[str, ...] = ()
    _ref: Optional[tuple] = field(default=None, repr=False)

    @property
    def id(self):
        return f"{self.name}-{DT_NAME[self.dtype]}"

    @property
    def key(self):
        """The problem without the knobs: cases that differ in knobs only share inputs, reference and bound."""
        p = self.p
        return (self.family, self.dtype, p["M"], p["N"], p["K"], p.get("epi_name"), p["data"], p["ldx"] != p["K"], p.get("D"), p.get("bm"))


def cdiv(a, b):
    return (a + b - 1) // b


def ke(dtype):
    """Elements of one 128-byte K-tile."""
    return 32 if dtype == F32 else 64


# ------------------------------------------------------------------------------------------------------------- the launcher's choice, restated
def _ring_mode(M, t):
    d = t["dring"]
    if not (d & 3) or M <= 0 or M > 256 or (M <= 128 and not (d & 4)):
        return 0
    return d & 3


def route(dtype, out_f32, epi, has_bias, M, N, K, knobs):
    """(kernel, BM, BN) launch_gemm<TI, TO, EPI> picks (gemm.h, the function's body) for the epilogues of this file."""
    t = dict(DEFAULTS, **knobs)
    i16 = dtype != F32
    o16 = i16 and not out_f32
    nk = K // ke(dtype)
    glu = epi == EPI_SWIGLU
    if M <= 256:
        if M > 128:
            if N >= 64 * 512:
                return "gemm_nt 128x128 glds2", 128, 128
            if glu and o16:
                mode = _ring_mode(M, t)
                if mode and not has_bias and N % 8 == 0:
                    return "gemm_ring 64x160" + (" nt" if mode == 2 else ""), 64, 160
            if glu and i16 and t["gateup_ring"] in (3, 4):
                return f"gemm_nt 64x64 glds{t['gateup_ring']}", 64, 64
            return "gemm_nt 64x64 glds2", 64, 64
        if M > 64:
            return ("gemm_nt 128x64", 128, 64) if N >= 64 * 128 else ("gemm_nt 128x32", 128, 32)
        return ("gemm_nt 64x64", 64, 64) if N >= 64 * 128 else ("gemm_nt 64x32", 64, 32)
    if glu and o16:
        mode, rb = t["big_m_gateup"], cdiv(M, 256)
        t256 = rb * cdiv(N, 256)
        pick = mode if mode >= 0 else (2 if (rb >= 4 and 160 <= t256 < 256) else 0)
        if pick and nk % 2 == 0 and nk >= 4 and N % 8 == 0:
            return ("gemm_nt_p8p", 256, 256) if pick == 1 else ("gemm_nt 256x256 8-phase", 256, 256)
    if N <= 64 and M >= 128 * 256:
        return "gemm_nt 128x64", 128, 64
    big = cdiv(M, 128) * cdiv(N, 128)
    if o16:
        bt = t["bigtile"]
        t256 = cdiv(M, 256) * cdiv(N, 256)
        cost256, cost128 = cdiv(t256, 256) * 256 * 4 / (1.4 if bt == 3 else 1.17), cdiv(big, 512) * 512
        if bt and ((t256 >= 256 and cost256 <= cost128) or t["bigtile_any"]):
            if t["persist"] and nk >= 4 and nk % 2 == 0 and N % 8 == 0:
                return "gemm_nt_p8p", 256, 256
            if bt == 2 and nk % 2 == 0:
                return "gemm_nt 256x256 4-wave", 256, 256
            if bt == 3 and nk % 2 == 0:
                return "gemm_nt 256x256 8-phase", 256, 256
            return "gemm_nt 256x256 2-stage", 256, 256
    if big >= 256:
        g = t["glds"]
        return f"gemm_nt 128x128 glds{g if g in (2, 3) else 0}", 128, 128
    return "gemm_nt 64x64", 64, 64


def pick_splitk(N, nk):
    """launch_gemm_splitk's slice count (gemm.h pick_splitk): a function of (N, K) only."""
    tiles = cdiv(N, 64) * 4
    s = (SPLIT_TARGET + tiles // 2) // tiles
    s = min(s, nk // SPLIT_MIN_KT)
    return max(1, min(s, SPLIT_MAX, 8))


def route_splitk(dtype, M, N, K, knobs):
    t = dict(DEFAULTS, **knobs)
    nk = K // ke(dtype)
    S = pick_splitk(N, nk)
    if M > 256:
        mode = t["big_m_split"]
        w128, w12864 = cdiv(M, 128) * cdiv(N, 128) * S, cdiv(M, 128) * cdiv(N, 64) * S
        pick = mode if mode >= 0 else (2 if w128 >= 136 else (3 if w12864 <= 256 else 0))
        if pick == 2:
            return "gemm_nt split 128x128 glds4", 128, 128, S
        if pick == 3:
            return "gemm_nt split 128x64 glds4", 128, 64, S
    mode = _ring_mode(M, t)
    if mode and t["dring_min_kt"] > 0 and nk // S >= t["dring_min_kt"]:
        return "gemm_ring split 64x64" + (" nt" if mode == 2 else ""), 64, 64, S
    return "gemm_nt split 64x64 glds4", 64, 64, S


# ------------------------------------------------------------------------------------------------------------- data
_RND = {}


def _rnd(key, shape, scale, dtype):
    """Shared among the cases (never modified): scale * N(0, 1), rounded to dtype once."""
    k = (key, tuple(shape), dtype, scale)
    if k not in _RND:
        g = _gen(zlib.crc32(repr((key, tuple(shape))).encode()))
        _RND[k] = (torch.randn(*shape, generator=g, dtype=F32).to(F64) * scale).to(F32).to(dtype)
    return _RND[k]


def _operands(data, dtype, M, N, K, ldx, ldw):
    """x [M][ldx], w [N][ldw] in the storage type; the pad columns hold values of the same kind (a stride mistake reads numbers, not NaN)."""
    if data == "grid":
        return _grid("gx", (M, ldx), 32, 16, dtype), _grid("gw", (N, ldw), 16, 64, dtype)
    return _rnd("rx", (M, ldx), 1.0, dtype), _rnd("rw", (N, ldw), 1.0 / math.sqrt(K), dtype)


_PROD = {}


def _prod(x, w, k0, k1, dt, KE, key=None):
    """x[:, k0:k1] w[:, k0:k1]^T. float64: one product; with a `key` (the case's own, never modified operands) it is shared by the cases that
    multiply the same operands (a small cache, emptied as it fills); float32: accumulated K-tile by K-tile in fp32."""
    if dt == F64:
        if key is None:
            return x[:, k0:k1].to(F64) @ w[:, k0:k1].to(F64).T
        k = (key, k0, k1, str(x.device))
        if k not in _PROD:
            if len(_PROD) >= 4:
                _PROD.clear()
            _PROD[k] = x[:, k0:k1].to(F64) @ w[:, k0:k1].to(F64).T
        return _PROD[k]
    acc = torch.zeros(x.shape[0], w.shape[0], dtype=F32, device=x.device)
    for a in range(k0, k1, KE):
        acc += x[:, a:min(a + KE, k1)].to(F32) @ w[:, a:min(a + KE, k1)].to(F32).T
    return acc


def _pkey(c, mutant, what):
    """Cache key of a product of the case's operands as they are (not for the mutants that change them)."""
    if mutant in ("row_stride_ignored", "operand_truncated_to_10_bits"):
        return None
    return (what, c.t["x"].data_ptr(), c.t["w"].data_ptr(), tuple(c.t["x"].shape), tuple(c.t["w"].shape), c.p["K"])


def _trunc10(v):
    """fp32 values with the low 13 mantissa bits cleared."""
    return (v.contiguous().view(torch.int32) & ~0x1FFF).view(F32)


def _rt(v, T, dt):
    """Round to T, back in dt (float64: one correctly rounded step)."""
    if dt == F64:
        return _round64(v, T) if v.device.type == "cpu" else v.to(F32).to(T).to(F64)
    return v.to(T).to(dt)


def _sigmoid(v):
    return 1.0 / (1.0 + torch.exp(-v))


def _gelu(v, erfc_form):
    if erfc_form:
        return 0.5 * v * torch.special.erfc(-v * math.sqrt(0.5))
    return 0.5 * v * (1.0 + torch.erf(v * math.sqrt(0.5)))


def _hardswish(v):
    return v * (v / 6.0 + 0.5).clamp(0.0, 1.0)


def _floor16(T):
    return 2.0 ** -24 if T == F16 else 0.0


# ------------------------------------------------------------------------------------------------------------- gemm
def f_gemm(c, dt, mutant=None, dev=None):
    p, T = c.p, c.dtype
    TO = F32 if p["out_f32"] else T
    M, N, K, KE, epi = p["M"], p["N"], p["K"], ke(T), p["epi"]
    mv = (lambda v: v.to(dev)) if dev else (lambda v: v)
    xf, wf = mv(c.t["x"]), mv(c.t["w"])
    x, w = xf[:, :K], wf[:, :K]
    if mutant == "row_stride_ignored":
        x = xf.reshape(-1)[:M * K].view(M, K)                       # rows read K apart
    if mutant == "operand_truncated_to_10_bits":
        x, w = _trunc10(x), _trunc10(w)
    k1 = K
    if mutant == "last_k_chunk_dropped":
        k1 = K - 8
    if mutant == "odd_tail_tile_skipped" and (K // KE) % 2 == 1:
        k1 = K - KE
    pre = _prod(x, w, 0, k1, dt, KE, _pkey(c, mutant, "v"))
    b = None
    if p["bias"]:
        b = mv(c.t["b"]).to(dt)
        if mutant == "bias_shifted_4_columns":
            b = torch.roll(b, -4)
        pre = pre + b
    want_tol = dt == F64 and mutant is None
    tol = None
    u = U[TO] if TO != F32 else 0.0
    e_lin = None
    if want_tol and p["data"] == "random":
        A = _prod(x.abs(), w.abs(), 0, K, F64, KE, _pkey(c, mutant, "abs"))
        if b is not None:
            A = A + b.abs()
        e_lin = 2 * (K + 4) * E * A
    if epi == EPI_BIAS or epi == EPI_RELU:
        v = pre.clamp(min=0.0) if epi == EPI_RELU else pre
        out = _rt(v, TO, dt)
        if e_lin is not None:
            tol = u * out.abs() + e_lin + _floor16(TO)
    elif epi == EPI_RESIDUAL:
        r = mv(c.t["r"])[:, :N].to(dt)
        inner = pre if mutant == "residual_before_rounding" else _rt(pre, TO, dt)
        out = _rt(inner + r, TO, dt)
        if e_lin is not None:
            tol = u * out.abs() + e_lin + u * pre.abs() + (E * out.abs() if TO == F32 else 0.0) + 2 * _floor16(TO)
    elif epi == EPI_GELU:
        xin = _rt(pre, T, dt) if T == F16 else pre
        if dt == F64:
            g = _gelu(xin, True)
            out = _rt(g, TO, dt)
            if want_tol:
                d = {F16: 0.0 * g, BF16: 0.5 * xin.abs() * 1.5e-7 + 2.0 ** -21 * g.abs(), F32: 2.0 ** -23 * xin.abs() + 2.0 ** -22 * g.abs()}[T]
                if e_lin is None:
                    tol = _step(out, TO) + d
                else:
                    tol = u * out.abs() + 1.13 * (e_lin + (U[F16] * pre.abs() if T == F16 else 0.0)) + d + _floor16(TO)
        else:
            out = _rt(_gelu(xin, T != F32), TO, dt)
    elif epi == EPI_HARDSWISH:
        h = _hardswish(pre)
        out = _rt(h, TO, dt)
        if want_tol:
            d = E * (pre.abs() * (pre.abs() / 3.0 + 0.5) + h.abs())
            tol = (_step(out, TO) + d) if e_lin is None else (u * out.abs() + 1.5 * e_lin + d + _floor16(TO))
    elif epi == EPI_SWIGLU:
        g, up = pre[:, 0::2], pre[:, 1::2]
        if mutant == "gate_up_swapped":
            g, up = up, g
        sg = _sigmoid(g)
        s = g * sg
        out = _rt(s * up, TO, dt)
        if want_tol:
            d = (s * up).abs() * ((1.0 - sg) * (g.abs() + 4.0) * 2.0 ** -23 + 5 * E)
            if e_lin is None:
                tol = _step(out, TO) + d
            else:
                eg, eu = e_lin[:, 0::2], e_lin[:, 1::2]
                tol = u * out.abs() + 1.1 * eg * up.abs() + s.abs() * eu + 1.1 * eg * eu + d + _floor16(TO)
    else:
        raise ValueError(epi)
    if mutant == "tile_row_written_twice":
        bm = p["bm"]
        n = min(bm, M - bm)
        out = out.clone()
        out[bm:bm + n] = out[:n]
    if mutant == "last_column_chunk_from_clamped_address":
        ch = 16 // (4 if TO == F32 else 2)
        out = out.clone()
        out[:, -ch:] = out[:, -2 * ch:-ch]
    return {"out": out}, {"out": tol}


# ------------------------------------------------------------------------------------------------------------- split-K
def _slices(nk, S, shifted=False):
    cut = [ks * nk // S for ks in range(S + 1)]
    if shifted:
        cut = [cut[0]] + [min(v + 1, nk) for v in cut[1:-1]] + [cut[-1]]
    return cut


def f_splitk(c, dt, mutant=None, dev=None):
    p, T = c.p, c.dtype
    M, N, K, KE, S = p["M"], p["N"], p["K"], ke(T), p["S"]
    mv = (lambda v: v.to(dev)) if dev else (lambda v: v)
    xf, wf = mv(c.t["x"]), mv(c.t["w"])
    x, w = xf[:, :K], wf[:, :K]
    if mutant == "row_stride_ignored":
        x = xf.reshape(-1)[:M * K].view(M, K)
    nk = K // KE
    cut = _slices(nk, S, mutant == "slice_boundary_off_by_one_tile")
    outs, tols = [], []
    for ks in range(S):
        k0, k1 = cut[ks] * KE, cut[ks + 1] * KE
        if ks == S - 1 and mutant == "last_k_chunk_dropped":
            k1 -= 8
        if ks == S - 1 and mutant == "odd_tail_tile_skipped" and nk % 2 == 1:
            k1 -= KE
        o = _prod(x, w, k0, k1, dt, KE, _pkey(c, mutant, "v"))
        if mutant == "tile_row_written_twice":
            bm = p["bm"]
            n = min(bm, M - bm)
            o = o.clone()
            o[bm:bm + n] = o[:n]
        outs.append(o if dt == F64 else o.to(dt))
        if dt == F64 and mutant is None and p["data"] == "random":
            tols.append(2 * (k1 - k0 + 4) * E * _prod(x.abs(), w.abs(), k0, k1, F64, KE))
    return {"part": torch.stack(outs)}, {"part": torch.stack(tols) if tols else None}


# ------------------------------------------------------------------------------------------------------------- rotary epilogue
def f_rope(c, dt, mutant=None, dev=None):
    p, T = c.p, c.dtype
    M, N, K, KE, D, RC = p["M"], p["N"], p["K"], ke(T), p["D"], p["rope_cols"]
    x, w = c.t["x"][:, :K], c.t["w"][:, :K]
    pre = _prod(x, w, 0, K, dt, KE, _pkey(c, mutant, "v")) + c.t["b"].to(dt)
    xr = pre if mutant == "projection_unrounded" else _rt(pre, T, dt)
    rope = c.t["rope"].to(dt)                                        # [M][D / 2][2]
    if mutant == "row_angles_of_previous_row":
        rope = torch.roll(rope, 1, 0)
    cols = N if mutant == "column_past_rope_cols_rotated" else RC
    n = torch.arange(cols)
    if mutant == "half_split_pairing":                                # (j, j + D / 2) of a head instead of (2 j, 2 j + 1)
        j = n % D
        first = j < D // 2
        partner = torch.where(first, n + D // 2, n - D // 2)
        pair = j % (D // 2)
    else:
        first = n % 2 == 0
        partner = torch.where(first, n + 1, n - 1)
        pair = (n % D) >> 1
    cos, sin = rope[:, pair, 0], rope[:, pair, 1]
    if mutant == "sine_sign_flipped":
        sin = -sin
    a, b = xr[:, :cols], xr[:, partner]
    sgn = torch.where(first, -1.0, 1.0).to(dt)
    bs = b * sin                                                      # one rounded product in the fp32 tier, then the fused multiply-add
    rot = a * cos + sgn * bs if dt == F64 else torch.addcmul(sgn * bs, a, cos)
    out = torch.cat([_rt(rot, T, dt), xr[:, cols:] if mutant != "projection_unrounded" else _rt(xr[:, cols:], T, dt)], 1)
    tol = None
    if dt == F64 and mutant is None:
        tol = torch.zeros_like(out)
        tol[:, :RC] = U[T] * out[:, :RC].abs() + 2 * E * ((a * cos).abs() + bs.abs()) + _floor16(T)
    return {"out": out}, {"out": tol}


FAMILIES = {"gemm": f_gemm, "splitk": f_splitk, "rope": f_rope}


def evaluate(c: Case, dt=F64, mutant=None, device=None):
    return FAMILIES[c.family](c, dt, mutant, device)[0]


def reference(c: Case, device=None, keep=True):
    """(outputs, tolerances) in float64; a tolerance of None = bit for bit; in a rope tolerance, 0 = bit for bit."""
    if c._ref is not None:
        return c._ref
    ref = FAMILIES[c.family](c, F64, None, device)
    if keep:
        c._ref = ref
    return ref


def emulate(c: Case):
    """The reference alone: fp32 arithmetic, rounded where the kernel rounds."""
    return evaluate(c, F32)


def out_dtype(c):
    return F32 if (c.family == "splitk" or c.p.get("out_f32")) else c.dtype


def check(c: Case, outs: Dict[str, torch.Tensor], device=None, keep=True):
    """[(what, worst error / bound, elements over the bound, all finite)] for a candidate's outputs: `out` as [M][n_out] or as the whole
    [M][ldc] buffer (its pad columns must hold SENT), `part` as [S][M][N] or the whole [SLAB_CAP][M][N] (slabs >= S must hold SENT)."""
    ref, tol = reference(c, device, keep)
    rep = []
    if c.family == "splitk":
        part = outs["part"]
        S = c.p["S"]
        if part.shape[0] > S:
            rep.append(("slabs_past_S", *_sent(part[S:])))
        rep.append(_cmp("part", part[:S], ref["part"], tol["part"]))
        return rep
    out, n_out = outs["out"], ref["out"].shape[1]
    if out.shape[1] > n_out:
        rep.append(("pad_columns", *_sent(out[:, n_out:])))
        out = out[:, :n_out]
    if c.family == "rope":                                            # the plain columns bit for bit, the rotated ones to their bound
        rc = c.p["rope_cols"]
        rep.append(_cmp("plain", out[:, rc:], ref["out"][:, rc:], None))
        rep.append(_cmp("rotated", out[:, :rc], ref["out"][:, :rc], tol["out"][:, :rc]))
        return rep
    rep.append(_cmp("out", out, ref["out"], tol["out"]))
    return rep


def _sent(v):
    bad = int((v.to(F64) != SENT).sum())
    return (float("inf") if bad else 0.0, bad, True)


def outside(rep):
    return any(over > 0 or not finite for _, _, over, finite in rep)


# ------------------------------------------------------------------------------------------------------------- the matrix
def hook_of(dtype, epi_name):
    """fp16: surya_op_gemm takes bias, residual, Hardswish, ReLU and GELU; SwiGLU and fp32 output go through surya_op_rec_gemm_f16."""
    if dtype == F16 and epi_name in ("swiglu", "swiglu_bias", "f32out"):
        return "rec_f16"
    return "op_gemm"


def n_for(epi_name, N):
    """SwiGLU halves the width and its output rows move in 16-byte chunks too: N such that N / 2 ends in ONE chunk past whole output tiles."""
    return GLU_N[N] if epi_name.startswith("swiglu") else N


GLU_N = {136: 144, 2024: 1936, 520: 528, 528: 528, 8200: 8208, 32776: 32784, 64: 64, 40: 48, 336: 336, 4104: 4112, 2824: 2832, 5704: 5712, 328: 336}


def make_gemm(arm, knobs, dtype, M, N0, nk, epi_name, data, strided=False, expect=None, kills=None, device_ref=False):
    epi, has_bias, inplace, out_f32 = EPIS[epi_name]
    N, K = n_for(epi_name, N0), nk * ke(dtype)
    TO = F32 if out_f32 else dtype
    n_out = N // 2 if epi == EPI_SWIGLU else N
    pad = 16 if strided else 0
    ldx, ldw, ldc = K + pad, K + 2 * pad, n_out + pad
    x, w = _operands(data, dtype, M, N, K, ldx, ldw)
    grid = data == "grid"
    t = dict(x=x, w=w, b=None, r=None)
    if has_bias:
        t["b"] = _grid("gb", (N,), 64, 64, dtype) if grid else _rnd("rb", (N,), 1.0, dtype)
    if epi == EPI_RESIDUAL:
        t["r"] = _grid("gr", (M, ldc), 32, 16, TO) if grid else _rnd("rr", (M, ldc), 1.0, TO)
    kernel, bm, bn = route(dtype, out_f32, epi, has_bias, M, N, K, knobs)
    if kills is None:
        kills = []
        if epi_name == "bias":
            kills.append("bias_shifted_4_columns")
            if grid and nk % 2 == 1 and nk >= 3:
                kills.append("odd_tail_tile_skipped")
        if epi_name == "nobias":
            kills += ["last_column_chunk_from_clamped_address", "last_k_chunk_dropped"]
            if not grid and dtype == F32:
                kills.append("operand_truncated_to_10_bits")
        if epi_name.startswith("residual") and grid and TO != F32:
            kills.append("residual_before_rounding")
        if epi_name.startswith("swiglu"):
            kills.append("gate_up_swapped")
        if epi_name == "relu" and M > bm:
            kills.append("tile_row_written_twice")
        if strided and M > 1:
            kills.append("row_stride_ignored")
    p = dict(M=M, N=N, K=K, nk=nk, epi=epi, epi_name=epi_name, bias=has_bias, inplace=inplace, out_f32=out_f32, ldx=ldx, ldw=ldw, ldc=ldc,
             ldr=ldc, data=data, hook=hook_of(dtype, epi_name), bm=bm, bn=bn, expect=expect, device_ref=device_ref)
    kn = "".join(f"-{k}{v}" for k, v in knobs.items())
    name = f"{arm}{kn}-M{M}-N{N}-kt{nk}-{epi_name}-{data}" + ("-ld" if strided else "")
    return Case("gemm", name, dtype, p, t, dict(knobs), arm, kernel, tuple(kills))


def _arm(out, arm, knobs, dtypes, shapes, epis, expect, strided_epi="residual"):
    """One arm: per dtype and shape every epilogue once on grid data and once on random data, the K-tile counts dealt round robin over the
    epilogues (every count at least once with the plain bias epilogue on grid data), and one strided case (ldx > K, ldw > K, ldc > N)."""
    for dtype in dtypes:
        for si, (M, N, nks) in enumerate(shapes):
            seen = set()
            for i, e in enumerate(epis):
                if e == "f32out" and dtype == F32:
                    continue
                for data, nk in (("grid", nks[i % len(nks)]), ("random", nks[(i + 1) % len(nks)])):
                    out.append(make_gemm(arm, knobs, dtype, M, N, nk, e, data, expect=expect))
                    if e == "bias" and data == "grid":
                        seen.add(nk)
            if "bias" in epis:
                for nk in nks:
                    if nk not in seen:
                        out.append(make_gemm(arm, knobs, dtype, M, N, nk, "bias", "grid", expect=expect))
            if si == 0:
                e = strided_epi if strided_epi in epis else epis[0]
                out.append(make_gemm(arm, knobs, dtype, M, N, nks[-1], e, "grid", strided=True, expect=expect))


D16 = (BF16, F16)
D3 = (F32, BF16, F16)
BIG = dict(bigtile_any=1)


def _expect_256(kind):
    """8-phase and 4-wave arms: odd K-tile counts fall back to the 2-stage tile on 8 waves, the persistent loop needs >= 4 even K-tiles."""
    def f(c):
        nk = c.p["nk"]
        if kind == "p8p":
            return "gemm_nt_p8p" if (nk >= 4 and nk % 2 == 0) else None
        if kind in ("8-phase", "4-wave"):
            return f"gemm_nt 256x256 {kind}" if nk % 2 == 0 else "gemm_nt 256x256 2-stage"
        return f"gemm_nt 256x256 {kind}"
    return f


def gemm_cases() -> List[Case]:
    out: List[Case] = []
    const = lambda s: (lambda c: s)
    # 64 x 64 register-staged, M > 256
    _arm(out, "t64", {}, D3, [(300, 136, (1, 3))], ALL_EPIS, const("gemm_nt 64x64"))
    # 128 x 128, three stagings (16-bit; fp32 in or out below)
    for g in (2, 3, 0):
        kn = dict(bigtile=0, glds=g)
        _arm(out, "t128", kn, D16, [(1930, 2024, (1, 2, 4, 5))], EPIS_16, const(f"gemm_nt 128x128 glds{g}"))
        for dtype in D16:                                            # 25 x 23 tiles: super-tile numbering on, ragged super-rows and super-columns
            out.append(make_gemm("t128", kn, dtype, 3080, 2824, 2, "bias", "grid", expect=const(f"gemm_nt 128x128 glds{g}"),
                                 kills=["bias_shifted_4_columns", "tile_row_written_twice"]))
    # 128 x 128 with fp32 in or out
    _arm(out, "t128f32", {}, (F32,), [(1930, 2024, (3,))], EPIS_16, const("gemm_nt 128x128 glds2"))
    _arm(out, "t128f32", {}, D16, [(1930, 2024, (3,))], ("f32out",), const("gemm_nt 128x128 glds2"))
    # 256 x 256: 2-stage on 8 waves, 2-stage on 4 waves, the 8-phase tile, the persistent 8-phase loop
    for arm, kn, nks, kind in (("t256", dict(bigtile=1, persist=0, **BIG), (1, 2, 3), "2-stage"), ("t256w4", dict(bigtile=2, persist=0, **BIG), (1, 2, 3), "4-wave"),
                               ("p8", dict(bigtile=3, persist=0, **BIG), (2, 4, 6), "8-phase"), ("p8p", dict(bigtile=3, persist=1, **BIG), (4, 6), "p8p")):
        _arm(out, arm, kn, D16, [(300, 520, nks)], EPIS_16, _expect_256(kind))
    # (the 4-wave tile takes even K-tile counts only -- launch_gemm, `bigtile == 2` -- so the table's 1 and 3 run the 8-wave tile under its knobs;
    # 2 and 4 K-tiles put every epilogue on the 4-wave tile itself)
    _arm(out, "t256w4", dict(bigtile=2, persist=0, **BIG), D16, [(300, 520, (2, 4))], EPIS_16, _expect_256("4-wave"))
    for arm, kn, M, N, nk, kind in (("t256", dict(bigtile=1, persist=0, **BIG), 4100, 4104, 3, "2-stage"), ("p8", dict(bigtile=3, persist=0, **BIG), 4100, 4104, 2, "8-phase"),
                                    ("p8p", dict(bigtile=3, persist=1, **BIG), 4100, 4104, 4, "p8p"), ("p8p", dict(bigtile=3, persist=1, **BIG), 5700, 5704, 4, "p8p")):
        out.append(make_gemm(arm, kn, BF16, M, N, nk, "bias", "grid", expect=_expect_256(kind), kills=["bias_shifted_4_columns", "tile_row_written_twice"],
                             device_ref=True))
    # odd K-tile counts under the 8-phase knobs take the 2-stage tile: same expectations
    for dtype in D16:
        for nk in (1, 3):
            out.append(make_gemm("p8", dict(bigtile=3, persist=0, **BIG), dtype, 300, 520, nk, "bias", "grid", expect=_expect_256("8-phase")))
    # big_m_gateup 1 and 2
    for mode, kern in ((1, "gemm_nt_p8p"), (2, "gemm_nt 256x256 8-phase")):
        _arm(out, f"biggu{mode}", dict(big_m_gateup=mode), D16, [(300, 528, (4, 6))], ("swiglu", "swiglu_bias"), const(kern), strided_epi="swiglu")
    # narrow output
    _arm(out, "narrow", {}, D3, [(32773, 64, (1,)), (32773, 40, (1,))], ALL_EPIS, const("gemm_nt 128x64"))
    # M <= 64, 64 < M <= 128
    for M in (1, 63):
        _arm(out, "m64", {}, D3, [(M, 136, (1, 3))], ALL_EPIS, const("gemm_nt 64x32"))
        _arm(out, "m64", {}, D3, [(M, 8200, (1, 3))], ALL_EPIS, const("gemm_nt 64x64"))
    _arm(out, "m128", {}, D3, [(100, 136, (1, 3))], ALL_EPIS, const("gemm_nt 128x32"))
    _arm(out, "m128", {}, D3, [(100, 8200, (1, 3))], ALL_EPIS, const("gemm_nt 128x64"))
    # 128 < M <= 256 (16-bit SwiGLU without a bias is the ring's: the decode gate|up arm below)
    m256 = lambda c: ("gemm_ring 64x160" if (c.p["epi_name"] == "swiglu" and c.dtype != F32) else "gemm_nt 64x64 glds2")
    _arm(out, "m256", {}, D3, [(200, 136, (1, 2, 3))], ALL_EPIS, m256)
    # (N = 32776 is the 128 x 128 direct-to-LDS tile of the "t128" arm at M <= 256: the epilogues that move data differently, not all ten again)
    _arm(out, "m256", {}, D3, [(200, 32776, (1, 2, 3))], ("bias", "nobias", "residual", "swiglu", "f32out"), const("gemm_nt 128x128 glds2"))
    # decode gate|up: the ring (dring 1, 2), the gemm_nt_kernel tiles with 2 / 3 / 4 stages (dring 0)
    for kn, kern in ((dict(dring=1), "gemm_ring 64x160"), (dict(dring=2), "gemm_ring 64x160 nt"), (dict(dring=0, gateup_ring=2), "gemm_nt 64x64 glds2"),
                     (dict(dring=0, gateup_ring=3), "gemm_nt 64x64 glds3"), (dict(dring=0, gateup_ring=4), "gemm_nt 64x64 glds4")):
        _arm(out, "gateup", kn, D16, [(200, 336, (1, 2, 5))], ("swiglu",), const(kern), strided_epi="swiglu")
    # dring = 5 at M = 63: launch_gemm asks the ring inside its M > 128 branch only, so this row is the 64 x 32 tile whatever dring says
    # (the +4 bit reaches launch_splitk_ring alone: the split-K arm below)
    _arm(out, "gateup", dict(dring=5), D16, [(63, 336, (1, 2, 5))], ("swiglu",), const("gemm_nt 64x32"), strided_epi="swiglu")
    return out


def make_splitk(knobs, dtype, M, N, nk, data, strided=False):
    K = nk * ke(dtype)
    pad = 16 if strided else 0
    ldx, ldw = K + pad, K + 2 * pad
    x, w = _operands(data, dtype, M, N, K, ldx, ldw)
    kernel, bm, bn, S = route_splitk(dtype, M, N, K, knobs)
    kills = ["slice_boundary_off_by_one_tile", "last_k_chunk_dropped"]
    if nk % 2 == 1:
        kills.append("odd_tail_tile_skipped")
    if M > bm:
        kills.append("tile_row_written_twice")
    if strided:
        kills.append("row_stride_ignored")
    p = dict(M=M, N=N, K=K, nk=nk, S=S, data=data, ldx=ldx, ldw=ldw, bm=bm, bn=bn, hook="splitk", device_ref=False, epi_name="slabs")
    kn = "".join(f"-{k}{v}" for k, v in knobs.items())
    return Case("splitk", f"splitk{kn}-M{M}-N{N}-kt{nk}-{data}" + ("-ld" if strided else ""), dtype, p, dict(x=x, w=w), dict(knobs), "splitk", kernel,
                tuple(kills))


SPLITK_ROWS = ((dict(), 63, "gemm_nt split 64x64 glds4"), (dict(), 200, "gemm_nt split 64x64 glds4"),
               (dict(dring_min_kt=4), 200, "gemm_ring split 64x64"), (dict(dring=5, dring_min_kt=4), 63, "gemm_ring split 64x64"),
               (dict(big_m_split=0), 320, "gemm_nt split 64x64 glds4"), (dict(big_m_split=2), 320, "gemm_nt split 128x128 glds4"),
               (dict(big_m_split=3), 320, "gemm_nt split 128x64 glds4"))


def splitk_cases() -> List[Case]:
    out = []
    for dtype in D16:
        for kn, M, kern in SPLITK_ROWS:
            for nk in (8, 27):
                for data in ("grid", "random"):
                    out.append(make_splitk(kn, dtype, M, 328, nk, data))
                    out[-1].p["expect"] = (lambda s: (lambda c: s))(kern)
            out.append(make_splitk(kn, dtype, M, 328, 27, "grid", strided=True))
            out[-1].p["expect"] = (lambda s: (lambda c: s))(kern)
    return out


ROPE_ROWS = (("t64", {}, 300, 3, D3, "gemm_nt 64x64"), ("t128", {}, None, 2, D3, "gemm_nt 128x128 glds2"),
             ("p8", dict(bigtile=3, persist=0, bigtile_any=1), 300, 2, D16, "gemm_nt 256x256 8-phase"),
             ("p8p", dict(bigtile=3, persist=1, bigtile_any=1), 300, 4, D16, "gemm_nt_p8p"))


def rope_cases() -> List[Case]:
    """D in {80, 32}, two heads: N = 3 heads D, rope_cols = 2 N / 3. The 128 x 128 tile needs 256 tiles of work: 8100 x 480 and 16300 x 192."""
    out = []
    for arm, knobs, M0, nk, dtypes, kern in ROPE_ROWS:
        for dtype in dtypes:
            for D in (80, 32):
                N = 3 * 2 * D
                M = M0 if M0 else (8100 if D == 80 else 16300)
                K = nk * ke(dtype)
                x, w = _operands("grid", dtype, M, N, K, K, K)
                g = _gen(zlib.crc32(repr(("angles", M, D)).encode()))
                ang = torch.rand(M, D // 2, generator=g, dtype=F64) * (2 * math.pi)
                rope = torch.stack([torch.cos(ang), torch.sin(ang)], -1).to(F32)
                t = dict(x=x, w=w, b=_grid("gb", (N,), 64, 64, dtype), rope=rope)
                kernel, bm, bn = route(dtype, False, EPI_BIAS, True, M, N, K, knobs)
                kills = ["half_split_pairing", "sine_sign_flipped", "column_past_rope_cols_rotated", "row_angles_of_previous_row"]
                if dtype != F32:
                    kills.append("projection_unrounded")
                p = dict(M=M, N=N, K=K, nk=nk, D=D, rope_cols=2 * N // 3, data="grid", ldx=K, ldw=K, ldc=N, bm=bm, bn=bn, hook="rope", device_ref=False,
                         expect=(lambda s: (lambda c: s))(kern), epi_name="rope")
                kn = "".join(f"-{k}{v}" for k, v in knobs.items())
                out.append(Case("rope", f"rope-{arm}{kn}-M{M}-D{D}-kt{nk}", dtype, p, t, dict(knobs), "rope-" + arm, kernel, tuple(kills)))
    return out


_CASES = None


def all_cases() -> List[Case]:
    """Built once per process and shared: the cases and their inputs are never modified."""
    global _CASES
    if _CASES is None:
        seen, _CASES = set(), []
        for c in gemm_cases() + splitk_cases() + rope_cases():
            if c.id not in seen:                                     # two rows of an arm may name the same case
                seen.add(c.id)
                _CASES.append(c)
    return _CASES
