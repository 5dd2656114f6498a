"""GPU: every non-GEMM kernel of the recognition engine alone, through its op-level entry point (surya_op_rec_*: the launch code RecModel
itself uses), in fp32, bf16 and fp16, against float64 under a bound that follows from the arithmetic (tests/rec_ops_ref.py: the cases, the
references, the bounds). The model-level tests hold these kernels to 2e-3 on a probability and 3e-2 x max on features through whole
networks 128 and 256 wide: an unsummed split-K slab, a norm over 4 x threads elements, a tie that goes to the later tile, a sum-exp that is
not rescaled, an unclamped row_len, a cache row in the neighbouring kv head or a scale byte in the wrong K-tile fits inside that, and the
thread geometries of dec_hidden = 1280 are never reached.

Every output buffer is filled with NaN (or a sentinel where the kernel writes part of it) before the call and sits between two guard bands
of a known value; afterwards the guards must be untouched and EVERY element is held to the bound. The worst error / bound ratio of every
output is printed (`RECOPS` lines)."""
import ctypes as C

import numpy as np
import pytest
import torch

import rec_ops_ref as R
from surya_amd import _lib as L
from test_gpu_lay_ops import Bufs

pytestmark = pytest.mark.gpu

CASES = R.all_cases()
DT = {torch.float32: L.DTYPE_F32, torch.bfloat16: L.DTYPE_BF16, torch.float16: L.DTYPE_F16}
I32, U8, F32 = torch.int32, torch.uint8, torch.float32


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(t):
    return None if t is None else t.cuda().contiguous()


def _p(t):
    return None if t is None else t.data_ptr()


@pytest.fixture
def knobs(hip_lib):
    """Set tuning knobs for one call; whatever a test set is back at its default afterwards."""
    defaults = {b"rnorm": 2, b"ghead": 2}

    def set_(key, value):
        L.check(hip_lib.surya_set_tuning(key, C.c_int(value)), "surya_set_tuning")
    yield set_
    for k, v in defaults.items():
        L.check(hip_lib.surya_set_tuning(k, C.c_int(v)), "surya_set_tuning")


def _mx_bufs(b, p, rows):
    if not p["mx"]:
        return None, None
    return b.out((rows, p["H"]), U8, fill=R.SENT_B), b.out((p["H"] // 128, p["srows"], 4), U8, fill=R.SENT_B)


def run_rms(lib, c, b, knobs):
    p = c.p
    x, w, src = _dev(c.t["x"]), _dev(c.t["w"]), _dev(c.t["src_row"])
    y = b.out((p["rows"], p["C"]), c.dtype)
    rc = lib.surya_op_rec_rmsnorm_rows(DT[c.dtype], _p(x), p["ldx"], _p(w), _p(y), p["C"], _p(src), p["rows"], p["C"], p["eps"], _stream())
    return rc, {"y": y}


def run_reduce(lib, c, b, knobs):
    p = c.p
    knobs(b"rnorm", p["rnorm"])
    part, w = _dev(c.t["part"]), _dev(c.t["w"])
    x = b.out((p["M"], p["H"]), c.dtype, init=c.t["x"].cuda())
    y = b.out((p["M"], p["H"]), c.dtype) if w is not None else None
    y8, sy = _mx_bufs(b, p, p["M"])
    rc = lib.surya_op_rec_reduce_norm(DT[c.dtype], _p(part), p["S"], p["M"], _p(x), _p(w), _p(y), p["H"], p["eps"], _p(y8), _p(sy), p["srows"], _stream())
    outs = {"x": x}
    if y is not None:
        outs["y"] = y
    if y8 is not None:
        outs.update(y8=y8, sy=sy)
    return rc, outs


def run_embed(lib, c, b, knobs):
    p = c.p
    knobs(b"ghead", p["ghead"])
    table, nt, act, kv, w = (_dev(c.t[k]) for k in ("table", "next_token", "active", "kv_len", "w"))
    rows = act.shape[0]
    row_len = b.out((rows,), I32, fill=R.SENT_I)
    x, y = b.out((rows, p["H"]), c.dtype), b.out((rows, p["H"]), c.dtype)
    y8, sy = _mx_bufs(b, p, rows)
    rc = lib.surya_op_rec_decode_embed(DT[c.dtype], _p(table), _p(nt), _p(act), _p(kv), p["Tmax"], _p(row_len), _p(x), _p(w), _p(y), rows, p["H"],
                                       p["eps"], _p(y8), _p(sy), p["srows"], _stream())
    torch.cuda.synchronize()
    assert torch.equal(nt.cpu(), c.t["next_token"]) and torch.equal(kv.cpu(), c.t["kv_len"]), "an input was written"
    outs = {"row_len": row_len, "x": x, "y": y}
    if y8 is not None:
        outs.update(y8=y8, sy=sy)
    return rc, outs


def run_head(lib, c, b, knobs):
    p, t = c.p, c.t
    knobs(b"ghead", p["ghead"])
    M, H, S = p["M"], p["H"], R.SLOTS
    d = {k: _dev(t[k]) for k in ("part", "hidden", "wb", "bb", "row_slot", "table", "wnorm", "forced_table", "flogit")}
    o = dict(out_token=b.out((S,), I32, fill=R.SENT_I), out_score=b.out((S,), F32, fill=R.SENT_F), out_bbox=b.out((S, 6), I32, fill=R.SENT_I),
             next_token=b.out((S,), I32, fill=R.SENT_I), kv_len=b.out((S,), I32, init=t["kv_len"].cuda()))
    a = L.RecHeadArgsC()
    for k in ("part", "hidden", "wb", "bb", "row_slot"):
        setattr(a, k, _p(d[k]))
    a.tiles_n, a.rows, a.H, a.eos_id, a.pad_id, a.len_inc = p["tiles_n"], M, H, p["eos"], p["pad"], p["len_inc"]
    a.max_kv_len, a.srows, a.bbox_size, a.eps = p["Tmax"], p["srows"], float(p["bbox_size"]), p["eps"]
    if p["alts"]:
        o["best_tot"] = b.out((S, 2), F32, fill=R.SENT_F)
        a.best_tot = _p(o["best_tot"])
    if p["fused"]:
        o.update(row_len=b.out((M,), I32, fill=R.SENT_I), x=b.out((M, H), c.dtype), y=b.out((M, H), c.dtype))
        a.table, a.wnorm, a.x, a.y, a.row_len = _p(d["table"]), _p(d["wnorm"]), _p(o["x"]), _p(o["y"]), _p(o["row_len"])
        y8, sy = _mx_bufs(b, p, M)
        if y8 is not None:
            o.update(y8=y8, sy=sy)
            a.y8, a.sy = _p(y8), _p(sy)
    if p["forced"]:
        o.update(greedy_token=b.out((S,), I32, fill=R.SENT_I), greedy_prob=b.out((S,), F32, fill=R.SENT_F), logprob=b.out((S,), F32, fill=R.SENT_F),
                 cursor=b.out((S,), I32, init=t["cursor"].cuda()))
        a.forced_table, a.forced_cursor, a.flogit, a.forced_stride = _p(d["forced_table"]), _p(o["cursor"]), _p(d["flogit"]), p["stride"]
        a.greedy_token, a.greedy_prob, a.logprob = _p(o["greedy_token"]), _p(o["greedy_prob"]), _p(o["logprob"])
    for k in ("out_token", "out_score", "out_bbox", "next_token", "kv_len"):
        setattr(a, k, _p(o[k]))
    rc = lib.surya_op_rec_head(DT[c.dtype], C.byref(a), _stream())
    torch.cuda.synchronize()
    return rc, o


def run_ropekv(lib, c, b, knobs):
    p = c.p
    ts, tp, rope = _dev(c.t["tok_slot"]), _dev(c.t["tok_pos"]), _dev(c.t["rope"])
    qkv = b.out(tuple(c.t["qkv"].shape), c.dtype, init=c.t["qkv"].cuda())
    kc = b.out((p["slots"], p["nkv"], p["Tmax"], p["D"]), c.dtype, fill=5.0)
    vc = b.out((p["slots"], p["nkv"], p["Tmax"], p["D"]), c.dtype, fill=5.0)
    rc = lib.surya_op_rec_rope_kv_append(DT[c.dtype], _p(qkv), _p(ts), _p(tp), _p(rope), _p(kc), _p(vc), qkv.shape[0], p["nq"], p["nkv"], p["D"],
                                         p["Tmax"], _stream())
    return rc, {"qkv": qkv, "kc": kc, "vc": vc}


def run_table(lib, c, b, knobs):
    p = c.p
    f, pos = _dev(c.t["inv_freq"]), _dev(c.t["pos_hw"])
    if p["kind"] == "decoder":
        tab = b.out((p["Tmax"], p["half"], 2), F32)
        rc = lib.surya_op_rec_rope_table(DT[c.dtype], L.REC_ROPE_DECODER, None, _p(f), _p(tab), p["Tmax"], p["half"], _stream())
    else:
        tab = b.out((p["P"], p["D"] // 2, 2), F32)
        rc = lib.surya_op_rec_rope_table(DT[c.dtype], L.REC_ROPE_VISION, _p(pos), _p(f), _p(tab), p["P"], p["D"], _stream())
    return rc, {"table": tab}


def run_rows(lib, c, b, knobs):
    p, k, t = c.p, c.p["kind"], c.t
    src, s2, s3, i1, i2, i3 = (_dev(t.get(n)) for n in ("src", "src2", "src3", "index", "index2", "index3"))
    if k == "convert_tiles":
        dst, kind, dims = b.out((p["P"], p["kout"]), c.dtype), L.REC_CONVERT_TILES, [p["P"], p["kin"], p["kout"]]
    elif k == "scatter_image":
        dst, kind, dims = b.out((p["dst_rows"], p["H"]), c.dtype), L.REC_SCATTER_IMAGE, [len(t["index"]), p["H"]]
    elif k == "scatter_rows":
        dst, kind, dims = b.out((p["dst_rows"], p["H"]), c.dtype), L.REC_SCATTER_ROWS, [len(t["index"]), p["H"]]
    else:
        dst, kind, dims = b.out((len(t["index"]), p["H"]), c.dtype), L.REC_EMBED_TOKENS, [len(t["index"]), p["H"]]
    d = np.asarray(dims, dtype=np.int32)
    rc = lib.surya_op_rec_rows(DT[c.dtype], kind, _p(dst), _p(src), _p(s2), _p(s3), _p(i1), _p(i2), _p(i3), L.np_ptr(d), _stream())
    return rc, {"dst": dst}


RUN = {"rms": run_rms, "reduce": run_reduce, "embed": run_embed, "head": run_head, "ropekv": run_ropekv, "table": run_table, "rows": run_rows}


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_kernel_alone_vs_float64(hip_lib, knobs, case):
    b = Bufs()
    rc, outs = RUN[case.family](hip_lib, case, b, knobs)
    assert rc == 0, rc
    b.check_guards()
    rep = R.check(case, {k: v.cpu() for k, v in outs.items()})
    for what, ratio, over, finite in rep:
        print(f"RECOPS {case.family} | {case.kernel} | {R.DT_NAME[case.dtype]} | {case.name} | {what} | {ratio:.3g}")
    bad = [(what, ratio, over, finite) for what, ratio, over, finite in rep if over or not finite]
    assert not bad, f"{case.id} [{case.kernel}]: (output, worst error / bound, elements over the bound, finite): {bad}"


def test_refusals(hip_lib, knobs):
    """What the launch code refuses comes back as an error code before anything is launched; surya_op_rmsnorm keeps its own refusals."""
    x = torch.zeros(8192, device="cuda")
    p, s = x.data_ptr(), _stream()
    f16, f32, bf = L.DTYPE_F16, L.DTYPE_F32, L.DTYPE_BF16
    assert hip_lib.surya_op_rmsnorm(f16, L.ptr(x), C.c_long(64), L.ptr(x), L.ptr(x), C.c_long(64), 1, 64, C.c_float(1e-6), C.c_void_p(s)) == L.SA_ERR_UNSUPPORTED
    assert hip_lib.surya_op_rec_rmsnorm_rows(7, p, 64, p, p, 64, None, 1, 64, 1e-6, s) == L.SA_ERR_UNSUPPORTED
    assert hip_lib.surya_op_rec_reduce_norm(f32, p, 9, 1, p, None, None, 64, 1e-6, None, None, 0, s) == L.SA_ERR_ARG
    assert hip_lib.surya_op_rec_reduce_norm(f32, p, 1, 1, p, None, None, 4100, 1e-6, None, None, 0, s) == L.SA_ERR_UNSUPPORTED
    assert hip_lib.surya_op_rec_reduce_norm(f32, p, 1, 1, p, None, None, 66, 1e-6, None, None, 0, s) == L.SA_ERR_UNSUPPORTED
    assert hip_lib.surya_op_rec_reduce_norm(f16, p, 1, 1, p, p, p, 128, 1e-6, p, p, 8, s) == L.SA_ERR_UNSUPPORTED      # MXFP8 beside bf16 only
    assert hip_lib.surya_op_rec_reduce_norm(bf, p, 1, 1, p, p, p, 160, 1e-6, p, p, 8, s) == L.SA_ERR_SHAPE
    assert hip_lib.surya_op_rec_decode_embed(f32, p, p, p, p, 8, p, p, p, p, 1, 130, 1e-6, None, None, 0, s) == L.SA_ERR_SHAPE
    assert hip_lib.surya_op_rec_decode_embed(f32, p, p, p, p, 8, p, p, p, p, 1, 128, 1e-6, p, p, 8, s) == L.SA_ERR_UNSUPPORTED
    d = np.asarray([1, 6], dtype=np.int32)
    assert hip_lib.surya_op_rec_rows(bf, L.REC_SCATTER_ROWS, p, p, None, None, p, None, None, L.np_ptr(d), s) == L.SA_ERR_SHAPE
    assert hip_lib.surya_op_rec_rows(bf, 9, p, p, None, None, p, None, None, L.np_ptr(d), s) == L.SA_ERR_ARG
    assert hip_lib.surya_op_rec_rope_table(f32, L.REC_ROPE_VISION, p, p, p, 4, 30, s) == L.SA_ERR_SHAPE
    a = L.RecHeadArgsC()
    for k in ("part", "hidden", "wb", "bb", "row_slot", "out_token", "out_score", "out_bbox", "next_token", "kv_len", "table", "wnorm", "x", "y", "row_len"):
        setattr(a, k, p)
    a.tiles_n, a.rows, a.H, a.max_kv_len = 4 * R.HEAD_THREADS + 1, 1, 128, 8
    assert hip_lib.surya_op_rec_head(f32, C.byref(a), s) == L.SA_ERR_STATE          # the fallback head has no fused embedding
    knobs(b"ghead", 1)
    a.tiles_n = 4
    assert hip_lib.surya_op_rec_head(f32, C.byref(a), s) == L.SA_ERR_STATE
    torch.cuda.synchronize()
