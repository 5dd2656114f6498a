"""Test infrastructure: one-kernel plans for the detector engine and the per-element error bound they are held to.

A micro-plan is a DetPlan whose first op is INPUT with cin == cout == C, so the "pixels" are an arbitrary fp32 [B, C, H, W] tensor, followed
by the one to three ops under test (the head plans need a few more to make the addends). surya_det_create runs any op list, and
surya_det_read_buffer returns every activation buffer, so every kernel is compared ALONE with float64:

  check_candidate walks the plan op by op. For an op the candidate ran, the reference is the float64 op (tests/det_plan_interp.py)
  applied to the CANDIDATE's own input buffers -- exact values of the storage type -- so no error of an earlier op is carried along.
  For an op folded into a fused form the intermediate does not exist on the device: the reference chain's storage-rounded value takes
  its place and the one-ulp flips of that rounding are pushed through the next op with the magnitude pass.

The bound, per element; nothing in it is measured. u = one unit in the last place relative to the value (fp32 2^-23, bf16 2^-7,
fp16 2^-10): half of it is the rounding to storage, the other half a rounding that flips because the fp32 value differs in its last bits.
  linear ops (CONV, DWCONV, GROUPED1X1, UPCAT, INPUT, UPSAMPLE_OUT, the head's z)
        tol = u |ref| + 2 (K + 4) 2^-24 A [+ u (|W2| |mid|) pushed through, for every folded intermediate]
        K = accumulated terms (k k cin; k k; the group width; 16 for a bilinear resize), A = the same op on |inputs|, |weights|, |bias|,
        |res| without the activation. Hardswish has slope <= 1.5: the factor 2.
  the folded head is two linear forms: v = z0 + sum up(z_s) with K = 1 + 16 per addend and A_v = |z0| + sum up(|z_s|), then z = W y + b
        with y = relu(v), K = cin: tol_z = u |z| + 2 (cin + 4) 2^-24 (|W| |y| + |b|) + |W| e_y, e_y = 2 (K_v + 4) 2^-24 A_v [+ u |y| in the
        16-bit types, where the kernel rounds y to storage]. (Tighter than one form of cin (1 + 16 addends) terms.)
  CONV with a residual is two ops of the reference (the convolution's output tensor, then the add) and the GEMM epilogue rounds at both: the
        interpreter does the same in the 16-bit types and the bound adds u |mid| for the flips of the first rounding.
  LITEMLA   tol = u |ref| + (g N + |ref| g D) / (D + 1e-5), g = 2 (HW + dim + 4) 2^-24, N = relu(q) (relu(k)^T |v|), D = relu(q) sum relu(k)
  sigmoid planes   tol = tol_z / 4 + 2^-20 (sigma' <= 1/4; for |z| <= 16 the argument scaling and eight fp32 operations of <= 1 ulp move
        sigma by < 2^-21) [+ u sigma in the 16-bit types: the kernels store expit in the model dtype, as the reference's module does, and
        the interpreter leaves the planes unrounded]
Every element of every compared buffer is checked, and the whole buffer must be finite.
Not a conftest; never imported by the product."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Set, Tuple

import torch

import det_plan_interp as I
from surya_amd.detection import plan as P

U = {None: 2.0 ** -23, torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}
E24 = 2.0 ** -24
STORAGES = (None, torch.bfloat16, torch.float16)          # None = the fp32 engine


@dataclass
class Variant:
    """One way to run a plan on the device: tuning knobs, the ops a fused form folds away, the dtypes that take it, the kernel it reaches."""
    tuning: Dict[str, int]
    kernel: str
    folded: Set[int] = field(default_factory=set)          # ops whose output buffer a fused form never writes (it lives in LDS / registers)
    silent: Set[int] = field(default_factory=set)          # ops that do not run under it: surya_det_forward_timed reports 0 ms for them
    f32: bool = True


@dataclass
class MicroPlan:
    name: str
    plan: P.DetPlan
    x: torch.Tensor                                          # fp32 [B, C, H, W]
    height: int = 32                                         # surya_det_config: sizes the planes and the heat maps
    width: int = 32
    labels: int = 1
    variants: List[Variant] = field(default_factory=list)
    f32: bool = True                                         # False: a 16-bit-only plan (fused forms)
    shapes: Dict[int, Tuple[int, int, int]] = field(default_factory=dict)    # buffer id -> (h, w, c)


# --------------------------------------------------------------------------------------------------------------------------------
# builders
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _op(pl, **kw):
    d = dict(in0=-1, in1=-1, out=-1, res=-1, cin=0, cout=0, k=0, stride=0, act=0, hin=1, win=1, hout=1, wout=1, w_idx=-1, b_idx=-1, p0=0, p1=0,
             tag="micro")
    d.update(kw)
    pl.ops.append(d)
    return len(pl.ops) - 1


class Builder:
    def __init__(self, name, B, C, H, W, seed, *, height=32, width=32, labels=1, f32=True):
        self.g = _gen(seed)
        self.pl = P.DetPlan()
        self.shapes = {}
        x = torch.randn(B, C, H, W, generator=self.g)
        self.mp = MicroPlan(name, self.pl, x, height, width, labels, [], f32, self.shapes)
        self.inp = self.buf(H, W, C)
        _op(self.pl, type=P.OP_INPUT, out=self.inp, cin=C, cout=C, hin=H, win=W, hout=H, wout=W)

    def buf(self, h, w, c):
        b = self.pl.new_buf(h * w * c)
        self.shapes[b] = (h, w, c)
        return b

    def randn(self, *shape, scale=1.0):
        return torch.randn(*shape, generator=self.g) * scale

    def conv(self, x, k, stride, cout, act, *, bias=True, res=-1, w=None):
        h, w_, cin = self.shapes[x]
        pad = ((stride - 1) + (k - 1)) // 2
        ho, wo = (h + 2 * pad - k) // stride + 1, (w_ + 2 * pad - k) // stride + 1
        kreal = k * k * cin
        wk = self.randn(cout, kreal, scale=kreal ** -0.5) if w is None else w            # [Cout][ky][kx][Cin]: fan-in scaling keeps activations O(1)
        wflat = torch.zeros(cout, P.pad64(kreal))
        wflat[:, :kreal] = wk
        out = self.buf(ho, wo, cout)
        i = _op(self.pl, type=P.OP_CONV, in0=x, out=out, res=res, cin=cin, cout=cout, k=k, stride=stride, act=act, hin=h, win=w_, hout=ho,
                wout=wo, w_idx=self.pl.add_weight(wflat), b_idx=self.pl.add_weight(self.randn(cout, scale=0.5)) if bias else -1, p0=pad,
                p1=wflat.shape[1])
        return out, i

    def dw(self, x, k, stride, act, *, bias=True, w=None):
        h, w_, c = self.shapes[x]
        pad = ((stride - 1) + (k - 1)) // 2 if k == 3 else k // 2
        ho, wo = (h + 2 * pad - k) // stride + 1, (w_ + 2 * pad - k) // stride + 1
        wk = self.randn(k * k, c, scale=1.0 / k) if w is None else w                      # [K*K][C]
        out = self.buf(ho, wo, c)
        i = _op(self.pl, type=P.OP_DWCONV, in0=x, out=out, cin=c, cout=c, k=k, stride=stride, act=act, hin=h, win=w_, hout=ho, wout=wo,
                w_idx=self.pl.add_weight(wk), b_idx=self.pl.add_weight(self.randn(c, scale=0.5)) if bias else -1, p0=pad)
        return out, i

    def pick(self, x, tap, stride=1):
        """A depthwise 3x3 with a single 1.0 at `tap`: an exact shifted (stride 1) or sub-sampled (stride 2) copy -- a second, different
        tensor for ops with two inputs, made without rounding."""
        c = self.shapes[x][2]
        w = torch.zeros(9, c)
        w[tap] = 1.0
        out, i = self.dw(x, 3, stride, P.ACT_NONE, bias=False, w=w)
        self.pl.ops[i]["tag"] = "micro_pick"
        return out, i

    def g1x1(self, x, gd):
        h, w_, c = self.shapes[x]
        out = self.buf(h, w_, c)
        i = _op(self.pl, type=P.OP_GROUPED1X1, in0=x, out=out, cin=c, cout=c, k=1, stride=1, hin=h, win=w_, hout=h, wout=w_,
                w_idx=self.pl.add_weight(self.randn(c, gd, scale=gd ** -0.5)), p0=gd)
        return out, i

    def litemla(self, qa, qb, dim):
        h, w_, c3 = self.shapes[qa]
        cout = 2 * (c3 // 3)                                  # heads_a * dim per input, two inputs
        out = self.buf(h, w_, cout)
        i = _op(self.pl, type=P.OP_LITEMLA, in0=qa, in1=qb, out=out, cin=c3, cout=cout, hin=h, win=w_, hout=h, wout=w_, p0=dim)
        return out, i

    def upcat(self, x, out, ho, wo, cout, p0):
        h, w_, c = self.shapes[x]
        return _op(self.pl, type=P.OP_UPCAT, in0=x, out=out, cin=c, cout=cout, hin=h, win=w_, hout=ho, wout=wo, p0=p0)

    def classify(self, x, L, *, upsum=False):
        h, w_, c = self.shapes[x]
        return _op(self.pl, type=P.OP_UPSUM_CLASSIFY if upsum else P.OP_CLASSIFY, in0=x, cin=c, cout=L, k=1, stride=1, hin=h, win=w_,
                   hout=h, wout=w_, w_idx=self.pl.add_weight(self.randn(L, c, scale=c ** -0.5)), b_idx=self.pl.add_weight(self.randn(L, scale=0.5)))

    def upsum_src(self, x, h0, w0):
        h, w_, c = self.shapes[x]
        return _op(self.pl, type=P.OP_UPSUM_SRC, in0=x, cin=c, cout=c, hin=h, win=w_, hout=h0, wout=w0)

    def upsample_out(self, hin, win, L, ho, wo):
        return _op(self.pl, type=P.OP_UPSAMPLE_OUT, cin=0, cout=L, hin=hin, win=win, hout=ho, wout=wo)

    def done(self, *variants):
        self.mp.variants = list(variants) or [Variant({}, "")]
        return self.mp


ACT = {"none": P.ACT_NONE, "hswish": P.ACT_HSWISH, "relu": P.ACT_RELU}


def dwconv_plans():
    """DWCONV: (k, s) x three shapes, each with dwconv_pipe 0 / 1 / 2 (dwconv_tx_kernel<FD = false>, dwconv_pipe_kernel, dwconv_tx_kernel<FD = true>).
      13 x 11, C = 24  Wo not a multiple of TX = 4, an odd number of 16-byte channel groups (bias + Hardswish)
      12 x 3,  C = 8   Wo < TX, fewer than 8 workgroups: the XCD re-mapping with per = 0 (no bias, no activation)
      9 x 10,  C = 136 thread count not a multiple of 256, grid not a multiple of 8 (bias + ReLU)"""
    out = []
    for k, s in ((3, 1), (3, 2), (5, 1), (5, 2)):
        for (h, w, c), bias, act in (((13, 11, 24), True, "hswish"), ((12, 3, 8), False, "none"), ((9, 10, 136), True, "relu")):
            b = Builder(f"dw{k}s{s}_{h}x{w}x{c}", 3, c, h, w, 100 + k * 10 + s)
            b.dw(b.inp, k, s, ACT[act], bias=bias)
            out.append(b.done(*[Variant({"dwconv_pipe": p}, kern) for p, kern in
                                ((0, "dwconv_tx_kernel<FD=false>"), (1, "dwconv_pipe_kernel"), (2, "dwconv_tx_kernel<FD=true>"))]))
    return out


# where launch_conv sends a 3x3 convolution at M = 494 / 140 rows (csrc/det_kernels.h): the register-staged conv_gemm_kernel's <128,128> and
# <128,64> tiles need >= 256 / >= 128 tiles, i.e. M * Cout in the millions -- out of reach of a test that takes seconds
CONV3_KERNEL = {
    (8, 32): ("conv_gemm_kernel<128,32>", "conv_gemm_kernel<128,32>"),
    (32, 32): ("conv_gemm_kernel<128,32>", "conv_gemm_kernel<128,32>"),
    (24, 68): ("conv_gemm_kernel<64,64>", "conv_gemm_kernel<64,64>"),
    (64, 64): ("gemm.h gather <128,64>", "conv_gemm_kernel<64,64,CIN64>"),
    (32, 128): ("gemm.h gather <128,128>", "conv_gemm_kernel<64,64,CIN64>"),
    (64, 136): ("gemm.h gather <128,128>", "conv_gemm_kernel<64,64,CIN64>"),
}


def conv3_plans():
    """CONV 3x3 through launch_conv, 19 x 13, B = 2: M = 494 (stride 1) and 140 (stride 2). Every plan runs four convolutions on the same
    input -- bias + Hardswish, bias + ReLU, neither bias nor activation, and bias + residual (the first one's output) -- so every tile
    configuration reached (CONV3_KERNEL: 16-bit, fp32) sees all four epilogues at both strides.
    det_fuse = 32 (16-bit) moves what the patch-in-LDS stem kernel takes to it: 32 -> 32 stride 1 with Hardswish (stem_conv_kernel<32,1,0>) and with
    the residual (<32,1,1>), 8 -> 32 stride 2 with Hardswish (<8,2,0>); the others stay on conv_gemm_kernel<128,32>."""
    out = []
    for cin, cout in CONV3_KERNEL:
        for s in (1, 2):
            b = Builder(f"conv3_{cin}to{cout}_s{s}", 2, cin, 19, 13, 200 + cin + cout + s)
            first, _ = b.conv(b.inp, 3, s, cout, ACT["hswish"])
            b.conv(b.inp, 3, s, cout, ACT["relu"])
            b.conv(b.inp, 3, s, cout, ACT["none"], bias=False)
            b.conv(b.inp, 3, s, cout, ACT["none"], res=first)
            k16, k32 = CONV3_KERNEL[(cin, cout)]
            vs = [Variant({"det_fuse": 0}, f"{k16} | fp32 {k32}")]
            if (cin, cout, s) in ((32, 32, 1), (8, 32, 2)):
                vs.append(Variant({"det_fuse": 32}, "stem_conv_kernel" + ("<32,1,0> + <32,1,1>" if cin == 32 else "<8,2,0>"), f32=False))
            out.append(b.done(*vs))
    return out


def conv1_plans():
    """CONV 1x1, P = 3 x 7 x 5 = 105 rows: Cin = 32 is half a K-tile in the 16-bit types and takes the gather path (gemm.h's <128,64> tile with
    one tap; fp32: the GEMM), Cin = 64 -> Cout = 72 takes the NT GEMM with each of its four epilogues (bias, Hardswish, ReLU, residual).
    This checks the op -> epilogue mapping; the GEMM tiles have their own tests."""
    out = []
    for cin in (32, 64):
        b = Builder(f"conv1_{cin}to72", 3, cin, 7, 5, 300 + cin)
        first, _ = b.conv(b.inp, 1, 1, 72, ACT["none"])
        b.conv(b.inp, 1, 1, 72, ACT["hswish"])
        b.conv(b.inp, 1, 1, 72, ACT["relu"])
        b.conv(b.inp, 1, 1, 72, ACT["none"], res=first)
        out.append(b.done(Variant({"det_fuse": 0}, "launch_gemm EPI_BIAS / HARDSWISH / RELU / RESIDUAL" if cin == 64 else
                                  "16-bit: gemm.h gather <128,64>, cTaps = 1 | fp32: launch_gemm")))
    return out


def grouped_plans():
    """GROUPED1X1: group widths 32, 16, 8 at C = 96, P = 3 x 7 x 5 = 105 pixels (not a multiple of the 64 a workgroup takes)."""
    out = []
    for gd in (32, 16, 8):
        b = Builder(f"g1x1_w{gd}", 3, 96, 7, 5, 400 + gd)
        b.g1x1(b.inp, gd)
        out.append(b.done(Variant({"det_fuse": 0}, "grouped1x1_kernel")))
    return out


def litemla_plans():
    """LITEMLA: head width 32 / 16, HW = 5 (1 x 5), 121 (11 x 11: one ragged chunk) and 300 (15 x 20: two chunks, the second ragged), 2 and 4
    heads; the second input is an exact one-pixel shift of the first (Builder.pick). det_fuse = 0: litemla_kv_kernel + litemla_out_kernel;
    det_fuse = 2 (width 32, all three dtypes): litemla_fused_kernel. `smallD`: q and k scaled by 2^-7, so D is comparable to the 1e-5 eps."""
    out = []
    for dim in (32, 16):
        for (h, w) in ((1, 5), (11, 11), (15, 20)):
            for heads in (2, 4):
                for small in ((False, True) if (dim, h, heads) == (32, 11, 2) else (False,)):
                    c3 = heads // 2 * 3 * dim
                    b = Builder(f"litemla_d{dim}_{h}x{w}_h{heads}" + ("_smallD" if small else ""), 3, c3, h, w, 500 + dim + h + heads)
                    if small:
                        x = b.mp.x.view(3, heads // 2, 3, dim, h, w)
                        x[:, :, :2] *= 2.0 ** -7
                    qb, _ = b.pick(b.inp, 5)                  # tap (ky 1, kx 2): the pixel to the right, zero in the last column
                    b.litemla(b.inp, qb, dim)
                    vs = [Variant({"det_fuse": 0}, f"litemla_kv_kernel<{dim}> + litemla_out_kernel<{dim}>")]
                    if dim == 32:
                        vs.append(Variant({"det_fuse": 2}, "litemla_fused_kernel<32>"))
                    out.append(b.done(*vs))
    return out


def upcat_plans():
    """UPCAT: two ops fill one 32-channel buffer (p0 = 0 and 16) from two different 16-channel sources; x2 (2 x 3 -> 4 x 6), x8 (1 x 1 -> 8 x 8
    and 2 x 3 -> 16 x 24) and a non-integer ratio (5 x 7 -> 13 x 9). Sources 1 x 1 and 2 x 3 hit every index clamp."""
    out = []
    for (h, w), (ho, wo) in (((2, 3), (4, 6)), ((1, 1), (8, 8)), ((2, 3), (16, 24)), ((5, 7), (13, 9))):
        b = Builder(f"upcat_{h}x{w}_to_{ho}x{wo}", 3, 16, h, w, 600 + h * 10 + ho)
        second, _ = b.dw(b.inp, 3, 1, ACT["none"], bias=True)
        cat = b.buf(ho, wo, 32)
        b.upcat(second, cat, ho, wo, 32, 0)
        b.upcat(b.inp, cat, ho, wo, 32, 16)
        out.append(b.done(Variant({}, "upsample_concat_kernel")))
    return out


def classify_plans():
    """CLASSIFY + UPSAMPLE_OUT (fp32 planes through `lowres`, the heat maps): labels 1, 2, 4; sources 8 x 8, 8 x 16, 3 x 5; x4 with det_up4 = 1
    (upsample_planes_x4_kernel) and 0 (upsample_planes4_kernel), 8 x 16 -> 24 x 36 (upsample_planes4_kernel: wout % 4 == 0, not x4) and
    3 x 5 -> 7 x 9 (the generic upsample_planes_kernel). C = 136: 17 channel groups, one more than the 16 lanes of a pixel take per step.
    The configuration is 64 x 64, so the 16 x 16 planes per label hold every case."""
    out = []
    for L, (h, w), (ho, wo), c in ((1, (8, 8), (32, 32), 136), (2, (8, 16), (32, 64), 24), (4, (3, 5), (12, 20), 136), (2, (8, 16), (24, 36), 136),
                                   (1, (3, 5), (7, 9), 8), (4, (8, 8), (32, 32), 24)):
        b = Builder(f"classify_L{L}_{h}x{w}_to_{ho}x{wo}", 3, c, h, w, 700 + L * 10 + ho, height=64, width=64, labels=L)
        b.classify(b.inp, L)
        b.upsample_out(h, w, L, ho, wo)
        x4 = (ho, wo) == (4 * h, 4 * w)
        vs = [Variant({"det_up4": 1}, "classify_sigmoid_kernel + " + ("upsample_planes_x4_kernel" if x4 else
                                                                      "upsample_planes4_kernel" if wo % 4 == 0 else "upsample_planes_kernel"))]
        if x4:
            vs.append(Variant({"det_up4": 0}, "classify_sigmoid_kernel + upsample_planes4_kernel"))
        out.append(b.done(*vs))
    return out


def head_plans():
    """UPSUM_SRC x 3 + UPSUM_CLASSIFY. Full resolution 16 x 32 (1 label) and 24 x 40 (2 labels; a half-outside last tile of the MFMA head
    kernel) with addends at /2, /4, /8: the 64-channel input is sub-sampled by exact depthwise picks and every level goes through its own
    1x1 convolution to C = 128, as the product's folded head does. det_head_blk 0 / 1 / 2: head_upsum_classify_kernel, the 4 x 2 and the
    4 x 1 blocked kernels. 16-bit: det_fuse = 4 folds the full-resolution 1x1 convolution in (head_z0 kernel), 132 runs the MFMA head.
    `r3`: 24 x 36 with addends at /3, /6, /12, which only the per-pixel kernel takes."""
    out = []
    for (h, w), L in (((16, 32), 1), ((24, 40), 2)):
        b = Builder(f"head_{h}x{w}_L{L}", 3, 64, h, w, 800 + h, height=128, width=160, labels=L)
        d1, _ = b.pick(b.inp, 4, 2)
        d2, _ = b.pick(d1, 8, 2)
        d3, _ = b.pick(d2, 0, 2)
        zs = [b.conv(d, 1, 1, 128, ACT["none"], bias=False)[0] for d in (d1, d2, d3)]
        z0, z0_op = b.conv(b.inp, 1, 1, 128, ACT["none"], bias=True)
        for z in zs:
            b.upsum_src(z, h, w)
        b.classify(z0, L, upsum=True)
        out.append(b.done(Variant({"det_fuse": 0, "det_head_blk": 0}, "head_upsum_classify_kernel"),
                          Variant({"det_fuse": 0, "det_head_blk": 1}, "head_upsum_classify_blk_kernel<2,4,8,2>"),
                          Variant({"det_fuse": 0, "det_head_blk": 2}, "head_upsum_classify_blk_kernel<2,4,8,1>"),
                          Variant({"det_fuse": 4, "det_head_blk": 1}, "head_z0_kernel (det_fused.h)", folded={z0_op}, silent={z0_op}, f32=False),
                          Variant({"det_fuse": 132, "det_head_blk": 1}, "head_mfma_kernel (det_head.h)", folded={z0_op}, silent={z0_op}, f32=False)))
    b = Builder("head_r3_24x36_L2", 3, 128, 24, 36, 850, height=128, width=160, labels=2)
    a1 = b.buf(8, 12, 128)
    b.upcat(b.inp, a1, 8, 12, 128, 0)
    a2, _ = b.pick(a1, 4, 2)
    a3, _ = b.pick(a2, 8, 2)
    for z in (a1, a2, a3):
        b.upsum_src(z, 24, 36)
    b.classify(b.inp, 2, upsum=True)
    out.append(b.done(*[Variant({"det_fuse": 0, "det_head_blk": k}, "head_upsum_classify_kernel (ratios 3 / 6 / 12)") for k in (0, 1, 2)]))
    return out


def fused_plans():
    """Fused pairs and triples (16-bit only), each with det_fuse = 0 (the op list: every op alone) and with only its own bit set (the fused
    kernel against the storage-rounded float64 chain; its intermediate lives on the chip only).
      dw5 + grouped 1x1          C = 64, 9 x 37                                         bit 1    dw5_g1x1_kernel
      dw3 + projection           128 -> 256 and 256 -> 512; stride 1 at 9 x 17 with a residual, stride 2 at 11 x 18   bit 8    dwproj_kernel<S>
      expand + dw3 s2 + proj     128 -> 256 -> 256 and 256 -> 512 -> 512 at 11 x 18     bits 64 + 8  mbconv_kernel
      FusedMBConv                64 -> 128 -> 64 stride 1 with a residual, 32 -> 128 -> 64 stride 2, at 10 x 34   bit 16   fmb_kernel
      the stem's residual pair   32 -> 32 -> 32 at 9 x 33                               bits 32 + 512  stem_res_kernel
    B = 3 everywhere: every shape has partial tiles, and at least 8 tiles so that every XCD's share of a persistent grid is non-empty."""
    out = []
    H, N = ACT["hswish"], ACT["none"]
    b = Builder("fused_dw5_g1x1_64_9x37", 3, 64, 9, 37, 900, f32=False)
    _, i = b.dw(b.inp, 5, 1, N, bias=False)
    b.g1x1(b.pl.ops[i]["out"], 32)
    out.append(b.done(Variant({"det_fuse": 0}, "dwconv_tx_kernel<5,1> + grouped1x1_kernel"),
                      Variant({"det_fuse": 1}, "dw5_g1x1_kernel", folded={i}, silent={i + 1}, f32=False)))
    for cm, cout in ((128, 256), (256, 512)):
        for s_, (h, w) in ((1, (9, 17)), (2, (11, 18))):
            b = Builder(f"fused_dw3_proj_{cm}to{cout}_s{s_}", 3, cm, h, w, 910 + cm // 64 + s_, f32=False)
            res = b.conv(b.inp, 1, 1, cout, N)[0] if s_ == 1 else -1
            mid, i = b.dw(b.inp, 3, s_, H)
            b.conv(mid, 1, 1, cout, N, res=res)
            out.append(b.done(Variant({"det_fuse": 0}, f"dwconv_tx_kernel<3,{s_}> + launch_gemm " + ("EPI_RESIDUAL" if s_ == 1 else "EPI_BIAS")),
                              Variant({"det_fuse": 8}, f"dwproj_kernel<{s_}>", folded={i}, silent={i + 1}, f32=False)))
    for cin, mid_c in ((128, 256), (256, 512)):
        b = Builder(f"fused_mbconv_{cin}to{mid_c}to{mid_c}_s2", 3, cin, 11, 18, 930 + cin // 64, f32=False)
        e, i = b.conv(b.inp, 1, 1, mid_c, H)
        d, _ = b.dw(e, 3, 2, H)
        b.conv(d, 1, 1, mid_c, N)
        out.append(b.done(Variant({"det_fuse": 0}, "launch_gemm EPI_HARDSWISH + dwconv_tx_kernel<3,2> + launch_gemm EPI_BIAS"),
                          Variant({"det_fuse": 72}, f"mbconv_kernel<{cin}>", folded={i, i + 1}, silent={i + 1, i + 2}, f32=False)))
    for cin, s_ in ((64, 1), (32, 2)):
        b = Builder(f"fused_fmb_{cin}to128to64_s{s_}", 3, cin, 10, 34, 940 + s_, f32=False)
        e, i = b.conv(b.inp, 3, s_, 128, H)
        b.conv(e, 1, 1, 64, N, res=b.inp if s_ == 1 else -1)
        out.append(b.done(Variant({"det_fuse": 0}, "gemm.h gather <128,128> EPI_HARDSWISH + launch_gemm " + ("EPI_RESIDUAL" if s_ == 1 else "EPI_BIAS")),
                          Variant({"det_fuse": 16}, f"fmb_kernel<{cin},{s_}>", folded={i}, silent={i + 1}, f32=False)))
    b = Builder("fused_stem_res_32_9x33", 3, 32, 9, 33, 950, f32=False)
    e, i = b.conv(b.inp, 3, 1, 32, H)
    b.conv(e, 3, 1, 32, N, res=b.inp)
    out.append(b.done(Variant({"det_fuse": 0}, "conv_gemm_kernel<128,32> x 2"),
                      Variant({"det_fuse": 544}, "stem_res_kernel", folded={i}, silent={i + 1}, f32=False)))
    return out


_CACHE: Optional[List[MicroPlan]] = None


def all_microplans() -> List[MicroPlan]:
    """Built once per process and shared: the plans and their inputs are never modified."""
    global _CACHE
    if _CACHE is None:
        _CACHE = (dwconv_plans() + conv3_plans() + conv1_plans() + grouped_plans() + litemla_plans() + upcat_plans() + classify_plans() +
                  head_plans() + fused_plans())
        names = [m.name for m in _CACHE]
        assert len(set(names)) == len(names)
    return _CACHE


# --------------------------------------------------------------------------------------------------------------------------------
# the bound
@dataclass
class Candidate:
    """What an implementation under test produced for a plan: every activation buffer it wrote (NHWC), the planes, the heat maps."""
    bufs: Dict[int, torch.Tensor]
    planes: Optional[torch.Tensor] = None
    heat: Optional[torch.Tensor] = None


def _k_terms(op):
    t = op["type"]
    if t == P.OP_CONV:
        return op["k"] * op["k"] * op["cin"]
    if t == P.OP_DWCONV:
        return op["k"] * op["k"]
    if t == P.OP_GROUPED1X1:
        return op["p0"]
    if t in (P.OP_UPCAT, P.OP_UPSAMPLE_OUT):
        return 16
    if t == P.OP_INPUT:
        return 1
    raise ValueError(t)


def check_candidate(mp: MicroPlan, storage, cand: Candidate, folded: Set[int] = frozenset()):
    """Walk mp.plan op by op (see the module docstring). Returns [(what, worst error / bound, elements over the bound, all finite)], one
    entry per compared buffer, for the planes and for the heat maps. Every element takes part."""
    pl, u = mp.plan, U[storage]
    f64 = torch.float64
    bufs: Dict[int, torch.Tensor] = {}           # what the reference op reads: the candidate's buffer, or the reference chain's where folded
    errs: Dict[int, torch.Tensor] = {}           # per-element allowance for how far the device's (virtual) value may be from bufs[.]
    st = I.PlanState()
    px = I.round_to(mp.x.to(f64), storage)
    report = []

    def compare(what, got, ref, tol):
        got = got.to(f64)
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        err = (got - ref).abs()
        finite = bool(torch.isfinite(got).all())
        over = int(((err > tol) | ~torch.isfinite(got)).sum())
        ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
        ratio = torch.nan_to_num(ratio, nan=float("inf"))
        report.append((what, float(ratio.max()), over, finite))

    def mag_pass(op, src, with_bias):
        """The op on |weights| (and |bias|) applied to `src` (buffer id -> non-negative tensor)."""
        tmp, s2 = dict(src), I.PlanState()
        I.apply_op(pl, op, tmp, s2, pixel_values=px.abs(), storage=storage, mag=True, with_bias=with_bias)
        return tmp[op["out"]]

    for oi, op in enumerate(pl.ops):
        t = op["type"]
        ins = [b for b in (op["in0"], op["in1"], op["res"]) if b >= 0]
        has_err = any(b in errs for b in ins)
        if t == P.OP_UPSUM_SRC:
            st.addends.append(op["in0"])
            continue
        if t in (P.OP_CLASSIFY, P.OP_UPSUM_CLASSIFY):
            add_ids, st.addends = (st.addends, []) if t == P.OP_UPSUM_CLASSIFY else ([], st.addends)
            s2 = I.PlanState()
            s2.addends = [bufs[a] for a in add_ids]
            I.apply_op(pl, op, bufs, s2, storage=storage)
            z, sig, y = s2.z, s2.planes, s2.y
            assert z.abs().max() <= 16, f"{mp.name}: |z| = {z.abs().max():.1f} > 16: the sigmoid bound does not hold"
            W_ = I.round_to(pl.weights[op["w_idx"]].to(f64), storage).abs()
            b_ = I.round_to(pl.weights[op["b_idx"]].to(f64), storage).abs()
            a_v = I.upsum_v(op, bufs[op["in0"]].abs(), [bufs[a].abs() for a in add_ids])
            a_z = (a_v @ W_.t() + b_).permute(0, 3, 1, 2)
            # two stages, each a linear form: v = z0 + sum up(z_s) (1 + 16 per addend terms), then z = W y + b (cin terms) with y = relu(v)
            a_z = (y.abs() @ W_.t() + b_).permute(0, 3, 1, 2)
            tol_z = u * z.abs() + 2 * (op["cin"] + 4) * E24 * a_z
            if add_ids:
                e_y = 2 * (1 + 16 * len(add_ids) + 4) * E24 * a_v + (u * y.abs() if storage is not None else 0.0)   # 16-bit: y is rounded to storage in the kernel
                tol_z = tol_z + (e_y @ W_.t()).permute(0, 3, 1, 2)
            if has_err or any(a in errs for a in add_ids):
                zero = lambda b: errs.get(b, torch.zeros_like(bufs[b]))
                e_v = I.upsum_v(op, zero(op["in0"]), [zero(a) for a in add_ids])
                tol_z = tol_z + (e_v @ W_.t()).permute(0, 3, 1, 2)
            tol = tol_z / 4 + 2.0 ** -20 + (u * sig if storage is not None else 0.0)
            compare(f"op{oi} planes", cand.planes, sig, tol)
            st.planes = cand.planes.to(f64)
            continue
        if t == P.OP_UPSAMPLE_OUT:
            s2 = I.PlanState()
            s2.planes = st.planes
            I.apply_op(pl, op, {}, s2, pixel_values=px, storage=None)
            ref = s2.heat
            tol = U[None] * ref.abs() + 2 * (16 + 4) * E24 * ref.abs()      # the planes are non-negative: A == ref
            compare(f"op{oi} heat", cand.heat, ref, tol)
            continue
        # ops that write an activation buffer
        tmp, s2 = dict(bufs), I.PlanState()
        if t == P.OP_UPCAT:
            tmp.pop(op["out"], None)
        I.apply_op(pl, op, tmp, s2, pixel_values=px, storage=storage)
        ref = tmp[op["out"]]
        if t == P.OP_LITEMLA:
            assert not has_err, "a folded intermediate in front of LiteMLA is not modelled"
            dim, HW = op["p0"], op["hin"] * op["win"]
            N, D = I.litemla_parts(op, bufs[op["in0"]], bufs[op["in1"]], abs_v=True)
            g = 2 * (HW + dim + 4) * E24
            D = D.repeat_interleave(dim, -1)
            r = ref.flatten(1, 2)
            tol = (u * r.abs() + (g * N + r.abs() * g * D) / (D + 1e-5)).reshape(ref.shape)
        else:
            src = {b: bufs[b].abs() for b in ins}
            A = mag_pass(op, src, True)
            tol = u * ref.abs() + 2 * (_k_terms(op) + 4) * E24 * A
            if has_err:
                tol = tol + mag_pass(op, {b: errs.get(b, torch.zeros_like(bufs[b])) for b in ins}, False)
            if t == P.OP_CONV and op["res"] >= 0 and storage is not None:
                # CONV + residual is two reference ops with a rounding between them (det_plan_interp.apply_op): the one-ulp flips of that
                # rounding pass through the add unchanged. A kernel that rounds once is half an ulp of `mid` away: inside this as well.
                tmp2 = dict(bufs)
                I.apply_op(pl, dict(op, res=-1), tmp2, I.PlanState(), pixel_values=px, storage=storage)
                tol = tol + u * tmp2[op["out"]].abs()
        sl = slice(op["p0"], op["p0"] + op["cin"]) if t == P.OP_UPCAT else slice(None)
        if oi in folded:
            assert storage is not None and t != P.OP_UPCAT, "fused forms exist for the 16-bit types"
            bufs[op["out"]] = ref
            errs[op["out"]] = u * ref.abs()              # the one-ulp flips of the intermediate's rounding (module docstring)
            continue
        got = cand.bufs[op["out"]]
        compare(f"op{oi} buf{op['out']}", got[..., sl], ref[..., sl], tol[..., sl])
        if t == P.OP_UPCAT and op["out"] in bufs:
            new = bufs[op["out"]].clone()
            new[..., sl] = got[..., sl].to(f64)
            bufs[op["out"]] = new
        elif t == P.OP_UPCAT:
            new = torch.full_like(ref, float("nan"))
            new[..., sl] = got[..., sl].to(f64)
            bufs[op["out"]] = new
        else:
            bufs[op["out"]] = got.to(f64)
    return report


def interp_candidate(mp: MicroPlan, storage, *, dtype=torch.float32, mutant=None) -> Candidate:
    """The interpreter itself as the implementation under test: fp32 arithmetic (the reference alone must stay inside the bound), or
    float64 with one of det_plan_interp.MUTANTS (must leave it)."""
    bufs, planes, heat = I.run_plan_buffers(mp.plan, mp.x, dtype=dtype, storage=storage, mutant=mutant)
    if planes is not None and storage is not None and dtype == torch.float32:
        planes = I.round_to(planes, storage)           # as the 16-bit engines store them
        if heat is not None:
            heat = torch.nn.functional.interpolate(planes, size=heat.shape[2:], mode="bilinear", align_corners=False)
    return Candidate(bufs, planes, heat)


# --------------------------------------------------------------------------------------------------------------------------------
# op lists surya_det_create must refuse on the host (include/surya_amd.h, above the op enum); nothing is allocated or launched for them
SA_ERR_ARG, SA_ERR_SHAPE, SA_ERR_UNSUPPORTED = -1, -2, -3


def create_rc(pl: P.DetPlan, *, height=32, width=32, labels=1, dtype=torch.bfloat16, max_batch=3) -> int:
    """surya_det_create's return code for an op list that is expected to be refused: the weight table holds host addresses nothing may
    read -- a refusal comes before any allocation or launch. (A plan that is accepted must go through HipDetModel.from_plan instead.)"""
    import ctypes as C
    from surya_amd import _lib as L
    from surya_amd.detection.model import DetOpC, _DTYPES
    lib = L.lib()
    lib.surya_det_create.argtypes = None
    keep = [w.contiguous() for w in pl.weights]
    ops = (DetOpC * len(pl.ops))(*[DetOpC(**{k: v for k, v in o.items() if k != "tag"}) for o in pl.ops])
    table = (C.c_void_p * max(1, len(keep)))(*[w.data_ptr() for w in keep])
    bufs = (C.c_size_t * len(pl.buf_elems))(*pl.buf_elems)
    c = L.DetConfigC(n_ops=len(pl.ops), max_batch=max_batch, height=height, width=width, num_labels=labels, dtype=_DTYPES[dtype])
    handle = C.c_void_p()
    rc = int(lib.surya_det_create(C.byref(c), ops, table, len(keep), bufs, len(pl.buf_elems), C.byref(handle)))
    assert rc != 0 and not handle.value, "this op list was expected to be refused"
    return rc


def refusal_cases():
    """[(name, plan, create_rc keywords, expected code)]: every parameter the create-time validation rejects."""
    def one(name, build, code, **kw):
        b = Builder(name, 3, kw.pop("C", 32), kw.pop("H", 8), kw.pop("W", 8), 1)
        build(b)
        return (name, b.pl, kw, code)

    def edit(b, i, **kw):
        b.pl.ops[i].update(kw)

    def shrink(b, buf):
        b.pl.buf_elems[buf] -= 1

    cases = []

    def in0_small(b):
        b.dw(b.inp, 3, 1, 0); shrink(b, b.inp)
    cases.append(one("in0_smaller_than_hin_win_cin", in0_small, SA_ERR_SHAPE))

    def in1_small(b):
        qb, _ = b.pick(b.inp, 5); b.litemla(b.inp, qb, 16); shrink(b, qb)
    cases.append(one("litemla_in1_too_small", in1_small, SA_ERR_SHAPE, C=96))

    def out_small(b):
        out, _ = b.dw(b.inp, 3, 1, 0); shrink(b, out)
    cases.append(one("out_smaller_than_hout_wout_cout", out_small, SA_ERR_SHAPE))

    def res_small(b):
        r = b.buf(8, 8, 16)                                   # half of what the residual of a 32-channel output needs
        b.upcat(b.inp, r, 8, 8, 16, 0)
        b.pl.ops[-1].update(cin=16)
        b.conv(b.inp, 1, 1, 32, 0, res=r)
    cases.append(one("res_not_sized_like_out", res_small, SA_ERR_SHAPE))

    def cls_big(b):
        b.classify(b.inp, 1)                                  # 16 x 16 planes; the 32 x 32 configuration holds 8 x 8 per label
    cases.append(one("classify_larger_than_planes", cls_big, SA_ERR_SHAPE, H=16, W=16))

    def upsum_big(b):
        d, _ = b.pick(b.inp, 4, 2); b.upsum_src(d, 16, 16); b.classify(b.inp, 1, upsum=True)
    cases.append(one("upsum_classify_larger_than_planes", upsum_big, SA_ERR_SHAPE, H=16, W=16))

    def heat_big(b):
        b.classify(b.inp, 1); b.upsample_out(8, 8, 1, 64, 64)
    cases.append(one("upsample_out_larger_than_heat", heat_big, SA_ERR_SHAPE))

    def mla_width(b):
        qb, _ = b.pick(b.inp, 5); _, i = b.litemla(b.inp, qb, 16); edit(b, i, cout=24)
    cases.append(one("litemla_cout_not_multiple_of_p0", mla_width, SA_ERR_SHAPE, C=48))

    def mla_odd(b):
        qb, _ = b.pick(b.inp, 5); _, i = b.litemla(b.inp, qb, 16); edit(b, i, cout=48)
    cases.append(one("litemla_odd_head_count", mla_odd, SA_ERR_SHAPE, C=96))

    def mla_dim(b):
        qb, _ = b.pick(b.inp, 5); b.litemla(b.inp, qb, 8)
    cases.append(one("litemla_head_width_8", mla_dim, SA_ERR_UNSUPPORTED, C=48))

    cases.append(one("grouped_width_64", lambda b: b.g1x1(b.inp, 64), SA_ERR_UNSUPPORTED, C=128))
    cases.append(one("grouped_cin_not_multiple_of_width", lambda b: b.g1x1(b.inp, 16), SA_ERR_SHAPE, C=40))
    cases.append(one("grouped_width_not_multiple_of_16_bytes", lambda b: b.g1x1(b.inp, 4), SA_ERR_SHAPE, C=32))
    cases.append(one("grouped_width_not_multiple_of_16_bytes_fp32", lambda b: b.g1x1(b.inp, 2), SA_ERR_SHAPE, C=32, dtype=torch.float32))

    def dw_c(b):
        _, i = b.dw(b.inp, 3, 1, 0); edit(b, i, cin=12, cout=12)
    cases.append(one("dwconv_cin_not_multiple_of_16_bytes", dw_c, SA_ERR_SHAPE))

    def dw_k(b):
        _, i = b.dw(b.inp, 5, 1, 0); edit(b, i, k=7, p0=3)
    cases.append(one("dwconv_k7", dw_k, SA_ERR_UNSUPPORTED))

    def up_c(b):
        cat = b.buf(16, 16, 32); i = b.upcat(b.inp, cat, 16, 16, 32, 0); edit(b, i, cin=12)
    cases.append(one("upcat_cin_not_multiple_of_16_bytes", up_c, SA_ERR_SHAPE))

    def up_over(b):
        cat = b.buf(16, 16, 40); b.upcat(b.inp, cat, 16, 16, 40, 16)
    cases.append(one("upcat_p0_plus_cin_over_cout", up_over, SA_ERR_SHAPE))

    cases.append(one("input_cout_not_multiple_of_16_bytes", lambda b: None, SA_ERR_SHAPE, C=12))
    cases.append(one("input_cout_not_multiple_of_16_bytes_fp32", lambda b: None, SA_ERR_SHAPE, C=6, dtype=torch.float32))

    def act_res(b):
        first, _ = b.conv(b.inp, 1, 1, 32, 0); b.conv(b.inp, 1, 1, 32, P.ACT_HSWISH, res=first)
    cases.append(one("conv_act_with_res", act_res, SA_ERR_UNSUPPORTED))

    def conv_cout(b):
        b.conv(b.inp, 3, 1, 6, 0)
    cases.append(one("conv_cout_not_multiple_of_4", conv_cout, SA_ERR_SHAPE))

    def conv_hout(b):
        _, i = b.conv(b.inp, 3, 2, 32, 0); edit(b, i, hout=8, wout=8); b.pl.buf_elems[-1] = 8 * 8 * 32
    cases.append(one("conv_hout_not_the_convolution_s", conv_hout, SA_ERR_SHAPE))

    def bad_index(b):
        _, i = b.dw(b.inp, 3, 1, 0); edit(b, i, in0=7)
    cases.append(one("buffer_index_out_of_range", bad_index, SA_ERR_ARG))

    def no_bias(b):
        i = b.classify(b.inp, 1); edit(b, i, b_idx=-1)
    cases.append(one("classify_without_bias", no_bias, SA_ERR_ARG))

    def unwritten(b):
        other = b.buf(8, 8, 32); b.pl.ops.pop(); b.dw(other, 3, 1, 0)       # no INPUT op: the depthwise reads a buffer nothing wrote
    cases.append(one("reads_a_buffer_nothing_wrote", unwritten, SA_ERR_SHAPE))

    def four_srcs(b):
        for _ in range(4):
            b.upsum_src(b.inp, 8, 8)
        b.classify(b.inp, 1, upsum=True)
    cases.append(one("four_upsum_sources", four_srcs, SA_ERR_UNSUPPORTED))
    return cases
