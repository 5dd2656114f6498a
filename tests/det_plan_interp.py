"""Test infrastructure: a plain-PyTorch interpreter of the detector's op list (surya_amd/detection/plan.py -> include/surya_amd.h
SA_DET_*), op by op as csrc/det_model.hip executes it. It lets the CPU tier check what the plan LOWERS -- BatchNorm folding, the NHWC
weight layouts, the K padding, the folded decode head's merged weights -- against the oracle (= the reference's own op order) without a
GPU (run_plan, fp32), and it is the float64 reference of the one-kernel plans of tests/det_microplan.py (run_plan_buffers / apply_op,
with the rounding to the storage type the op list does through HBM, and a magnitude pass for the error bound). Never imported by the
product."""
import torch
import torch.nn.functional as F

from surya_amd.detection import plan as P

# The mutants of tests/test_det_microplan_cpu.py: each makes the interpreter wrong the way a kernel plausibly is. A micro-plan that none
# of them pushes over its bound tests nothing.
MUTANTS = ("pad_replicate", "swap_kxky", "last_group_repeat", "drop_last_token", "align_corners", "p0_off_group", "no_eps")


def _act(y, act):
    if act == P.ACT_HSWISH:
        return F.hardswish(y)
    if act == P.ACT_RELU:
        return F.relu(y)
    return y


def _nchw(t):
    return t.permute(0, 3, 1, 2)          # buffers are NHWC like the device's


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def round_to(t, storage):
    """t rounded to `storage` (round to nearest even, as the kernels' stores do) and back; None = no rounding."""
    return t if storage is None else t.to(storage).to(t.dtype)


def vec_elems(storage):
    """Elements per 16 bytes of the storage type: the kernels' vector width, the `group` of the last_group_repeat / p0_off_group mutants."""
    return 8 if storage in (torch.bfloat16, torch.float16) else 4


def _conv2d(x, w, b, stride, pad, groups, mutant):
    if mutant == "swap_kxky":
        w = w.transpose(2, 3)
    if mutant == "pad_replicate" and pad > 0:
        return F.conv2d(F.pad(x, (pad, pad, pad, pad), mode="replicate"), w, b, stride=stride, padding=0, groups=groups)
    return F.conv2d(x, w, b, stride=stride, padding=pad, groups=groups)


def _resize(x_nchw, size, mutant):
    return F.interpolate(x_nchw, size=size, mode="bilinear", align_corners=(mutant == "align_corners"))


def _repeat_last_group(t, V, mutant):
    """last_group_repeat: the last 16-byte channel group holds a copy of the one before it (a vector loop that stops one group early
    or indexes its last group wrongly)."""
    if mutant != "last_group_repeat" or t.shape[-1] < 2 * V:
        return t
    t = t.clone()
    t[..., -V:] = t[..., -2 * V:-V]
    return t


class PlanState:
    """What the ops of a plan hand on outside the activation buffers."""

    def __init__(self):
        self.addends = []          # UPSUM_SRC: [(buffer tensor)]
        self.y = None              # classifier input (after ReLU and the rounding to storage of UPSUM_CLASSIFY)
        self.z = None              # pre-sigmoid values [B, L, h, w]
        self.planes = None         # sigmoid planes [B, L, h, w], unrounded
        self.heat = None           # [B, L, hout, wout], unrounded


def litemla_parts(op, qa, qb, *, mutant=None, abs_v=False):
    """LiteMLA's numerator [B, HW, heads * dim] and denominator [B, HW, heads] (before the eps): out = num / (den + eps).
    abs_v: |v| in place of v -- the magnitude N of the numerator; the denominator D is a sum of non-negative terms already."""
    dim, heads = op["p0"], op["cout"] // op["p0"]
    qa, qb = qa.flatten(1, 2), qb.flatten(1, 2)                                        # [B, HW, heads_a * 3 * dim] each
    nums, dens = [], []
    for h in range(heads):
        src, hh = (qa, h) if h < heads // 2 else (qb, h - heads // 2)
        q, k_, v = (src[..., hh * 3 * dim + j * dim: hh * 3 * dim + (j + 1) * dim] for j in range(3))
        q, k_ = F.relu(q), F.relu(k_)
        if abs_v:
            v = v.abs()
        v1 = torch.cat([v, torch.ones_like(v[..., :1])], -1)
        if mutant == "drop_last_token":
            k_, v1 = k_[:, :-1], v1[:, :-1]
        o = q @ (k_.transpose(1, 2) @ v1)                                              # [B, HW, dim + 1]
        nums.append(o[..., :dim])
        dens.append(o[..., dim:])
    return torch.cat(nums, -1), torch.cat(dens, -1)


def upsum_v(op, z0, addends, *, mutant=None):
    """The folded head's sum in front of the ReLU: z0 + the addends resized to z0's size."""
    y = z0
    for z in addends:
        y = y + _nhwc(_resize(_nchw(z), (op["hin"], op["win"]), mutant))
    return y


def apply_op(pl, op, bufs, st, *, pixel_values=None, storage=None, mutant=None, mag=False, with_bias=True):
    """One op of pl on `bufs` (buffer id -> NHWC tensor; its dtype is the arithmetic's) and `st` (PlanState). Every buffer is rounded
    to `storage` when it is written; planes and heat are not. mutant: one of MUTANTS.
    mag: the magnitude pass -- the same op on |weights| and |bias| without the activation; the caller hands in |inputs| (or per-element
    input errors, with with_bias=False) and gets the per-element sum of |terms| (or the propagated error)."""
    t = op["type"]
    V = vec_elems(storage)
    dt = pixel_values.dtype if pixel_values is not None else next(iter(bufs.values())).dtype

    def weight(idx):
        if idx < 0:
            return None
        w = round_to(pl.weights[idx].to(dt), storage)
        return w.abs() if mag else w

    W_ = weight(op["w_idx"])
    b_ = weight(op["b_idx"]) if with_bias else None
    act = (lambda y, a: y) if mag else _act
    out = None
    if t == P.OP_INPUT:
        x = _nhwc(pixel_values.to(dt))
        out = F.pad(x, (0, op["cout"] - x.shape[-1]))
    elif t == P.OP_CONV:
        k, cin, cout = op["k"], op["cin"], op["cout"]
        # the engine's 1x1 path has a residual epilogue and an activation epilogue, not both: surya_det_create refuses the pair, no plan builds it
        assert not (op["act"] != P.ACT_NONE and op["res"] >= 0), "CONV with both act and res"
        assert W_.shape == (cout, op["p1"]) and op["p1"] % 64 == 0 and op["p1"] >= k * k * cin
        w = W_[:, : k * k * cin].reshape(cout, k, k, cin).permute(0, 3, 1, 2)        # [Cout][ky][kx][Cin] -> OIHW
        assert (W_[:, k * k * cin:] == 0).all()                                       # the K padding is zero
        y = _conv2d(_nchw(bufs[op["in0"]]), w, b_, op["stride"], op["p0"], 1, mutant)
        y = act(y, op["act"])
        if op["res"] >= 0:
            # the reference's two tensor ops, each in the model dtype: the convolution's output, then the residual add. The GEMM epilogue rounds
            # at both (csrc/gemm.h EPI_RESIDUAL: "rounded projection + residual, rounded"), and so do the fused forms that repeat it; the
            # register-staged conv_gemm_kernel and the stem kernels add the residual in fp32 and round once -- half an ulp of the convolution's
            # output away, which the bound of tests/det_microplan.py allows for
            y = (y if mag else round_to(y, storage)) + _nchw(bufs[op["res"]])
        assert y.shape[2:] == (op["hout"], op["wout"])
        out = _nhwc(y)
    elif t == P.OP_DWCONV:
        k, c = op["k"], op["cin"]
        w = W_.t().reshape(c, 1, k, k)                                                # [K*K][C] -> depthwise OIHW
        y = act(_conv2d(_nchw(bufs[op["in0"]]), w, b_, op["stride"], op["p0"], c, mutant), op["act"])
        assert y.shape[2:] == (op["hout"], op["wout"])
        out = _nhwc(y)
    elif t == P.OP_GROUPED1X1:
        c, gd = op["cin"], op["p0"]
        out = _nhwc(F.conv2d(_nchw(bufs[op["in0"]]), W_.reshape(c, gd, 1, 1), None, groups=c // gd))
    elif t == P.OP_LITEMLA:
        assert not mag, "LiteMLA has no linear magnitude pass: see litemla_parts"
        num, den = litemla_parts(op, bufs[op["in0"]], bufs[op["in1"]], mutant=mutant)
        dim = op["p0"]
        eps = 0.0 if mutant == "no_eps" else 1e-5
        o = num / (den + eps).repeat_interleave(dim, -1)
        out = o.reshape(o.shape[0], op["hin"], op["win"], op["cout"])
    elif t == P.OP_UPCAT:
        src = bufs[op["in0"]]
        if op["out"] not in bufs:
            bufs[op["out"]] = torch.zeros(src.shape[0], op["hout"], op["wout"], op["cout"], dtype=src.dtype)
        up = round_to(_repeat_last_group(_nhwc(_resize(_nchw(src), (op["hout"], op["wout"]), mutant)), V, mutant), storage)
        p0 = op["p0"]
        if mutant == "p0_off_group":
            p0 = p0 + V if p0 + op["cin"] + V <= op["cout"] else max(p0 - V, 0)
        bufs[op["out"]][..., p0: p0 + op["cin"]] = up
        return
    elif t == P.OP_UPSUM_SRC:
        st.addends.append(bufs[op["in0"]])
        return
    elif t in (P.OP_CLASSIFY, P.OP_UPSUM_CLASSIFY):
        y = bufs[op["in0"]]
        if t == P.OP_UPSUM_CLASSIFY:
            y = upsum_v(op, y, st.addends, mutant=mutant)
            st.addends = []
            if not mag:
                y = round_to(F.relu(y), storage)       # the kernel rounds relu(v) to the storage type: what the reference stores after its ReLU
        y = _repeat_last_group(y, V, mutant)
        st.y = y
        st.z = _nchw(y @ W_.t() + b_) if b_ is not None else _nchw(y @ W_.t())
        st.planes = st.z if mag else torch.special.expit(st.z)
        return
    elif t == P.OP_UPSAMPLE_OUT:
        st.heat = _resize(st.planes, (op["hout"], op["wout"]), mutant)
        return
    else:
        raise ValueError(f"unknown op type {t}")
    bufs[op["out"]] = round_to(_repeat_last_group(out, V, mutant), storage)


def run_plan_buffers(pl: P.DetPlan, x: torch.Tensor, *, dtype=torch.float64, storage=None, mutant=None):
    """The whole plan on pixels x [B, C, H, W]: arithmetic in `dtype`; with storage = torch.bfloat16 / float16 the weights and the
    input are rounded to it first and every buffer when it is written (planes and heat stay unrounded).
    Returns (bufs: buffer id -> NHWC tensor, planes, heat)."""
    bufs, st = {}, PlanState()
    px = round_to(x.to(dtype), storage)
    for op in pl.ops:
        apply_op(pl, op, bufs, st, pixel_values=px, storage=storage, mutant=mutant)
    return bufs, st.planes, st.heat


def run_plan(pl: P.DetPlan, pixel_values: torch.Tensor):
    """pixel_values [B, 3, H, W] fp32 (normalised) -> (sigmoid planes [B, L, H/4, W/4], heat maps [B, L, H, W])."""
    _, planes, heat = run_plan_buffers(pl, pixel_values.float(), dtype=torch.float32)
    return planes, heat
