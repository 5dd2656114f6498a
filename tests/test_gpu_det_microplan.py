"""GPU: every detector kernel alone, on a plan of one to three ops, against float64 under a bound that follows from the arithmetic
(tests/det_microplan.py: the plans, the bound, the walk). The model-level tests compare the 16-bit op list with the fp32 oracle only
through the whole network (max <= 3e-2 on the sigmoid map): a wrong border tap, a dropped channel group or a mis-clamped bilinear
neighbour disappears in that, and every form that is "bit-identical to the op list" would be identically wrong.

One case = one plan in one dtype: one tiny engine (HipDetModel.from_plan), then one forward per variant of the plan (sa::Tuning knobs:
dwconv_pipe, det_fuse, det_up4, det_head_blk), every activation buffer read back with surya_det_read_buffer, the planes through `lowres`
and the heat maps. EVERY element of every buffer is held to the bound and must be finite; the worst error / bound ratio per buffer is
printed. In front of every variant the op list runs once on other pixels, so an element a kernel never writes does not keep a right value
from an earlier run (under SURYA_AMD_POISON=1 the arena starts as NaN as well).
Which kernel each case reaches is written in the plan builders' docstrings and printed with the ratios."""
import ctypes as C

import pytest
import torch

import det_microplan as M
from surya_amd.detection import plan as P

pytestmark = pytest.mark.gpu

DEFAULTS = {"det_fuse": 1023, "dwconv_pipe": 2, "det_up4": 1, "det_head_blk": 1}
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
PLANS = M.all_microplans()
CASES = [(mp, dt) for mp in PLANS for dt in DTYPES if mp.f32 or dt != torch.float32]


def _tune(lib, knobs):
    from surya_amd import _lib as L
    for k, v in knobs.items():
        L.check(lib.surya_set_tuning(k.encode(), C.c_int(v)), "surya_set_tuning")


def _run(model, mp, variant):
    """One forward; everything the device wrote, on the host."""
    B = mp.x.shape[0]
    heat, low = model.forward(mp.x.cuda().contiguous(), want_lowres=True)
    skip = {mp.plan.ops[i]["out"] for i in variant.folded}
    bufs = {b: model.read_buffer(b, B, shape).cpu() for b, shape in mp.shapes.items() if b not in skip}
    planes = heat_out = None
    for op in mp.plan.ops:
        if op["type"] in (P.OP_CLASSIFY, P.OP_UPSUM_CLASSIFY):
            n = B * op["cout"] * op["hin"] * op["win"]
            planes = low.flatten()[:n].view(B, op["cout"], op["hin"], op["win"]).cpu()
        if op["type"] == P.OP_UPSAMPLE_OUT:
            n = B * op["cout"] * op["hout"] * op["wout"]
            heat_out = heat.flatten()[:n].view(B, op["cout"], op["hout"], op["wout"]).cpu()
    return M.Candidate(bufs, planes, heat_out)


@pytest.mark.parametrize("mp,dtype", CASES, ids=[f"{m.name}-{str(d).split('.')[-1]}" for m, d in CASES])
def test_kernel_alone_vs_float64(hip_lib, mp, dtype):
    from surya_amd.detection.model import HipDetModel
    storage = None if dtype == torch.float32 else dtype
    model = HipDetModel.from_plan(mp.plan, height=mp.height, width=mp.width, num_labels=mp.labels, dtype=dtype, max_batch=mp.x.shape[0])
    failures = []
    try:
        for v in mp.variants:
            if dtype == torch.float32 and not v.f32:
                continue
            # scrub: the op list on OTHER pixels overwrites every buffer, the planes and (through the allocator's reuse) the heat maps, so an
            # element this variant's kernels fail to write holds another input's value -- not what an earlier variant or case left there
            _tune(hip_lib, {**DEFAULTS, "det_fuse": 0})
            model.forward((0.5 - mp.x.flip(0)).cuda().contiguous(), want_lowres=True)
            _tune(hip_lib, {**DEFAULTS, **v.tuning})
            if v.silent:
                # the fused form really took these ops: surya_det_forward_timed reports 0 ms for an op that did not run
                _, rows = model.forward_timed(mp.x.cuda().contiguous())
                assert all(rows[i][1] == 0.0 for i in v.silent), (mp.name, v.tuning, [ms for _, ms in rows])
            rep = M.check_candidate(mp, storage, _run(model, mp, v), v.folded)
            print(f"{mp.name} {str(dtype).split('.')[-1]} {v.tuning} [{v.kernel}]: " +
                  ", ".join(f"{what} {ratio:.3f}" for what, ratio, _, _ in rep))
            failures += [(v.tuning, what, ratio, over) for what, ratio, over, finite in rep if over or not finite]
    finally:
        _tune(hip_lib, DEFAULTS)
    assert not failures, f"{mp.name}: elements over the bound (tuning, buffer, worst error / bound, count): {failures}"


REFUSALS = M.refusal_cases()


@pytest.mark.parametrize("name,pl,kw,code", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_create_refuses(hip_lib, name, pl, kw, code):
    """Every parameter the create-time validation rejects comes back as its error code from surya_det_create; nothing is launched."""
    assert M.create_rc(pl, **kw) == code
