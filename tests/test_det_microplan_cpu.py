"""CPU: the micro-plan harness of tests/det_microplan.py checks itself. For every plan of the GPU matrix (tests/test_gpu_det_microplan.py)
and every storage type:
  * the reference alone stays inside the bound: the interpreter in fp32 (outputs rounded to the storage type) against float64;
  * the bound bites: at least one of a fixed list of wrong interpreters (det_plan_interp.MUTANTS: replicated border padding, kx / ky
    swapped, the last 16-byte channel group repeated, LiteMLA's last token dropped, align_corners=True, UPCAT's channel offset off by one
    group, LiteMLA's eps omitted) leaves it on at least one element. A plan that no mutant can fail tests nothing."""
import pytest
import torch

import det_microplan as M
import det_plan_interp as I
from surya_amd.detection import plan as P

PLANS = M.all_microplans()
NAMES = {None: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}


def _applies(mut, mp):
    """A mutant that changes nothing in a plan's ops is not run (it cannot leave the bound)."""
    types = {o["type"] for o in mp.plan.ops}
    spatial = any(o["type"] in (P.OP_CONV, P.OP_DWCONV) and o["k"] > 1 and "pick" not in o["tag"] for o in mp.plan.ops)
    return {"pad_replicate": spatial, "swap_kxky": spatial, "last_group_repeat": True,
            "drop_last_token": P.OP_LITEMLA in types, "no_eps": "smallD" in mp.name,
            "align_corners": bool(types & {P.OP_UPCAT, P.OP_UPSUM_CLASSIFY, P.OP_UPSAMPLE_OUT}), "p0_off_group": P.OP_UPCAT in types}[mut]


@pytest.mark.parametrize("mp", PLANS, ids=[m.name for m in PLANS])
def test_reference_inside_bound_and_mutants_outside(mp):
    for storage in M.STORAGES:
        if storage is None and not mp.f32:
            continue
        rep = M.check_candidate(mp, storage, M.interp_candidate(mp, storage))
        worst = max(r for _, r, _, _ in rep)
        assert rep and all(over == 0 and finite for _, _, over, finite in rep), (mp.name, NAMES[storage], rep)
        killers = []
        for mut in I.MUTANTS:
            if not _applies(mut, mp):
                continue
            r2 = M.check_candidate(mp, storage, M.interp_candidate(mp, storage, dtype=torch.float64, mutant=mut))
            if any(over > 0 for _, _, over, _ in r2):
                killers.append((mut, max(r for _, r, _, _ in r2)))
        print(f"{mp.name} {NAMES[storage]}: fp32 reference at {worst:.3f} of the bound; mutants over it: " +
              ", ".join(f"{m} x{r:.3g}" for m, r in killers))
        assert killers, f"{mp.name} {NAMES[storage]}: no mutant leaves the bound"
        if "smallD" in mp.name:
            assert any(m == "no_eps" for m, _ in killers), f"{mp.name} {NAMES[storage]}: the eps is invisible"


REFUSALS = M.refusal_cases()


@pytest.mark.parametrize("name,pl,kw,code", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_create_refuses_on_the_host(hip_lib, name, pl, kw, code):
    """surya_det_create's validation runs before anything is allocated or launched, so it needs no device: every op that does not fit its
    buffers, and every parameter no kernel takes, comes back as the documented error code."""
    assert M.create_rc(pl, **kw) == code
