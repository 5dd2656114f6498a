"""CPU: the per-kernel harness of the layout / table-recognition engine (tests/lay_ops_ref.py) checks itself, and the host-only window
tables are checked against the reference's own roll + pad + window_partition.
  * window tables: surya_lay_window_tables (what LayoutModel::init uploads) against oracle_window_tables on an index tensor;
  * the bounds hold: for every case of the GPU matrix (tests/test_gpu_lay_ops.py) the fp32 evaluation of the reference, rounded where the
    kernel rounds, stays inside the bound on every element;
  * the bounds bite: every deliberately wrong evaluation a case is meant to catch (Case.kills) leaves the bound on it, and every mutant of
    lay_ops_ref.MUTANTS is caught by at least one case."""
import ctypes as C

import numpy as np
import pytest
import torch

import lay_ops_ref as R
from surya_amd import _lib as L

CASES = R.all_cases()


# grid, shift asked, shift expected: one window; whole windows; padded; min side == window forces shift 0
GRIDS = [(8, 8, 0, 0), (16, 24, 0, 0), (16, 24, 4, 4), (12, 20, 0, 0), (12, 20, 4, 4), (11, 13, 0, 0), (11, 13, 4, 4), (8, 16, 4, 0)]


@pytest.mark.parametrize("h,w,shift,shift_used", GRIDS, ids=[f"{g[0]}x{g[1]}-s{g[2]}" for g in GRIDS])
def test_window_tables_match_the_reference_steps(hip_lib, h, w, shift, shift_used):
    perm_ref, pads_ref, (hp, wp), su = R.oracle_window_tables(h, w, 8, shift)
    assert su == shift_used
    perm = np.full(h * w, -1, dtype=np.int32)
    pads = np.full(max(1, hp * wp - h * w), -1, dtype=np.int32)
    n_pad, hw, used = C.c_int32(-1), (C.c_int32 * 2)(), C.c_int32(-1)
    rc = hip_lib.surya_lay_window_tables(h, w, 8, shift, L.np_ptr(perm), L.np_ptr(pads), C.byref(n_pad), hw, C.byref(used))
    assert rc == 0
    assert (hw[0], hw[1], used.value, n_pad.value) == (hp, wp, shift_used, hp * wp - h * w)
    assert np.array_equal(perm, perm_ref.numpy())
    assert np.array_equal(pads[:n_pad.value], pads_ref.numpy())
    # every window-order row is a token's or a padding row, once
    assert sorted(perm.tolist() + pads[:n_pad.value].tolist()) == list(range(hp * wp))


def test_window_tables_refuse(hip_lib):
    assert hip_lib.surya_lay_window_tables(7, 16, 8, 0, None, None, None, None, None) == L.SA_ERR_UNSUPPORTED
    assert hip_lib.surya_lay_window_tables(16, 16, 8, 8, None, None, None, None, None) == L.SA_ERR_ARG
    assert hip_lib.surya_lay_window_tables(0, 16, 8, 0, None, None, None, None, None) == L.SA_ERR_ARG


def test_cross_plan_matches_the_harness(hip_lib):
    for Lk in (1, 64, 127, 128, 143, 255, 256, 257, 576, 1024, 1025, 4096):
        ch, rg, lkp = C.c_int32(), C.c_int32(), C.c_int32()
        assert hip_lib.surya_lay_cross_plan(Lk, C.byref(ch), C.byref(rg), C.byref(lkp)) == 0
        assert (ch.value, rg.value, lkp.value) == R.cross_plan(Lk)
        assert rg.value * ch.value >= Lk > (rg.value - 1) * ch.value and rg.value <= 8


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_reference_inside_bound_and_mutants_outside(case):
    rep = R.check(case, R.emulate(case))
    worst = max(r for _, r, _, _ in rep)
    assert rep and all(over == 0 and finite for _, _, over, finite in rep), (case.id, rep)
    killers = []
    for mut in case.kills:
        assert mut in R.MUTANTS[case.family]
        r2 = R.check(case, R.evaluate(case, torch.float64, mut))
        if any(over > 0 for _, _, over, _ in r2):
            killers.append((mut, max(r for _, r, _, _ in r2)))
    print(f"{case.id} [{case.kernel}]: fp32 reference at {worst:.3f} of the bound; mutants over it: " + ", ".join(f"{m} x{r:.3g}" for m, r in killers))
    assert [m for m, _ in killers] == list(case.kills), f"{case.id}: not caught: {set(case.kills) - {m for m, _ in killers}}"


def test_every_mutant_has_a_case():
    for fam, muts in R.MUTANTS.items():
        for m in muts:
            assert any(c.family == fam and m in c.kills for c in CASES), (fam, m)


def test_own_embedding_equals_the_oracle():
    """embed_own carries the w / 2 mutant; unmutated it must be the oracle's embedding bit for bit."""
    for c in CASES:
        if c.family == "embed":
            assert torch.equal(R.embed_own(c).to(torch.float64), R.reference(c)[0]["x"])


def test_own_rmsnorm_equals_the_oracle():
    """The oracle's adetr_rms_norm computes in fp32 whatever it is given, so the float64 reference is written out in lay_ops_ref; evaluated in
    fp32 it must be the oracle's function bit for bit (clamped variance, 1 + w, the clamp to the dtype's range)."""
    from oracle import layout_oracle as LO
    for c in CASES:
        if c.family == "rms":
            assert torch.equal(LO.adetr_rms_norm(c.t["x"], c.t["w"], c.p["eps"]), R.emulate(c)["y"]), c.id
