"""CPU: the per-kernel harness of the recognition engine's non-GEMM kernels (tests/rec_ops_ref.py) checks itself.
  * the bounds hold: for every case of the GPU matrix (tests/test_gpu_rec_ops.py) the fp32 evaluation of the reference, rounded where the
    kernel rounds, stays inside the bound on every element;
  * the bounds bite: every deliberately wrong evaluation a case is meant to catch (Case.kills) leaves the bound on it, every mutant of
    rec_ops_ref.MUTANTS is caught by at least one case, and the RoPE-table mutants -- whose margin is not derived from the kernel -- exceed it
    by orders of magnitude;
  * inputs are values of the dtype the device gets them in, and no head case needed more than two redraws of its bbox rows."""
import pytest
import torch

import rec_ops_ref as R

CASES = R.all_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_reference_inside_bound_and_mutants_outside(case):
    ok, key = R.representable(case)
    assert ok, (case.id, key)
    assert case.redraws <= 2, (case.id, case.redraws)
    rep = R.check(case, R.emulate(case))
    worst = max(r for _, r, _, _ in rep)
    assert rep and all(over == 0 and finite for _, _, over, finite in rep), (case.id, rep)
    killers = []
    for mut in case.kills:
        assert mut in R.MUTANTS[case.family], mut
        r2 = R.check(case, R.evaluate(case, torch.float64, mut))
        if any(over > 0 for _, _, over, _ in r2):
            ratio = max(r for _, r, _, _ in r2)
            killers.append((mut, ratio))
            if case.family == "table":
                assert ratio > R.TABLE_MUTANT_MARGIN, (case.id, mut, ratio)
    print(f"{case.id} [{case.kernel}]: fp32 reference at {worst:.3f} of the bound; mutants over it: " + ", ".join(f"{m} x{r:.3g}" for m, r in killers))
    assert [m for m, _ in killers] == list(case.kills), f"{case.id}: not caught: {set(case.kills) - {m for m, _ in killers}}"


def test_every_mutant_has_a_case():
    for fam, muts in R.MUTANTS.items():
        for m in muts:
            assert any(c.family == fam and m in c.kills for c in CASES), (fam, m)


def test_the_issue_s_mutants_are_all_listed():
    listed = {m for muts in R.MUTANTS.values() for m in muts}
    want = {"slab_dropped", "norm_of_old_x", "eps_clamped", "mean_over_threads", "shadow_lanes_counted", "tie_takes_last", "tile_order",
            "sumexp_not_rescaled", "done_score_kept", "next_not_pad", "len_not_incremented", "row_len_unclamped", "bbox_no_bias", "bbox_rounds",
            "bbox_rows_shifted", "interleaved_pairs", "sin_sign", "pos_is_token_index", "k_head_off_by_nq", "v_rotated", "hw_swapped",
            "scatter_is_gather", "negative_id_written", "scale_wrong_ktile", "table_pos_off_by_one", "table_cos_sin_swapped"}
    assert want <= listed, want - listed
