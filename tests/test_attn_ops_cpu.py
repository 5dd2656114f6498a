"""CPU: the per-kernel harness of the attention kernels (tests/attn_ops_ref.py) checks itself.
  * the bounds hold: for every case of the GPU matrix (tests/test_gpu_attn_ops_f64.py) the fp32 evaluation in the kernel's order of operations,
    rounded where the kernel rounds, stays STRICTLY inside the bound on every element (the worst ratio per family and dtype is printed);
  * the bounds bite: every deliberately wrong evaluation a case is meant to catch (Case.kills) leaves the bound on it, and every mutant of
    attn_ops_ref.MUTANTS is caught by at least one case;
  * the constructions are what they claim: a marked key holds >= 0.9 of its query's weight and the forbidden key, made visible, misses the bound
    by a factor >= 10; the uniform cases needed few redraws and every element is away from a rounding boundary; the late-spike rows raise the
    running maximum more than once and leave fp16 subnormals; poison is where the text says;
  * the two MXFP8 hooks refuse what they cannot run before anything is launched."""
import collections
import math

import pytest
import torch

import attn_ops_ref as R
from surya_amd import _lib as L

CASES = R.all_cases()
F64 = torch.float64
WORST = collections.defaultdict(float)


def _fam(c):
    return ("kv8" if c.p.get("kv8") else c.family) + "-" + c.p["family"] + "-" + R.DT_NAME[c.dtype]


def _mut_family(m):
    return next(f for f, ms in R.MUTANTS.items() if m in ms)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_emulation_inside_bound_and_mutants_outside(case):
    emu = R.emulate(case)
    worst = 0.0
    for pinned in ((True, False) if case.family == "dec" else (True,)):
        rep = R.check(case, emu, pinned=pinned)
        assert rep and all(over == 0 and finite for _, _, over, finite in rep), (case.id, pinned, rep)
        worst = max(worst, max(r for _, r, _, _ in rep))
    assert worst < 1.0, (case.id, worst)                           # strictly inside
    WORST[_fam(case)] = max(WORST[_fam(case)], worst)
    killers = []
    for mut in case.kills:
        assert any(mut in ms for ms in R.MUTANTS.values()), mut
        r2 = R.check(case, R.evaluate(case, F64, mut))
        if R.outside(r2):
            killers.append((mut, max(r for _, r, _, _ in r2)))
    print(f"{case.id} [{case.kernel}]: fp32 emulation at {worst:.3f} of the bound; mutants outside: " + ", ".join(f"{m} x{r:.3g}" for m, r in killers))
    assert [m for m, _ in killers] == list(case.kills), f"{case.id}: not caught: {set(case.kills) - {m for m, _ in killers}}"


def test_worst_ratio_per_family():
    """Printed after the parametrised test above ran (file order): the fp32 emulation's worst error / bound per family and dtype."""
    for k in sorted(WORST):
        print(f"ATTNOPS-CPU {k}: {WORST[k]:.3f}")
        assert WORST[k] < 1.0


def test_every_mutant_has_a_case():
    for fam, muts in R.MUTANTS.items():
        for m in muts:
            assert any(m in c.kills for c in CASES), (fam, m)
    for c in CASES:                                                # a case lists only mutants of its own kind
        for m in c.kills:
            f = _mut_family(m)
            assert f == c.family or (f == "kv8" and c.p.get("kv8")) or (f == "mx" and c.p.get("mx")), (c.id, m)


def test_matrix_is_the_one_the_issue_sets():
    seg = [c for c in CASES if c.family == "seg"]
    dec = [c for c in CASES if c.family == "dec" and not c.p["kv8"]]
    kv8 = [c for c in CASES if c.family == "dec" and c.p["kv8"]]
    for dt in R.DTYPES:
        assert {c.p["D"] for c in seg if c.dtype == dt and not c.p["causal"]} == {32, 64, 80, 128}
        assert {(c.p["D"], c.p["heads"], c.p["group"]) for c in seg if c.dtype == dt and c.p["causal"]} == {(128, 10, 5)}
        assert {(c.p["d"], c.p["nq"] // c.p["nkv"]) for c in dec if c.dtype == dt} == set(R.HEAD_SHAPES)
        assert {c.p["S"] for c in dec if c.dtype == dt} == {1, 2, 3, 4, 5, 7, 8}
        for fams in ({c.p["family"] for c in seg if c.dtype == dt}, {c.p["family"] for c in dec if c.dtype == dt}):
            assert fams == {"random", "uniform", "marked", "spike", "poison"}
    for c in seg:
        assert tuple(c.p["lens"]) == R.SEG_LENS and (2 <= c.p["heads"] <= 4 or c.p["causal"])
        assert c.p["o_row"] > c.p["heads"] * c.p["D"]
    for c in dec + kv8:
        assert tuple(c.t["lens"].tolist()) == R.DEC_LENS and max(R.DEC_LENS) == c.p["Tmax"] - 1
        sl = c.t["slots"].tolist()
        assert len(set(sl)) == len(sl) and c.p["n_slots"] == len(sl) + R.SPARE_SLOTS and sl != sorted(sl)
    assert {(c.p["d"], c.p["nq"] // c.p["nkv"]) for c in kv8} == {(128, 5), (64, 4)} and all(c.dtype == torch.bfloat16 for c in kv8)
    assert any(c.p["mx"] and c.p["nq"] * c.p["d"] > 128 for c in dec) and any(c.p["mx"] for c in kv8)


def test_inputs_are_values_of_their_types_and_slabs_are_exact():
    for c in CASES:
        for k, v in c.t.items():
            if torch.is_tensor(v) and v.is_floating_point():
                want = torch.float32 if k in ("part", "rope", "ksc", "vsc") else (torch.bfloat16 if c.p.get("kv8") else c.dtype)
                assert v.dtype == want, (c.id, k)
        if c.family == "dec":
            S = c.p["S"]
            fwd = c.t["bias"].float() + 0
            for s in range(S):
                fwd = fwd + c.t["part"][s]
            rev = c.t["part"][:S].flip(0).sum(0) + c.t["bias"].float()
            assert torch.equal(fwd, rev) and torch.equal(fwd.to(c.t["bias"].dtype).float(), fwd), c.id      # any order, and T(.) is the identity
            assert bool(torch.isnan(c.t["part"][S:]).all())


def test_marked_keys_carry_the_weight_and_forbidden_keys_would_show():
    n = 0
    for c in CASES:
        if c.p["family"] != "marked":
            continue
        n += 1
        if c.family == "seg":
            H, G, D = c.p["heads"], c.p["group"], c.p["D"]
            for sg in c.p["segs"]:
                L = sg["L"]
                q = R._strided(c.t["q"], sg["q_off"], L, c.p["q_row"], H, c.p["q_head"], D).to(F64).permute(1, 0, 2)
                k = R._strided(c.t["k"], sg["k_off"], L, c.p["k_row"], H // G, c.p["k_head"], D).to(F64).permute(1, 0, 2)[torch.arange(H) // G]
                s = (q @ k.transpose(-1, -2) * c.p["scale"]).masked_fill(~R._seg_vis(L, L, c.p["causal"], None), -math.inf)
                pr = torch.softmax(s, -1).permute(1, 0, 2)                                      # [L, H, L]
                mk = sg["marks"]
                sel = mk >= 0
                got = pr.gather(-1, mk.clamp(min=0)[..., None])[..., 0]
                assert bool((got[sel] >= 0.9).all()), (c.id, L, float(got[sel].min()))
                assert L < 3 or bool((~sel).any()), (c.id, L)
            leak = "causal_plus_one" if c.p["causal"] else "segment_leak"
        else:
            mk = c.p["marks"]
            assert bool((mk == -1).any()) and bool((mk == c.t["lens"].long()[:, None]).any()) and bool((mk == 0).any())
            leak = "reads_row_past_len"
        rep = R.check(c, R.evaluate(c, F64, leak))
        assert max(r for _, r, _, _ in rep) >= 10.0, (c.id, leak, rep)
    assert n >= 9


def test_marked_decode_weights():
    for c in CASES:
        if c.family == "dec" and c.p["family"] == "marked":
            pm = R.reference(c)[1]["pmark"]
            sel = c.p["marks"] >= 0
            assert bool(sel.any()) and bool((pm[sel] >= 0.9).all()), (c.id, float(pm[sel].min()))


def test_uniform_cases_needed_few_redraws_and_are_unambiguous():
    n = 0
    for c in CASES:
        if c.p["family"] != "uniform":
            continue
        n += 1
        if c.dtype == torch.float32:
            assert c.redraws == 0
            continue
        out = R.FAMILIES[c.family](c, F64)[0]["out"]
        own = c.p["own"] if c.family == "seg" else torch.ones_like(out, dtype=torch.bool)
        assert bool(R._far(torch.nan_to_num(out), c.dtype)[own].all()), c.id                 # no element is exempt
        cols = sum(sg["L"] > 0 for sg in c.p["segs"]) * c.p["heads"] // c.p["group"] * c.p["D"] if c.family == "seg" else c.p["M"] * c.p["nkv"] * c.p["d"]
        print(f"ATTNOPS-CPU {c.id}: {c.redraws} redrawn V columns of {cols}")
        assert c.redraws <= cols // 4, (c.id, c.redraws, cols)
    assert n >= 12


def test_spike_cases_raise_the_maximum_and_leave_fp16_subnormals():
    for c in CASES:
        if c.p["family"] != "spike":
            continue
        if c.family == "seg":
            sg = c.p["segs"][-1]                                                               # the 200-key segment: chunks 0, 1 and 3
            H, D, L = c.p["heads"], c.p["D"], sg["L"]
            q = R._strided(c.t["q"], sg["q_off"], L, c.p["q_row"], H, c.p["q_head"], D).to(F64).permute(1, 0, 2)
            k = R._strided(c.t["k"], sg["k_off"], L, c.p["k_row"], H // c.p["group"], c.p["k_head"], D).to(F64).permute(1, 0, 2)[torch.arange(H) // c.p["group"]]
            s = (q @ k.transpose(-1, -2) * c.p["scale"]).masked_fill(~R._seg_vis(L, L, c.p["causal"], None), -math.inf)
            rises = R._rises(s, R._seg_groups(torch.bfloat16, L))
            assert float(rises[:, -1].min()) >= 3, c.id                                       # the last query sees all three
            e = torch.exp(s[:, -1] - s[:, -1].amax(-1, keepdim=True))
            assert float(e.sort(-1).values[:, -2].max()) < 2.0 ** -14, c.id                    # everything but the spike: fp16 subnormal or zero
        else:
            assert "wave_record_unshifted" in c.kills or c.dtype == torch.float32
            e2 = R.reference(c)[1]["e2"]
            assert float(e2.max()) < 2.0 ** -14, (c.id, float(e2.max()))                        # everything but the top spike: fp16 subnormal or zero
            aux, ln = R.reference(c)[1], c.t["lens"]
            if c.dtype == torch.float32 and not c.p["kv8"]:                                     # one group of 64- / 128-key tiles: first and last tile
                assert float(aux["rises"][ln >= 144].min()) >= 2, c.id
                continue
            second = 261 if c.p["kv8"] else 131                                                 # contexts that hold wave 0's spike of its second tile
            assert bool((ln >= second).any()) and float(aux["rises"][ln >= second].min()) >= 3, c.id   # two rises in one wave + the combine
            assert float(aux["spread"][ln >= 42].min()) >= 10.0, c.id                           # the waves' records differ: keys 5 and 40 and the last key


def test_poison_is_where_the_text_says():
    for c in CASES:
        if c.p["family"] != "poison":
            continue
        if c.family == "seg":
            own_rows = c.p["own"].any(1)
            q = c.t["q"].float()
            assert bool(torch.isnan(q[~own_rows]).all()) and not bool(torch.isnan(q[own_rows][:, :c.p["heads"] * c.p["D"]]).any())
            if c.p["causal"]:
                for sg, sl in zip(c.p["segs"], c.p["slots"]):
                    assert bool(torch.isnan(c.t["k"][sl, :, sg["L"]:].float()).all()) and not bool(torch.isnan(c.t["k"][sl, :, :sg["L"]].float()).any())
        elif not c.p["kv8"]:
            for r, ln in enumerate(R.DEC_LENS):
                sl = int(c.t["slots"][r])
                for kv in (c.t["kc"], c.t["vc"]):
                    assert bool(torch.isnan(kv[sl, :, ln:].float()).all()) and not bool(torch.isnan(kv[sl, :, :ln].float()).any())
        else:
            for r, ln in enumerate(R.DEC_LENS):
                sl = int(c.t["slots"][r])
                assert bool((c.t["k8"][sl, :, ln:] == 0x7f).all()) and bool(torch.isnan(c.t["ksc"][sl, :, ln:]).all())
                assert bool(torch.isfinite(c.t["vsc"][sl]).all()) and bool((c.t["vsc"][sl, :, ln:] == 1024.0).all())


def test_mx_hooks_refuse_before_any_launch(hip_lib):
    """NULL copy pointers, srows < rows, heads * head_dim off the 128-column scale tiles: SA_ERR_ARG; dtypes whose kernels have no copy:
    SA_ERR_UNSUPPORTED. None of these reaches the device (the pointers are made up)."""
    p, s = 4096, None
    A, U_ = L.SA_ERR_ARG, L.SA_ERR_UNSUPPORTED
    lib = hip_lib
    dec = lambda dt, d, heads, kvh, o8, so, srows, rows=2: lib.surya_op_decode_attn_mx(dt, d, p, 1, p, p, p, p, p, p, p, rows, heads, kvh, 64, 0.1, s, o8, so, srows)
    kv8 = lambda d, heads, kvh, o8, so, srows, rows=2: lib.surya_op_decode_attn_kv8_mx(d, p, 1, p, p, p, p, p, p, p, p, p, rows, heads, kvh, 64, 0.1, s, o8, so, srows)
    for dt in (L.DTYPE_F32, L.DTYPE_BF16, L.DTYPE_F16):
        assert dec(dt, 128, 10, 2, None, p, 2) == A
        assert dec(dt, 128, 10, 2, p, None, 2) == A
        assert dec(dt, 128, 10, 2, p, p, 1) == A                   # srows < rows
        assert dec(dt, 32, 2, 2, p, p, 2) == A                     # 64 columns: no whole scale tile
        assert dec(dt, 128, 10, 2, p, p, 2, rows=0) == A
        assert dec(dt, 128, 10, 3, p, p, 2) == A                   # heads % kv_heads
    for d, heads in ((128, 10), (128, 16), (64, 8), (32, 4)):
        assert dec(L.DTYPE_F32, d, heads, 2, p, p, 2) == U_        # decode_attn_mfma_kernel has no copy
        assert dec(L.DTYPE_F16, d, heads, 2, p, p, 2) == U_        # nor has the fp16 form of decode_attn_flash2_kernel
    assert dec(7, 128, 10, 2, p, p, 2) == U_
    assert dec(L.DTYPE_BF16, 96, 4, 2, p, p, 2) == U_              # no rung of the ladder
    assert kv8(128, 10, 2, None, p, 2) == A and kv8(128, 10, 2, p, None, 2) == A and kv8(128, 10, 2, p, p, 1) == A
    assert kv8(32, 2, 2, p, p, 2) == A and kv8(128, 10, 3, p, p, 2) == A
    assert kv8(96, 4, 2, p, p, 2) == U_ and kv8(128, 18, 2, p, p, 2) == U_
