"""CPU: the per-kernel harness of the GEMM (tests/gemm_ops_ref.py) checks itself.
  * the bounds hold: for every problem of the GPU matrix (tests/test_gpu_gemm_ops.py) the fp32 evaluation -- fp32 accumulation K-tile by K-tile,
    rounded where the kernel rounds -- stays inside the bound on every element, strictly where there is a bound, and is bit-equal on grid
    data where the text says bit for bit (the worst ratio per arm and dtype is printed);
  * the bounds bite: every deliberately wrong evaluation a case lists (Case.kills) leaves the bound on it, and every mutant has a case;
  * the matrix is the one the arms' table sets: every case's knobs reach the kernel its arm names (route() restates launch_gemm's choice;
    the GPU file confirms the two arms a launch reports on: the slice count and the ring's status word), shapes are the table's: two tile rows and
    columns where the arm allows, a ragged last tile row (below 32 rows except at the table's 300 rows) and a last tile column of one 16-byte chunk;
  * launch_gemm refuses K = 0, misaligned strides and bases before any launch (made-up pointers: nothing reaches a device).
Cases that differ in knobs only share one problem (inputs, reference, bound): each problem is evaluated once."""
import collections
import ctypes as C

import pytest
import torch

import gemm_ops_ref as R
from surya_amd import _lib as L

CASES = R.all_cases()
F64 = torch.float64
WORST = collections.defaultdict(float)
PROBLEMS = {}
for _c in CASES:
    PROBLEMS.setdefault(_c.key, []).append(_c)
FIRST = [v[0] for v in PROBLEMS.values()]


@pytest.mark.parametrize("case", FIRST, ids=[c.id for c in FIRST])
def test_emulation_inside_bound_and_mutants_outside(case):
    same = PROBLEMS[case.key]
    kills = sorted({m for c in same for m in c.kills})
    assert all(sorted(c.kills) == kills for c in same), case.id            # knob variants of a problem list the same mutants
    rep = R.check(case, R.emulate(case), keep=False)
    worst = max(r for _, r, _, _ in rep)
    assert all(over == 0 and finite for _, _, over, finite in rep), (case.id, rep)
    _, tol = R.reference(case, keep=False)
    exact = all(v is None for v in tol.values())
    assert (worst == 0.0) if exact else (worst < 1.0), (case.id, worst)
    if case.p["data"] == "grid" and case.p["epi_name"] in ("bias", "nobias", "relu", "f32out", "residual", "residual_inplace", "slabs"):
        assert exact, case.id                                               # bit for bit, as the text says
    for c in same:
        WORST[(c.arm, R.DT_NAME[c.dtype])] = max(WORST[(c.arm, R.DT_NAME[c.dtype])], worst)
    killers = []
    for mut in kills:
        assert mut in R.MUTANTS[case.family], mut
        r2 = R.check(case, R.evaluate(case, F64, mut), keep=False)
        if R.outside(r2):
            killers.append(mut)
    assert killers == kills, f"{case.id}: not caught: {set(kills) - set(killers)}"


def test_worst_ratio_per_arm():
    """Printed after the parametrised test above ran (file order): the fp32 emulation's worst error / bound per arm and dtype."""
    for k in sorted(WORST):
        print(f"GEMMOPS-CPU {k[0]} {k[1]}: {WORST[k]:.3f}")
        assert WORST[k] < 1.0


def test_every_mutant_has_a_case():
    for fam, muts in R.MUTANTS.items():
        for m in muts:
            assert any(m in c.kills for c in CASES if c.family == fam), (fam, m)
    for c in CASES:
        if "operand_truncated_to_10_bits" in c.kills:
            assert c.dtype == torch.float32 and c.p["data"] == "random", c.id


def test_every_case_reaches_the_kernel_its_arm_names():
    for c in CASES:
        assert c.kernel == c.p["expect"](c), (c.id, c.kernel, c.p["expect"](c))
    kernels = {c.kernel for c in CASES}
    for k in ("gemm_nt 64x64", "gemm_nt 64x32", "gemm_nt 128x32", "gemm_nt 128x64", "gemm_nt 64x64 glds2", "gemm_nt 64x64 glds3", "gemm_nt 64x64 glds4",
              "gemm_nt 128x128 glds0", "gemm_nt 128x128 glds2", "gemm_nt 128x128 glds3", "gemm_nt 256x256 2-stage", "gemm_nt 256x256 4-wave",
              "gemm_nt 256x256 8-phase", "gemm_nt_p8p", "gemm_ring 64x160", "gemm_ring 64x160 nt", "gemm_ring split 64x64", "gemm_nt split 64x64 glds4",
              "gemm_nt split 128x128 glds4", "gemm_nt split 128x64 glds4"):
        assert k in kernels, k


def test_matrix_is_the_one_the_table_sets():
    by_arm = collections.defaultdict(list)
    for c in CASES:
        by_arm[c.arm].append(c)
    kts = lambda arm, M, N: {c.p["nk"] for c in by_arm[arm] if c.p["M"] == M and c.p["N"] in (N, R.GLU_N.get(N))}
    assert kts("t64", 300, 136) == {1, 3}
    assert kts("t128", 1930, 2024) == {1, 2, 4, 5} and kts("t128", 3080, 2824) == {2}
    assert {c.knobs["glds"] for c in by_arm["t128"]} == {2, 3, 0} and all(c.knobs["bigtile"] == 0 for c in by_arm["t128"])
    assert kts("t128f32", 1930, 2024) == {3}
    assert kts("t256", 300, 520) == {1, 2, 3} and kts("t256w4", 300, 520) == {1, 2, 3, 4} and kts("t256", 4100, 4104) == {3}
    assert kts("p8", 300, 520) == {1, 2, 3, 4, 6} and kts("p8", 4100, 4104) == {2}
    assert kts("p8p", 300, 520) == {4, 6} and kts("p8p", 4100, 4104) == {4} and kts("p8p", 5700, 5704) == {4}
    assert kts("biggu1", 300, 528) == {4, 6} and kts("biggu2", 300, 528) == {4, 6}
    assert kts("narrow", 32773, 64) == {1} and kts("narrow", 32773, 40) == {1}
    for M in (1, 63):
        assert kts("m64", M, 136) == {1, 3} and kts("m64", M, 8200) == {1, 3}
    assert kts("m128", 100, 136) == {1, 3} and kts("m128", 100, 8200) == {1, 3}
    assert kts("m256", 200, 136) == {1, 2, 3} and kts("m256", 200, 32776) == {1, 2, 3}
    assert kts("gateup", 200, 336) == {1, 2, 5}
    assert {(c.p["M"], c.p["nk"]) for c in by_arm["splitk"]} == {(M, nk) for M in (63, 200, 320) for nk in (8, 27)}
    assert {c.p["S"] for c in by_arm["splitk"]} == {2, 6}                      # pick_splitk at N = 328: 8 K-tiles -> 2 slices, 27 -> 6 (uneven: 4 or 5 tiles)
    # every arm and dtype: every epilogue the hook offers, on both kinds of data; one strided case
    for arm, cs in by_arm.items():
        if arm == "splitk" or arm.startswith("rope"):
            continue
        for dt in {c.dtype for c in cs}:
            mine = [c for c in cs if c.dtype == dt]
            for e in {c.p["epi_name"] for c in mine}:
                assert {c.p["data"] for c in mine if c.p["epi_name"] == e} == {"grid", "random"}, (arm, dt, e)
            assert any(c.p["ldx"] > c.p["K"] and c.p["ldw"] > c.p["K"] and c.p["ldc"] > c.p["N"] // (2 if c.p["epi"] == R.EPI_SWIGLU else 1) for c in mine), (arm, dt)
    full = set(R.EPIS_16)
    for arm in ("t64", "t128", "t256", "t256w4", "p8", "p8p", "narrow", "m64", "m128", "m256"):
        for dt in R.D16:
            assert full <= {c.p["epi_name"] for c in by_arm[arm] if c.dtype == dt}, (arm, dt)
    # shapes: a last tile row below 32 rows and a last tile column of one 16-byte chunk wherever there is more than one tile
    for c in CASES:
        p = c.p
        if c.family == "rope":
            continue
        n_out, w_out = (p["N"] // 2, p["bn"] // 2) if p.get("epi") == R.EPI_SWIGLU else (p["N"], p["bn"])
        chunk = 4 if R.out_dtype(c) == torch.float32 else 8
        if p["M"] > p["bm"] and p["M"] != 320:                                  # the table's rows: a ragged last tile row (320 split-K rows: whole tiles)
            assert p["M"] % p["bm"] != 0, c.id
            assert p["M"] % p["bm"] < 32 or (p["M"], p["bm"]) in ((300, 64), (300, 256), (5700, 256), (200, 128)), c.id
        if n_out > w_out and not (c.arm == "narrow"):                           # (the table's 2024, 5704 and 328 columns leave 104, 72 and 72 on 128 / 256)
            assert n_out % w_out in ((104, 72) if (n_out in (2024, 5704) or (n_out, w_out) == (328, 128)) else (8, chunk)), (c.id, n_out, w_out)
    big = [c for c in CASES if c.p.get("device_ref")]
    assert len(big) == 4 and all(2 <= c.p["nk"] <= 6 and c.p["epi_name"] == "bias" for c in big)
    for dt in R.D16:                                                            # ... and on the 4-wave kernel itself, not only under its knobs
        w4 = [c for c in by_arm["t256w4"] if c.dtype == dt and c.kernel == "gemm_nt 256x256 4-wave"]
        assert full <= {c.p["epi_name"] for c in w4} and {c.p["data"] for c in w4} == {"grid", "random"}
    rope = [c for c in CASES if c.family == "rope"]
    assert {c.p["D"] for c in rope} == {80, 32} and all(c.p["N"] == 6 * c.p["D"] and c.p["rope_cols"] == 4 * c.p["D"] for c in rope)
    assert {c.kernel for c in rope} == {"gemm_nt 64x64", "gemm_nt 128x128 glds2", "gemm_nt 256x256 8-phase", "gemm_nt_p8p"}


def test_inputs_are_values_of_their_types_and_grid_sums_are_exact():
    seen = set()
    for c in CASES:
        for k, v in c.t.items():
            if v is None:
                continue
            want = torch.float32 if k == "rope" else (R.out_dtype(c) if k == "r" else c.dtype)
            assert v.dtype == want, (c.id, k)
        if c.p["data"] != "grid" or c.key in seen or c.p["M"] > 400:
            continue
        seen.add(c.key)
        x, w = c.t["x"][:, :c.p["K"]].double(), c.t["w"][:, :c.p["K"]].double()
        assert c.p["K"] <= 3072 and float(x.abs().max()) <= 2 and float(w.abs().max()) <= 0.25
        fwd = R._prod(c.t["x"][:, :c.p["K"]], c.t["w"][:, :c.p["K"]], 0, c.p["K"], torch.float32, R.ke(c.dtype))
        assert torch.equal(fwd.double(), x @ w.T), c.id                         # the fp32 accumulation is the exact number


def test_launch_gemm_refuses_before_any_launch(hip_lib):
    """K <= 0, a row stride or a base off the 16-byte chunks, a bias off its 4 elements: SA_ERR_SHAPE from the host (the pointers are made
    up; a launch would fault). The same calls with every operand in order are not made here: they would launch."""
    lib, p, s = hip_lib, 4096, None
    SH = L.SA_ERR_SHAPE
    l = C.c_long
    for dt, chunk in ((L.DTYPE_F32, 4), (L.DTYPE_BF16, 8), (L.DTYPE_F16, 8)):
        g = lambda X=p, ldx=64, W=p, ldw=64, Cc=p, ldc=64, b=p, Rr=None, ldr=0, K=64, epi=L.EPI_BIAS: \
            lib.surya_op_gemm(dt, 0, epi, X, l(ldx), W, l(ldw), Cc, l(ldc), b, Rr, l(ldr), 300, 64, K, s)
        assert g(K=0) == SH and g(K=-64) == SH
        assert g(ldx=65) == SH and g(ldx=64 + chunk // 2) == SH and g(ldw=65) == SH and g(ldc=64 + chunk // 2) == SH
        assert g(X=p + 8) == SH and g(W=p + 8) == SH and g(Cc=p + 8) == SH and g(b=p + 2) == SH
        assert g(Rr=p, ldr=64 + chunk // 2, epi=L.EPI_RESIDUAL) == SH and g(Rr=p + 8, ldr=64, epi=L.EPI_RESIDUAL) == SH
        r = lambda rope=p, D=32, cols=64, ldx=64, K=64: lib.surya_op_gemm_rope(dt, p, l(ldx), p, l(64), p, l(96), p, rope, cols, D, 300, 96, K, s)
        assert r(K=0) == SH and r(ldx=65) == SH and r(rope=p + 8) == SH and r(D=30, cols=60) == SH
    sp = C.c_int(0)
    for f in (lib.surya_op_gemm_splitk_bf16, lib.surya_op_gemm_splitk_f16):
        assert f(p, l(512), p, l(512), p, 200, 328, 0, C.byref(sp), s) == SH
        assert f(p, l(513), p, l(512), p, 200, 328, 512, C.byref(sp), s) == SH
        assert f(p, l(512), p, l(516), p, 200, 328, 512, C.byref(sp), s) == SH
        assert f(p + 8, l(512), p, l(512), p, 200, 328, 512, C.byref(sp), s) == SH
        assert f(p, l(512), p, l(512), p + 8, 200, 328, 512, C.byref(sp), s) == SH
    assert lib.surya_op_rec_gemm_f16(0, L.EPI_SWIGLU, p, l(68), p, l(64), p, l(32), None, None, l(0), 300, 64, 64, None, None, s) == SH
    assert lib.surya_op_rec_gemm_f16(1, L.EPI_BIAS, p, l(64), p, l(64), p, l(64), None, None, l(0), 300, 64, 0, None, None, s) == SH
