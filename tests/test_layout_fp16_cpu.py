"""CPU: the host half of the layout / table-recognition engine's float16 mode, and the per-kernel fp16 harness checking itself.

(a) polygons_of_predictions(dtype="float16") -- what LayoutPredictor's header / footer rule and the result polygons are computed with when
    the model runs in fp16 -- against torch fp16 TENSOR arithmetic in the operation order of the reference (surya/layout/util.py:4-40), on
    4096 random tokens that include boxes whose cx +- w / 2 and skewed corners pass 1024, where the fp16 spacing is 1: equal as float64.
    The bf16 and fp32 arms of the same function are unchanged: compared, on the same tokens, with the formulas they had before fp16 was
    added, restated here.
(b) tests/lay_ops_fp16.py (the helper of tests/test_gpu_lay_ops_fp16.py): the fp32 emulation ("the reference alone") of every fp16 case
    stays inside its bound, every mutant of lay_ops_ref.MUTANTS leaves it on at least one fp16 case, and the fp16-only cases bite: P with
    its subnormal entries flushed to zero is outside the bound, and the reference module restated in fp16 gives +-65504 / zeros on the
    overflow rows."""
import numpy as np
import pytest
import torch

import lay_ops_fp16 as H

F16 = torch.float16


# ------------------------------------------------------------------------------------------------ (a) polygon arithmetic
def _tokens(n=4096, seed=5):
    """Float tokens (cx, cy, w, h, xskew, yskew) as the loop forms them: box * 1024 in the model dtype. A quarter of them sit at the far
    edge with wide boxes and large skews, so cx + w / 2 and x2 + skew exceed 1024."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(0, 1024, size=(n, 6)).astype(np.float32)
    far = slice(0, n // 4)
    t[far, 0:2] = rng.uniform(900, 1024, size=(n // 4, 2))
    t[far, 2:4] = rng.uniform(300, 1024, size=(n // 4, 2))
    t[far, 4:6] = rng.uniform(512, 1024, size=(n // 4, 2))
    t[n // 4:n // 2, 4:6] = 512 + rng.uniform(-3, 3, size=(n // 4, 2))         # skews around zero: floor() and the skew_min rule
    sizes = rng.integers(50, 3000, size=(n, 2))
    return t, sizes


def _torch_polygons(tok, sizes, bbox_scaler, skew_scaler, dtype, skew_min=0.001):
    """surya/layout/util.py:4-40 with `pred` a tensor of `dtype`: the same statements, one row at a time vectorised over rows."""
    b = torch.from_numpy(tok).to(dtype)
    cx, cy, width, height = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    x1 = cx - width / 2
    y1 = cy - height / 2
    x2 = cx + width / 2
    y2 = cy + height / 2
    skew_x = torch.floor((b[:, 4] - skew_scaler) / 2)
    skew_y = torch.floor((b[:, 5] - skew_scaler) / 2)
    skew_x[torch.abs(skew_x) < skew_min] = 0
    skew_y[torch.abs(skew_y) < skew_min] = 0
    polygon = [x1 - skew_x, y1 - skew_y, x2 - skew_x, y1 + skew_y, x2 + skew_x, y2 + skew_y, x1 + skew_x, y2 - skew_y]
    w_scale, h_scale = sizes[:, 0] / bbox_scaler, sizes[:, 1] / bbox_scaler
    out = np.empty((tok.shape[0], 4, 2), np.float64)
    for i in range(4):
        out[:, i, 0] = polygon[2 * i].double().numpy() * w_scale             # .item() * scale: Python floats
        out[:, i, 1] = polygon[2 * i + 1].double().numpy() * h_scale
    return out


def test_fp16_polygons_equal_torch_fp16_arithmetic():
    from surya_amd.layout.predictor import polygons_of_predictions, _round_f16
    tok, sizes = _tokens()
    tok = _round_f16(tok)                                          # the tokens themselves are fp16 values (box * 1024 in the model dtype)
    got = polygons_of_predictions(tok, sizes, 1024, 512, dtype="float16")
    want = _torch_polygons(tok, sizes, 1024, 512, F16)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    # the spacing of 1 is exercised: corners above 1024 exist, and fp32 arithmetic on the same tokens gives other polygons there
    raw = want / (sizes[:, None, :] / 1024.0)
    assert (raw > 1024).sum() > 200
    f32 = polygons_of_predictions(tok, sizes, 1024, 512, dtype="float32")
    assert (f32 != got).any(axis=(1, 2)).sum() > 100


def test_round_f16_is_the_numpy_round_trip():
    from surya_amd.layout.predictor import _round_f16
    a = np.array([0.1, 1024.5, 1025.5, 2049.0, 65504.0, 1e-8, -3.3], np.float32)
    assert np.array_equal(_round_f16(a), a.astype(np.float16).astype(np.float32))
    assert _round_f16(a).dtype == np.float32 and _round_f16(a)[1] == 1024.0 and _round_f16(a)[2] == 1026.0      # ties to even


def _old_polygons(preds, sizes, bbox_scaler, skew_scaler, dtype, skew_min=0.001):
    """polygons_of_predictions as it was with two dtypes (bf16 by integer rounding of the fp32 bit pattern, fp32 as is)."""
    def rb(a):
        u = np.ascontiguousarray(a, np.float32).view(np.uint32)
        return ((u + (((u >> 16) & 1) + 0x7FFF)) & 0xFFFF0000).view(np.float32)
    R = rb if dtype in ("bfloat16", "bf16") else (lambda a: a)
    p = R(np.asarray(preds, np.float32))
    sz = np.asarray(sizes, np.float64).reshape(-1, 2)
    w_scale, h_scale = sz[:, 0] / bbox_scaler, sz[:, 1] / bbox_scaler
    two = np.float32(2)
    cx, cy = p[:, 0], p[:, 1]
    hw, hh = R(p[:, 2] / two), R(p[:, 3] / two)
    x1, y1, x2, y2 = R(cx - hw), R(cy - hh), R(cx + hw), R(cy + hh)
    skew_x = np.floor(R(R(p[:, 4] - np.float32(skew_scaler)) / two))
    skew_y = np.floor(R(R(p[:, 5] - np.float32(skew_scaler)) / two))
    skew_x = np.where(np.abs(skew_x) < skew_min, np.float32(0), skew_x)
    skew_y = np.where(np.abs(skew_y) < skew_min, np.float32(0), skew_y)
    xs = np.stack([R(x1 - skew_x), R(x2 - skew_x), R(x2 + skew_x), R(x1 + skew_x)], -1).astype(np.float64) * w_scale[:, None]
    ys = np.stack([R(y1 - skew_y), R(y1 + skew_y), R(y2 + skew_y), R(y2 - skew_y)], -1).astype(np.float64) * h_scale[:, None]
    return np.stack([xs, ys], -1)


@pytest.mark.parametrize("dtype", ["bfloat16", "bf16", "float32"])
def test_bf16_and_fp32_polygons_are_unchanged(dtype):
    from surya_amd.layout.predictor import polygons_of_predictions
    tok, sizes = _tokens()
    assert np.array_equal(polygons_of_predictions(tok, sizes, 1024, 512, dtype=dtype), _old_polygons(tok, sizes, 1024, 512, dtype))
    if dtype != "float32":
        assert np.array_equal(polygons_of_predictions(tok, sizes, 1024, 512, dtype=dtype),
                              _torch_polygons(tok, sizes, 1024, 512, torch.bfloat16))


def test_model_dtype_name():
    from types import SimpleNamespace
    from surya_amd.layout.predictor import model_dtype_name
    assert [model_dtype_name(SimpleNamespace(dtype=d)) for d in (torch.float32, torch.bfloat16, F16)] == ["float32", "bfloat16", "float16"]
    assert model_dtype_name(object()) == "float32"


# ------------------------------------------------------------------------------------------------ (b) the fp16 bounds
CASES = H.all_cases()


@pytest.mark.parametrize("case", CASES, ids=[H.case_id(c) for c in CASES])
def test_fp16_reference_inside_bound_and_mutants_outside(case):
    rep = H.check(case, H.emulate(case))
    worst = max(r for _, r, _, _ in rep)
    assert rep and all(over == 0 and finite for _, _, over, finite in rep), (H.case_id(case), rep)
    killers = []
    for mut in case.kills:
        assert mut in H.MUTANTS[case.family]
        r2 = H.check(case, H.evaluate(case, torch.float64, mut))
        if any(over > 0 for _, _, over, _ in r2):
            killers.append((mut, max(r for _, r, _, _ in r2)))
    print(f"{H.case_id(case)} [{case.kernel}]: fp32 reference at {worst:.3f} of the bound; mutants over it: " + ", ".join(f"{m} x{r:.3g}" for m, r in killers))
    assert [m for m, _ in killers] == list(case.kills), f"{H.case_id(case)}: not caught: {set(case.kills) - {m for m, _ in killers}}"


def test_every_mutant_has_an_fp16_case():
    """Every mutant a 16-bit case can catch is caught by an fp16 case. One mutant of lay_ops_ref.MUTANTS is out of reach of both 16-bit
    types and lay_ops_ref assigns it to fp32 cases alone: geglu's gelu_exact. The exact GELU differs from the tanh form by at most
    4.7e-4 absolute and 1.4e-4 |gate| relative to the gate, and the GEGLU bound carries 1.13 u |gate| for the rounding of the gate to
    storage: 1.1e-3 |gate| at u = 2^-10 (8.8e-3 |gate| in bf16), so the two forms lie inside each other's bound for every gate."""
    import lay_ops_ref as B
    sixteen = {(c.family, m) for c in B.all_cases() if c.dtype == torch.bfloat16 for m in c.kills}
    every = {(fam, m) for fam, muts in H.MUTANTS.items() for m in muts}
    assert every - sixteen == {("geglu", "gelu_exact")}
    for fam, m in sorted(sixteen):
        assert any(c.family == fam and m in c.kills for c in CASES), (fam, m)
    x = torch.linspace(-8, 8, 160001, dtype=torch.float64)
    diff = (0.5 * x * (1 + torch.erf(x / 2 ** 0.5)) - H.R._gelu_tanh(x)).abs()
    assert float(diff.max()) < 4.8e-4 and float((diff / x.abs().clamp(min=1e-9)).max()) < 1.13 * 2.0 ** -10


def test_fp16_case_list_is_the_bf16_list_plus_the_fp16_only_cases():
    """Same shapes as bf16 (tests/lay_ops_ref.py), fp16 inputs, u = 2^-10 and r_P = 2^-11 in the bounds; the LayerNorm widths of the
    row-in-registers kernel on both kernels."""
    import lay_ops_ref as B
    bf = [c for c in B.all_cases() if c.dtype == torch.bfloat16]
    mine = {c.name: c for c in CASES}
    assert all(c.dtype == F16 for c in CASES) and len(mine) == len(CASES)
    for c in bf:
        assert c.name in mine and mine[c.name].family == c.family and mine[c.name].kills == c.kills, c.name
        assert {k: v for k, v in mine[c.name].p.items()} == c.p, c.name
    for C in H.LN_ROWS_WIDTHS:
        kinds = {c.kernel for c in CASES if c.family == "ln" and c.p["C"] == C}
        assert kinds == {"layernorm_rows_bf16_kernel<fp16>", "layernorm_kernel<fp16>"}, (C, kinds)
    assert H.R.U[F16] == 2.0 ** -10 and torch.bfloat16 in B.U and F16 not in B.U          # the shared module is left as it is
    for c in CASES:
        if c.family in ("window", "cross", "prompt"):
            _, aux = H.R.FAMILIES[c.family](c, torch.float64, None)
            assert aux["rp"] == 2.0 ** -11
            break


@pytest.mark.parametrize("name", ["cross-subnormalP-Lk576", "win-subnormalP"])
def test_flushed_subnormal_p_is_outside_the_bound(name):
    """With every subnormal entry of P flushed to zero the gap-11 rows return the spike's V = -1 in every dimension: several times the bound.
    The gap-24 rows do not move (their other entries round to zero anyway)."""
    c = next(c for c in CASES if c.name == name)
    out = H.evaluate(c, torch.float64)["out"].clone()
    if c.family == "cross":
        flushed = out.clone()
        flushed[0] = -1.0                                          # row 0: gap 11
    else:
        flushed = out.clone()
        flushed[:32] = -1.0                                        # queries 0 .. 31: gap 11
    rep = H.check(c, {"out": flushed})
    ratio = max(r for _, r, _, _ in rep)
    print(f"{name}: flushed P at {ratio:.1f} x the bound")
    assert ratio > 3.0
    keep = out.clone()
    if c.family == "cross":
        keep[1] = -1.0
    else:
        keep[32:] = -1.0
    assert all(over == 0 for _, _, over, _ in H.check(c, {"out": keep}))


def test_reference_norm_in_fp16_clamps_to_65504_and_zeroes_the_inf_row():
    """The facts the overflow cases rest on, from the restated reference module on the CPU (surya/common/adetr/decoder.py:29-47)."""
    for c in CASES:
        if c.name == "rms-f16-overflow-inf":
            y = H.rms_f16(c.t["x"], c.t["w"], c.p["eps"])
            n = H.exact_norm_rows(c, y)
            assert n >= 16 and set(y[0].abs().unique().tolist()) != {65504.0}
            # the float64 reference of the harness agrees with the module on those rows
            ref = H.reference(c)[0]["y"]
            assert torch.equal(ref[1], torch.zeros_like(ref[1])) and torch.equal(ref[0].abs() == 65504.0, y[0].abs() == 65504.0)
            return
    raise AssertionError("case missing")
