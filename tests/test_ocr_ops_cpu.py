"""CPU: the per-kernel harness of the OCR-error classifier (tests/ocr_ops_ref.py) checks itself.
  * the bounds hold: for every case of the GPU matrix (tests/test_gpu_ocr_ops.py) the fp32 evaluation of the reference, rounded where the
    kernel rounds, stays inside the bound on every element;
  * the bounds bite: every deliberately wrong evaluation a case is meant to catch (Case.kills) leaves the bound on it, and every mutant of
    ocr_ops_ref.MUTANTS is caught by at least one case;
  * the cases are the ones they claim to be (starts off the 64-row grid, an ascending text that raises the running max in every chunk, fp16
    subnormals in the gap-11 spike row, ...);
  * the op-level hooks refuse what they cannot run before anything is launched."""
import ctypes as C

import numpy as np
import pytest
import torch

import ocr_ops_ref as R
from surya_amd import _lib as L

CASES = R.all_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_reference_inside_bound_and_mutants_outside(case):
    rep = R.check(case, R.emulate(case))
    worst = max(r for _, r, _, _ in rep)
    assert rep and all(over == 0 and finite for _, _, over, finite in rep), (case.id, rep)
    assert worst < 1.0, (case.id, rep)                            # strictly inside
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
        assert len(muts) >= 2, fam
        for m in muts:
            assert any(c.family == fam and m in c.kills for c in CASES), (fam, m)


def test_every_kernel_has_its_dtypes_and_shapes():
    by = lambda fam: [c for c in CASES if c.family == fam]
    for fam in ("ln", "embed_ln", "gather", "cls_head", "gemm"):
        assert {c.dtype for c in by(fam)} == set(R.DTYPES), fam
    assert {c.dtype for c in by("cls_attn")} == set(R.DTYPES16)
    for fam in ("ln", "embed_ln"):
        assert {(c.p["C"], c.p["rows"]) for c in by(fam)} >= {(C_, r) for C_ in (64, 256, 320, 768) for r in (1, 4, 5, 130)}
    assert {(c.p["heads"], c.p["D"]) for c in by("cls_attn")} == {(1, 32), (3, 80), (12, 64), (2, 128)}
    pinned = {(c.p["M"], c.p["N"], c.p["K"], c.p["ldx"] // c.p["K"], c.p["epi"], c.dtype) for c in by("gemm") if c.p["pinned"]}
    assert len(pinned) == 3 * 3 * 2 * 4 * 3
    assert {(c.p["epi"], c.dtype) for c in by("gemm") if not c.p["pinned"] and c.p["M"] == 300} == {(e, d) for e in R.GEMM_EPIS for d in R.DTYPES}


def test_embed_cases_reach_the_table_edges():
    for c in CASES:
        if c.family != "embed_ln":
            continue
        ids, tp = c.t["ids"].tolist(), c.t["tok_pos"].tolist()
        assert c.t["word"].shape[0] == R.VOCAB <= 64 and c.t["pos"].shape[0] == R.MAX_POS <= 520
        assert ids[0] == -5 and max(tp) <= R.MAX_POS - 1 and min(tp) >= 0
        if c.p["rows"] >= 4:
            assert ids[:4] == [-5, 0, R.VOCAB - 1, R.VOCAB + 3] and tp[2] == R.MAX_POS - 1 and c.p["same_rows"] == [(0, 1), (2, 3)]
        if c.p["rows"] >= 5:
            assert len(set(ids)) < len(ids) and len(set(tp)) < len(tp)              # repeated ids and positions


def test_attn_cases_are_what_they_claim():
    for c in CASES:
        if c.family != "cls_attn":
            continue
        p = c.p
        assert all(s % 64 for s in p["starts"]) and sorted(set(p["lens"])) == sorted(R.ATTN_LENS)
        for i, kind in enumerate(p["kinds"]):
            q, k, v, Ln = R._text_views(c, torch.float64, i)
            sc = torch.einsum("hd,lhd->hl", q, k) * p["scale"]
            cm = sc.view(p["heads"], -1, 64).amax(-1) if Ln % 64 == 0 else None
            if kind == "asc":
                assert bool((cm[:, 1:] > cm[:, :-1] + 1.0).all()), "every chunk must raise the running max"
            elif kind == "desc":
                assert bool((cm[:, 1:] < cm[:, :-1] - 1.0).all()), "chunk 0 must set the running max"
            elif kind.startswith("spike"):
                others = torch.cat([sc[:, :R.SPIKE_KEY], sc[:, R.SPIKE_KEY + 1:]], -1)
                pr = torch.exp(others - sc[:, R.SPIKE_KEY:R.SPIKE_KEY + 1])
                if kind == "spike24":
                    assert float(pr.max()) < 2.0 ** -25                              # everything else rounds to zero in fp16
                else:
                    assert float(pr.max()) < 2.0 ** -14 and float(pr.min()) > 2.0 ** -24, "the other entries must be fp16 subnormals"


def test_hooks_refuse_before_any_launch(hip_lib):
    """NULL pointers and sizes <= 0: SA_ERR_ARG; sizes the vector accesses cannot take: SA_ERR_SHAPE; what the kernels do not have:
    SA_ERR_UNSUPPORTED. None of these reaches the device (the pointers are made up)."""
    p, s = 4096, None
    A, S, U_ = L.SA_ERR_ARG, L.SA_ERR_SHAPE, L.SA_ERR_UNSUPPORTED
    lib = hip_lib
    for dt in (L.DTYPE_F32, L.DTYPE_BF16, L.DTYPE_F16):
        assert lib.surya_op_ocrerr_embed_ln(dt, None, p, p, p, p, p, p, 1, 64, 8, 1e-12, s) == A
        assert lib.surya_op_ocrerr_embed_ln(dt, p, p, p, p, p, p, p, 0, 64, 8, 1e-12, s) == A
        assert lib.surya_op_ocrerr_embed_ln(dt, p, p, p, p, p, p, p, 1, 66, 8, 1e-12, s) == S
        assert lib.surya_op_ocrerr_layernorm(dt, p, p, p, None, 1, 64, 1e-12, s) == A
        assert lib.surya_op_ocrerr_layernorm(dt, p, p, p, p, 1, 0, 1e-12, s) == A
        assert lib.surya_op_ocrerr_layernorm(dt, p, p, p, p, 1, 62, 1e-12, s) == S
        assert lib.surya_op_ocrerr_gather_rows(dt, p, None, p, 1, 64, s) == A
        assert lib.surya_op_ocrerr_gather_rows(dt, p, p, p, -1, 64, s) == A
        assert lib.surya_op_ocrerr_gather_rows(dt, p, p, p, 1, 6, s) == S
        assert lib.surya_op_ocrerr_cls_head(dt, p, p, p, p, None, 1, 64, 2, s) == A
        assert lib.surya_op_ocrerr_cls_head(dt, p, p, p, p, p, 1, 64, 0, s) == A
        assert lib.surya_op_ocrerr_gemm(dt, R.EPI_BIAS, 1, p, 64, p, p, None, None, 1, 64, 64, s) == A
        assert lib.surya_op_ocrerr_gemm(dt, R.EPI_BIAS, 1, p, 64, p, p, p, None, 0, 64, 64, s) == A
        assert lib.surya_op_ocrerr_gemm(dt, R.EPI_RESIDUAL, 1, p, 64, p, p, p, None, 1, 64, 64, s) == A          # residual without R
        assert lib.surya_op_ocrerr_gemm(dt, R.EPI_BIAS, 1, p, 64, p, p, p, None, 1, 64, 48, s) == S               # K in whole 128-byte chunks
        assert lib.surya_op_ocrerr_gemm(dt, R.EPI_BIAS, 1, p, 64, p, p, p, None, 1, 62, 64, s) == S
        assert lib.surya_op_ocrerr_gemm(dt, R.EPI_BIAS, 1, p, 32, p, p, p, None, 1, 64, 64, s) == S               # ldx < K
        assert lib.surya_op_ocrerr_gemm(dt, 3, 1, p, 64, p, p, p, None, 1, 64, 64, s) == U_                       # SwiGLU is not the classifier's
    assert lib.surya_op_ocrerr_layernorm(7, p, p, p, p, 1, 64, 1e-12, s) == U_
    _attn_refusals(lib)


def _attn_refusals(lib):
    p, s = 4096, None
    A, S, U_ = L.SA_ERR_ARG, L.SA_ERR_SHAPE, L.SA_ERR_UNSUPPORTED
    one, ln = np.asarray([3], dtype=np.int32), np.asarray([5], dtype=np.int32)
    st, lp = L.np_ptr(one), L.np_ptr(ln)
    big = L.np_ptr(np.asarray([513], dtype=np.int32))
    zero = L.np_ptr(np.asarray([0], dtype=np.int32))
    f = lib.surya_op_ocrerr_cls_attn
    assert f(L.DTYPE_F32, 64, p, st, lp, 1, p, 768, 12, 512, 0.125, s) == U_                # 16-bit storage only
    for dt in (L.DTYPE_BF16, L.DTYPE_F16):
        assert f(dt, 64, None, st, lp, 1, p, 768, 12, 512, 0.125, s) == A
        assert f(dt, 64, p, None, lp, 1, p, 768, 12, 512, 0.125, s) == A
        assert f(dt, 64, p, st, lp, 0, p, 768, 12, 512, 0.125, s) == A
        assert f(dt, 64, p, st, big, 1, p, 768, 12, 512, 0.125, s) == S                     # len > max_len
        assert f(dt, 64, p, st, zero, 1, p, 768, 12, 512, 0.125, s) == S                    # len < 1
        assert f(dt, 64, p, st, lp, 1, p, 768, 12, 4097, 0.125, s) == U_                    # max_len > 4096
        assert f(dt, 64, p, st, lp, 1, p, 768, 12, 4096, 0.125, s) == U_                    # 12 x 4096 floats of P: LDS over 64 KB
        assert f(dt, 48, p, st, lp, 1, p, 96, 2, 512, 0.125, s) == U_                       # head_dim not one of 32, 64, 80, 128
        assert f(dt, 36, p, st, lp, 1, p, 72, 2, 512, 0.125, s) == S                        # head_dim % 8
        assert f(dt, 64, p, st, lp, 1, p, 760, 12, 512, 0.125, s) == S                      # dim != heads * head_dim
