"""CPU: tests/golden/rec_fp16.pt (tools/make_golden_rec_fp16.py) -- the reference's own fp16-vs-fp32 deviation on the recogniser's conditioned
REC-FULL fixtures -- is tied to those fixtures and fit to be the fp16 engine's yardstick (tests/test_gpu_rec_fp16.py)."""
import os

import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SETS = [("cond8", "rec_full_cond8.pt", 8), ("cond256", "rec_full_cond256.pt", 256)]


@pytest.fixture(scope="module")
def gold():
    return torch.load(os.path.join(GOLD, "rec_fp16.pt"))


def test_fixture_is_small_and_holds_numbers_only(gold):
    assert os.path.getsize(os.path.join(GOLD, "rec_fp16.pt")) < 512 * 1024
    assert set(gold) == {"cond8", "cond256"}

    def leaves(v):
        if isinstance(v, dict):
            for x in v.values():
                yield from leaves(x)
        elif isinstance(v, (list, tuple)):
            for x in v:
                yield from leaves(x)
        else:
            yield v
    for leaf in leaves(gold):
        assert isinstance(leaf, (int, float, torch.Tensor)), type(leaf)
        if isinstance(leaf, torch.Tensor):
            assert leaf.numel() <= 48 * 256                        # per-step, per-line numbers: no logits rows, no weights


@pytest.mark.parametrize("key,fname,n", SETS)
def test_keys_shapes_and_anchors(gold, key, fname, n):
    g, f = torch.load(os.path.join(GOLD, fname)), gold[key]
    steps = g["tokens"].shape[0]
    assert steps == 48 and g["tokens"].shape == (48, n)
    assert f["fp16_dev"].shape == (48, n) and f["fp16_dev"].dtype == torch.float32
    assert f["fp16_free_tokens"].shape == (48, n) and f["fp16_free_tokens"].dtype == torch.int64
    assert torch.equal(f["tokens"], g["tokens"])
    assert f["tiles_sum"] == g["tiles_sum"]
    if key == "cond8":
        assert f["pick"] == list(g["pick"]) and f["fp16_dev_top"].shape == (48, 8)
        assert (f["fp16_dev_top"] <= f["fp16_dev"]).all()
    assert torch.isfinite(f["fp16_dev"]).all() and (f["fp16_dev"] >= 0).all()


@pytest.mark.parametrize("key,fname,n", SETS)
def test_reference_fp16_deviation_is_small_and_below_bf16(gold, key, fname, n):
    """The unfit cap of tests/test_gpu_bf16_parity.py (0.05 of max|logit|) divided by 8 for three more significand bits; and on the worst line
    of every step the reference's fp16 run is closer to its fp32 run than its bf16 run."""
    g, f = torch.load(os.path.join(GOLD, fname)), gold[key]
    scale = g["logits_absmax"].amax(-1)
    rel = f["fp16_dev"].amax(-1) / scale
    print(f"{key}: reference fp16 deviation {float(rel.max()):.5f} x max|logit| (bf16 {float((g['bf16_dev'].amax(-1) / scale).max()):.5f}); "
          f"free-running fp16 == fp32 on {int((f['fp16_free_tokens'] == g['tokens']).all(0).sum())}/{n} lines "
          f"(bf16 {int((g['bf16_free_tokens'] == g['tokens']).all(0).sum())}/{n}); sure share {f['sure_share']:.4f}")
    assert float(rel.max()) <= 0.05 / 8
    assert (f["fp16_dev"].amax(-1) < g["bf16_dev"].amax(-1)).all()


@pytest.mark.parametrize("key,fname,n", SETS)
def test_recorded_sure_share_follows_from_the_fixtures(gold, key, fname, n):
    """`sure_share` -- the share of positions the fp16 argmax check can cover -- is the margins of the fp32 fixture against 2 x the tolerance
    2 x fp16_dev (worst line of the step) + (5e-3 / 8) x max|logit|; at least 0.9 everywhere."""
    g, f = torch.load(os.path.join(GOLD, fname)), gold[key]
    scale = g["logits_absmax"].amax(-1)
    tol = 2 * f["fp16_dev"].amax(-1) + (5e-3 / 8) * scale
    val = g["logits_top"]["values"]
    share = float(((val[..., 0] - val[..., 1]) > 2 * tol[:, None]).float().mean())
    assert abs(share - f["sure_share"]) < 1e-6 and share >= 0.9
