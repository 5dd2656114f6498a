"""CPU: the OCR-error classifier's weight table per compute dtype. float32 / bfloat16 fold the 1 / sqrt(64) = 1 / 8 of the query into the
q rows and bias (a power of two: exact where no weight leaves the normal range); float16 must NOT: a q weight below 8 x 2^-14 = 4.9e-4
turns subnormal under the fold and loses significand bits, so its table carries the reference's q rows as they are
(SA_OCRERR_Q_PRESCALED, include/surya_amd.h) and the engine hands 1 / 8 to attention."""
import torch

from surya_amd.ocr_error.config import ocr_error_config
from surya_amd.ocr_error.model import N_GLOBALS, N_PER_LAYER, repack_ocr_error_weights
from surya_amd.synth import make_ocr_error_weights


def _state_dict(cfg):
    """Synthetic weights whose q_lin rows hold trained-model magnitudes: a third of the entries around 1e-4 (2^-14 = 6.1e-5 is the
    smallest normal fp16 number; 1e-4 / 8 = 1.25e-5 is subnormal, step 6e-8: 7 significand bits where the unfolded value has 11)."""
    sd = {k: v.clone() for k, v in make_ocr_error_weights(cfg, 0, "conditioned").items()}
    g = torch.Generator().manual_seed(3)
    for i in range(cfg.n_layers):
        for leaf in ("weight", "bias"):
            t = sd[f"distilbert.transformer.layer.{i}.attention.q_lin.{leaf}"]
            small = 1e-4 * (1.0 + 0.5 * torch.rand(t.shape, generator=g)) * torch.sign(torch.randn(t.shape, generator=g))
            pick = torch.rand(t.shape, generator=g) < 1.0 / 3.0
            t[pick] = small[pick]
    return sd


def _q_rows(cfg, table, layer):
    w, b = table[N_GLOBALS + layer * N_PER_LAYER], table[N_GLOBALS + layer * N_PER_LAYER + 1]
    return w[: cfg.dim], b[: cfg.dim], w[cfg.dim:], b[cfg.dim:]


def test_fp16_table_keeps_the_reference_q_rows():
    cfg = ocr_error_config("OCRERR-TINY")
    assert cfg.head_dim == 64
    sd = _state_dict(cfg)
    table = repack_ocr_error_weights(cfg, sd, torch.float16, "cpu")
    lost = 0
    for i in range(cfg.n_layers):
        a = f"distilbert.transformer.layer.{i}.attention."
        qw, qb, kvw, kvb = _q_rows(cfg, table, i)
        assert qw.dtype == torch.float16
        assert torch.equal(qw, sd[a + "q_lin.weight"].half())
        assert torch.equal(qb, sd[a + "q_lin.bias"].half())
        assert torch.equal(kvw, torch.cat([sd[a + "k_lin.weight"], sd[a + "v_lin.weight"]], 0).half())
        assert torch.equal(kvb, torch.cat([sd[a + "k_lin.bias"], sd[a + "v_lin.bias"]], 0).half())
        # what the fold would have cost: folded-then-unfolded differs from the plain rounding on the small weights
        w = sd[a + "q_lin.weight"]
        lost += int(((w / 8).half().float() * 8 != w.half().float()).sum())
    assert lost > 0, "the state dict holds no weight that the fold would damage: the test shows nothing"


def test_bf16_and_fp32_tables_keep_the_fold():
    cfg = ocr_error_config("OCRERR-TINY")
    sd = _state_dict(cfg)
    for dtype in (torch.bfloat16, torch.float32):
        table = repack_ocr_error_weights(cfg, sd, dtype, "cpu")
        for i in range(cfg.n_layers):
            a = f"distilbert.transformer.layer.{i}.attention."
            qw, qb, kvw, _ = _q_rows(cfg, table, i)
            assert torch.equal(qw, (sd[a + "q_lin.weight"].float() / 8).to(dtype))
            assert torch.equal(qb, (sd[a + "q_lin.bias"].float() / 8).to(dtype))
            assert torch.equal(kvw, torch.cat([sd[a + "k_lin.weight"], sd[a + "v_lin.weight"]], 0).to(dtype))
            # the fold is exact there: unfolding returns the plain rounding of the reference's weight
            assert torch.equal(qw.float() * 8, sd[a + "q_lin.weight"].to(dtype).float())


def test_other_head_dims_are_never_folded():
    cfg = ocr_error_config("OCRERR-TINY")
    cfg = type(cfg)(**{**cfg.__dict__, "n_heads": cfg.dim // 32})
    assert cfg.head_dim == 32
    sd = make_ocr_error_weights(cfg, 0, "conditioned")
    for dtype in (torch.float16, torch.bfloat16, torch.float32):
        qw = _q_rows(cfg, repack_ocr_error_weights(cfg, sd, dtype, "cpu"), 0)[0]
        assert torch.equal(qw, sd["distilbert.transformer.layer.0.attention.q_lin.weight"].to(dtype))
