"""GPU: the HIP OCR-error classifier (surya_ocrerr_*) against the reference's recorded logits (tests/golden/ocr_error_*.pt), against
the plain-PyTorch restatement (tests/ocr_error_util.py) on random shapes, batch independence, the [CLS]-only last layer against the
full one, and OCRErrorPredictor end to end."""
import os
import random
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from surya_amd import _lib as L  # noqa: E402
from surya_amd.ocr_error.config import ocr_error_config  # noqa: E402
from surya_amd.ocr_error.model import HipOCRErrorModel, pack_ids  # noqa: E402
from surya_amd.synth import make_ocr_error_weights, make_wordpiece_vocab, write_ocr_error_checkpoint  # noqa: E402
from ocr_error_util import TorchOCRError  # noqa: E402

FIXTURES = ("tiny", "default")
_SD = {}


def golden(name):
    return torch.load(os.path.join(HERE, "golden", f"ocr_error_{name}.pt"))


def weights(cfg):
    key = (cfg.n_layers, cfg.dim)
    if key not in _SD:
        _SD[key] = make_ocr_error_weights(cfg, 0, "conditioned")
    return _SD[key]


def model(cfg, dtype, max_texts=64, max_tokens=None):
    return HipOCRErrorModel(cfg, weights(cfg), dtype=dtype, device="cuda:0", max_texts=max_texts, max_tokens=max_tokens or max_texts * 512)


def run(m, seqs):
    ids, lens = pack_ids(seqs)
    return m.forward(ids, lens)


def cls_only(v):
    L.check(L.lib().surya_set_tuning(b"ocrerr_cls_only", int(v)), "surya_set_tuning")


@pytest.fixture(autouse=True)
def _restore_tuning():
    yield
    cls_only(1)


@pytest.mark.parametrize("name", FIXTURES)
def test_fp32_matches_reference(name):
    g = golden(name)
    cfg = ocr_error_config(g["config"])
    lg, lb = run(model(cfg, torch.float32), g["ids"])
    ref = g["logits_fp32"]
    assert float((lg - ref).abs().max()) <= 1e-4 * float(ref.abs().max())
    assert lb.long().tolist() == ref.argmax(-1).tolist()


@pytest.mark.parametrize("name", FIXTURES)
def test_bf16_within_reference_bf16_error(name):
    g = golden(name)
    cfg = ocr_error_config(g["config"])
    lg, lb = run(model(cfg, torch.bfloat16), g["ids"])
    ref, ref_bf = g["logits_fp32"], g["logits_bf16_ref"]
    amax = float(ref.abs().max())
    bound = max(3e-2 * amax, 1.5 * float((ref_bf - ref).abs().max()))
    err = float((lg - ref).abs().max())
    assert err <= bound, (err, bound)
    top2 = torch.sort(ref, -1, descending=True).values
    clear = (top2[:, 0] - top2[:, 1]) > 2 * bound
    assert float(clear.float().mean()) >= 0.8
    assert lb.long()[clear].tolist() == ref.argmax(-1)[clear].tolist()


def _mixed_batch(cfg, n, seed, lo=1, hi=512):
    rng = random.Random(seed)
    return [[101] + [rng.randrange(104, cfg.vocab_size) for _ in range(rng.randint(lo, hi) - 1)] for _ in range(n)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_batch_independence(dtype):
    cfg = ocr_error_config("OCRERR-DEFAULT")
    seqs = _mixed_batch(cfg, 24, 5)
    m_small, m_big = model(cfg, dtype, max_texts=24), model(cfg, dtype, max_texts=64)
    alone = torch.cat([run(m_small, [s])[0] for s in seqs])
    together, _ = run(m_small, seqs)
    order = list(range(len(seqs)))
    random.Random(7).shuffle(order)
    filler = _mixed_batch(cfg, 40, 9)
    mixed, _ = run(m_big, [seqs[i] for i in order] + filler)
    shuffled = torch.empty_like(together)
    shuffled[order] = mixed[: len(seqs)]
    assert torch.equal(alone, together)
    assert torch.equal(alone, shuffled)


def test_cls_only_last_layer_matches_full_layer():
    cfg = ocr_error_config("OCRERR-DEFAULT")
    seqs = _mixed_batch(cfg, 32, 11)
    for dtype in (torch.float32, torch.bfloat16):
        m = model(cfg, dtype)
        cls_only(1)
        a, la = run(m, seqs)
        cls_only(0)
        b, lb = run(m, seqs)
        if dtype == torch.float32:
            # fp32: the [CLS] path runs the same attention kernel over the text's first query tile and GEMM tiles that walk K in the same
            # order: the same bits
            assert torch.equal(a, b)
        else:
            # bf16: the [CLS] query goes through cls_attn_kernel (fp32 dot products in another association than attn_mfma_kernel's
            # MFMA sums; the same bf16 rounding of P): agreement to rounding, which can move a bf16-rounded value by one step
            assert float((a - b).abs().max()) <= 1e-3 * float(b.abs().max()) or torch.equal(a, b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_random_shapes_vs_restatement(dtype):
    cfg = ocr_error_config("OCRERR-DEFAULT")
    seqs = _mixed_batch(cfg, 64, 21)
    got, lb = run(model(cfg, dtype), seqs)
    ref32 = TorchOCRError(cfg, weights(cfg), torch.float32, "cuda:0").logits(seqs, batch=16)
    amax = float(ref32.abs().max())
    if dtype == torch.float32:
        assert float((got - ref32).abs().max()) <= 1e-4 * amax
    else:
        refbf = TorchOCRError(cfg, weights(cfg), torch.bfloat16, "cuda:0").logits(seqs, batch=16)
        bound = max(3e-2 * amax, 1.5 * float((refbf - ref32).abs().max()))
        assert float((got - ref32).abs().max()) <= bound


@pytest.fixture(scope="module")
def ckpt_dir(tmp_path_factory):
    cfg = ocr_error_config("OCRERR-TINY")
    return write_ocr_error_checkpoint(str(tmp_path_factory.mktemp("ocrerr_ckpt")), cfg, weights(cfg), make_wordpiece_vocab(0))


def test_predictor_end_to_end(ckpt_dir):
    from surya_amd.ocr_error import OCRErrorPredictor
    g = golden("tiny")
    p = OCRErrorPredictor(checkpoint=ckpt_dir, dtype=torch.float32)
    want = [{0: "good", 1: "bad"}[i] for i in g["logits_fp32"].argmax(-1).tolist()]
    r = p(g["texts"])
    assert r.texts == g["texts"] and r.labels == want
    assert p(g["texts"], batch_size=1).labels == want
    assert p([]).labels == []
    # more texts than one engine call holds (64 texts / 64 x 512 tokens): split and reassembled in order
    many = g["texts"] * 5
    assert p(many).labels == want * 5
    # an over-long text is truncated, not rejected
    assert len(p(["word " * 3000]).labels) == 1
