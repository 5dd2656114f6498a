"""CPU: the OCR-error classifier's host side -- tokenizer vs the reference's recorded ids, the plain-PyTorch restatement vs the
reference's recorded logits, config reading, the checkpoint-directory loader, the chunk planner, the schema, load_predictors and the
engine's exported symbols. Fixtures: tests/golden/ocr_error_{tiny,default}.pt (tools/make_golden_ocr_error.py)."""
import importlib.util
import os
import sys

import pytest
import torch

from surya_amd.ocr_error.config import OCRErrorConfig, ocr_error_config, ocr_error_config_from_reference_json, config_to_reference_json
from surya_amd.ocr_error.predictor import OCRErrorModelLoader, plan_chunks
from surya_amd.ocr_error.schema import OCRErrorDetectionResult
from surya_amd.ocr_error.tokenizer import WordPieceTokenizer, vocab_from_list
from surya_amd.synth import make_ocr_error_weights, make_wordpiece_vocab, write_ocr_error_checkpoint

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from ocr_error_util import TorchOCRError  # noqa: E402

sys.path.insert(0, ROOT)
from oracle import ref_shim  # noqa: E402

FIXTURES = ("tiny", "default")


def golden(name):
    return torch.load(os.path.join(HERE, "golden", f"ocr_error_{name}.pt"))


def tokenizer_for(cfg):
    return WordPieceTokenizer(vocab_from_list(make_wordpiece_vocab(0)), max_positions=cfg.max_position_embeddings)


@pytest.mark.parametrize("name", FIXTURES)
def test_tokenizer_matches_reference_ids(name):
    g = golden(name)
    cfg = ocr_error_config(g["config"])
    tk = tokenizer_for(cfg)
    vocab = make_wordpiece_vocab(0)
    for text, want in zip(g["texts"], g["ids"]):
        got = tk.encode(text)
        assert got == want, f"{text[:60]!r}: {got[:20]} vs {want[:20]}"
        assert got[0] == vocab.index("[CLS]") and got[-1] == vocab.index("[SEP]")
    lens = [len(i) for i in g["ids"]]
    assert max(lens) == 512                                    # the long text is truncated to model_max_length
    assert min(lens) == 2                                      # the empty text is [CLS] [SEP]
    # memoised words give the same ids on a second pass
    assert [tk.encode(t) for t in g["texts"]] == g["ids"]


def test_tokenizer_specials_and_long_words():
    tk = tokenizer_for(ocr_error_config("OCRERR-TINY"))
    v = tk.vocab
    ids = tk.tokenize_ids("x[CLS]y [SEP] " + "z" * 101)
    assert ids[1] == v["[CLS]"] and ids[3] == v["[SEP]"] and ids[-1] == v["[UNK]"]
    assert tk.tokenize_ids("Café") == tk.tokenize_ids("cafe")       # lower-case + accent strip


@pytest.mark.skipif(not ref_shim.available(), reason="the reference sources are not present")
def test_tokenizer_live_cross_check_with_reference():
    spec = importlib.util.spec_from_file_location("make_golden_ocr_error", os.path.join(ROOT, "tools", "make_golden_ocr_error.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    cfg = ocr_error_config("OCRERR-TINY")
    vocab = make_wordpiece_vocab(0)
    _, ref_tok = mg.build_reference(cfg, make_ocr_error_weights(cfg, 0, "conditioned"), vocab)
    texts = mg.make_texts(987, 40)
    enc = ref_tok(texts, padding="longest", truncation=True, return_tensors="pt")
    want = [row[: int(m.sum())].tolist() for row, m in zip(enc.input_ids, enc.attention_mask)]
    assert tokenizer_for(cfg)(texts) == want


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_matches_reference_logits(name):
    g = golden(name)
    cfg = ocr_error_config(g["config"])
    m = TorchOCRError(cfg, make_ocr_error_weights(cfg, 0, "conditioned"))
    got = m.logits(g["ids"], batch=len(g["ids"]))
    ref = g["logits_fp32"]
    assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


def test_config_reader_accepts_reference_json_and_rejects_switches():
    cfg = ocr_error_config("OCRERR-DEFAULT")
    assert ocr_error_config_from_reference_json(config_to_reference_json(cfg)) == OCRErrorConfig(id2label={0: "good", 1: "bad"})
    raw = config_to_reference_json(cfg)
    for key, val in (("activation", "relu"), ("n_heads", 7), ("n_heads", 16), ("dim", 100), ("max_position_embeddings", 10 ** 5)):
        bad = dict(raw, **{key: val})
        with pytest.raises(ValueError):
            ocr_error_config_from_reference_json(bad)
    sin = ocr_error_config_from_reference_json(dict(raw, sinusoidal_pos_embds=True))
    assert sin.sinusoidal_pos_embds


def test_checkpoint_directory_round_trip(tmp_path):
    cfg = ocr_error_config("OCRERR-TINY")
    sd = make_ocr_error_weights(cfg, 3, "conditioned")
    vocab = make_wordpiece_vocab(0)
    write_ocr_error_checkpoint(str(tmp_path), cfg, sd, vocab)
    ld = OCRErrorModelLoader(str(tmp_path))
    assert ld.cfg.dim == cfg.dim and ld.cfg.n_layers == cfg.n_layers and ld.cfg.vocab_size == cfg.vocab_size
    assert ld.cfg.labels == {0: "good", 1: "bad"}
    assert set(ld.sd) == set(sd)
    for k in sd:
        assert torch.equal(ld.sd[k], sd[k]), k
    tk = ld.processor()
    assert tk.vocab == vocab_from_list(vocab) and tk.max_length == 512
    g = golden("tiny")
    assert tk(g["texts"]) == g["ids"]


def test_chunk_planner():
    assert plan_chunks([], 4, 100) == []
    assert plan_chunks([512], 64, 512) == [(0, 1)]
    lens = [5, 7, 100, 3, 3, 3, 3, 3, 60, 1]
    ch = plan_chunks(lens, 3, 100)
    assert [i for a, b in ch for i in range(a, b)] == list(range(len(lens)))     # order kept, every text once
    for a, b in ch:
        assert 1 <= b - a <= 3 and sum(lens[a:b]) <= 100
    assert plan_chunks([10] * 10, 64, 25) == [(0, 2), (2, 4), (4, 6), (6, 8), (8, 10)]
    with pytest.raises(ValueError):
        plan_chunks([513], 4, 512)


def test_schema_fields_match_reference():
    assert list(OCRErrorDetectionResult.model_fields) == ["texts", "labels"]
    r = OCRErrorDetectionResult(texts=["a"], labels=["good"])
    assert r.labels == ["good"]


def test_load_predictors_keys(monkeypatch):
    import surya_amd.models as M
    made = []
    for nm in ("LayoutPredictor", "OCRErrorPredictor", "RecognitionPredictor", "DetectionPredictor", "TableRecPredictor"):
        monkeypatch.setattr(M, nm, lambda device=None, dtype=None, _n=nm: made.append((_n, device, dtype)) or _n)
    out = M.load_predictors(device="cuda", dtype="bfloat16")
    assert list(out) == ["layout", "ocr_error", "recognition", "detection", "table_rec"]
    assert out["ocr_error"] == "OCRErrorPredictor" and all(d == torch.bfloat16 for _, _, d in made)


def test_engine_exports_ocr_error_symbols(hip_lib):
    for n in ("surya_ocrerr_create", "surya_ocrerr_destroy", "surya_ocrerr_forward"):
        assert hasattr(hip_lib, n)
