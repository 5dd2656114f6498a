"""Record OCR-error classifier fixtures from the REAL reference modules (build container only).

    python tools/make_golden_ocr_error.py

Imports VikParuchuri/surya @ v0.14.6's DistilBertForSequenceClassification and DistilBertTokenizer (surya/ocr_error) through
oracle/ref_shim plus the four shims below, loads the seeded synthetic weights (surya_amd.synth.make_ocr_error_weights, "conditioned")
and vocabulary (make_wordpiece_vocab) into them, and records, per configuration (OCRERR-TINY, OCRERR-DEFAULT), for a seeded text set
(make_texts): the reference tokenizer's ids (`padding="longest", truncation=True` over all texts at once, as OCRErrorPredictor calls
it), the fp32 logits of one padded call, and the logits of the same call in bf16 (the reference's own bf16 error is the yardstick of
the HIP bf16 tolerance). -> tests/golden/ocr_error_{tiny,default}.pt (ids and logits only, no weights).

Shims the reference's ocr_error modules need under transformers 5.x:
  * transformers.onnx no longer exists: a stub module with OnnxConfig = object (model/config.py imports it);
  * transformers.tokenization_utils lost _is_control / _is_punctuation / _is_whitespace: taken from transformers.tokenization_python;
  * transformers.pytorch_utils lost find_pruneable_heads_and_indices / prune_linear_layer: placeholders (head pruning is never used);
  * DistilBertModel.get_head_mask: returns [None] * n_layers, and config._attn_implementation = "eager"."""
from __future__ import annotations

import os
import random
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch

GOLD = os.path.join(ROOT, "tests", "golden")


def install_ocr_error_shims():
    from oracle import ref_shim
    ref_shim.install()
    import transformers
    import transformers.pytorch_utils as pu
    import transformers.tokenization_python as tpy
    import transformers.tokenization_utils as tu
    if "transformers.onnx" not in sys.modules:
        m = types.ModuleType("transformers.onnx")
        m.OnnxConfig = object
        sys.modules["transformers.onnx"] = m
        transformers.onnx = m
    for n in ("_is_control", "_is_punctuation", "_is_whitespace"):
        if not hasattr(tu, n):
            setattr(tu, n, getattr(tpy, n))

    def _unused(*a, **k):
        raise NotImplementedError("head pruning is not used by the OCR-error model")

    for n in ("find_pruneable_heads_and_indices", "prune_linear_layer"):
        if not hasattr(pu, n):
            setattr(pu, n, _unused)
    ref_shim.purge_bare_namespaces()
    from surya.ocr_error.model import config as rc
    from surya.ocr_error.model import encoder as re_
    from surya.ocr_error import tokenizer as rt
    re_.DistilBertModel.get_head_mask = lambda self, hm, n, *a, **k: [None] * n
    return rc, re_, rt


def build_reference(cfg, sd, vocab, max_length=512):
    """(reference model fp32 eval, reference tokenizer) for a config, a state dict and a vocabulary list."""
    rc, re_, rt = install_ocr_error_shims()
    rcfg = rc.DistilBertConfig(vocab_size=cfg.vocab_size, max_position_embeddings=cfg.max_position_embeddings,
                               sinusoidal_pos_embds=cfg.sinusoidal_pos_embds, n_layers=cfg.n_layers, n_heads=cfg.n_heads, dim=cfg.dim,
                               hidden_dim=cfg.hidden_dim, pad_token_id=cfg.pad_token_id, num_labels=cfg.num_labels)
    rcfg._attn_implementation = "eager"
    model = re_.DistilBertForSequenceClassification(rcfg).eval()
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not [k for k in missing if "position_ids" not in k] and not unexpected, (missing, unexpected)
    d = tempfile.mkdtemp(prefix="ocrerr_vocab_")
    vf = os.path.join(d, "vocab.txt")
    with open(vf, "w", encoding="utf-8") as f:
        f.write("\n".join(vocab) + "\n")
    tok = rt.DistilBertTokenizer(vf, model_max_length=max_length)
    return model, tok


def make_texts(seed: int, n_prose: int = 24):
    """The fixture text set: seeded prose of vocabulary-like words, plus accented text, CJK, punctuation runs, control characters, a word
    over 100 characters, literal [CLS] / [SEP] inside a text, the empty string and one text longer than 512 tokens."""
    rng = random.Random(seed)
    words = ["the", "model", "page", "text", "error", "and", "of", "in", "is", "good", "bad", "table", "line", "word", "ocr", "to", "it",
             "Hello", "World", "résumé", "naïve", "Ångström", "ﬁnance", "3.14", "2024", "e-mail", "don't", "U.S.A.", "x^2", "qzx", "tion"]
    texts = []
    for _ in range(n_prose):
        n = rng.choice((1, 3, 8, 20, 40, 90))
        texts.append(" ".join(rng.choice(words) for _ in range(n)) + rng.choice((".", "!", "?", "", " ...")))
    texts += [
        "Café naïve façade résumé crème brûlée – Ångström, Œuvre, Straße",
        "中文的一是不了人我在有他这 mixed with English 中国",
        "!!!???...---;;;:::((()))[[]]{{}}@@##$$%%^^&&**",
        "ctrl\x00chars\x07here​ and\ttabs\nnew\r\nlines \x85 � end",
        "short " + "a" * 101 + " tail " + "b" * 100,
        "before [CLS] middle [SEP] after[SEP]glued [MASK] [cls] [UNK]",
        "",
        " ".join(rng.choice(words) for _ in range(700)),
    ]
    return texts


def record(name: str, seed: int, n_prose: int):
    from surya_amd.ocr_error.config import ocr_error_config
    from surya_amd.synth import make_ocr_error_weights, make_wordpiece_vocab
    cfg = ocr_error_config(name)
    sd = make_ocr_error_weights(cfg, 0, "conditioned")
    vocab = make_wordpiece_vocab(0)
    model, tok = build_reference(cfg, sd, vocab)
    texts = make_texts(seed, n_prose)
    enc = tok(texts, padding="longest", truncation=True, return_tensors="pt")
    ids = [row[: int(m.sum())].tolist() for row, m in zip(enc.input_ids, enc.attention_mask)]
    t0 = time.time()
    with torch.inference_mode():
        lf = model(enc.input_ids, attention_mask=enc.attention_mask).logits.float().clone()
        model_bf = model.to(torch.bfloat16)
        lb = model_bf(enc.input_ids, attention_mask=enc.attention_mask).logits.float().clone()
    print(f"{name}: {len(texts)} texts, padded length {enc.input_ids.shape[1]}, {time.time() - t0:.1f}s; fp32 labels "
          f"{lf.argmax(-1).tolist()}; bf16 max err {float((lb - lf).abs().max()):.4g} of max|logit| {float(lf.abs().max()):.4g}", flush=True)
    g = {"config": name, "weights": "make_ocr_error_weights(cfg, 0, 'conditioned')", "vocab": "make_wordpiece_vocab(0)", "seed": seed,
         "texts": texts, "ids": ids, "logits_fp32": lf, "logits_bf16_ref": lb, "max_length": 512}
    torch.save(g, os.path.join(GOLD, "ocr_error_" + name.split("-")[1].lower() + ".pt"))


def main():
    record("OCRERR-TINY", 21, 32)
    record("OCRERR-DEFAULT", 22, 24)
    for f in sorted(os.listdir(GOLD)):
        if f.startswith("ocr_error_"):
            print(f, os.path.getsize(os.path.join(GOLD, f)))


if __name__ == "__main__":
    main()
