"""OCRErrorPredictor: drop-in for surya.ocr_error.OCRErrorPredictor (surya/ocr_error/__init__.py:13-63) on the HIP classifier.

Same call signature and result schema. The reference tokenises every text, pads the batch to its longest text and runs the model on
`batch_size` rows at a time; a text's label does not depend on that padding (masked keys, [CLS]-row head), so here the texts of one
engine call are packed without padding. An engine call holds at most `batch_size` texts and at most `max_tokens` packed tokens; the
host tokenises the next call's texts while the device runs the current one. There is no CPU fallback for the model."""
from __future__ import annotations

import os
from typing import List, Optional, Sequence, Tuple

import torch

from ..common.predictor import BasePredictor, ModelLoader
from ..settings import settings
from .config import OCRErrorConfig, ocr_error_config
from .model import HipOCRErrorModel
from .schema import OCRErrorDetectionResult
from .tokenizer import WordPieceTokenizer, vocab_from_list

DEFAULT_MAX_TEXTS = 64                    # OCRErrorPredictor.default_batch_sizes["cuda"]


def plan_chunks(lengths: Sequence[int], max_texts: int, max_tokens: int) -> List[Tuple[int, int]]:
    """Consecutive [start, end) ranges of the texts, in order, each with at most max_texts texts and at most max_tokens tokens
    (a single text never exceeds max_tokens: it is truncated to the model's length first)."""
    if max_texts < 1 or max_tokens < 1:
        raise ValueError("max_texts and max_tokens must be positive")
    out, start, tok = [], 0, 0
    for i, n in enumerate(lengths):
        if n > max_tokens:
            raise ValueError(f"text {i}: {n} tokens > max_tokens {max_tokens}")
        if i > start and (i - start == max_texts or tok + n > max_tokens):
            out.append((start, i))
            start, tok = i, 0
        tok += n
    if len(lengths) > start:
        out.append((start, len(lengths)))
    return out


class OCRErrorModelLoader(ModelLoader):
    """checkpoint: None / config name (synthetic weights and vocabulary), {"config": OCRErrorConfig, "state_dict": {...}, "vocab": [...]}
    (optionally "tokenizer": a WordPieceTokenizer), or a directory in the reference's on-disk format (ocr_error/loader.py:14-59):
    config.json, *.safetensors with the reference's parameter names, vocab.txt and tokenizer_config.json."""

    def __init__(self, checkpoint=None):
        super().__init__(checkpoint)
        ck = checkpoint if checkpoint is not None else settings.OCR_ERROR_MODEL_CHECKPOINT
        self.tokenizer = None
        if isinstance(ck, dict):
            self.cfg, self.sd = ck["config"], ck["state_dict"]
            self.tokenizer = ck.get("tokenizer")
            if self.tokenizer is None:
                self.tokenizer = WordPieceTokenizer(vocab_from_list(ck["vocab"]), max_positions=self.cfg.max_position_embeddings)
        elif isinstance(ck, str) and os.path.isdir(ck):
            from ..layout.config import read_checkpoint_dir
            from .config import ocr_error_config_from_reference_json
            raw, self.sd, _ = read_checkpoint_dir(ck)
            self.cfg = ocr_error_config_from_reference_json(raw)
            self.tokenizer = WordPieceTokenizer.from_dir(ck, max_positions=self.cfg.max_position_embeddings)
        else:
            from ..synth import make_ocr_error_weights, make_wordpiece_vocab
            name = ck if isinstance(ck, str) and ck.startswith("OCRERR-") else "OCRERR-DEFAULT"
            self.cfg = ocr_error_config(name)
            self.sd = make_ocr_error_weights(self.cfg, 0, "conditioned")
            self.tokenizer = WordPieceTokenizer(vocab_from_list(make_wordpiece_vocab(0)), max_positions=self.cfg.max_position_embeddings)
        if not isinstance(self.cfg, OCRErrorConfig):
            raise TypeError("checkpoint['config'] must be an OCRErrorConfig")

    def model(self, device=None, dtype=None, max_texts: Optional[int] = None, max_tokens: Optional[int] = None) -> HipOCRErrorModel:
        if device is None or device == "cuda":
            device = "cuda:0"
        n = max_texts or DEFAULT_MAX_TEXTS
        return HipOCRErrorModel(self.cfg, self.sd, dtype=dtype or torch.bfloat16, device=device, max_texts=n,
                                max_tokens=max_tokens or n * self.tokenizer.max_length)

    def processor(self, device=None, dtype=None) -> WordPieceTokenizer:
        return self.tokenizer


class OCRErrorPredictor(BasePredictor):
    model_loader_cls = OCRErrorModelLoader
    batch_size = settings.OCR_ERROR_BATCH_SIZE
    default_batch_sizes = {"cpu": 8, "mps": 8, "cuda": 64, "xla": 32}

    def __call__(self, texts: List[str], batch_size: Optional[int] = None) -> OCRErrorDetectionResult:
        return self.batch_ocr_error_detection(texts, batch_size)

    def batch_ocr_error_detection(self, texts: List[str], batch_size: Optional[int] = None) -> OCRErrorDetectionResult:
        texts = list(texts)
        if not texts:
            return OCRErrorDetectionResult(texts=[], labels=[])
        if batch_size is None:
            batch_size = self.get_batch_size()
        m, tok = self.model, self.processor
        max_texts = max(1, min(int(batch_size), m.max_texts))
        max_tokens = m.max_tokens
        labels_host = torch.empty(len(texts), dtype=torch.int32, pin_memory=True)
        stream = torch.cuda.current_stream(m.device)
        # Greedy packing while tokenising: a call is enqueued as soon as the next text would not fit, and the host goes on tokenising
        # the following texts while the device runs it (the forward only enqueues; the labels come back by an async copy).
        start, seqs, n_tok = 0, [], 0
        for i, t in enumerate(texts):
            ids = tok.encode(t)
            if seqs and (len(seqs) == max_texts or n_tok + len(ids) > max_tokens):
                self._enqueue(seqs, start, labels_host, stream)
                start, seqs, n_tok = i, [], 0
            seqs.append(ids)
            n_tok += len(ids)
        self._enqueue(seqs, start, labels_host, stream)
        stream.synchronize()
        names = m.cfg.labels
        return OCRErrorDetectionResult(texts=texts, labels=[names[int(v)] for v in labels_host.tolist()])

    def _enqueue(self, seqs, start, labels_host, stream):
        lens = [len(s) for s in seqs]
        flat = torch.tensor([t for s in seqs for t in s], dtype=torch.int32)
        _, lb = self.model.enqueue(flat, lens, stream)
        labels_host[start:start + len(seqs)].copy_(lb, non_blocking=True)
