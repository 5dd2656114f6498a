"""Configuration of the OCR-error classifier: DistilBertConfig (surya/ocr_error/model/config.py:14-58) as a dataclass, two named
configs, and the reader of a reference config.json."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import torch

ID2LABEL = {0: "good", 1: "bad"}          # surya/ocr_error/model/config.py:9-12
SUPPORTED_HEAD_DIMS = (32, 64, 80, 128)   # attention kernels of the HIP engine


@dataclass(frozen=True)
class OCRErrorConfig:
    vocab_size: int = 30522
    max_position_embeddings: int = 512
    sinusoidal_pos_embds: bool = False
    n_layers: int = 6
    n_heads: int = 12
    dim: int = 768
    hidden_dim: int = 3072
    num_labels: int = 2
    pad_token_id: int = 0
    layer_norm_eps: float = 1e-12          # every LayerNorm of the model (encoder.py:54, :417, :420)
    id2label: Optional[Dict[int, str]] = None

    @property
    def head_dim(self) -> int:
        return self.dim // self.n_heads

    @property
    def labels(self) -> Dict[int, str]:
        return dict(self.id2label) if self.id2label else {i: ID2LABEL.get(i, f"LABEL_{i}") for i in range(self.num_labels)}

    def validate(self) -> "OCRErrorConfig":
        bad = []
        if self.dim % self.n_heads:
            bad.append(f"dim {self.dim} is not a multiple of n_heads {self.n_heads}")
        elif self.head_dim not in SUPPORTED_HEAD_DIMS:
            bad.append(f"head_dim {self.head_dim} (the HIP engine implements {SUPPORTED_HEAD_DIMS})")
        if self.dim % 64 or self.hidden_dim % 64:
            bad.append(f"dim {self.dim} / hidden_dim {self.hidden_dim} must be multiples of 64 (GEMM K chunks)")
        if not 1 <= self.max_position_embeddings <= 4096:
            bad.append(f"max_position_embeddings {self.max_position_embeddings} (1 .. 4096)")
        if self.n_layers < 1 or self.num_labels < 1:
            bad.append(f"n_layers {self.n_layers} / num_labels {self.num_labels} must be positive")
        if bad:
            raise ValueError("OCR-error model: unsupported configuration: " + "; ".join(bad))
        return self


CONFIGS = {
    # test size: 2 layers, dim 128, 2 heads (head_dim 64), small vocabulary (synth.make_wordpiece_vocab's default size)
    "OCRERR-TINY": OCRErrorConfig(vocab_size=1024, n_layers=2, n_heads=2, dim=128, hidden_dim=512),
    # the reference's defaults (DistilBertConfig.__init__)
    "OCRERR-DEFAULT": OCRErrorConfig(),
}


def ocr_error_config(name: str) -> OCRErrorConfig:
    if name not in CONFIGS:
        raise KeyError(f"unknown OCR-error config {name!r}; known: {sorted(CONFIGS)}")
    return CONFIGS[name]


def ocr_error_config_from_reference_json(raw: dict) -> OCRErrorConfig:
    """config.json of the reference checkpoint (DistilBertConfig.to_dict) -> OCRErrorConfig. Raises ValueError on switches the engine
    does not implement (activation other than erf GELU, head dims outside SUPPORTED_HEAD_DIMS, ...)."""
    act = raw.get("activation", "gelu")
    if act != "gelu":
        raise ValueError(f"OCR-error model: unsupported architecture switches in config.json: activation = {act!r} (the HIP engine implements 'gelu')")
    if raw.get("problem_type") not in (None, "single_label_classification"):
        raise ValueError(f"OCR-error model: unsupported architecture switches in config.json: problem_type = {raw['problem_type']!r}")
    id2label = raw.get("id2label")
    if id2label:
        id2label = {int(k): v for k, v in id2label.items()}
    num_labels = int(raw.get("num_labels", len(id2label) if id2label else 2))
    d = OCRErrorConfig()
    cfg = OCRErrorConfig(vocab_size=int(raw.get("vocab_size", d.vocab_size)),
                         max_position_embeddings=int(raw.get("max_position_embeddings", d.max_position_embeddings)),
                         sinusoidal_pos_embds=bool(raw.get("sinusoidal_pos_embds", False)),
                         n_layers=int(raw.get("n_layers", raw.get("num_hidden_layers", d.n_layers))),
                         n_heads=int(raw.get("n_heads", raw.get("num_attention_heads", d.n_heads))),
                         dim=int(raw.get("dim", raw.get("hidden_size", d.dim))),
                         hidden_dim=int(raw.get("hidden_dim", d.hidden_dim)),
                         num_labels=num_labels, pad_token_id=int(raw.get("pad_token_id", 0) or 0),
                         id2label=id2label or None)
    return cfg.validate()


def sinusoidal_table(n_pos: int, dim: int) -> torch.Tensor:
    """create_sinusoidal_embeddings (encoder.py:40-45): float64 angles pos / 10000^(2 (j // 2) / dim), sin on even and cos on odd
    columns, stored as fp32."""
    j = np.arange(dim)
    ang = np.arange(n_pos)[:, None] / np.power(10000, 2 * (j // 2) / dim)[None, :]
    out = torch.zeros(n_pos, dim)
    out[:, 0::2] = torch.FloatTensor(np.sin(ang[:, 0::2]))
    out[:, 1::2] = torch.FloatTensor(np.cos(ang[:, 1::2]))
    return out


def config_to_reference_json(cfg: OCRErrorConfig) -> dict:
    """The config.json a reference DistilBertConfig with these values writes (the keys ocr_error_config_from_reference_json reads)."""
    return {"model_type": "distilbert", "architectures": ["DistilBertForSequenceClassification"], "activation": "gelu",
            "vocab_size": cfg.vocab_size, "max_position_embeddings": cfg.max_position_embeddings,
            "sinusoidal_pos_embds": cfg.sinusoidal_pos_embds, "n_layers": cfg.n_layers, "n_heads": cfg.n_heads, "dim": cfg.dim,
            "hidden_dim": cfg.hidden_dim, "pad_token_id": cfg.pad_token_id, "dropout": 0.1, "attention_dropout": 0.1,
            "seq_classif_dropout": 0.2, "initializer_range": 0.02,
            "id2label": {str(k): v for k, v in cfg.labels.items()}, "label2id": {v: k for k, v in cfg.labels.items()}}


__all__ = ["OCRErrorConfig", "CONFIGS", "ID2LABEL", "ocr_error_config", "ocr_error_config_from_reference_json", "sinusoidal_table",
           "config_to_reference_json"]
