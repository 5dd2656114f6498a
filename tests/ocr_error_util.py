"""Test infrastructure: a plain-PyTorch restatement of the OCR-error classifier (DistilBertForSequenceClassification,
surya/ocr_error/model/encoder.py) on PADDED batches with the reference's masked softmax, in fp32 or bf16, on any device.
Also the yardstick ("baseline") of tools/ocr_error_bench.py."""
from __future__ import annotations

import math
from typing import List, Sequence

import torch
import torch.nn.functional as F


def pad_batch(seqs: Sequence[Sequence[int]], pad_id: int = 0):
    L = max(len(s) for s in seqs)
    ids = torch.full((len(seqs), L), pad_id, dtype=torch.long)
    mask = torch.zeros((len(seqs), L), dtype=torch.long)
    for i, s in enumerate(seqs):
        ids[i, : len(s)] = torch.tensor(list(s), dtype=torch.long)
        mask[i, : len(s)] = 1
    return ids, mask


class TorchOCRError:
    """Weights cast once to `dtype` on `device`; __call__(ids [B, L], mask [B, L]) -> fp32 logits [B, num_labels]."""

    def __init__(self, cfg, sd, dtype=torch.float32, device="cpu"):
        self.cfg, self.dtype, self.device = cfg, dtype, torch.device(device)
        self.w = {k: v.to(device=self.device, dtype=dtype) for k, v in sd.items()}
        if cfg.sinusoidal_pos_embds:
            from surya_amd.ocr_error.config import sinusoidal_table
            self.w["distilbert.embeddings.position_embeddings.weight"] = sinusoidal_table(cfg.max_position_embeddings, cfg.dim).to(
                device=self.device, dtype=dtype)

    def _lin(self, x, name):
        return F.linear(x, self.w[name + ".weight"], self.w[name + ".bias"])

    def _ln(self, x, name):
        return F.layer_norm(x, (self.cfg.dim,), self.w[name + ".weight"], self.w[name + ".bias"], eps=self.cfg.layer_norm_eps)

    @torch.no_grad()
    def __call__(self, ids: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
        c, w = self.cfg, self.w
        ids, mask = ids.to(self.device), mask.to(self.device)
        B, L = ids.shape
        nh, d = c.n_heads, c.dim // c.n_heads
        x = w["distilbert.embeddings.word_embeddings.weight"][ids] + w["distilbert.embeddings.position_embeddings.weight"][:L][None]
        x = self._ln(x, "distilbert.embeddings.LayerNorm")
        masked = (mask == 0).view(B, 1, 1, L)
        for i in range(c.n_layers):
            p = f"distilbert.transformer.layer.{i}."
            sh = lambda t: t.view(B, L, nh, d).transpose(1, 2)
            q = sh(self._lin(x, p + "attention.q_lin")) / math.sqrt(d)
            k = sh(self._lin(x, p + "attention.k_lin"))
            v = sh(self._lin(x, p + "attention.v_lin"))
            s = torch.matmul(q, k.transpose(2, 3)).masked_fill(masked, torch.finfo(q.dtype).min)
            a = torch.matmul(F.softmax(s, dim=-1), v).transpose(1, 2).reshape(B, L, c.dim)
            x = self._ln(self._lin(a, p + "attention.out_lin") + x, p + "sa_layer_norm")
            h = self._lin(F.gelu(self._lin(x, p + "ffn.lin1")), p + "ffn.lin2")
            x = self._ln(h + x, p + "output_layer_norm")
        pooled = F.relu(self._lin(x[:, 0], "pre_classifier"))
        return self._lin(pooled, "classifier").float()

    def logits(self, seqs: Sequence[Sequence[int]], batch: int = 64) -> torch.Tensor:
        out: List[torch.Tensor] = []
        for i in range(0, len(seqs), batch):
            ids, mask = pad_batch(seqs[i:i + batch], self.cfg.pad_token_id)
            out.append(self(ids, mask).cpu())
        return torch.cat(out, 0)
