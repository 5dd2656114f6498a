"""HipOCRErrorModel: the DistilBERT sequence classifier behind libsurya_amd.so's surya_ocrerr_* entry points.

Python here is plumbing only (weight re-layout at load, device memory via torch, ctypes marshalling); all arithmetic runs in the HIP
library. There is no fallback: constructing this without the built library or without a GPU raises."""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence, Tuple

import torch

from .. import _lib as L
from .config import OCRErrorConfig, sinusoidal_table

N_GLOBALS, N_PER_LAYER = 8, 12           # SA_OW_GLOBALS, SA_OL_COUNT (include/surya_amd.h)


class OcrErrConfigC(C.Structure):
    _fields_ = [("vocab", C.c_int32), ("max_pos", C.c_int32), ("dim", C.c_int32), ("heads", C.c_int32), ("hidden", C.c_int32),
                ("layers", C.c_int32), ("num_labels", C.c_int32), ("ln_eps", C.c_float), ("max_texts", C.c_int32),
                ("max_tokens", C.c_int32), ("dtype", C.c_int32)]


def repack_ocr_error_weights(cfg: OCRErrorConfig, sd, dtype: torch.dtype, device) -> List[torch.Tensor]:
    """Reference state dict (DistilBertForSequenceClassification names) -> the table of include/surya_amd.h (SA_OW_* then SA_OL_* per
    layer). q_lin | k_lin | v_lin are fused into one [3 dim, dim] weight. For head_dim 64 in float32 / bfloat16 the q rows and bias are
    multiplied by 1 / 8 (a power of two, exact in formats whose exponent range the weights never leave: the engine's q is then the
    reference's q_lin(x) / sqrt(d), encoder.py:174, bit for bit). A float16 table is NOT folded (SA_OCRERR_Q_PRESCALED): a weight below
    8 x 2^-14 = 4.9e-4 would become subnormal and lose bits, so it carries the reference's q rows and the engine scales in attention."""
    out: List[torch.Tensor] = []
    f = lambda k: sd[k].float()

    def put(t):
        out.append(t.to(device=device, dtype=dtype).contiguous())

    word = f("distilbert.embeddings.word_embeddings.weight")
    if word.shape != (cfg.vocab_size, cfg.dim):
        raise ValueError(f"word_embeddings {tuple(word.shape)} != ({cfg.vocab_size}, {cfg.dim}) of the config")
    put(word)
    if cfg.sinusoidal_pos_embds:
        put(sinusoidal_table(cfg.max_position_embeddings, cfg.dim))
    else:
        put(f("distilbert.embeddings.position_embeddings.weight"))
    put(f("distilbert.embeddings.LayerNorm.weight")); put(f("distilbert.embeddings.LayerNorm.bias"))
    put(f("pre_classifier.weight")); put(f("pre_classifier.bias"))
    put(f("classifier.weight")); put(f("classifier.bias"))
    qscale = 1.0 / 8.0 if cfg.head_dim == 64 and dtype != torch.float16 else 1.0
    for i in range(cfg.n_layers):
        p = f"distilbert.transformer.layer.{i}."
        a = p + "attention."
        put(torch.cat([f(a + "q_lin.weight") * qscale, f(a + "k_lin.weight"), f(a + "v_lin.weight")], 0))
        put(torch.cat([f(a + "q_lin.bias") * qscale, f(a + "k_lin.bias"), f(a + "v_lin.bias")], 0))
        put(f(a + "out_lin.weight")); put(f(a + "out_lin.bias"))
        put(f(p + "sa_layer_norm.weight")); put(f(p + "sa_layer_norm.bias"))
        put(f(p + "ffn.lin1.weight")); put(f(p + "ffn.lin1.bias"))
        put(f(p + "ffn.lin2.weight")); put(f(p + "ffn.lin2.bias"))
        put(f(p + "output_layer_norm.weight")); put(f(p + "output_layer_norm.bias"))
    assert len(out) == N_GLOBALS + N_PER_LAYER * cfg.n_layers
    return out


_DTYPES = {torch.float32: L.DTYPE_F32, torch.bfloat16: L.DTYPE_BF16, torch.float16: L.DTYPE_F16}


def pack_ids(seqs: Sequence[Sequence[int]]) -> Tuple[torch.Tensor, List[int]]:
    """Token id lists -> (packed int32 CPU tensor, lengths)."""
    lens = [len(s) for s in seqs]
    flat = [t for s in seqs for t in s]
    return torch.tensor(flat, dtype=torch.int32), lens


class HipOCRErrorModel:
    def __init__(self, cfg: OCRErrorConfig, state_dict, dtype: torch.dtype = torch.bfloat16, device="cuda:0", max_texts: int = 64,
                 max_tokens: int = 64 * 512):
        if not torch.cuda.is_available():
            raise L.SuryaAmdError("HipOCRErrorModel needs a GPU (MI355X); there is no CPU fallback")
        if dtype not in _DTYPES:
            raise ValueError("dtype must be float32 (reference mode), bfloat16 or float16")
        cfg.validate()
        self.lib = L.lib()
        self.cfg, self.dtype, self.device = cfg, dtype, torch.device(device)
        self.max_texts, self.max_tokens = int(max_texts), int(max_tokens)
        torch.cuda.set_device(self.device)
        self.weights = repack_ocr_error_weights(cfg, state_dict, dtype, self.device)
        self.c = OcrErrConfigC(vocab=cfg.vocab_size, max_pos=cfg.max_position_embeddings, dim=cfg.dim, heads=cfg.n_heads,
                               hidden=cfg.hidden_dim, layers=cfg.n_layers, num_labels=cfg.num_labels, ln_eps=cfg.layer_norm_eps,
                               max_texts=self.max_texts, max_tokens=self.max_tokens,
                               dtype=_DTYPES[dtype])
        table = (C.c_void_p * len(self.weights))(*[t.data_ptr() for t in self.weights])
        self.handle = C.c_void_p()
        L.check(self.lib.surya_ocrerr_create(C.byref(self.c), table, len(self.weights), C.byref(self.handle)), "surya_ocrerr_create")
        self._logits = torch.empty((self.max_texts, cfg.num_labels), dtype=torch.float32, device=self.device)
        self._labels = torch.empty((self.max_texts,), dtype=torch.int32, device=self.device)

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            self.lib.surya_ocrerr_destroy(h)
            self.handle = None

    @property
    def max_length(self) -> int:
        return self.cfg.max_position_embeddings

    def enqueue(self, packed_ids: torch.Tensor, text_len: Sequence[int], stream=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Enqueue one forward; returns DEVICE views (logits fp32 [n, num_labels], labels int32 [n]) that the next call overwrites.
        packed_ids: int32 (CPU or device) with sum(text_len) ids in [0, vocab)."""
        n = len(text_len)
        if n == 0:
            return self._logits[:0], self._labels[:0]
        if n > self.max_texts:
            raise ValueError(f"{n} texts > max_texts {self.max_texts}")
        lens = (C.c_int32 * n)(*[int(v) for v in text_len])
        total = sum(lens)
        if total > self.max_tokens:
            raise ValueError(f"{total} packed tokens > max_tokens {self.max_tokens}")
        if min(lens) < 1 or max(lens) > self.cfg.max_position_embeddings:
            raise ValueError(f"text lengths must lie in 1 .. {self.cfg.max_position_embeddings}")
        if packed_ids.numel() != total:
            raise ValueError(f"packed_ids holds {packed_ids.numel()} ids, the lengths sum to {total}")
        if packed_ids.device.type == "cpu":
            lo, hi = int(packed_ids.min()), int(packed_ids.max())
            if lo < 0 or hi >= self.cfg.vocab_size:
                raise ValueError(f"token ids must lie in 0 .. {self.cfg.vocab_size - 1} (got {lo} .. {hi})")
            ids = packed_ids.to(self.device, dtype=torch.int32, non_blocking=True)
        else:
            ids = packed_ids.to(dtype=torch.int32).contiguous()
        self._ids_keepalive = ids
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        L.check(self.lib.surya_ocrerr_forward(self.handle, L.ptr(ids), lens, n, L.ptr(self._logits), L.ptr(self._labels),
                                              C.c_void_p(s.cuda_stream)), "surya_ocrerr_forward")
        return self._logits[:n], self._labels[:n]

    def forward(self, packed_ids: torch.Tensor, text_len: Sequence[int]) -> Tuple[torch.Tensor, torch.Tensor]:
        """(logits fp32 [n, num_labels], labels int32 [n]) as CPU tensors (synchronises)."""
        lg, lb = self.enqueue(packed_ids, text_len)
        return lg.cpu(), lb.cpu()

    __call__ = forward
