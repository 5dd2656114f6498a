"""Checkpoint loading for the recognition model: checkpoint -> tokenizer, HipRecModel, processor; config.json -> RecConfig."""
import json
import os
from typing import Optional

import torch

from ..common.predictor import ModelLoader
from ..config import DecoderConfig, EncoderConfig, RecConfig, rec_config
from ..settings import settings
from .model import HipRecModel
from .processor import SuryaOCRProcessor
from .tokenizer import ByteMathTokenizer, OCRTokenizer


class RecognitionModelLoader(ModelLoader):
    """`checkpoint` may be None (synthetic config named by SURYA_AMD_REC_CONFIG), a dict
    {"config": RecConfig, "state_dict": {...}}, or a directory holding the reference's HF-format files
    (config.json + *.safetensors; recognition/loader.py:25-82)."""

    def __init__(self, checkpoint=None):
        super().__init__(checkpoint)
        self._cfg: Optional[RecConfig] = None
        self._sd = self._special_tokens = None

    def _resolve(self):
        if self._cfg is not None:
            return
        ck = self.checkpoint
        if isinstance(ck, dict):
            self._cfg, self._sd = ck["config"], ck["state_dict"]
            self._special_tokens = ck.get("special_tokens")
        elif isinstance(ck, str) and os.path.isdir(ck):
            from safetensors.torch import load_file
            with open(os.path.join(ck, "config.json")) as f:
                raw = json.load(f)
            self._cfg = rec_config_from_reference_json(raw)
            self._special_tokens = raw.get("special_ocr_tokens")
            self._sd = None if self._receives_weights() else {}
            for fn in sorted(os.listdir(ck)):
                if fn.endswith(".safetensors") and self._sd is not None:
                    self._sd.update(load_file(os.path.join(ck, fn)))
        else:
            from ..synth import make_rec_weights
            self._cfg = rec_config(ck if isinstance(ck, str) else settings.SURYA_AMD_REC_CONFIG)
            self._sd = None if self._receives_weights() else make_rec_weights(self._cfg, 0)

    @staticmethod
    def _receives_weights() -> bool:
        """SURYA_AMD_BROADCAST_WEIGHTS with an initialised process group: only rank 0 reads / builds the state dict."""
        if not settings.SURYA_AMD_BROADCAST_WEIGHTS:
            return False
        from .. import dist as sdist
        rank, world = sdist.world_info()
        return world > 1 and rank != 0

    def tokenizer(self) -> OCRTokenizer:
        self._resolve()
        if isinstance(self.checkpoint, str) and os.path.isdir(self.checkpoint):
            # Real checkpoint: the id layout is DEFINED by the files (processor/tokenizer.py:224-260) -- the Qwen2 BPE that
            # ships with it sets qwen_offset, special_ocr_tokens["all"] sets the tag range, exactly len(unique tags) wide.
            # No placeholder tags, no byte-tokenizer stand-in: either would shift every UTF-16 id silently.
            from transformers import Qwen2Tokenizer
            math_tok = Qwen2Tokenizer.from_pretrained(self.checkpoint)      # raises if the vocabulary files are missing
            if not self._special_tokens or not self._special_tokens.get("all"):
                raise ValueError(f"{self.checkpoint}/config.json has no special_ocr_tokens; cannot lay out token ids")
            tok = OCRTokenizer(self._special_tokens, math_tok, reserve_special=0)
            # the lm_head may be PADDED beyond the tokenizer (the reference never ties the two sizes); ids the tokenizer does not
            # know can then be emitted and decode to nothing. A tokenizer LARGER than the head cannot be right.
            if tok.vocab_size > self._cfg.decoder.vocab_size:
                raise ValueError(f"token-id layout mismatch: qwen_offset {tok.qwen_offset} + {tok.num_special} tags + 65536 "
                                 f"UTF-16 units = {tok.vocab_size} > decoder.vocab_size = {self._cfg.decoder.vocab_size}")
            if tok.vocab_size < self._cfg.decoder.vocab_size:
                import warnings
                warnings.warn(f"decoder.vocab_size {self._cfg.decoder.vocab_size} exceeds the tokenizer's {tok.vocab_size} ids "
                              "(padded lm_head); ids beyond the tokenizer decode to nothing")
            return tok
        # synthetic configs only: one id per UTF-8 byte stands in for the BPE, and the tag range is padded to the
        # config's fixed width (a randomly initialised model can emit any id)
        return OCRTokenizer(self._special_tokens, ByteMathTokenizer(self._cfg.qwen_offset),
                            reserve_special=self._cfg.num_special_tokens)

    def model(self, device=None, dtype=None, **caps) -> HipRecModel:
        self._resolve()
        if device is None:
            device = settings.TORCH_DEVICE_MODEL
        if device == "cuda":
            device = "cuda:0"
        if dtype is None:
            dtype = torch.bfloat16          # recognition/loader.py:35-38 picks bf16 on GPUs with native bf16
        tok = self.tokenizer()
        sysm = tok.system_tokens
        from .predictor import RecognitionPredictor         # (the predictor imports this module)
        caps.setdefault("max_slots", settings.RECOGNITION_BATCH_SIZE or RecognitionPredictor.default_batch_sizes["cuda"])
        caps.setdefault("max_kv_len", 1536 + 32)
        if settings.SURYA_AMD_BROADCAST_WEIGHTS:
            from .. import dist as sdist
            caps.setdefault("broadcast_weights", sdist.collectives_on())
        return HipRecModel(self._cfg, self._sd, image_token_id=sysm["<IMAGE>"], pad_token_id=sysm["<PAD>"],
                           eos_token_id=sysm["</S>"], dtype=dtype, device=device, **caps)

    def processor(self, device=None, dtype=None) -> SuryaOCRProcessor:
        self._resolve()
        e = self._cfg.encoder
        return SuryaOCRProcessor(self.tokenizer(), self._cfg.num_register_tokens, e.patch_size, e.spatial_merge_size)


def rec_config_from_reference_json(raw: dict) -> RecConfig:
    """Map a SuryaModelConfig config.json (surya/common/surya/config.py) onto RecConfig."""
    ve, de = raw.get("vision_encoder", {}), raw.get("decoder", {})
    enc = EncoderConfig(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in ve.items()
                           if k in EncoderConfig.__dataclass_fields__})
    dkw = {k: v for k, v in de.items() if k in DecoderConfig.__dataclass_fields__}
    if "head_dim" not in dkw and "hidden_size" in dkw and "num_attention_heads" in dkw:
        dkw["head_dim"] = dkw["hidden_size"] // dkw["num_attention_heads"]
    dec = DecoderConfig(**dkw)
    return RecConfig(name="checkpoint", encoder=enc, decoder=dec, bbox_size=raw.get("bbox_size", 1025),
                     image_embed_encoding_size=raw.get("image_embed_encoding_size", 1024),
                     image_embed_encoding_multiplier=raw.get("image_embed_encoding_multiplier", 256),
                     num_register_tokens=raw.get("num_register_tokens", 4))
