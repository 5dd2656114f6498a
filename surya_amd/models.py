"""load_predictors (surya/models.py:16-24): the five predictors of the library under the reference's keys."""
from __future__ import annotations

from typing import Dict

import torch

from .common.predictor import BasePredictor
from .detection.predictor import DetectionPredictor
from .layout.predictor import LayoutPredictor
from .ocr_error.predictor import OCRErrorPredictor
from .recognition.predictor import RecognitionPredictor
from .table_rec.predictor import TableRecPredictor


def _dtype(dtype):
    if isinstance(dtype, str):
        return getattr(torch, dtype.replace("torch.", ""))
    return dtype


def load_predictors(device: str | torch.device | None = None, dtype: torch.dtype | str | None = None) -> Dict[str, BasePredictor]:
    """`dtype` reaches the four models the reference loads in settings.MODEL_DTYPE (float16 on a GPU): layout, OCR-error, detection and
    table recognition. The recogniser has float32 and bfloat16 only -- the reference's loader picks bfloat16 for it on a GPU with native
    bf16 (surya/recognition/loader.py:32-38) -- so float16 here gives it bfloat16; RecognitionPredictor(dtype=torch.float16) itself raises."""
    dtype = _dtype(dtype)
    rec_dtype = torch.bfloat16 if dtype == torch.float16 else dtype
    return {
        "layout": LayoutPredictor(device=device, dtype=dtype),
        "ocr_error": OCRErrorPredictor(device=device, dtype=dtype),
        "recognition": RecognitionPredictor(device=device, dtype=rec_dtype),
        "detection": DetectionPredictor(device=device, dtype=dtype),
        "table_rec": TableRecPredictor(device=device, dtype=dtype),
    }
