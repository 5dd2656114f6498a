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
    dtype = _dtype(dtype)
    return {
        "layout": LayoutPredictor(device=device, dtype=dtype),
        "ocr_error": OCRErrorPredictor(device=device, dtype=dtype),
        "recognition": RecognitionPredictor(device=device, dtype=dtype),
        "detection": DetectionPredictor(device=device, dtype=dtype),
        "table_rec": TableRecPredictor(device=device, dtype=dtype),
    }
