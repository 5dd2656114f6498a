"""Result object of OCRErrorPredictor, field for field surya/ocr_error/schema.py:6-8."""
from __future__ import annotations

from typing import List

from pydantic import BaseModel


class OCRErrorDetectionResult(BaseModel):
    texts: List[str]
    labels: List[str]
