"""OCR-error classifier (surya/ocr_error): DistilBERT text-quality labels "good" / "bad" on the HIP engine."""
from .config import ID2LABEL, OCRErrorConfig, ocr_error_config  # noqa: F401
from .predictor import OCRErrorModelLoader, OCRErrorPredictor  # noqa: F401
from .schema import OCRErrorDetectionResult  # noqa: F401
