"""Output schemas of RecognitionPredictor (fields of surya/recognition/schema.py:10-40)."""
from __future__ import annotations

import math
from typing import List, Optional

import inspect

from pydantic import BaseModel, Field, field_validator, model_serializer

from ..common.geometry import PolygonBox


class TaskNames:   # surya/common/surya/schema.py:1-11
    block_without_boxes = "block_without_boxes"
    ocr_with_boxes = "ocr_with_boxes"
    ocr_without_boxes = "ocr_without_boxes"


TASK_NAMES = [TaskNames.block_without_boxes, TaskNames.ocr_with_boxes, TaskNames.ocr_without_boxes]


class BaseChar(PolygonBox):
    text: str
    confidence: Optional[float] = 0

    @field_validator("confidence", mode="before")
    @classmethod
    def _nan_to_zero(cls, v):
        if v is None or (isinstance(v, float) and math.isnan(v)):
            return 0
        try:
            return 0 if math.isnan(float(v)) else v
        except (TypeError, ValueError):
            return v


class CharAlternative(BaseModel):
    """One reading of a character (RecognitionPredictor.top_k): the decoded token, its probability among the allowed tokens,
    and the token id (a lone UTF-16 surrogate has no text of its own: "" with its id kept)."""
    text: str
    confidence: float
    token_id: int


_EXCLUDE_IF = "exclude_if" in inspect.signature(Field).parameters          # pydantic >= 2.12: the exclusion runs inside pydantic-core


class TextChar(BaseChar):
    bbox_valid: bool = True
    # the `top_k` most likely readings, best first (entry 0 is the character's own); None unless the call asked for them, and
    # then left out of the serialised form, which stays the reference's (model_json_schema lists the field all the same). The
    # exclusion costs model_dump one predicate call per character (tools/hostbench/dump_cost.py: no difference to a TextChar
    # without the field at 3.6-5 us per character; the wrap serialiser that older pydantic needs takes 3.6 to 9.7 us).
    # `greedy` (RecognitionPredictor.align): the model's own reading at the token the character takes its confidence from -- text,
    # probability, token id; it equals the character where the model agrees with the aligned text. None, and left out like
    # `alternatives`, everywhere else.
    # `plain` / `plain_confidence` (RecognitionPredictor.boost_words): the character the model would have emitted here without the boost,
    # given the same prefix, and the emitted character's probability without the boost, both at the token the character takes its
    # confidence from (the rule of `greedy`). None, and left out likewise, on every line that was not boosted.
    if _EXCLUDE_IF:
        alternatives: Optional[List[CharAlternative]] = Field(default=None, exclude_if=lambda v: v is None)
        greedy: Optional[CharAlternative] = Field(default=None, exclude_if=lambda v: v is None)
        plain: Optional[str] = Field(default=None, exclude_if=lambda v: v is None)
        plain_confidence: Optional[float] = Field(default=None, exclude_if=lambda v: v is None)
    else:
        alternatives: Optional[List[CharAlternative]] = None
        greedy: Optional[CharAlternative] = None
        plain: Optional[str] = None
        plain_confidence: Optional[float] = None

        @model_serializer(mode="wrap")
        def _without_absent_alternatives(self, handler):
            d = handler(self)
            if self.alternatives is None:
                d.pop("alternatives", None)
            if self.greedy is None:
                d.pop("greedy", None)
            if self.plain is None:
                d.pop("plain", None)
            if self.plain_confidence is None:
                d.pop("plain_confidence", None)
            return d


class TextWord(BaseChar):
    bbox_valid: bool = True


class LineHypothesis(BaseModel):
    """One reading of a line out of a beam-search call (RecognitionPredictor.beam_width): its text and characters, assembled like a
    TextLine's, `confidence` computed like a TextLine's, `log_prob` = the sum of log p(token | image, preceding tokens) over its tokens,
    eos included, without length normalisation (comparable with `align`'s log_prob), and whether the reading reached its end
    (`finished`) or was cut by the token budget or the repeat rule."""
    text: str
    confidence: Optional[float] = 0
    log_prob: float
    finished: bool
    chars: List[TextChar]
    words: List[TextWord] | None = None


class LineReading(BaseModel):
    """One candidate reading of a line that was re-read (RecognitionPredictor.reread): the picture it was read from -- "original",
    "contrast", "rot90", "rot180" or "rot270" -- with its text and line confidence."""
    variant: str
    text: str
    confidence: Optional[float] = 0


class TextLine(BaseChar):
    chars: List[TextChar]
    original_text_good: bool = False
    words: List[TextWord] | None = None
    # RecognitionPredictor.align: log p(text, eos | image), the sum of the forced tokens' log-probabilities; in a beam-search call the
    # score of the line's best reading. None, and left out of the serialised form, in every other result.
    # `hypotheses` (RecognitionPredictor.beam_width): the line's n best readings, finished ones by log_prob descending, then unfinished
    # ones; entry 0 is the line itself. None, and left out like log_prob, everywhere else.
    # `pattern_matched` (RecognitionPredictor.__call__(pattern=)): whether the line, read under a pattern, ended with EOS where the
    # pattern accepts -- False for a line cut by the token budget, the repeat rule or the no-output token (its text is then a proper
    # prefix of a match, or empty). None, and left out likewise, for a line without a pattern.
    # `lexicon_index` (RecognitionPredictor.lexicon): the index, in the line's own word list, of the entry the line read -- >= 0 iff the
    # line ended (EOS or pad) on a whole entry; -1 for a line cut by the token budget, the repeat rule or the no-output token (its text is
    # then a proper prefix of an entry, or empty). None, and left out likewise, for a line without a lexicon.
    # `boost_matches` (RecognitionPredictor.boost_words): the indices, in the line's own list, of the entries some live match completed
    # while the line was read, in order of completion, each once; [] if none. None, and left out likewise, for a line that was not boosted.
    # `rectified` (RecognitionPredictor.rectify): whether the line's pixels were warped upright from its quadrilateral; its characters'
    # polygons are then tilted quads on the page. None, and left out likewise, while `rectify` is None.
    # `unrolled` (RecognitionPredictor.unroll): whether the line's pixels were unrolled along its centre line; its characters' polygons
    # are then tilted quads that follow the bend. None, and left out likewise, while `unroll` is None.
    # `variant` (RecognitionPredictor.reread): the picture the line's reading comes from, "original" | "contrast" | "rot90" | "rot180" |
    # "rot270"; `readings`: every candidate of a line that was re-read, the first reading first, then the variants in that order; None
    # for a line that was read once. Both None, and left out likewise, while `reread` is None.
    if _EXCLUDE_IF:
        log_prob: Optional[float] = Field(default=None, exclude_if=lambda v: v is None)
        hypotheses: Optional[List[LineHypothesis]] = Field(default=None, exclude_if=lambda v: v is None)
        pattern_matched: Optional[bool] = Field(default=None, exclude_if=lambda v: v is None)
        lexicon_index: Optional[int] = Field(default=None, exclude_if=lambda v: v is None)
        boost_matches: Optional[List[int]] = Field(default=None, exclude_if=lambda v: v is None)
        rectified: Optional[bool] = Field(default=None, exclude_if=lambda v: v is None)
        unrolled: Optional[bool] = Field(default=None, exclude_if=lambda v: v is None)
        variant: Optional[str] = Field(default=None, exclude_if=lambda v: v is None)
        readings: Optional[List[LineReading]] = Field(default=None, exclude_if=lambda v: v is None)
    else:
        log_prob: Optional[float] = None
        hypotheses: Optional[List[LineHypothesis]] = None
        pattern_matched: Optional[bool] = None
        lexicon_index: Optional[int] = None
        boost_matches: Optional[List[int]] = None
        rectified: Optional[bool] = None
        unrolled: Optional[bool] = None
        variant: Optional[str] = None
        readings: Optional[List[LineReading]] = None

        @model_serializer(mode="wrap")
        def _without_absent_log_prob(self, handler):
            d = handler(self)
            if self.log_prob is None:
                d.pop("log_prob", None)
            if self.hypotheses is None:
                d.pop("hypotheses", None)
            if self.pattern_matched is None:
                d.pop("pattern_matched", None)
            if self.lexicon_index is None:
                d.pop("lexicon_index", None)
            if self.boost_matches is None:
                d.pop("boost_matches", None)
            if self.rectified is None:
                d.pop("rectified", None)
            if self.unrolled is None:
                d.pop("unrolled", None)
            if self.variant is None:
                d.pop("variant", None)
            if self.readings is None:
                d.pop("readings", None)
            return d


class RankedCandidate(BaseModel):
    """One candidate text of a line out of RecognitionPredictor.rank: `index` is its position in the caller's list, `log_prob` the float64
    sum of log p(token | image, preceding tokens) over its `n_tokens` tokens, eos included (TextLine.log_prob's definition: comparable
    with `align` and with beam hypotheses), `probability` the softmax of log_prob over the line's DISTINCT candidates, and `greedy_match`
    whether the model's own reading under the candidate's prefix equals the candidate at every token."""
    index: int
    text: str
    log_prob: float
    n_tokens: int
    probability: float
    greedy_match: bool


class LineRanking(PolygonBox):
    """A line's candidates by log_prob descending, then index ascending; `best` is the caller's index of the first. polygon / bbox as a
    TextLine has them; no characters or words are assembled."""
    candidates: List[RankedCandidate]
    best: int


class RankResult(BaseModel):
    lines: List[LineRanking]
    image_bbox: List[float]


class OCRResult(BaseModel):
    text_lines: List[TextLine]
    image_bbox: List[float]
