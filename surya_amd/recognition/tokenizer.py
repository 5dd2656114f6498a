"""OCR tokenizer: UTF-16 code units + special tags + (pluggable) BPE for math spans.

Behaviour of SuryaOCRTokenizer / InnerOCRTokenizer (surya/common/surya/processor/tokenizer.py:26-320):
id layout  [0, qwen_offset) math BPE  |  [qwen_offset, special_token_offset) tags  |  then one id per UTF-16 code unit.
The Qwen2 BPE vocabulary ships with the checkpoint (unavailable offline); `ByteMathTokenizer` is the synthetic stand-in
(one id per UTF-8 byte) so the three-range decode logic is exercised end to end.
"""
from __future__ import annotations

import html
import re
from typing import Dict, List, Optional, Sequence

import numpy as np

from .schema import TaskNames, TASK_NAMES

DEFAULT_SPECIAL_TOKENS: Dict[str, List[str]] = {
    "system": ["</S>", "<PAD>", "<IMAGE>", "<REG1>", "<REG2>", "<REG3>", "<REG4>", "<EOI>", "<NOP>", "<ROT>", "<NO-MATH>",
               "<OCR-WB>", "<OCR-WOB>", "<BLOCKS-WOB>"],
    "formatting": ["<b>", "</b>", "<i>", "</i>", "<u>", "</u>", "<del>", "</del>", "<sup>", "</sup>", "<sub>", "</sub>",
                   "<mark>", "</mark>", "<br>", "<code>", "</code>"],
    "math_external": ["<math>", '<math display="inline">', '<math display="block">', "</math>"],
}
DEFAULT_SPECIAL_TOKENS["all"] = (DEFAULT_SPECIAL_TOKENS["system"] + DEFAULT_SPECIAL_TOKENS["formatting"]
                                 + DEFAULT_SPECIAL_TOKENS["math_external"])


class ByteMathTokenizer:
    """Stand-in for the checkpoint's Qwen2 BPE: ids 0..255 = UTF-8 bytes; `size` ids reserved."""

    def __init__(self, size: int):
        assert size >= 256
        self.size = size

    def __len__(self):
        return self.size

    def __call__(self, text: str):
        return {"input_ids": list(text.encode("utf-8"))}

    def decode(self, ids: Sequence[int]) -> str:
        return bytes(i for i in ids if 0 <= i < 256).decode("utf-8", errors="ignore")


def _prefix_regex(tokens: Sequence[str]):
    """Longest-first alternation anchored at the start (tokenizer.py:18-23); never matches when empty."""
    if not tokens:
        return re.compile(r"(?!x)x")
    return re.compile("^(" + "|".join(re.escape(t) for t in sorted(tokens, key=len, reverse=True)) + ")")


class OCRTokenizer:
    def __init__(self, special_tokens: Optional[Dict[str, List[str]]] = None, math_tokenizer=None, qwen_offset: int = 256,
                 reserve_special: int = 0):
        self.special_tokens = special_tokens or DEFAULT_SPECIAL_TOKENS
        self.math_tokenizer = math_tokenizer or ByteMathTokenizer(qwen_offset)
        self.qwen_offset = len(self.math_tokenizer)
        self.SPECIAL_TOKEN_MAPPING: Dict[str, int] = {}
        for tag in self.special_tokens.get("all", []):
            if tag not in self.SPECIAL_TOKEN_MAPPING:
                self.SPECIAL_TOKEN_MAPPING[tag] = self.qwen_offset + len(self.SPECIAL_TOKEN_MAPPING)
        # synthetic configs reserve a fixed-size tag range (RecConfig.num_special_tokens): a randomly initialised model can
        # emit any id, so every reserved id gets a placeholder tag (a real checkpoint defines all of its tag ids)
        for n in range(len(self.SPECIAL_TOKEN_MAPPING), reserve_special):
            self.SPECIAL_TOKEN_MAPPING[f"<RSV-{n}>"] = self.qwen_offset + n
        self.num_special = len(self.SPECIAL_TOKEN_MAPPING)
        self.REVERSE_SPECIAL_TOKEN_MAPPING = {v: k for k, v in self.SPECIAL_TOKEN_MAPPING.items()}
        self.special_token_offset = self.qwen_offset + self.num_special
        self._system = _prefix_regex(self.special_tokens.get("system", []))
        self._math = _prefix_regex(self.special_tokens.get("math_external", []))
        self._format = _prefix_regex(self.special_tokens.get("formatting", []))
        self.system_tokens = {t: self.SPECIAL_TOKEN_MAPPING[t] for t in self.special_tokens.get("system", [])}

    @property
    def vocab_size(self) -> int:
        return self.special_token_offset + 65536

    # ---------------------------------------------------------------------------------- constrained output
    ALWAYS_ALLOWED = ("</S>", "<PAD>", "<NOP>")      # a constrained line must still be able to stop, pad or say "no output"

    @staticmethod
    def _units(chars: str) -> List[int]:
        """UTF-16 code units of the characters of `chars` (a non-BMP character has two: its surrogates)."""
        raw = chars.encode("utf-16le", errors="surrogatepass")
        return [raw[i] + (raw[i + 1] << 8) for i in range(0, len(raw), 2)]

    def token_mask(self, allow: Optional[str] = None, block: Optional[str] = None, vocab_size: Optional[int] = None) -> np.ndarray:
        """Allowed-id set as uint32 words over `vocab_size` ids (default: this tokenizer's; a model may pad its vocabulary): bit (c & 31) of
        word (c >> 5) set = id c may be emitted. The format of HipRecModel.set_token_masks / surya_rec_set_token_masks.

        allow: an id is allowed iff it is the UTF-16 code unit of one of the characters (special_token_offset + unit), or EOS, pad or the
        no-output token, which are always allowed. Nothing else: no formatting or math tags, no math-BPE ids. A character outside the BMP
        allows BOTH of its surrogates, each by itself: this OVER-permits (any allowed high surrogate may pair with any allowed low one).
        block: every id is allowed except the code units of the characters (the three ids above cannot be blocked). A character outside the
        BMP raises ValueError: blocking its surrogates would block every character that shares one.
        Exactly one of the two is given."""
        if (allow is None) == (block is None):
            raise ValueError("token_mask takes exactly one of allow / block")
        if not isinstance(allow if allow is not None else block, str):
            raise TypeError("an allowlist / blocklist is a str of characters")
        V = self.vocab_size if vocab_size is None else int(vocab_size)
        bits = np.zeros(((V + 31) // 32) * 32, bool)
        if allow is not None:
            ids = [self.special_token_offset + u for u in self._units(allow)]
        else:
            if any(ord(ch) > 0xFFFF for ch in block):
                raise ValueError("a blocklist takes characters of the Basic Multilingual Plane only (a surrogate is shared by 1024 characters)")
            bits[:V] = True
            ids = [self.special_token_offset + u for u in self._units(block)]
        ids = [i for i in ids if i < V]
        bits[ids] = allow is not None
        bits[[self.SPECIAL_TOKEN_MAPPING[t] for t in self.ALWAYS_ALLOWED if t in self.SPECIAL_TOKEN_MAPPING]] = True
        return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1).astype(np.uint32)

    # --------------------------------------------------------------------------------------------- encode
    def _tokenize_ocr(self, text: str) -> List[int]:
        """InnerOCRTokenizer._tokenize (tokenizer.py:68-125)."""
        out: List[int] = []
        in_math = False
        text = html.unescape(text)
        while text:
            m = self._system.search(text)
            if m:
                out.append(self.SPECIAL_TOKEN_MAPPING[m.group(1)]); text = text[m.end():]
                continue
            m = self._math.search(text)
            if m:
                tag = m.group(1)
                if tag.startswith("<math"):
                    in_math = True
                elif tag == "</math>":
                    in_math = False
                out.append(self.SPECIAL_TOKEN_MAPPING[tag]); text = text[m.end():]
                continue
            if in_math:
                end = text.find("</math>")
                if end < 0:
                    # unterminated <math>: the whole remainder is math. The reference slices text[:-1] / text[-1:] here
                    # (:99-101) and never terminates; a hang in the pre-processing pool is not behaviour worth keeping.
                    out += self.math_tokenizer(text)["input_ids"]
                    text = ""
                    continue
                span = text[:end]
                out += self.math_tokenizer(span)["input_ids"]
                text = text[end:]
                continue
            m = self._format.search(text)
            if m:
                out.append(self.SPECIAL_TOKEN_MAPPING[m.group(1)]); text = text[m.end():]
                continue
            raw = text[0].encode("utf-16le")
            out += [raw[i] + (raw[i + 1] << 8) + self.special_token_offset for i in range(0, len(raw), 2)]
            text = text[1:]
        return out

    def __call__(self, texts, tasks=None):
        if isinstance(texts, str):
            texts, tasks = [texts], [tasks]
        ids = []
        for text, task in zip(texts, tasks):
            task = task or TaskNames.ocr_with_boxes
            assert task in TASK_NAMES, f"Invalid task: {task}"
            if task in (TaskNames.ocr_with_boxes, TaskNames.ocr_without_boxes):
                ids.append(self._tokenize_ocr(text))
            else:
                ids.append(list(self.math_tokenizer(text)["input_ids"]))
        return {"input_ids": ids}

    # --------------------------------------------------------------------------------------------- decode
    def _decode_ocr(self, token_ids: Sequence[int]) -> str:
        """InnerOCRTokenizer.decode (tokenizer.py:173-221): runs of math ids / UTF-16 ids / single tags."""
        text, buf, buf_math = "", [], False

        def flush():
            nonlocal text, buf, buf_math
            if buf:
                if buf_math:
                    text += self.math_tokenizer.decode(buf)
                else:
                    b = bytearray()
                    for t in buf:
                        n = t - self.special_token_offset
                        b.append(n & 0xFF); b.append((n >> 8) & 0xFF)
                    text += b.decode("utf-16le", errors="ignore")
            buf, buf_math = [], False

        for t in token_ids:
            if t < self.qwen_offset:
                if buf and not buf_math:
                    flush()
                buf.append(t); buf_math = True
            elif t >= self.special_token_offset:
                if buf and buf_math:
                    flush()
                buf.append(t); buf_math = False
            elif t in self.REVERSE_SPECIAL_TOKEN_MAPPING:
                flush()
                text += self.REVERSE_SPECIAL_TOKEN_MAPPING[t]
            else:
                raise ValueError(f'Unexpected token value while decoding, got "{t}" in token_ids {list(token_ids)}')
        flush()
        return text

    def decode(self, token_ids, task: str = TaskNames.ocr_with_boxes) -> str:
        assert task in TASK_NAMES, f"Invalid task: {task}"
        token_ids = [int(t) for t in token_ids]
        if task in (TaskNames.ocr_with_boxes, TaskNames.ocr_without_boxes):
            return self._decode_ocr(token_ids)
        return self.math_tokenizer.decode(token_ids)


class MaskTable:
    """The distinct token masks of one call and the id of each: identical masks (the same allowed set, however it was written) are
    stored -- and uploaded -- once. `id_for(None, None)` is -1, the unconstrained line."""

    def __init__(self, tokenizer: OCRTokenizer, vocab_size: Optional[int] = None, limit: Optional[int] = None):
        self.tokenizer, self.vocab_size, self.limit = tokenizer, vocab_size, limit
        self.rows: List[np.ndarray] = []
        self._by_bytes: Dict[bytes, int] = {}
        self._by_spec: Dict[tuple, int] = {}

    def id_for(self, allow: Optional[str] = None, block: Optional[str] = None) -> int:
        if allow is None and block is None:
            return -1
        if allow is not None and block is not None:
            raise ValueError("a line takes an allowlist or a blocklist, not both")
        spec = (allow, block)
        if spec not in self._by_spec:
            m = self.tokenizer.token_mask(allow, block, self.vocab_size)
            key = m.tobytes()
            if key not in self._by_bytes:
                if self.limit is not None and len(self.rows) >= self.limit:
                    raise ValueError(f"more than {self.limit} distinct allowlists / blocklists in one call")
                self._by_bytes[key] = len(self.rows)
                self.rows.append(m)
            self._by_spec[spec] = self._by_bytes[key]
        return self._by_spec[spec]

    def add_row(self, mask: np.ndarray, what: str = "allowlists / blocklists") -> int:
        """The id of a ready-made row (the allowed set of a pattern state, recognition/pattern.py), merged with identical rows."""
        key = mask.tobytes()
        if key not in self._by_bytes:
            if self.limit is not None and len(self.rows) >= self.limit:
                raise ValueError(f"more than {self.limit} distinct {what} in one call")
            self._by_bytes[key] = len(self.rows)
            self.rows.append(mask)
        return self._by_bytes[key]

    def __len__(self):
        return len(self.rows)

    def array(self) -> np.ndarray:
        """uint32 [n_masks, words]."""
        return np.stack(self.rows) if self.rows else np.zeros((0, 0), np.uint32)
