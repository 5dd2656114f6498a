"""WordPiece tokenizer of the OCR-error classifier: the behaviour of DistilBertTokenizer (surya/ocr_error/tokenizer.py, a BERT tokenizer)
as OCRErrorPredictor calls it -- `processor(texts, padding="longest", truncation=True)` -- restated for speed on page text:

  1. the special tokens ([UNK] [SEP] [PAD] [CLS] [MASK]) are cut out of the text verbatim and never split;
  2. basic step on the rest: drop NUL, U+FFFD and control characters (Unicode category C*, except tab / newline / CR), map whitespace
     (space, tab, newline, CR, category Zs) to a space, put spaces around CJK ideographs, NFC-normalise, split on whitespace; then per
     word: lower-case (do_lower_case) and strip accents (NFD, drop category Mn) unless strip_accents is False -- or strip them alone
     when strip_accents is True --, and split off every punctuation character (ASCII non-alphanumerics and category P*);
  3. greedy longest-match-first WordPiece per word, continuation pieces prefixed "##"; a word over 100 characters, or one with no
     complete cover, becomes [UNK];
  4. [CLS] + pieces + [SEP], truncated to the model's maximum length (the pieces are cut, the two specials stay).

Words repeat heavily on a page, so step 2's per-word work and step 3 are memoised per instance (word -> ids)."""
from __future__ import annotations

import json
import os
import re
import unicodedata
from typing import Dict, List, Optional, Sequence

SPECIAL_TOKENS = ("[UNK]", "[SEP]", "[PAD]", "[CLS]", "[MASK]")
MAX_CHARS_PER_WORD = 100


def _is_cjk(cp: int) -> bool:
    return (0x4E00 <= cp <= 0x9FFF or 0x3400 <= cp <= 0x4DBF or 0x20000 <= cp <= 0x2A6DF or 0x2A700 <= cp <= 0x2B73F
            or 0x2B740 <= cp <= 0x2B81F or 0x2B820 <= cp <= 0x2CEAF or 0xF900 <= cp <= 0xFAFF or 0x2F800 <= cp <= 0x2FA1F)


def _is_punct(ch: str) -> bool:
    cp = ord(ch)
    if 33 <= cp <= 47 or 58 <= cp <= 64 or 91 <= cp <= 96 or 123 <= cp <= 126:
        return True
    return unicodedata.category(ch).startswith("P")


class WordPieceTokenizer:
    def __init__(self, vocab: Dict[str, int], *, do_lower_case: bool = True, strip_accents: Optional[bool] = None,
                 tokenize_chinese_chars: bool = True, model_max_length: int = 512, max_positions: Optional[int] = None):
        self.vocab = vocab
        self.do_lower_case = do_lower_case
        self.strip_accents = strip_accents
        self.tokenize_chinese_chars = tokenize_chinese_chars
        self.model_max_length = int(model_max_length)
        self.max_length = min(self.model_max_length, int(max_positions)) if max_positions else self.model_max_length
        missing = [t for t in SPECIAL_TOKENS if t not in vocab]
        if missing:
            raise ValueError(f"vocabulary lacks the special tokens {missing}")
        self.unk_id, self.cls_id, self.sep_id, self.pad_id = (vocab["[UNK]"], vocab["[CLS]"], vocab["[SEP]"], vocab["[PAD]"])
        self._special_re = re.compile("(" + "|".join(re.escape(t) for t in SPECIAL_TOKENS) + ")")
        self._char_memo: Dict[str, str] = {}
        self._word_memo: Dict[str, List[int]] = {}

    @classmethod
    def from_dir(cls, path: str, max_positions: Optional[int] = None) -> "WordPieceTokenizer":
        """vocab.txt (one token per line, id = line number) and tokenizer_config.json (do_lower_case, strip_accents,
        tokenize_chinese_chars, model_max_length) of a checkpoint directory."""
        vocab: Dict[str, int] = {}
        with open(os.path.join(path, "vocab.txt"), encoding="utf-8") as f:
            for i, line in enumerate(f):
                vocab[line.rstrip("\n")] = i             # a repeated line takes the later id, as BERT's load_vocab does
        tc = {}
        p = os.path.join(path, "tokenizer_config.json")
        if os.path.exists(p):
            with open(p) as f:
                tc = json.load(f)
        mml = tc.get("model_max_length", 512)
        if not isinstance(mml, (int, float)) or mml > 1 << 30:      # transformers writes a huge sentinel for "no limit"
            mml = 1 << 30
        return cls(vocab, do_lower_case=tc.get("do_lower_case", True), strip_accents=tc.get("strip_accents"),
                   tokenize_chinese_chars=tc.get("tokenize_chinese_chars", True), model_max_length=int(mml), max_positions=max_positions)

    # ------------------------------------------------------------------------------------------------ basic step
    def _char(self, ch: str) -> str:
        out = self._char_memo.get(ch)
        if out is None:
            cp = ord(ch)
            cat = unicodedata.category(ch)
            if ch in " \t\n\r" or cat == "Zs":
                out = " "
            elif cp == 0 or cp == 0xFFFD or cat.startswith("C"):
                out = ""
            elif self.tokenize_chinese_chars and _is_cjk(cp):
                out = " " + ch + " "
            else:
                out = ch
            self._char_memo[ch] = out
        return out

    def _word_ids(self, word: str) -> List[int]:
        ids = self._word_memo.get(word)
        if ids is not None:
            return ids
        w = word
        if self.do_lower_case:
            w = w.lower()
            if self.strip_accents is not False:
                w = "".join(c for c in unicodedata.normalize("NFD", w) if unicodedata.category(c) != "Mn")
        elif self.strip_accents:
            w = "".join(c for c in unicodedata.normalize("NFD", w) if unicodedata.category(c) != "Mn")
        parts: List[str] = []
        cur: List[str] = []
        for c in w:
            if _is_punct(c):
                if cur:
                    parts.append("".join(cur))
                    cur = []
                parts.append(c)
            else:
                cur.append(c)
        if cur:
            parts.append("".join(cur))
        ids = []
        for tok in " ".join(parts).split():
            ids.extend(self._wordpiece(tok))
        self._word_memo[word] = ids
        return ids

    def _wordpiece(self, tok: str) -> List[int]:
        if len(tok) > MAX_CHARS_PER_WORD:
            return [self.unk_id]
        out, start, n, vocab = [], 0, len(tok), self.vocab
        while start < n:
            end = n
            hit = None
            while start < end:
                sub = tok[start:end] if start == 0 else "##" + tok[start:end]
                hit = vocab.get(sub)
                if hit is not None:
                    break
                end -= 1
            if hit is None:
                return [self.unk_id]
            out.append(hit)
            start = end
        return out

    # ------------------------------------------------------------------------------------------------ public
    def tokenize_ids(self, text: str) -> List[int]:
        """Ids of the text's pieces, without [CLS] / [SEP] and untruncated."""
        ids: List[int] = []
        for seg in self._special_re.split(text):
            if not seg:
                continue
            if seg in SPECIAL_TOKENS:
                ids.append(self.vocab[seg])
                continue
            clean = unicodedata.normalize("NFC", "".join(map(self._char, seg)))
            for word in clean.split():
                ids.extend(self._word_ids(word))
        return ids

    def encode(self, text: str) -> List[int]:
        """[CLS] + pieces + [SEP], truncated to max_length tokens."""
        body = self.tokenize_ids(text)[: max(0, self.max_length - 2)]
        return [self.cls_id] + body + [self.sep_id]

    def __call__(self, texts: Sequence[str]) -> List[List[int]]:
        return [self.encode(t) for t in texts]


def vocab_from_list(tokens: Sequence[str]) -> Dict[str, int]:
    return {t: i for i, t in enumerate(tokens)}
