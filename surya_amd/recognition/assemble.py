"""Output assembly of the recognition predictor: finished token streams -> TextLine / TextChar objects (reference
recognition/__init__.py:609-771 + :886-925). Plain functions of the processor (three stop ids and the tokenizer) and the call's
`flat` dict; RecognitionPredictor keeps one-line delegations under its historical method names."""
import re
from array import array
from typing import List, Optional

import numpy as np

from ..common.geometry import PolygonBox, coerce_polygon
from ..common.imageops import Curve, curve_size, curve_to_page, quad_homography, quad_size
from .postprocess import (clean_math_tags, detect_repeat_token, fix_unbalanced_tags, prediction_to_polygon_batch, unwrap_math,
                          words_from_chars)
from .processor import NOMATH_TOKEN
from .schema import CharAlternative, LineHypothesis, TaskNames, TextChar, TextLine

_SCRIPT_TAG = re.compile(r"<SCRIPT-\w+>")
_CHAR_FIELDS = frozenset(("polygon", "confidence", "text", "bbox_valid"))
assert _CHAR_FIELDS | {"alternatives", "greedy", "plain", "plain_confidence"} == frozenset(TextChar.model_fields), "TextChar fields changed: update _text_char"
_new_char, _set = TextChar.__new__, object.__setattr__


def _text_char(polygon, confidence, text, bbox_valid) -> TextChar:
    """TextChar.model_construct(...) with all four fields given, without its per-call field loop (1.9 -> 0.55 us; a page of
    text is ~10^4 of these). Same object state: __dict__, fields_set, no extras, no private attributes."""
    m = _new_char(TextChar)
    _set(m, "__dict__", {"polygon": polygon, "confidence": confidence, "text": text, "bbox_valid": bbox_valid, "alternatives": None,
                         "greedy": None, "plain": None, "plain_confidence": None})
    _set(m, "__pydantic_fields_set__", set(_CHAR_FIELDS))        # (alternatives, greedy, plain*: the defaults, as in TextChar(...) without them)
    _set(m, "__pydantic_extra__", None)
    _set(m, "__pydantic_private__", None)
    return m


_LINE_FIELDS = ("polygon", "confidence", "text", "chars", "original_text_good", "words", "log_prob", "hypotheses", "pattern_matched",
                "lexicon_index", "boost_matches", "rectified", "variant", "readings", "unrolled")
assert frozenset(_LINE_FIELDS) == frozenset(TextLine.model_fields), "TextLine fields changed: update _text_line"
_new_line = TextLine.__new__
_BLANK_POLY = np.array([[0, 0], [0, 1], [1, 1], [1, 0]], np.float64)


def _text_line(polygon, confidence, text, chars, words) -> TextLine:
    """TextLine(...) for values that are already in validated form (polygon = coerce_polygon(...), confidence not NaN, chars a
    list of TextChar): the object state validation would produce, without walking the character list again."""
    m = _new_line(TextLine)
    _set(m, "__dict__", {"polygon": polygon, "confidence": confidence, "text": text, "chars": chars,
                         "original_text_good": False, "words": words, "log_prob": None, "hypotheses": None, "pattern_matched": None,
                         "lexicon_index": None, "boost_matches": None, "rectified": None, "variant": None, "readings": None,
                         "unrolled": None})
    _set(m, "__pydantic_fields_set__", {"polygon", "confidence", "text", "chars", "words"})     # as TextLine(text=, polygon=, ...)
    _set(m, "__pydantic_extra__", None)
    _set(m, "__pydantic_private__", None)
    return m


class AltDecoder:
    """Token id -> text of ONE alternative, cached for a call: a UTF-16 unit decodes alone (a lone surrogate gives ""), special and
    math ids decode through the tokenizer as `line_runs` decodes their runs. The three stop ids (eos, pad, no-output: "the line ends
    here") never become characters of a line and read "" as alternatives; their token_id says which one it was."""

    def __init__(self, proc):
        self.tk = proc.ocr_tokenizer
        self.cache = {proc.eos_token_id: "", proc.pad_token_id: "", proc.no_output_token: ""}

    def __call__(self, t: int) -> str:
        s = self.cache.get(t)
        if s is None:
            tk = self.tk
            if t >= tk.special_token_offset:
                s = array("H", [(t - tk.special_token_offset) & 0xFFFF]).tobytes().decode("utf-16le", errors="ignore")
            else:
                s = tk.decode([t], task=TaskNames.ocr_without_boxes if t >= tk.qwen_offset else TaskNames.block_without_boxes)
            self.cache[t] = s
        return s


def attach_alternatives(chars, csrc, alts, top_k, decode) -> None:
    """chars[i].alternatives = the first `top_k` alternatives of token csrc[i] -- the token the character takes its confidence
    from -- without the missing entries (id -1: fewer ids were allowed). alts = (ids [T, 4], probabilities [T, 4])."""
    ids, pr = alts[0].tolist(), alts[1].tolist()
    for ch, j in zip(chars, csrc):
        ch.alternatives = [CharAlternative.model_construct(text=decode(t), confidence=p, token_id=t)
                           for t, p in zip(ids[j][:top_k], pr[j][:top_k]) if t >= 0]
        ch.__pydantic_fields_set__.add("alternatives")


def attach_greedy(chars, csrc, forced, decode) -> None:
    """chars[i].greedy = the model's own reading at token csrc[i] -- the token the character takes its confidence from -- of an
    aligned line. forced = (greedy ids [T], their probabilities [T], log-probabilities of the forced ids [T])."""
    ids, pr = forced[0].tolist(), forced[1].tolist()
    for ch, j in zip(chars, csrc):
        ch.greedy = CharAlternative.model_construct(text=decode(ids[j]), confidence=pr[j], token_id=ids[j])
        ch.__pydantic_fields_set__.add("greedy")


def set_log_prob(line: TextLine, forced) -> TextLine:
    """line.log_prob = the sum of an aligned line's forced log-probabilities, eos included (float64 sum of the fp32 values)."""
    line.log_prob = float(np.sum(np.asarray(forced[2], np.float64)))
    line.__pydantic_fields_set__.add("log_prob")
    return line


def set_pattern_matched(flat, sorted_pos, tokens, line: TextLine) -> TextLine:
    """line.pattern_matched for a line read under a pattern (flat["pattern_tables"], flat["start_states"] by sorted position): the host
    replay of the automaton over the line's tokens -- true iff the line ended with EOS in an accepting state. A line without a
    pattern keeps None."""
    tables = flat.get("pattern_tables")
    if tables is not None:
        st = int(flat["start_states"][sorted_pos])
        if st >= 0:
            line.pattern_matched = bool(tables.matched(st, tokens))
            line.__pydantic_fields_set__.add("pattern_matched")
    return line


def set_lexicon_index(flat, sorted_pos, tokens, line: TextLine) -> TextLine:
    """line.lexicon_index for a line read under a lexicon (flat["lexicon_tables"], flat["lexicon_starts"] by sorted position): the host
    replay of the automaton over the line's tokens (not a comparison of the cleaned text) -- the entry's index in the line's own list
    iff the line ended in a terminal state, else -1. A line without a lexicon keeps None."""
    tables = flat.get("lexicon_tables")
    if tables is not None:
        st = int(flat["lexicon_starts"][sorted_pos])
        if st >= 0:
            line.lexicon_index = int(tables.entry_of(tables.lexicon_of_start(st), tokens))
            line.__pydantic_fields_set__.add("lexicon_index")
    return line


def boost_items(flat, items):
    """The items of a boosted call with their sixth element -- (plain ids [T], the emitted tokens' plain probabilities [T]) -- in the
    form of one alternative per token, and the flat dict that assembles them so: the characters then take `plain` from the token
    `alternatives` and `greedy` take theirs from."""
    inner = {**flat, "boost_tables": None, "top_k": 1}
    return inner, [tuple(it[:5]) + ((np.asarray(it[5][0])[:, None], np.asarray(it[5][1])[:, None]),) if len(it) > 5 and it[5] is not None
                   else tuple(it[:5]) for it in items]


def set_boost_fields(flat, sorted_pos, tokens, line: TextLine) -> TextLine:
    """A line of a boosted call (flat["boost_tables"], flat["boost_roots"] by sorted position), assembled with its plain readings as
    one-entry alternatives: a boosted line gets boost_matches -- the host replay of the automaton over its tokens -- and its characters
    plain / plain_confidence; a line that was not boosted keeps None everywhere."""
    root = int(flat["boost_roots"][sorted_pos])
    for ch in line.chars:
        alt, ch.alternatives = ch.alternatives, None
        ch.__pydantic_fields_set__.discard("alternatives")
        if root >= 0 and alt:
            ch.plain, ch.plain_confidence = alt[0].text, alt[0].confidence
            ch.__pydantic_fields_set__.update(("plain", "plain_confidence"))
    if root >= 0:
        line.boost_matches = [int(i) for i in flat["boost_tables"].matches(root, tokens)]
        line.__pydantic_fields_set__.add("boost_matches")
    return line


def line_quad(flat, orig):
    """The quad line `orig` was warped from (a call with `rectify` set keeps flat["quads"] by original position), else None."""
    curves = flat.get("curves")
    if curves is not None and curves[orig] is not None:       # (a call with `unroll` set keeps flat["curves"] likewise: a Curve)
        return curves[orig]
    quads = flat.get("quads")
    return None if quads is None else quads[orig]


def set_rectified(flat, orig, line: TextLine) -> TextLine:
    """line.rectified in a call with `rectify` set: whether this line was warped. Every other call leaves None."""
    if flat.get("quads") is not None:
        line.rectified = flat["quads"][orig] is not None
        line.__pydantic_fields_set__.add("rectified")
    if flat.get("curves") is not None:                        # likewise in a call with `unroll` set: whether the line was unrolled
        line.unrolled = flat["curves"][orig] is not None
        line.__pydantic_fields_set__.add("unrolled")
    return line


def quad_to_page(P, quad, res_scale):
    """Corners P [..., 2] (float64, in place) of a rectified line's characters, in rectified-crop coordinates, onto the page: clamped
    into [0, W] x [0, H], mapped through the line's homography in float64, then the high-res rescale with int() truncation of the
    ordinary path (chars_of). This replaces its shift and clamp-into-bbox: the characters of a tilted line are tilted quads. (The
    mapped coordinates are rounded to 1e-6 px in front of the truncation, so that the round-off of the solve never moves a corner
    that sits on an integer down a pixel.) An UNROLLED line (`quad` is a Curve) goes through curve_to_page the same way: its
    characters come back as tilted quads that follow the bend."""
    if isinstance(quad, Curve):
        W, H, _ = curve_size(*quad)
        uv = np.stack([np.clip(P[..., 0], 0.0, float(W)), np.clip(P[..., 1], 0.0, float(H))], -1)
        xy = curve_to_page(uv, *quad)
        P[..., 0] = np.trunc(np.round(xy[..., 0], 6) * (1.0 / res_scale[0]))
        P[..., 1] = np.trunc(np.round(xy[..., 1], 6) * (1.0 / res_scale[1]))
        return P
    W, H = quad_size(quad)
    h = quad_homography(quad, W, H)
    u, v = np.clip(P[..., 0], 0.0, float(W)), np.clip(P[..., 1], 0.0, float(H))
    w = h[6] * u + h[7] * v + h[8]
    x, y = (h[0] * u + h[1] * v + h[2]) / w, (h[3] * u + h[4] * v + h[5]) / w
    P[..., 0] = np.trunc(np.round(x, 6) * (1.0 / res_scale[0]))
    P[..., 1] = np.trunc(np.round(y, 6) * (1.0 / res_scale[1]))
    return P


def assemble_beam_batch(proc, flat, items, drop_repeated_text, return_words, bbox_size) -> List[TextLine]:
    """A beam-search call's lines: items = [(sorted position, original position, hypotheses)], hypotheses the loop's BeamHypothesis list
    of the line, best first. Every hypothesis goes through assemble_batch like a greedy line (tokens, per-token probabilities as scores,
    box rows; drop_repeated_text and return_words apply to each); the TextLine is hypothesis 0 with log_prob and `hypotheses` set. A line
    without a hypothesis (no candidate at all) is the empty line."""
    flat_items, owner = [], []
    for i, (sp, orig, hyps) in enumerate(items):
        for h in hyps or [None]:
            flat_items.append((sp, orig, [], [], np.zeros((1, 6), np.float32)) if h is None else (sp, orig, h.tokens, h.scores, h.bboxes))
            owner.append(i)
    lines = assemble_batch(proc, flat, flat_items, drop_repeated_text, return_words, bbox_size)
    out, at = [], 0
    for i, (_, _, hyps) in enumerate(items):
        n = max(len(hyps), 1)
        mine = lines[at:at + n]
        at += n
        line = mine[0]
        line.hypotheses = [LineHypothesis(text=ln.text, confidence=ln.confidence, log_prob=h.log_prob, finished=h.finished, chars=ln.chars,
                                          words=ln.words) for ln, h in zip(mine, hyps)]
        line.__pydantic_fields_set__.add("hypotheses")
        if hyps:
            line.log_prob = float(hyps[0].log_prob)
            line.__pydantic_fields_set__.add("log_prob")
        out.append(line)
    return out


def get_bboxes_text(proc, flat, predicted_tokens, scores, predicted_polygons, drop_repeated_text=False, csrc_out=None) -> list:
    """Token stream -> per line (texts, confidences, bbox_valid, polygons [n, 4, 2]) (reference :609-771): the stream is cut
    into runs of math-BPE ids, single special tags and UTF-16 ids; only the last kind carries per-character boxes.
    Array form of the reference's per-token loop: run boundaries, close-polygon filtering and the
    char -> box index map are numpy expressions per line; Python only walks the (few) runs of a line. Lines come back as
    None (<NOP>), or a tuple that `chars_of` turns into TextChars after the geometry has been applied in bulk."""
    eos, pad, nop = proc.eos_token_id, proc.pad_token_id, proc.no_output_token
    out = []
    for tokens, polys, sc in zip(predicted_tokens, predicted_polygons, scores):
        if csrc_out is not None:
            csrc_out.append(None)                    # replaced below for a line that has characters of its own
        if nop in tokens:
            out.append(None)
            continue
        if drop_repeated_text and detect_repeat_token(tokens):
            out.append(([""], np.zeros(1), np.zeros(1, bool), _BLANK_POLY[None].copy()))
            continue
        tid = np.asarray(tokens, np.int64)
        stop = np.nonzero((tid == eos) | (tid == pad))[0]
        n = int(stop[0]) if len(stop) else len(tid)
        n = min(n, len(polys), len(sc))              # zip() of the reference stops at the shortest of the three
        if n == 0:
            out.append(([], np.zeros(0), np.zeros(0, bool), np.zeros((0, 4, 2))))
            continue
        tid = tid[:n]
        P = np.asarray(polys[:n], np.float64)
        conf = np.asarray(sc[:n], np.float64)
        # clean_close_polygons: a box is dropped when all 4 corners sit within 0.1 of the PREVIOUS box of its run (util.py:100-120)
        far = (np.abs(P[1:] - P[:-1]).reshape(n - 1, 8).max(axis=1) > 0.1).tolist() if n > 1 else []
        texts, src, csrc, valid = line_runs(proc, tid.tolist(), far)
        if not texts:
            out.append(([], np.zeros(0), np.zeros(0, bool), np.zeros((0, 4, 2))))
        else:
            v = np.asarray(valid, bool)
            pp = P[src]
            pp[~v] = _BLANK_POLY
            out.append((texts, conf[csrc], v, pp))
            if csrc_out is not None:
                csrc_out[-1] = csrc
    return out


def line_runs(proc, ids: list, far: list):
    """The runs of one token stream (already cut at eos / pad): per output char its text, the token whose BOX it takes, the
    token whose CONFIDENCE it takes, bbox_valid. `far[j]`: box j + 1 differs from box j by more than 0.1 in some corner. The
    reference indexes a run's unfiltered confidences with the index into its FILTERED boxes (:700-712): kept as is."""
    tk = proc.ocr_tokenizer
    q_off, s_off = tk.qwen_offset, tk.special_token_offset
    n = len(ids)
    texts, src, csrc, valid = [], [], [], []
    if n and min(ids) >= s_off:
        kind = None                                  # one UTF-16 run (the usual line of text)
    else:
        kind = [0 if t < q_off else (1 if t < s_off else 2) for t in ids]
    a_ = 0
    while a_ < n:
        if kind is None:
            k, b_ = 2, n
        else:
            k = kind[a_]
            b_ = a_ + 1
            if k != 1:
                while b_ < n and kind[b_] == k:
                    b_ += 1
        if k == 2:
            # a run of UTF-16 code units decodes in one piece (tokenizer._decode_ocr's flush of a non-math buffer)
            # (ids above the tokenizer's range -- a checkpoint with a padded lm_head -- wrap into 16 bits like the byte masking
            # of tokenizer._decode_ocr instead of raising OverflowError)
            text = array("H", [(t - s_off) & 0xFFFF for t in ids[a_:b_]]).tobytes().decode("utf-16le", errors="ignore")
            if text:
                boxes = [a_] + [j for j in range(a_ + 1, b_) if far[j - 1]]
                L, nb = len(text), len(boxes)
                texts.extend(text)
                src.extend(boxes[:L] if L <= nb else boxes + [boxes[-1]] * (L - nb))      # char i -> box min(i, nb - 1)
                csrc.extend(range(a_, a_ + L) if L <= nb else list(range(a_, a_ + nb)) + [a_ + nb - 1] * (L - nb))
                valid.extend([True] * L)
        else:
            text = tk.decode(ids[a_:b_], task=TaskNames.ocr_without_boxes if k == 1 else TaskNames.block_without_boxes)
            if not (k == 1 and (text == NOMATH_TOKEN or _SCRIPT_TAG.match(text))):
                texts.append(text); src.append(a_); csrc.append(a_); valid.append(False)
        a_ = b_
    return texts, src, csrc, valid


def chars_of(line, res_scale, line_bbox, quad=None) -> List[TextChar]:
    """TextChars of one line with the reference's per-char geometry (:905-909: rescale by the high-res factor with int()
    truncation, shift to the line's corner, clamp into the line's bbox) applied to all of the line's polygons at once;
    objects are built without re-validating fields that were just computed (pydantic model_construct). A rectified line
    (`quad`) takes quad_to_page instead of the shift and clamp."""
    texts, conf, valid, P = line
    if not texts:
        return []
    P = P.copy()
    if quad is not None:
        quad_to_page(P, quad, res_scale)
    else:
        P[..., 0] = np.trunc(P[..., 0] * (1.0 / res_scale[0])) + line_bbox[0]
        P[..., 1] = np.trunc(P[..., 1] * (1.0 / res_scale[1])) + line_bbox[1]
        np.clip(P[..., 0], line_bbox[0], line_bbox[2], out=P[..., 0])
        np.clip(P[..., 1], line_bbox[1], line_bbox[3], out=P[..., 1])
    polys = P.tolist()
    conf = [0.0 if c != c else c for c in conf.tolist()]               # BaseChar: NaN -> 0, stored as a float
    return [_text_char(pg, c, t, v) for pg, c, t, v in zip(polys, conf, texts, valid.tolist())]


def assemble_line(proc, flat, sorted_pos, orig, tokens, sc, bbox_rows, drop_repeated_text, return_words, bbox_size, alts=None) -> TextLine:
    """One line's TextLine from its finished token stream (reference :609-771 + :886-925). alts = (ids [T, 4], probabilities [T, 4])
    of the line's tokens with flat["top_k"] set: every character of the stream gets `alternatives` (characters that
    fix_unbalanced_tags inserts keep None)."""
    if (flat.get("quads") is not None or flat.get("curves") is not None) and not flat.get("_quads_set"):      # a call with `rectify` / `unroll`: the line, then whether it was warped
        line = assemble_line(proc, {**flat, "_quads_set": True}, sorted_pos, orig, tokens, sc, bbox_rows, drop_repeated_text, return_words,
                             bbox_size, alts=alts)
        return set_rectified(flat, orig, line)
    if flat.get("boost_tables") is not None:          # a boosted call: alts = (plain ids [T], the emitted tokens' plain probabilities [T])
        inner, its = boost_items(flat, [(sorted_pos, orig, tokens, sc, bbox_rows, alts)])
        line = assemble_line(proc, inner, sorted_pos, orig, tokens, sc, bbox_rows, drop_repeated_text, return_words, bbox_size,
                             alts=its[0][5] if len(its[0]) > 5 else None)
        return set_boost_fields(flat, sorted_pos, tokens, line)
    if flat.get("lexicon_tables") is not None:        # a call with lexicons: likewise (it may hold pattern lines too)
        line = assemble_line(proc, {**flat, "lexicon_tables": None}, sorted_pos, orig, tokens, sc, bbox_rows, drop_repeated_text, return_words,
                             bbox_size, alts=alts)
        return set_lexicon_index(flat, sorted_pos, tokens, line)
    if flat.get("pattern_tables") is not None:        # a call with patterns: the plain line, then the host replay of its automaton
        line = assemble_line(proc, {**flat, "pattern_tables": None}, sorted_pos, orig, tokens, sc, bbox_rows, drop_repeated_text, return_words,
                             bbox_size, alts=alts)
        return set_pattern_matched(flat, sorted_pos, tokens, line)
    if alts is not None and flat.get("forced"):       # an aligned line: alts = (greedy ids, probabilities, forced log-probabilities)
        forced, flat = alts, {**flat, "forced": False}
        line = assemble_line(proc, flat, sorted_pos, orig, tokens, sc, bbox_rows, drop_repeated_text, return_words, bbox_size,
                             alts=(forced[0][:, None], forced[1][:, None]))
        for ch in line.chars:                         # the same char -> token map as alternatives: entry 0 of a one-entry list
            if ch.alternatives is not None:
                ch.greedy, ch.alternatives = ch.alternatives[0], None
                ch.__pydantic_fields_set__.discard("alternatives")
                ch.__pydantic_fields_set__.add("greedy")
        return set_log_prob(line, forced)
    polygon, res_scale = flat["polygons"][orig], flat["res_scales"][orig]
    polys = prediction_to_polygon_batch(bbox_rows[None], [flat["slices"][sorted_pos].shape], bbox_size, bbox_size // 2)
    csrc = [] if alts is not None else None
    chars = get_bboxes_text(proc, flat, [tokens], [sc], polys, drop_repeated_text, csrc_out=csrc)[0]
    if chars is None or not chars[0]:      # <NOP> (input text was good) or nothing decoded (reference :889-899)
        return TextLine(text="", polygon=polygon, chars=[], confidence=1, original_text_good=True)
    # mean of the characters' confidences as the TextChar objects hold them (NaN -> 0, schema.py), reference :899-903
    confidence = float(np.mean(np.where(np.isnan(chars[1]), 0.0, chars[1])))
    box = PolygonBox(polygon=polygon)
    chars = chars_of(chars, res_scale, box.bbox, line_quad(flat, orig))
    if alts is not None and csrc[0] is not None:
        attach_alternatives(chars, csrc[0], alts, flat.get("top_k") or 1, AltDecoder(proc))
    chars = fix_unbalanced_tags(chars, proc.ocr_tokenizer.special_tokens)
    text = clean_math_tags(unwrap_math("".join(c.text for c in chars)))
    return TextLine(text=text, polygon=polygon, chars=chars, confidence=confidence,
                    words=words_from_chars(chars, box) if return_words else [])


def assemble_batch(proc, flat, items, drop_repeated_text, return_words, bbox_size) -> List[TextLine]:
    """TextLines of several finished lines at once; items = [(sorted_pos, orig, tokens, scores, bbox_rows[T, 6])], with a sixth
    element (alternative ids [T, 4], probabilities [T, 4]) when the call asked for alternatives (flat["top_k"]). The same
    result as `assemble_line` per item (tests/test_assemble_cpu.py compares the two), but the numpy work -- box tokens ->
    polygons, close-box filter, per-char rescale / shift / clamp -- is done ONCE for the whole batch instead of ~25 small
    array calls per line, and TextLine is built from values that are already in validated form. Python walks only the token
    runs (`line_runs`) and creates the character objects. ~430 -> 80-90 us per 45-character line (tools/hostbench/assemble_cost.py)."""
    if (flat.get("quads") is not None or flat.get("curves") is not None) and not flat.get("_quads_set"):
        out = assemble_batch(proc, {**flat, "_quads_set": True}, items, drop_repeated_text, return_words, bbox_size)
        return [set_rectified(flat, it[1], line) for it, line in zip(items, out)]
    if flat.get("boost_tables") is not None:
        inner, its = boost_items(flat, items)
        out = assemble_batch(proc, inner, its, drop_repeated_text, return_words, bbox_size)
        return [set_boost_fields(flat, it[0], it[2], line) for it, line in zip(items, out)]
    if flat.get("lexicon_tables") is not None:
        out = assemble_batch(proc, {**flat, "lexicon_tables": None}, items, drop_repeated_text, return_words, bbox_size)
        return [set_lexicon_index(flat, it[0], it[2], line) for it, line in zip(items, out)]
    if flat.get("pattern_tables") is not None:
        out = assemble_batch(proc, {**flat, "pattern_tables": None}, items, drop_repeated_text, return_words, bbox_size)
        return [set_pattern_matched(flat, it[0], it[2], line) for it, line in zip(items, out)]
    if flat.get("forced"):          # aligned lines: the sixth element is (greedy ids, probabilities, forced log-probabilities) [T] each
        plain = {**flat, "forced": False}
        forced_of = [it[5] for it in items]
        out = _assemble_batch_forced(proc, plain, [tuple(it[:5]) for it in items], forced_of, drop_repeated_text, return_words, bbox_size)
        return [set_log_prob(line, f) for line, f in zip(out, forced_of)]
    return _assemble_batch_forced(proc, flat, items, None, drop_repeated_text, return_words, bbox_size)


def _assemble_batch_forced(proc, flat, items, forced_of, drop_repeated_text, return_words, bbox_size) -> List[TextLine]:
    """assemble_batch; forced_of (or None): per item the forced-decoding outputs its characters take `greedy` from."""
    eos, pad, nop = proc.eos_token_id, proc.pad_token_id, proc.no_output_token
    out: List[Optional[TextLine]] = [None] * len(items)
    work, t_max = [], 0
    decode = None
    for i, it in enumerate(items):
        sp, orig, tokens, sc, rows = it[:5]
        if nop in tokens or (drop_repeated_text and detect_repeat_token(tokens)):
            if forced_of is not None:
                out[i] = assemble_line(proc, {**flat, "forced": True}, sp, orig, tokens, sc, rows, drop_repeated_text, return_words, bbox_size,
                                       alts=forced_of[i])
                continue
            out[i] = assemble_line(proc, flat, sp, orig, tokens, sc, rows, drop_repeated_text, return_words, bbox_size,
                                   alts=it[5] if len(it) > 5 else None)
            continue
        n = len(tokens)
        for j, t in enumerate(tokens):
            if t == eos or t == pad:
                n = j
                break
        n = min(n, len(rows), len(sc))
        if n == 0:
            out[i] = TextLine(text="", polygon=flat["polygons"][orig], chars=[], confidence=1, original_text_good=True)
            continue
        work.append((i, n))
        t_max = max(t_max, n)
    if not work:
        return out
    W = len(work)
    R = np.zeros((W, t_max, 6), np.float32)
    for w, (i, n) in enumerate(work):
        R[w, :n] = items[i][4][:n]
    P = prediction_to_polygon_batch(R, [flat["slices"][items[i][0]].shape for i, _ in work], bbox_size,
                                    bbox_size // 2).astype(np.float64)                       # [W, t_max, 4, 2]
    far = (np.abs(P[:, 1:] - P[:, :-1]).reshape(W, t_max - 1, 8).max(axis=2) > 0.1).tolist() if t_max > 1 else [[]] * W
    keep, all_w, all_src, all_conf, all_valid, counts, geo, quad_of = [], [], [], [], [], [], [], []
    for w, (i, n) in enumerate(work):
        sp, orig, tokens, sc, rows = items[i][:5]
        texts, src, csrc, valid = line_runs(proc, tokens[:n], far[w])
        if not texts:                      # nothing decoded (reference :889-899)
            out[i] = TextLine(text="", polygon=flat["polygons"][orig], chars=[], confidence=1, original_text_good=True)
            continue
        polygon = coerce_polygon(flat["polygons"][orig])
        xs, ys = [p[0] for p in polygon], [p[1] for p in polygon]
        bbox = [min(xs), min(ys), max(xs), max(ys)]
        rs = flat["res_scales"][orig]
        keep.append((i, texts, valid, polygon, bbox, csrc))
        quad_of.append(line_quad(flat, orig))
        all_w.extend([w] * len(src)); all_src.extend(src); all_valid.extend(valid)
        all_conf.extend([0.0 if sc[j] != sc[j] else sc[j] for j in csrc])          # TextChar's NaN -> 0 rule
        counts.append(len(src))
        geo.append((1.0 / rs[0], 1.0 / rs[1], bbox[0], bbox[1], bbox[2], bbox[3]))
    if not keep:
        return out
    PP = P[all_w, all_src]                                                                    # [C, 4, 2]
    v_all = np.asarray(all_valid, bool)
    PP[~v_all] = _BLANK_POLY
    g = np.repeat(np.asarray(geo, np.float64), counts, axis=0)[:, :, None]                    # [C, 6, 1]
    if any(q is not None for q in quad_of):                   # rectified lines: their corners in crop coordinates, mapped below
        crop = PP.copy()
    PP[..., 0] = np.minimum(np.maximum(np.trunc(PP[..., 0] * g[:, 0]) + g[:, 2], g[:, 2]), g[:, 4])
    PP[..., 1] = np.minimum(np.maximum(np.trunc(PP[..., 1] * g[:, 1]) + g[:, 3], g[:, 3]), g[:, 5])
    a = 0
    for (i, *_), c, q in zip(keep, counts, quad_of):
        if q is not None:
            PP[a:a + c] = quad_to_page(crop[a:a + c], q, flat["res_scales"][items[i][1]])
        a += c
    polys = PP.tolist()
    conf_arr = np.asarray(all_conf, np.float64)
    special = proc.ocr_tokenizer.special_tokens
    a = 0
    for (i, texts, valid, polygon, bbox, csrc), c in zip(keep, counts):
        b = a + c
        confidence = float(np.mean(conf_arr[a:b]))
        chars = [_text_char(pg, cf, t, v) for pg, cf, t, v in zip(polys[a:b], all_conf[a:b], texts, valid)]
        a = b
        if len(items[i]) > 5 and items[i][5] is not None:
            decode = decode or AltDecoder(proc)
            attach_alternatives(chars, csrc, items[i][5], flat["top_k"], decode)
        if forced_of is not None:
            decode = decode or AltDecoder(proc)
            attach_greedy(chars, csrc, forced_of[i], decode)
        if not all(valid):                                   # tags only come from special / math runs (bbox_valid False)
            chars = fix_unbalanced_tags(chars, special)
            text = "".join(ch.text for ch in chars)
        else:
            text = "".join(texts)
        if "<" in text:
            text = clean_math_tags(unwrap_math(text))
        words = words_from_chars(chars, PolygonBox(polygon=polygon)) if return_words else []
        out[i] = _text_line(polygon, confidence, text, chars, words)
    return out
