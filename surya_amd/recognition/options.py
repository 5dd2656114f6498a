"""The per-line decoding options and the extra per-step output sets of the recognition call path, each described ONCE (DESIGN.md
section 4t). predictor.py and loop.py spell out no option's keys or setters: every stage the data passes through -- the flat dict, the
rank's share, a streamed chunk, prepare_lines' dict, DeviceLoop.admit, the slot setters, the switches -- is a loop over LINE_OPTIONS or a
helper below.

A per-line option is "a table per call plus one integer per line, -1 = off": the call's dict carries the table under `table_key`
(and what else the call fixes, `call_keys`), every dict of lines one integer per line under `line_key`. LineConstraints holds the
table as `cons_table` and the integers per image as `cons_per_image`; the model takes the table with `set_table` (None = off) and the
integers of freshly prefilled slots with `set_slot(slots, values, *call values)`. `count(table)` is the number of rows / states a
line's integer may name, `admit_msg` what DeviceLoop.admit says to one that names none.

An extra output set is what the model reports per step beside token, score and box; at most one is on in a loop. `fields` are the
loop's matrices [lines, cap, *tail] (attribute name, dtype, tail, fill), `read` / `wait` the model's calls (after a prefill / a
decode call), `last` the predictor attribute `generate` publishes the matrices under."""
from collections import namedtuple
from dataclasses import dataclass

import numpy as np


ExtraField = namedtuple("ExtraField", "attr dtype tail fill")
ExtraSet = namedtuple("ExtraSet", "name fields read wait last")
_A = (4,)                                                     # SA_MAX_ALTERNATIVES (loop.py)
ALTERNATIVES = ExtraSet("alternatives", (ExtraField("alt_tok_mat", np.int32, _A, -1), ExtraField("alt_p_mat", np.float32, _A, 0)),
                        "read_alternatives", "wait_alternatives", "last_alternatives")
FORCED = ExtraSet("forced", (ExtraField("greedy_tok_mat", np.int32, (), 0), ExtraField("greedy_p_mat", np.float32, (), 0),
                             ExtraField("logp_mat", np.float32, (), 0)), "read_forced", "wait_forced", "last_forced")
BOOST_PLAIN = ExtraSet("boost", (ExtraField("plain_tok_mat", np.int32, (), 0), ExtraField("plain_p_mat", np.float32, (), 0)),
                       "read_boost", "wait_boost", "last_boost")
EXTRA_SETS = (ALTERNATIVES, FORCED, BOOST_PLAIN)
EXTRA_ATTRS = {f.attr: (s, i) for s in EXTRA_SETS for i, f in enumerate(s.fields)}


@dataclass(frozen=True, eq=False)
class LineOption:
    name: str
    table_key: str
    line_key: str
    cons_table: str
    cons_per_image: str
    set_table: str
    set_slot: str
    count: callable
    admit_msg: str
    call_keys: tuple = ()
    excludes: tuple = ()              # the loop modes ("beam", "forced", "alternatives") and options (by name) it cannot run beside ...
    excludes_msg: str = ""            # ... and what DeviceLoop.run says to a caller who asks for both
    extra: ExtraSet = None            # the extra output set that is on while the option is


def _n_states(tables) -> int:
    return int(tables.n_states)


MASKS = LineOption("masks", "token_masks", "mask_ids", "table", "per_image", "set_token_masks", "set_slot_masks", len,
                   "mask ids must name rows of the call's token-mask table")
PATTERNS = LineOption("patterns", "pattern_tables", "start_states", "patterns", "per_image_state", "set_patterns", "set_slot_patterns",
                      _n_states, "start states must name states of the call's pattern tables",
                      excludes=("beam", "forced"), excludes_msg="patterns exclude beam search and forced decoding")
LEXICON = LineOption("lexicon", "lexicon_tables", "lexicon_starts", "lexicons", "per_image_lex", "set_lexicon", "set_slot_lexicon",
                     _n_states, "lexicon start states must name states of the call's lexicon tables",
                     excludes=("beam", "forced"), excludes_msg="lexicons exclude beam search and forced decoding")
BOOST = LineOption("boost", "boost_tables", "boost_roots", "boost", "per_image_root", "set_boost", "set_slot_boost",
                   _n_states, "boost roots must name states of the call's boost tables", call_keys=("boost_weight",),
                   excludes=("alternatives", "beam", "forced", "patterns", "lexicon"),
                   excludes_msg="boosting excludes alternatives, beam search, forced decoding, patterns and lexicons", extra=BOOST_PLAIN)
# The order is the upload order and the set_slot_* order (every table sits behind the mask table, every slot value behind the slot's
# mask id); options are switched off in reverse.
LINE_OPTIONS = (MASKS, PATTERNS, LEXICON, BOOST)


def requested(d) -> list:
    """The options a dict carries the table of, in table order."""
    return [o for o in LINE_OPTIONS if d.get(o.table_key) is not None]


def option_extra(d):
    """The extra output set that the options requested in `d` switch on, or None."""
    return next((o.extra for o in requested(d) if o.extra is not None), None)


def call_part(cons) -> dict:
    """What a call with LineConstraints `cons` fixes once: every requested option's table and call values. A call with `cons` always
    carries the mask table (as its array), whatever the lines' ids."""
    out = {}
    for o in LINE_OPTIONS:
        table = getattr(cons, o.cons_table)
        if table is not None:
            out[o.table_key] = table.array() if o is MASKS else table
            out.update((k, getattr(cons, k)) for k in o.call_keys)
    return out


def line_part(cons, slice_map, pages=None) -> dict:
    """Every requested option's integers, one per line in page order, for `pages` (default: all) holding slice_map[i] lines."""
    out = {}
    for o in LINE_OPTIONS:
        if getattr(cons, o.cons_table) is not None:
            per = getattr(cons, o.cons_per_image)
            out[o.line_key] = cons.line_ids(slice_map, per if pages is None else [per[p] for p in pages])
    return out


def attach(flat, cons) -> tuple:
    """Put call_part and line_part (for flat's pages so far) into `flat`; -> the per-line keys, which are by line id like the slices."""
    lines = line_part(cons, flat["slice_map"])
    flat.update(call_part(cons), **lines)
    return tuple(lines)


def take(d, idx=None) -> dict:
    """The requested options of `d` as a dict of their own: tables and call values as they are, the lines' integers for lines `idx`
    (default: all, the list itself)."""
    out = {}
    for o in requested(d):
        out[o.table_key] = d[o.table_key]
        out.update((k, d[k]) for k in o.call_keys)
        out[o.line_key] = d[o.line_key] if idx is None else [d[o.line_key][i] for i in idx]
    return out


def empty_rows(xs, rows, mid) -> tuple:
    """The matrices of set `xs` for `rows` new lines: [rows, *mid, *tail], filled with the fields' fill values."""
    return tuple(np.full((rows,) + tuple(mid) + f.tail, f.fill, f.dtype) for f in xs.fields)
