"""The recognition device loop: continuous batching over KV slots until every line stopped (reference recognition/__init__.py:501-607).
One DeviceLoop per RecognitionPredictor.generate call owns ALL loop state -- queue, slot table, token / score / box matrices, admitted
chunks, look-ahead queue, the decode call in flight -- so a loop that died leaves nothing behind but what the model handle keeps
(unconsumed look-ahead images: `run` discards them first). It knows the model surface, not the predictor."""
from collections import deque, namedtuple
from contextlib import ExitStack

import numpy as np

from ..settings import settings
from . import options
from .postprocess import detect_repeat_token

FEED_END = object()          # what a `generate(feed=...)` callable returns once no further lines will come
_REP = 40                    # detect_repeat_token's window
_REP_COLS = np.arange(-_REP, 0)
SA_MAX_ALTERNATIVES = 4      # alternatives the model reports per token (include/surya_amd.h)
SA_MAX_BEAMS = 4             # widest beam: the best B of B x 4 candidates is exact beam search for B <= 4

# One reading of a line out of a beam run: token ids (eos included when finished), each token's probability, box rows [T, 6], the sum
# of the tokens' log-probabilities as the device accumulated it, and whether the reading reached eos / pad.
BeamHypothesis = namedtuple("BeamHypothesis", "tokens scores bboxes log_prob finished")


class DeviceLoop:
    """on_done(line, tokens, scores, bbox_rows[T, 6]) is called once per line, as soon as its stream is final; on_flush() after
    every host synchronisation point that finished at least one line (so a caller can hand the lines over in batches).

    `feed` (optional) makes the line list open-ended: `feed(block)` returns the next `prepare_lines` dict whose prompts carry
    the ids that continue the ones already admitted (queue order == id order), None when nothing is ready (only for block =
    False) or FEED_END. The loop polls it between decode calls and blocks on it only when it has nothing left to run, so lines
    can be admitted while their producer (the detector of a streamed detect -> recognise call) still works on later pages.
    Scheduling decisions never change a line's stream (slot / batch-composition invariance), so the result per line is the
    one the closed list gives.

    Per-line options (recognition/options.py: LINE_OPTIONS -- masks, patterns, lexicon, boost -- with every key and model method named
    below): the dict handed to `run` may carry an option's table under its `table_key` (uploaded once with `set_table`, in table order,
    before the first prefill) and every admitted dict one integer per prompt under its `line_key`, naming a row / state of the table,
    -1 = off for the line (the key may be absent or None: all -1). A line's integer stays with the line: `set_slot` puts it on whatever
    slot the line is prefilled into, in table order, so a reused slot takes its new line's values; from then on the model moves the
    slot's state itself, token by token, on the device. Options are switched off in reverse order on the way out, also after an
    exception. An option whose table is absent (or empty) is off: it keeps no array, its model entry points are never called -- a model
    without them works -- and an integer other than -1 under its key fails `admit`. What the options differ in:
      masks     the table is uint32 [n, words], the call's distinct allowed-id sets; every other option's table sits behind it.
      patterns  PatternTables, whose states' allowed sets are rows of the mask table. Not with beam search or forced decoding.
      lexicon   LexiconTables; needs a mask table of at least one row; the model rewrites the slot's own mask row. A line follows a
                pattern or a lexicon, not both. Not with beam search or forced decoding.
      boost     BoostTables, whose word_row names the mask row of the word-unit set, with the call's beta ("boost_weight"), handed to
                `set_slot` behind the roots. Switches the boost output set on (below). Not with alternatives, beam search, forced
                decoding, patterns or lexicons.

    Extra per-step outputs (options.py: EXTRA_SETS; at most one per loop): the model reports more per step than token, score and box;
    the loop keeps it per line in the set's matrices [lines, cap, *tail] -- readable as attributes of the loop, None while their set is
    off -- and hands a finished line's rows to `on_done` as further arguments. A set that is off has no arrays, and the model's `read` /
    `wait` calls for it are never made.
      alternatives  (`alternatives=True`) alt_tok_mat / alt_p_mat [lines, cap, 4]: the SA_MAX_ALTERNATIVES most likely tokens of every
                    step, id -1 = no such entry. set_alternatives switches the mode on for the run and off on the way out.
      forced        (`forced=True`) greedy_tok_mat / greedy_p_mat / logp_mat [lines, cap]: the model's own argmax, that argmax's
                    probability and the emitted token's log-probability. set_forced switches the mode likewise.
      boost         (with the boost option) plain_tok_mat / plain_p_mat [lines, cap]: the token the model would have emitted without
                    the boost and the emitted token's probability without it.

    Forced decoding (`forced=True`, not together with alternatives or token masks): every admitted dict carries "forced_ids", one id
    list per prompt; the loop sets a line's list on whatever slot the line is prefilled into (set_forced_tokens, behind the options'
    slot setters), the line's token budget is the length of its list (an empty list: the line free-runs on the budget it came with),
    and the repeat rule is skipped -- a ground-truth line of forty dashes must not stop early. The model emits the forced ids. Not
    requested: set_forced / set_forced_tokens are never called -- a model without them works.

    Candidate fans (`fan=True`, with `forced=True` only): "forced_ids" holds per prompt a non-empty LIST of non-empty id lists, the
    line's candidates. A line takes as many slots as it has candidates and is prefilled ONCE (the model's prefill_shared: the first of its
    slots is the lead, the prompt's cache rows are copied to the others), each slot forced to one candidate. Lines are admitted from the
    head of the queue while their candidates fit the empty slots and their prompt tokens, counted once per line, fit max_prefill; a line
    that does not fit waits for slots to drain and nothing behind it overtakes it (the look-ahead encoder queue stays in order). From
    the prefill on a line's candidates are independent: each has its own budget, its list's length, finishes on its own and frees its
    slot on its own. The loop's per-line arrays then hold one row per CANDIDATE (row cand_base[line] + j), and predicted_tokens / scores
    stay empty. `on_done(line, results)` fires when the line's last candidate finished: per candidate, in the order given, the tuple
    (greedy ids, their probabilities, forced log-probabilities). Without `fan` prefill_shared is never called.

    Beam search (`beam=B`, 2..4; not together with alternatives or forced decoding): the model keeps the B best readings of a line in
    a group of B consecutive slots, so `slots // B` lines are in flight and everything above that says "slot" means a group. A line is
    prefilled once, into its group's lead slot g * B (its mask id goes to all B slots); the model selects, places and forks on the
    device (csrc/beam_core.h states the rules) and reports per step and slot the token, the parent slot inside the group, the rank,
    the token's probability and the cumulative log-probability. The loop keeps per group [B, cap] token / probability / box histories,
    re-indexed by the parents each step in array form; a child's box is the step's box of its parent's slot. A line ends when all its
    beams are finished, when its token budget is reached (also right after the prefill), or when the repeat rule fires on the
    best-scored live beam. `on_done(line, hypotheses)` gets a list of BeamHypothesis, finished ones by log_prob descending, then the
    unfinished ones; empty beams (fewer candidates than slots) are dropped. The mode is switched on for the run and off on the way
    out, also after an exception. beam=None: set_beam / read_beam / wait_beam are never called -- a model without them works.

    The prompt store (`store="keep"` or `store="restore"`; None: prefill_keep / restore are never called -- a model without them works):
    every admitted dict carries "store_first", one first store row per prompt. A loop run handles either fresh lines or restored lines,
    never both.
      keep     the lines are fresh (tiles, look-ahead encoder and prefill batching as ever), prefilled with the model's prefill_keep,
               which leaves every prompt in the store at its row, and a line stops after the prefill's token: the loop only encodes.
               Not with candidate fans.
      restore  the lines carry no tiles ("tiles" / "tile_offs" may be None): prefill_batch's counterpart calls the model's
               restore(first rows, one slot list per line) for as many lines as there are free slots / groups / candidate fans, behind
               the same set_slot_* and set_forced_tokens calls, and reads the prefill's outputs as ever. There is no encoder, no
               look-ahead queue, no max_prefill chunking and no `min_prefill_ratio` wait: a landing is a copy, so any free slot is
               refilled at once. A store row may be admitted once per run (a line restored twice in one call would be two lines)."""

    def __init__(self, model, eos, pad, nop, slots, overall_max_tokens, min_prefill_ratio, on_done=None, on_flush=None, feed=None,
                 alternatives=False, forced=False, beam=None, store=None, fan=False):
        assert store in (None, "keep", "restore"), "store is None, 'keep' or 'restore'"
        assert not (store == "keep" and (fan or beam)), "prompts are kept by plain greedy prefills, not by candidate fans or beam groups"
        self.store, self.store_first = store, []               # per line: the first store row of its prompt
        self.beam = int(beam) if beam else 0
        if self.beam:
            assert 2 <= self.beam <= SA_MAX_BEAMS and slots >= self.beam, "beam width must be 2..4 and fit the slots"
            assert not (alternatives or forced), "beam search excludes per-token alternatives and forced decoding"
            self.model_slots = slots
            slots //= self.beam                                # from here on a "slot" of this loop is a GROUP of `beam` model slots
            self.lane = np.arange(self.beam)
        self.model, self.eos, self.pad, self.nop, self.slots = model, eos, pad, nop, slots
        self.overall_max_tokens, self.min_prefill_ratio = overall_max_tokens, min_prefill_ratio
        self.on_done, self.on_flush, self.feed, self.feed_done = on_done, on_flush, feed, feed is None
        self.steps_per_sync = max(1, min(settings.RECOGNITION_STEPS_PER_SYNC, 8))
        self.max_prefill = model.c.max_prefill_tokens
        self.queue = deque()                                   # ids of the admitted lines that wait for a slot, in id order
        self.grids, self.prompt_ids, self.predicted_tokens, self.scores = [], [], [], []      # per line
        self.chunk_tiles, self.chunk_offs, self.chunk_base = [], [], []      # per admitted dict: its tile tensor, local tile offsets, first id
        self.line_chunk = np.zeros(0, np.int64)                # id -> index into the three lists above
        self.batch_bboxes = np.zeros((0, overall_max_tokens, 6), np.float32)
        # Token bookkeeping in array form: one row per line, written for all active slots of a step at once (the per-token Python
        # loop cost 1.2-1.6 us per token, a third of the device's own time per decode call, and fought the assembly thread for
        # the GIL). slot_line is THE slot table: the line id a slot decodes, -1 for an empty slot.
        self.cap = max(1, overall_max_tokens) + 1
        self.tok_mat = np.zeros((0, self.cap), np.int64)
        self.sc_mat = np.zeros((0, self.cap), np.float32)
        self.line_len, self.max_tok = np.zeros(0, np.int64), np.zeros(0, np.int64)      # tokens so far / token budget per line
        self.slot_line = np.full(slots, -1, np.int64)
        self.alternatives, self.forced = bool(alternatives), bool(forced)
        assert not (self.forced and self.alternatives), "forced decoding and alternatives exclude each other"
        self.extra, self.extra_mats = None, ()                 # the one extra output set of this run (options.EXTRA_SETS) and its matrices
        if self.alternatives or self.forced:
            self._use_extra(options.ALTERNATIVES if self.alternatives else options.FORCED)
        self.forced_ids = []                                   # per line: its forced id list (forced only); with `fan` per candidate row
        self.fan = bool(fan)
        assert not self.fan or self.forced, "candidate fans need forced decoding"
        self.cand_base, self.n_cand, self.cand_left = [], [], []      # fan, per line: its first row, its candidates, those still running
        self.row_line = []                                     # fan, per candidate row: its line
        if self.beam:
            # per group: the beams' token / probability / box histories [groups, beam, cap(, 6)], re-indexed by `parents` every step; their
            # lengths, cumulative scores, finished flags and whether the slot holds a beam at all
            B, cap = self.beam, self.cap
            self.b_tok, self.b_p = np.zeros((slots, B, cap), np.int64), np.zeros((slots, B, cap), np.float32)
            self.b_box = np.zeros((slots, B, cap, 6), np.float32)
            self.b_len, self.b_score = np.zeros((slots, B), np.int64), np.full((slots, B), -np.inf, np.float32)
            self.b_fin, self.b_alive = np.ones((slots, B), bool), np.zeros((slots, B), bool)
        # the per-line options that are ON in this loop (options.LINE_OPTIONS, in table order; `run` fills it): option -> [rows / states
        # of its uploaded table, id -> the line's integer (-1 = off for the line), the call values its slot setter takes]
        self.line_opts = {}
        # Look-ahead encoding (RECOGNITION_ENCODE_AHEAD, default on): the vision encoder of the next up-to-batch-size queued
        # lines runs on the model's second stream while the current lines decode; prefill then only scatters the finished
        # embeddings and runs the decoder over the prompts. Scheduling decisions (which lines, which slots, when) are unchanged.
        self.look_ahead, self.ahead = settings.RECOGNITION_ENCODE_AHEAD, deque()      # ahead: the encoded ids, in id order
        if store == "restore":
            self.look_ahead, self.max_prefill = False, float("inf")      # nothing to encode, nothing to chunk
        self.ahead_cap = max(model.c.max_prefill_tokens, model.c.max_slots)
        self.merge2 = model.cfg.encoder.spatial_merge_size ** 2
        self.inflight, self.ring = None, 0                     # the decode call whose outputs were not read yet: (steps, ring half)

    @property
    def num_active(self) -> int:
        return int(np.count_nonzero(self.slot_line >= 0))

    @property
    def num_empty(self) -> int:
        return self.slots - self.num_active

    def _use_extra(self, xs):
        assert self.extra is None and not self.grids, "one extra output set per loop, chosen before the first line"
        self.extra, self.extra_mats = xs, options.empty_rows(xs, 0, (self.cap,))

    def __getattr__(self, name):
        # (reached for names the instance does not have:) alt_tok_mat ... plain_p_mat, the matrix while its set is on, else None
        xs, i = options.EXTRA_ATTRS.get(name) or (None, 0)
        if xs is None:
            raise AttributeError(name)
        return self.extra_mats[i] if self.__dict__.get("extra") is xs else None

    def admit(self, d):
        """Append the lines of one prepare_lines dict (ids continue the admitted ones)."""
        new = d["prompts"]
        base, m = len(self.grids), len(new)
        if m == 0:
            return
        assert [p.id for p in new] == list(range(base, base + m)), "fed prompts must continue the admitted ids"
        mt = np.asarray([d["max_tokens"][p.id] for p in new], np.int64)
        rows = m                                               # rows of the token matrices the lines take: one each, or one per candidate
        if self.fan:
            cands = [[[int(t) for t in ids] for ids in line] for line in d["forced_ids"]]
            assert len(cands) == m, "forced_ids: one list of candidates per prompt"
            assert all(0 < len(line) <= self.slots and all(line) for line in cands), \
                "a line needs 1..slots candidates, each a non-empty id list"
            assert all(len(ids) <= b for line, b in zip(cands, mt.tolist()) for ids in line), "a candidate exceeds its line's token budget"
            fi = [ids for line in cands for ids in line]
            rows = len(fi)
            for k, line in enumerate(cands):
                self.cand_base.append(len(self.row_line))
                self.row_line.extend([base + k] * len(line))
                self.n_cand.append(len(line)); self.cand_left.append(len(line))
            mt = np.asarray([len(ids) for ids in fi], np.int64)
        elif self.forced:
            fi = [[int(t) for t in ids] for ids in d["forced_ids"]]
            assert len(fi) == m, "forced_ids: one id list per prompt"
            mt = np.asarray([len(ids) or b for ids, b in zip(fi, mt.tolist())], np.int64)      # the budget is the list's length
        assert int(mt.max()) <= self.overall_max_tokens, "a fed line's token budget exceeds the call's overall_max_tokens"
        if self.store:
            first = [int(f) for f in d["store_first"]]
            assert len(first) == m and all(f >= 0 for f in first), "store_first: one store row per prompt"
            assert len(set(first)) == m and set(first).isdisjoint(self.store_first), "a store row is admitted once per run"
            self.store_first.extend(first)
        self.grids.extend(d["grids"])
        self.prompt_ids.extend(d["prompt_ids"])
        self.predicted_tokens.extend([] for _ in range(m))
        self.scores.extend([] for _ in range(m))
        self.chunk_tiles.append(d.get("tiles")); self.chunk_offs.append(d.get("tile_offs")); self.chunk_base.append(base)
        # (restored lines have no tile tensor whose boundary a prefill could not cross: they all count as one chunk)
        self.line_chunk = np.concatenate([self.line_chunk, np.full(m, 0 if self.store == "restore" else len(self.chunk_base) - 1, np.int64)])
        self.batch_bboxes = np.concatenate([self.batch_bboxes, np.zeros((rows, self.overall_max_tokens, 6), np.float32)])
        self.tok_mat = np.concatenate([self.tok_mat, np.zeros((rows, self.cap), np.int64)])
        self.sc_mat = np.concatenate([self.sc_mat, np.zeros((rows, self.cap), np.float32)])
        if self.extra is not None:                             # (rows == m but for fans, which are forced)
            self.extra_mats = tuple(np.concatenate(pair) for pair in zip(self.extra_mats, options.empty_rows(self.extra, rows, (self.cap,))))
        if self.forced:
            self.forced_ids.extend(fi)
        self.line_len = np.concatenate([self.line_len, np.zeros(rows, np.int64)])
        self.max_tok = np.concatenate([self.max_tok, mt])
        for o in options.LINE_OPTIONS:
            vals, on = d.get(o.line_key), self.line_opts.get(o)
            if vals is None and on is None:
                continue                                       # off and not named: nothing to check, nothing to keep
            vals = np.full(m, -1, np.int64) if vals is None else np.asarray(vals, np.int64)
            assert vals.shape == (m,) and int(vals.min()) >= -1 and int(vals.max()) < (on[0] if on else 0), o.admit_msg
            if on:
                on[1] = np.concatenate([on[1], vals])
        self.queue.extend(range(base, base + m))

    def tiles_of(self, first_id, last_id):
        """Tile rows of the consecutive lines first_id..last_id (all of one admitted dict)."""
        c = int(self.line_chunk[first_id])
        assert c == int(self.line_chunk[last_id])
        o, b0 = self.chunk_offs[c], self.chunk_base[c]
        return self.chunk_tiles[c][int(o[first_id - b0]): int(o[last_id - b0 + 1])]

    def poll(self, block):
        """Admit what the feed has ready; with `block`, wait for the next dict (or the end)."""
        got = False
        while not self.feed_done:
            nxt = self.feed(block and not got)
            self.feed_done = nxt is FEED_END
            if nxt is None or self.feed_done:
                break
            self.admit(nxt)
            got = got or bool(nxt["prompts"])

    def _finish_beam(self, p_idx, g):
        """The line of group g is final: its beams as hypotheses, finished ones by score descending, then the unfinished ones."""
        order = sorted(np.flatnonzero(self.b_alive[g]).tolist(), key=lambda b: (not self.b_fin[g, b], -float(self.b_score[g, b]), b))
        hyps = []
        for b in order:
            n = int(self.b_len[g, b])
            hyps.append(BeamHypothesis(self.b_tok[g, b, :n].tolist(), self.b_p[g, b, :n].tolist(),
                                       self.b_box[g, b, :max(min(n, self.overall_max_tokens), 1)].copy(), float(self.b_score[g, b]),
                                       bool(self.b_fin[g, b])))
        if hyps:
            self.predicted_tokens[p_idx], self.scores[p_idx] = hyps[0].tokens, hyps[0].scores
        if self.on_done is not None:
            self.on_done(p_idx, hyps)

    def _beam_step(self, g, p, pos, first, tok, par, prob, logp, boxes):
        """One selection for groups g (lines p, `pos` tokens so far): tok / par / prob / logp [n, beam] as the model reports them per slot,
        boxes [n, beam, 6] the step's box of every slot BEFORE the selection. Histories move with `par`; a live child appends its token,
        its probability and its parent's box; a frozen beam keeps what it has; parent -1 empties the slot. -> the lines that end."""
        B, lane = self.beam, self.lane
        src = np.where(par >= 0, par, lane[None, :])
        if first:
            was_fin = np.zeros(par.shape, bool)
            self.b_len[g] = 0
        else:
            ix = src[:, :, None]
            self.b_tok[g] = np.take_along_axis(self.b_tok[g], ix, 1)
            self.b_p[g] = np.take_along_axis(self.b_p[g], ix, 1)
            self.b_box[g] = np.take_along_axis(self.b_box[g], ix[:, :, :, None], 1)
            self.b_len[g] = np.take_along_axis(self.b_len[g], src, 1)
            was_fin = np.take_along_axis(self.b_fin[g], src, 1)
        alive = par >= 0
        live = alive & ~was_fin
        gi, bi = np.nonzero(live)
        col = pos[gi]
        self.b_tok[g[gi], bi, col] = tok[gi, bi]
        self.b_p[g[gi], bi, col] = prob[gi, bi]
        self.b_box[g[gi], bi, col] = boxes[gi, src[gi, bi]]
        blen = self.b_len[g]
        blen[live] = (pos[:, None] + 1 + np.zeros_like(par))[live]
        self.b_len[g] = blen
        ends = (tok == self.eos) | (tok == self.pad)
        if first:
            ends |= tok == self.nop
        fin = ~alive | was_fin | ends
        self.b_fin[g], self.b_alive[g], self.b_score[g] = fin, alive, logp
        new_len = pos + 1
        self.line_len[p] = new_len
        stop = fin.all(axis=1) | (new_len >= self.max_tok[p])
        # repeat rule (DeviceLoop.absorb's) on the best-ranked live beam: highest score, lower slot on a tie
        for ci in np.flatnonzero(~stop & (new_len >= _REP)).tolist():
            sc = np.where(fin[ci], -np.inf, logp[ci])
            b = int(np.argmax(sc))
            t_ = self.b_tok[g[ci], b, :new_len[ci]]
            if np.unique(t_[-_REP:]).size <= 5 and detect_repeat_token(t_.tolist()):
                stop[ci] = True
        return stop

    def _finish_fan(self, row):
        """Candidate row `row` is final; its line is once all its candidates are."""
        line = self.row_line[row]
        self.cand_left[line] -= 1
        if self.cand_left[line] or self.on_done is None:
            return
        res = []
        for r in range(self.cand_base[line], self.cand_base[line] + self.n_cand[line]):
            n = int(self.line_len[r])
            res.append(tuple(a[r, :n].copy() for a in self.extra_mats))
        self.on_done(line, res)

    def _finish(self, p_idx):
        if self.fan:
            return self._finish_fan(p_idx)
        L_ = int(self.line_len[p_idx])
        self.predicted_tokens[p_idx] = self.tok_mat[p_idx, :L_].tolist()
        self.scores[p_idx] = self.sc_mat[p_idx, :L_].tolist()
        if self.on_done is not None:
            self.on_done(p_idx, self.predicted_tokens[p_idx], self.scores[p_idx],
                         self.batch_bboxes[p_idx, :max(min(L_, self.overall_max_tokens), 1)], *(a[p_idx, :L_].copy() for a in self.extra_mats))

    def _put(self, p, pos, t, s_, b_, more=()):
        """Token t / score s_ / box b_ (/ `more`: the extra set's values, one array per matrix) of lines p at positions pos (arrays over
        the lines of one step)."""
        self.tok_mat[p, pos] = t
        self.sc_mat[p, pos] = s_
        for a, v in zip(self.extra_mats, more):
            a[p, pos] = v
        m = pos < self.overall_max_tokens
        if m.all():
            self.batch_bboxes[p, pos] = b_
        elif m.any():
            self.batch_bboxes[p[m], pos[m]] = b_[m]
        self.line_len[p] = pos + 1

    def _read_extra(self, sl_) -> list:
        """The extra set's values of the prefill's token (it has alternatives / a greedy reading / a plain reading too) for slots sl_."""
        return [a[0, sl_] for a in getattr(self.model, self.extra.read)(1)] if self.extra is not None else ()

    def _flush_active(self):
        """Tell the model which slots still decode (ascending) and let the caller collect the lines that just finished."""
        act = np.flatnonzero(self.slot_line >= 0)
        if self.beam:
            act = (act[:, None] * self.beam + self.lane[None, :]).reshape(-1)       # whole groups, ascending
        self.model.set_active(act.tolist())
        if self.on_flush is not None:
            self.on_flush()

    def absorb(self, call):
        """Host half of one decode call: append its tokens, apply the stop rules (reference :583-595)."""
        k, ring = call
        tok, sc, bb = self.model.wait_outputs(k, ring)
        if self.beam:
            return self._absorb_beam(k, bb, self.model.wait_beam(k, ring))
        ex = getattr(self.model, self.extra.wait)(k, ring) if self.extra is not None else ()
        slot_line, line_len, max_tok, tok_mat, eos, pad = self.slot_line, self.line_len, self.max_tok, self.tok_mat, self.eos, self.pad
        changed = False
        for step in range(k):
            s_idx = np.flatnonzero(slot_line >= 0)
            if s_idx.size == 0:
                break
            p = slot_line[s_idx]
            pos = line_len[p]
            t = tok[step, s_idx]
            self._put(p, pos, t, sc[step, s_idx], bb[step, s_idx], [a[step, s_idx] for a in ex] if ex else ())
            new_len = pos + 1
            stop = (t == eos) | (t == pad) | (new_len >= max_tok[p])
            # repeat rule: <= 5 distinct ids in the last 40 and the last u ids equal to the u before; the distinct count is
            # screened in array form, only the few candidate lines run the exact rule
            c = np.flatnonzero(~stop & (new_len >= _REP))
            if c.size and not self.forced:                          # (a forced text may repeat as it likes)
                win = np.sort(tok_mat[p[c, None], new_len[c, None] + _REP_COLS], axis=1)
                few = c[(np.diff(win, axis=1) != 0).sum(axis=1) + 1 <= 5]
                for ci in few.tolist():
                    if detect_repeat_token(tok_mat[p[ci], :new_len[ci]].tolist()):
                        stop[ci] = True
            if stop.any():
                changed = True
                for ci in np.flatnonzero(stop).tolist():
                    slot_line[int(s_idx[ci])] = -1
                    self._finish(int(p[ci]))
        if changed:
            self._flush_active()

    def _absorb_beam(self, k, bb, out):
        bt, bpar, _, bprob, blogp = out
        changed = False
        for step in range(k):
            g = np.flatnonzero(self.slot_line >= 0)
            if g.size == 0:
                break
            p = self.slot_line[g]
            sl = g[:, None] * self.beam + self.lane[None, :]
            stop = self._beam_step(g, p, self.line_len[p], False, bt[step][sl], bpar[step][sl], bprob[step][sl], blogp[step][sl], bb[step][sl])
            for ci in np.flatnonzero(stop).tolist():
                changed = True
                self.slot_line[int(g[ci])] = -1
                self._finish_beam(int(p[ci]), int(g[ci]))
        if changed:
            self._flush_active()

    def encode_ahead(self):
        """Start the encoder pass of the next queued lines: up to a batch, within the look-ahead capacity, of ONE admitted dict."""
        grids, line_chunk = self.grids, self.line_chunk
        cand, ntok_img = [], 0
        for i in self.queue:
            t = int(grids[i][0]) * int(grids[i][1]) // self.merge2
            if len(cand) >= self.slots or (cand and ntok_img + t > self.ahead_cap):
                break
            if cand and line_chunk[i] != line_chunk[cand[0]]:
                break                                  # one tile tensor per encoder pass: the next admitted dict waits its turn
            cand.append(i)
            ntok_img += t
        self.model.encode_ahead(self.tiles_of(cand[0], cand[-1]), [grids[i] for i in cand])
        self.ahead.extend(cand)

    def _prefill(self, take, grids, prompt_ids, slots):
        """The model's prefill of lines `take` into `slots` (fan: one slot list per line, prefill_shared): from the look-ahead queue, whose
        head they are, or with their own tiles."""
        if self.store == "restore":                    # no tiles, no encoder: the prompts come out of the store
            return self.model.restore([self.store_first[i] for i in take], slots if self.fan else [[s] for s in slots])
        prefill = self.model.prefill_shared if self.fan else self.model.prefill
        if self.store == "keep":
            first = [self.store_first[i] for i in take]
            prefill = lambda tiles, grids_, ids_, slots_: self.model.prefill_keep(tiles, grids_, ids_, slots_, first)
        if self.look_ahead:
            for i in take:
                assert self.ahead.popleft() == i
            prefill(None, grids, prompt_ids, slots)
            if not self.ahead and self.queue:
                self.encode_ahead()                    # the next lines' encoder pass runs beside the decode steps that follow
        else:
            prefill(self.tiles_of(take[0], take[-1]), grids, prompt_ids, slots)      # queue order == id order

    def _prefill_fan(self):
        """prefill_batch with candidate fans: lines from the head of the queue while their candidates fit the empty slots (ascending) and
        their prompts, once each, max_prefill. The caller made sure that the head line fits."""
        queue, ahead, look_ahead, line_chunk = self.queue, self.ahead, self.look_ahead, self.line_chunk
        empty = np.flatnonzero(self.slot_line < 0).tolist()
        if look_ahead and not ahead:
            self.encode_ahead()
        take, fans, ntok, used = [], [], 0, 0
        while queue and (not look_ahead or len(take) < len(ahead)):
            i = queue[0]
            L_, k = len(self.prompt_ids[i]), self.n_cand[i]
            if used + k > len(empty) or (take and (ntok + L_ > self.max_prefill or line_chunk[i] != line_chunk[take[0]])):
                break
            take.append(queue.popleft())
            fans.append(empty[used: used + k])
            ntok += L_
            used += k
        assert take, "the head line's candidates must fit the empty slots"
        rows = np.asarray([self.cand_base[i] + j for i in take for j in range(self.n_cand[i])], np.int64)
        sl_ = np.asarray([s for f in fans for s in f], np.int64)
        self.model.set_forced_tokens(sl_.tolist(), [self.forced_ids[r] for r in rows.tolist()])
        self._prefill(take, [self.grids[i] for i in take], [self.prompt_ids[i] for i in take], fans)
        tok, sc, bb = self.model.read_outputs(1)
        first = tok[0, sl_]
        self._put(rows, np.zeros(len(rows), np.int64), first, sc[0, sl_], bb[0, sl_], self._read_extra(sl_))
        go_on = (first != self.eos) & (first != self.nop) & (self.max_tok[rows] > 1)
        for r, s, go in zip(rows.tolist(), sl_.tolist(), go_on.tolist()):
            if go:
                self.slot_line[s] = r                               # (in fan mode THE slot table names candidate rows)
            else:
                self._finish(r)
        self._flush_active()

    def _fits(self) -> bool:
        """Whether the head of the queue can be prefilled now: always without fans (one empty slot does), else all its candidates fit."""
        return not self.fan or self.n_cand[self.queue[0]] <= self.num_empty

    def prefill_batch(self):
        """Fill the empty slots (ascending) from the head of the queue; a line whose first token already stops never takes its slot."""
        if self.fan:
            return self._prefill_fan()
        queue, ahead, look_ahead, line_chunk = self.queue, self.ahead, self.look_ahead, self.line_chunk
        empty = np.flatnonzero(self.slot_line < 0).tolist()
        if look_ahead and not ahead:
            self.encode_ahead()                        # nothing encoded yet (first batch): the prefill below waits for it
        take, ntok = [], 0
        while queue and len(take) < len(empty) and (not look_ahead or len(take) < len(ahead)):
            L_ = len(self.prompt_ids[queue[0]])
            if take and (ntok + L_ > self.max_prefill or line_chunk[queue[0]] != line_chunk[take[0]]):
                break
            take.append(queue.popleft())
            ntok += L_
        slots = empty[: len(take)]
        grids, prompt_ids = [self.grids[i] for i in take], [self.prompt_ids[i] for i in take]
        if self.beam:
            return self._prefill_beam(take, slots, grids, prompt_ids)
        for o, (_, vals, args) in self.line_opts.items():       # in table order, behind the mask ids; the first token is constrained too
            getattr(self.model, o.set_slot)(slots, vals[take].tolist(), *args)
        if self.forced:
            self.model.set_forced_tokens(slots, [self.forced_ids[i] for i in take])      # the first token is forced too
        self._prefill(take, grids, prompt_ids, slots)
        tok, sc, bb = self.model.read_outputs(1)
        ids_, sl_ = np.asarray(take, np.int64), np.asarray(slots, np.int64)
        first = tok[0, sl_]
        self._put(ids_, np.zeros(len(take), np.int64), first, sc[0, sl_], bb[0, sl_], self._read_extra(sl_))
        go_on = (first != self.eos) & (first != self.nop)
        if self.forced:
            go_on &= self.max_tok[ids_] > 1                         # a one-id list is complete with the prefill's token
        if self.store == "keep":
            go_on[:] = False                                        # the prompt is in the store: that was all
        for p_id, s, go in zip(take, slots, go_on.tolist()):
            if go:                                                  # prefill stop rule (reference :559-563)
                self.slot_line[s] = p_id
            else:
                self._finish(p_id)
        self._flush_active()

    def _prefill_beam(self, take, groups, grids, prompt_ids):
        """prefill_batch in beam mode: a line is prefilled once, into the lead slot of its group; the model's first selection spreads the
        best first tokens over the group. A line's mask id goes to every slot of its group."""
        B = self.beam
        g = np.asarray(groups, np.int64)
        sl = g[:, None] * B + self.lane[None, :]
        if options.MASKS in self.line_opts:                     # (masks only: patterns, lexicons and boosting exclude beam search)
            getattr(self.model, options.MASKS.set_slot)(sl.reshape(-1).tolist(), np.repeat(self.line_opts[options.MASKS][1][take], B).tolist())
        self._prefill(take, grids, prompt_ids, (g * B).tolist())
        _, _, bb = self.model.read_outputs(1)
        bt, bpar, _, bprob, blogp = self.model.read_beam(1)
        p = np.asarray(take, np.int64)
        stop = self._beam_step(g, p, np.zeros(len(take), np.int64), True, bt[0][sl], bpar[0][sl], bprob[0][sl], blogp[0][sl], bb[0][sl])
        for p_id, gg, st in zip(take, groups, stop.tolist()):
            if st:
                self._finish_beam(p_id, gg)
            else:
                self.slot_line[gg] = p_id
        self._flush_active()

    def run(self, prep=None):
        """Admit `prep` (if any) and loop until the queue, the slots and the feed are exhausted."""
        m = self.model
        # the options whose table came with `prep` and names at least one row / state
        on = [(o, prep[o.table_key]) for o in options.requested(prep or {}) if o.count(prep[o.table_key]) > 0]
        running = {k for k in ("beam", "forced", "alternatives") if getattr(self, k)} | {o.name for o, _ in on}
        for o, _ in on:
            assert running.isdisjoint(o.excludes), o.excludes_msg

        def option_on(o, table):
            getattr(m, o.set_table)(table)                 # once per call, behind the tables before it
            self.line_opts[o] = [o.count(table), np.zeros(0, np.int64), tuple(float(prep[k]) for k in o.call_keys)]
            if o.extra is not None:
                self._use_extra(o.extra)
        # (requested, switch on, switch off): switched on in this order, off in reverse on the way out, also after an exception, so the
        # next call starts on the greedy, unmasked kernels without candidates. What was not requested never touches its entry points.
        modes = [(self.beam, lambda: m.set_beam(self.beam, self.nop), lambda: m.set_beam(None)),
                 (self.forced, lambda: m.set_forced(True), lambda: m.set_forced(False)),      # (at most one of the first three: __init__)
                 (self.alternatives, lambda: m.set_alternatives(True), lambda: m.set_alternatives(False))]
        modes += [(True, lambda o=o, t=t: option_on(o, t), lambda o=o: getattr(m, o.set_table)(None)) for o, t in on]
        with ExitStack() as undo:
            for wanted, on, off in modes:
                if wanted:
                    on()
                    undo.callback(off)
            return self._run(prep)

    def _run(self, prep):
        if callable(getattr(self.model, "discard_ahead", None)):
            self.model.discard_ahead()                 # a previous loop that ended early (exception) must not poison this one
        if prep is not None:
            self.admit(prep)
        # The device runs one decode call ahead of the host: call n + 1 is enqueued before call n's tokens are looked at,
        # so the bookkeeping above overlaps with GPU work. A line that stops inside call n rides along in call n + 1
        # (its outputs are dropped: the slot is unmapped by then); new lines are admitted only with nothing in flight.
        while True:
            if not self.feed_done:
                self.poll(block=not (self.queue or self.inflight or self.num_active > 0))
            if not (self.queue or self.inflight or self.num_active > 0):
                if self.feed_done:
                    break
                continue
            if self.queue and self._fits() and ((self.num_empty / self.slots) > self.min_prefill_ratio or
                                                (self.store == "restore" and self.num_empty > 0)):
                if self.inflight:
                    self.absorb(self.inflight)
                    self.inflight = None
                else:
                    self.prefill_batch()
                continue
            # steps some active line can still need once the call in flight is done (token budgets are known up front)
            act = self.slot_line[self.slot_line >= 0]
            budget = (int((self.max_tok[act] - self.line_len[act]).max()) if act.size else 0) - (self.inflight[0] if self.inflight else 0)
            if budget <= 0 and not self.inflight and act.size:
                budget = 1                             # a line admitted with a one-token budget still gets its stop-rule step
            nxt = None
            if budget > 0:
                nxt = (min(self.steps_per_sync, budget), self.ring)
                self.model.decode_async(*nxt)
                self.ring ^= 1
            if self.inflight:
                self.absorb(self.inflight)
            self.inflight = nxt
