"""CPU: every per-line decoding option of recognition/options.py (LINE_OPTIONS) carries ONE set of lines unchanged through every stage
of the call path -- the flat dict after the width sort, the rank's share in sharded_prediction_loop, prepare_lines' dict, a streamed
chunk, DeviceLoop.admit and the set_slot_* call of the prefilled slots -- on a fake model built from the option table itself, so a
fifth option is covered the day its descriptor exists. 5 lines on 2 pages, 4 slots, a token budget of 3: the smallest case with a slot
reused and a line left waiting in the queue."""
from types import SimpleNamespace

import numpy as np
import pytest

from surya_amd.recognition import options
from surya_amd.recognition import predictor as P
from surya_amd.recognition.loop import DeviceLoop
from surya_amd.recognition.options import EXTRA_SETS, LINE_OPTIONS
from surya_amd.settings import settings
from test_scheduler_cpu import EOS, NOP, PAD, StreamFakeModel, _fake_detector

SLOTS, BUDGET, N_STATES = 4, 3, 7
# two pages of 3 + 2 lines; the widths make the width sort a real permutation (sorted position k = original line ORDER[k])
WIDTHS = [[20, 50, 30], [60, 10]]
POLYS = [[[[2, 10 + 20 * k], [2 + w, 10 + 20 * k], [2 + w, 19 + 20 * k], [2, 19 + 20 * k]] for k, w in enumerate(page)] for page in WIDTHS]
LINE_OF = {tuple(tuple(pt) for pt in pl): i for i, pl in enumerate(pl for page in POLYS for pl in page)}      # polygon -> original line
ORDER = [3, 1, 2, 0, 4]
VALUES = [2, -1, 5, 0, 3]                                      # the option's integer per original line: states of the table, and "off"
KEY = lambda line: 2 + 10 * line                               # the fake model's stream key: one that runs to the token budget


class OptionFakeModel(StreamFakeModel):
    """The scheduler fake plus the entry points the option table names, recorded: `events` the table calls in order, `slot_calls` the
    slot setters' names per prefill, `seen[option name][line]` the value on the slot a line was prefilled into. A slot value must
    have been set for THIS prefill; the extra sets' read / wait calls answer zeros of their fields' shapes."""

    def __init__(self, max_slots):
        super().__init__(max_slots)
        self.events, self.tables, self.slot_val, self.slot_calls, self.seen, self.slot_lines, self.call_args = [], {}, {}, [[]], {}, {}, {}

    def __getattr__(self, name):
        for o in LINE_OPTIONS:
            if name == o.set_table:
                return lambda table, o=o: self._table(o, table)
            if name == o.set_slot:
                return lambda slots, vals, *args, o=o: self._slots(o, slots, vals, args)
        for xs in EXTRA_SETS:
            if name in (xs.read, xs.wait):
                return lambda n, ring=0, xs=xs: tuple(np.zeros((n, self.max_slots) + f.tail, f.dtype) for f in xs.fields)
        raise AttributeError(name)

    def _table(self, o, table):
        assert not self.inflight and self.prefill_out is None
        self.events.append((o.name, table is not None))
        if table is not None:
            self.tables[o.name] = table

    def _slots(self, o, slots, vals, args):
        assert self.events and (o.name, True) in self.events and (o.name, False) not in self.events, "slot values while the option is off"
        assert not self.inflight and len(slots) == len(vals) == len(set(slots))
        self.slot_calls[-1].append(o.name)
        self.call_args[o.name] = args
        for s, v in zip(slots, vals):
            assert s not in self.active and -1 <= v < N_STATES
            self.slot_val[(o.name, s)] = v

    def prefill(self, tiles, grid_hw, input_ids, slot_ids):
        super().prefill(tiles, grid_hw, input_ids, slot_ids)
        for ids, s in zip(input_ids, slot_ids):
            line = (ids[0] - 1000 - 2) // 10
            self.slot_lines.setdefault(s, []).append(line)
            for name in self.slot_calls[-1]:
                self.seen.setdefault(name, {})[line] = self.slot_val.pop((name, s))      # KeyError: prefilled without its value
        self.slot_calls.append([])


class FakeMaskTable:
    def __init__(self, rows):
        self.arr = np.ones((rows, 4), np.uint32)

    def __len__(self):
        return len(self.arr)

    def array(self):
        return self.arr


def make_cons(on):
    """A LineConstraints with the options `on` requested, each with VALUES in per-line form, every other one off (masks: an empty
    table, which a real call's constraints never have -- it is how a test gets an option without the mask table beside it)."""
    cons = object.__new__(P.LineConstraints)
    tables = {}
    for o in LINE_OPTIONS:
        is_on = o in on
        table = (FakeMaskTable(N_STATES if is_on else 0) if o is options.MASKS else SimpleNamespace(n_states=N_STATES) if is_on else None)
        setattr(cons, o.cons_table, table)
        setattr(cons, o.cons_per_image, [VALUES[:3], VALUES[3:]] if is_on else [-1, -1] if o is options.MASKS else None)
        for k in o.call_keys:
            setattr(cons, k, 2.5)
        if is_on:
            tables[o.name] = table.arr if o is options.MASKS else table
    return cons, tables


class Recorder:
    """A predictor on fakes whose stages are wrapped: `flats` what prepare_lines was handed, `preps` what it returned, `admitted` the
    dicts DeviceLoop.admit took, `loops` the loops, `asm_flats` the flat dicts assembly read."""

    def __init__(self, monkeypatch, cons):
        self.flats, self.preps, self.admitted, self.loops, self.asm_flats = [], [], [], [], []
        rec = self

        class Loop(DeviceLoop):
            def __init__(self, *a, **kw):
                super().__init__(*a, **kw)
                rec.loops.append(self)

            def admit(self, d):
                rec.admitted.append(d)
                super().admit(d)
        monkeypatch.setattr(P, "DeviceLoop", Loop)
        from surya_amd.recognition.schema import TextLine
        pred = self.pred = object.__new__(P.RecognitionPredictor)
        pred.model = OptionFakeModel(SLOTS)
        pred.processor = SimpleNamespace(eos_token_id=EOS, pad_token_id=PAD, no_output_token=NOP)
        pred.last_timing, pred.process_group, pred.shard_lines, pred.device_preprocess = {}, None, False, True
        pred._constraints = lambda *a, **k: cons

        def preprocess(prompts, pages):
            keys = [KEY(LINE_OF[p.image.poly]) for p in prompts]
            offs = np.arange(len(prompts) + 1) * 4
            tiles = np.repeat(np.asarray(keys, np.float32), 4)[:, None] * np.ones((1, 3), np.float32)
            return tiles, offs, [(2, 2)] * len(prompts), [[1000 + k, 5, 6] for k in keys]

        def assemble_batch(flat, items, *a):
            rec.asm_flats.append(flat)
            return [TextLine(text="", polygon=flat["polygons"][it[1]], confidence=1.0, chars=[]) for it in items]

        real_prepare = pred.prepare_lines

        def prepare_lines(flat, math_mode=True):
            rec.flats.append(flat)
            rec.preps.append(real_prepare(flat, math_mode))
            return rec.preps[-1]
        pred.preprocess_prompts_device, pred._assemble_batch, pred.prepare_lines = preprocess, assemble_batch, prepare_lines

    def lines_of(self, d):
        """The original line of every prompt of a prepared dict, in the dict's order."""
        return [LINE_OF[p.image.poly] for p in d["prompts"]]


@pytest.fixture
def small(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    old = (settings.RECOGNITION_STEPS_PER_SYNC, settings.RECOGNITION_ENCODE_AHEAD, settings.RECOGNITION_MAX_TOKENS)
    settings.RECOGNITION_STEPS_PER_SYNC, settings.RECOGNITION_ENCODE_AHEAD, settings.RECOGNITION_MAX_TOKENS = 2, True, BUDGET
    yield
    settings.RECOGNITION_STEPS_PER_SYNC, settings.RECOGNITION_ENCODE_AHEAD, settings.RECOGNITION_MAX_TOKENS = old


def call_values(on) -> dict:
    """What a call passes beside the lists for the options `on` (boost's weight), as _call's keywords."""
    return {k: 2.5 for o in on for k in o.call_keys}


def pages():
    from PIL import Image
    return [Image.new("RGB", (80, 80)) for _ in POLYS], [P.TaskNames.ocr_with_boxes] * len(POLYS)


def check_device_side(rec, o, tables, lines):
    """What the loop and the model saw of option `o` for `lines` (original lines, in line id order): admit kept the values in line
    order, every line's value reached the slot the line was prefilled into, the table is the one handed in, no other option's entry
    point was touched, a slot was reused and a line waited."""
    m, loop = rec.pred.model, rec.loops[-1]
    assert list(loop.line_opts) == [o] and loop.line_opts[o][0] == N_STATES
    assert loop.line_opts[o][1].tolist() == [VALUES[i] for i in lines]
    assert m.seen == {o.name: {i: VALUES[i] for i in lines}}
    assert m.events == [(o.name, True), (o.name, False)] and m.tables[o.name] is tables[o.name]
    assert all(calls in ([o.name], []) for calls in m.slot_calls)
    assert m.call_args[o.name] == tuple(2.5 for _ in o.call_keys)
    if len(lines) > SLOTS:
        assert max(len(v) for v in m.slot_lines.values()) > 1 and len(m.slot_lines) == SLOTS      # a slot reused, after a line waited


@pytest.mark.usefixtures("small")
@pytest.mark.parametrize("o", LINE_OPTIONS, ids=lambda o: o.name)
def test_one_set_of_lines_through_the_serial_call(monkeypatch, o):
    """_call with polygons: flat after the width sort, prepare_lines' dict, admit, the slot setters."""
    cons, tables = make_cons([o])
    rec = Recorder(monkeypatch, cons)
    images, tasks = pages()
    res = rec.pred._call(images, tasks, None, None, SLOTS, None, None, POLYS, None, False, True, False, False, **call_values([o]))
    assert [len(r.text_lines) for r in res] == [3, 2]
    flat, prep = rec.flats[0], rec.preps[0]
    assert rec.lines_of(prep) == ORDER
    for d in (flat, prep, rec.admitted[0]):
        assert d[o.line_key] == [VALUES[i] for i in ORDER] and all(k not in d for p in LINE_OPTIONS if p not in (o, options.MASKS) for k in (p.table_key, p.line_key))
    for d in (flat, prep):
        assert d[o.table_key] is tables[o.name] and all(d[k] == 2.5 for k in o.call_keys)
    assert flat[options.MASKS.line_key] == [-1] * 5 or o is options.MASKS      # a call with constraints always carries the mask keys
    check_device_side(rec, o, tables, ORDER)


@pytest.mark.usefixtures("small")
@pytest.mark.parametrize("rank", [0, 1])
@pytest.mark.parametrize("o", LINE_OPTIONS, ids=lambda o: o.name)
def test_one_set_of_lines_through_the_ranks_share(monkeypatch, o, rank):
    """sharded_prediction_loop on rank `rank` of 2: the rank's prepare_lines, loop and slots see the whole table and its own lines."""
    from surya_amd import dist as sdist
    monkeypatch.setattr(sdist, "collectives_on", lambda group=None: True)
    monkeypatch.setattr(sdist, "world_info", lambda group=None: (rank, 2))
    monkeypatch.setattr(sdist, "collective_device", lambda dev, group=None: "cpu")
    monkeypatch.setattr(sdist, "assert_same_inputs", lambda *a, **k: None)
    monkeypatch.setattr(sdist, "gather_line_outputs", lambda toks, scores, boxes, mine, n_total, max_tokens, **k: (toks, scores, boxes))
    cons, tables = make_cons([o])
    rec = Recorder(monkeypatch, cons)
    images, tasks = pages()
    flat = rec.pred.slice_bboxes(images, tasks, polygons=POLYS)
    keys = ("slices", "input_text", "task_names") + options.attach(flat, cons)
    for k in keys:
        flat[k] = [flat[k][i] for i in ORDER]
    rec.pred.sharded_prediction_loop(flat, SLOTS, True)
    mine = ORDER[rank::2]
    local, prep = rec.flats[0], rec.preps[0]
    assert rec.lines_of(prep) == mine
    for d in (local, prep, rec.admitted[0]):
        assert d[o.line_key] == [VALUES[i] for i in mine]
    assert local[o.table_key] is tables[o.name] and prep[o.table_key] is tables[o.name] and all(prep[k] == 2.5 for k in o.call_keys)
    check_device_side(rec, o, tables, mine)


@pytest.mark.usefixtures("small")
@pytest.mark.parametrize("o", LINE_OPTIONS, ids=lambda o: o.name)
def test_one_set_of_lines_through_a_streamed_chunk(monkeypatch, o):
    """_call_streamed, one detector batch of both pages: the first dict carries the table, the chunk the lines' values in chunk (width)
    order, and flat -- which the assembly thread reads -- holds them before the chunk is admitted."""
    cons, tables = make_cons([o])
    rec = Recorder(monkeypatch, cons)
    images, tasks = pages()
    at_admit = []
    real_feed_admit = DeviceLoop.admit

    def admit(self, d):
        if d["prompts"]:
            at_admit.append(list(rec.asm_flat_now[o.line_key]))
        real_feed_admit(self, d)
    monkeypatch.setattr(DeviceLoop, "admit", admit)
    real_attach = options.attach

    def attach(flat, c):
        rec.asm_flat_now = flat
        return real_attach(flat, c)
    monkeypatch.setattr(options, "attach", attach)
    res = rec.pred._call_streamed(images, tasks, _fake_detector(POLYS, 2), None, SLOTS, [None, None], False, True, False, False, {}, 0.0,
                                  cons=cons)
    assert [len(r.text_lines) for r in res] == [3, 2]
    first, chunk = rec.admitted[0], rec.admitted[1]
    assert first["prompts"] == [] and first[o.table_key] is tables[o.name] and all(first[k] == 2.5 for k in o.call_keys)
    assert o.line_key not in first and rec.lines_of(chunk) == ORDER
    assert chunk[o.line_key] == [VALUES[i] for i in ORDER] == at_admit[0]
    assert all(f is rec.asm_flat_now and f[o.table_key] is tables[o.name] for f in rec.asm_flats)
    check_device_side(rec, o, tables, ORDER)


@pytest.mark.usefixtures("small")
def test_options_switch_on_in_table_order_and_off_in_reverse(monkeypatch):
    """masks + patterns + lexicon in one run: tables uploaded in table order, slot values set in table order before every prefill,
    switched off in reverse -- also when the loop dies."""
    three = list(LINE_OPTIONS[:3])
    cons, tables = make_cons(three)
    rec = Recorder(monkeypatch, cons)
    images, tasks = pages()
    rec.pred._call(images, tasks, None, None, SLOTS, None, None, POLYS, None, False, True, False, False, **call_values(three))
    m = rec.pred.model
    names = [o.name for o in three]
    assert m.events == [(n, True) for n in names] + [(n, False) for n in reversed(names)]
    assert [c for c in m.slot_calls if c] == [names] * 2 and m.slot_calls[-1] == []      # two prefills: 4 lines, then the one that waited
    assert m.seen == {n: dict(enumerate(VALUES)) for n in names}
    m.events.clear()

    def boom(n, ring):
        raise RuntimeError("device lost")
    m.decode_async = boom
    with pytest.raises(RuntimeError, match="device lost"):
        rec.pred._call(images, tasks, None, None, SLOTS, None, None, POLYS, None, False, True, False, False, **call_values(three))
    assert m.events == [(n, True) for n in names] + [(n, False) for n in reversed(names)]
