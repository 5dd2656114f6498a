"""CPU: constrained output on the host side -- OCRTokenizer.token_mask bits, the merge of identical masks (MaskTable), the predictor's
argument forms (LineConstraints), and the device loop's contract with the model: the table is uploaded once before the first prefill, a
line's mask id is set on the slot it is prefilled into (slot reuse included), and a call without lists never touches the mask entry points.
The model is the fake of tests/test_scheduler_cpu.py, which enforces the C-ABI contracts of the loop."""
from types import SimpleNamespace

import numpy as np
import pytest

from surya_amd.config import rec_config
from surya_amd.recognition.loader import RecognitionModelLoader
from surya_amd.recognition.predictor import LineConstraints
from surya_amd.recognition.tokenizer import MaskTable, OCRTokenizer
from surya_amd.settings import settings

from test_scheduler_cpu import FakeModel, expected, make


def bits_of(mask):
    return np.flatnonzero(np.unpackbits(mask.view(np.uint8), bitorder="little"))


@pytest.fixture(scope="module")
def tok():
    return OCRTokenizer()


def always(tok):
    return {tok.SPECIAL_TOKEN_MAPPING[t] for t in ("</S>", "<PAD>", "<NOP>")}


def test_allowlist_bits_are_the_code_units_and_the_three_control_ids(tok):
    m = tok.token_mask(allow="0123456789.,-")
    assert m.dtype == np.uint32 and m.shape == ((tok.vocab_size + 31) // 32,)
    want = {tok.special_token_offset + ord(c) for c in "0123456789.,-"} | always(tok)
    assert set(bits_of(m).tolist()) == want
    # no formatting or math tag, no math-BPE id
    for tag in ("<b>", "</b>", "<br>", "<math>", "</math>", "<IMAGE>", "<OCR-WB>"):
        assert tok.SPECIAL_TOKEN_MAPPING[tag] not in want
    assert not any(b < tok.qwen_offset for b in want)
    # the ids are the ones the tokenizer itself produces for that text
    assert set(tok("0123456789.,-", "ocr_with_boxes")["input_ids"][0]) <= want
    # bit c & 31 of word c >> 5
    c = tok.special_token_offset + ord("7")
    assert (int(m[c >> 5]) >> (c & 31)) & 1


def test_allowlist_of_a_non_bmp_character_allows_both_surrogates(tok):
    m = set(bits_of(tok.token_mask(allow="\U0001F600")).tolist())          # U+1F600 = D83D DE00
    assert m == {tok.special_token_offset + 0xD83D, tok.special_token_offset + 0xDE00} | always(tok)
    assert set(tok("\U0001F600", "ocr_with_boxes")["input_ids"][0]) <= m


def test_blocklist_allows_everything_else_and_refuses_non_bmp(tok):
    m = tok.token_mask(block="O0")
    b = set(bits_of(m).tolist())
    V = tok.vocab_size
    assert b == set(range(V)) - {tok.special_token_offset + ord("O"), tok.special_token_offset + ord("0")}
    # EOS / pad / no-output cannot be blocked (they are not characters), tags and math ids stay allowed
    assert always(tok) <= b and tok.SPECIAL_TOKEN_MAPPING["<b>"] in b and 5 in b
    with pytest.raises(ValueError):
        tok.token_mask(block="a\U0001F600")
    with pytest.raises(ValueError):
        tok.token_mask()
    with pytest.raises(ValueError):
        tok.token_mask(allow="a", block="b")
    with pytest.raises(TypeError):
        tok.token_mask(allow=["a", "b"])


def test_mask_covers_a_padded_model_vocabulary(tok):
    V = tok.vocab_size + 100                                               # not a multiple of 32 beyond the tokenizer's range
    m = tok.token_mask(block="x", vocab_size=V)
    assert m.shape == ((V + 31) // 32,)
    b = bits_of(m)
    assert b.max() == V - 1 and len(b) == V - 1                            # ids past V stay clear, the padding ids are "everything else"
    small = tok.token_mask(allow="￿", vocab_size=tok.special_token_offset + 100)      # a unit the model cannot emit is dropped
    assert set(bits_of(small).tolist()) == always(tok)


def test_identical_masks_are_stored_once(tok):
    t = MaskTable(tok)
    assert t.id_for(None, None) == -1 and len(t) == 0
    a = t.id_for("0123456789")
    assert t.id_for("9876543210") == a and t.id_for("00112233445566778899") == a      # the same set, written differently
    b = t.id_for(None, "abc")
    assert b != a and t.id_for(None, "cba") == b and t.id_for("0123456789") == a
    assert len(t) == 2 and t.array().shape == (2, (tok.vocab_size + 31) // 32) and t.array().dtype == np.uint32
    assert np.array_equal(t.array()[a], tok.token_mask(allow="0123456789"))
    with pytest.raises(ValueError):
        t.id_for("a", "b")
    lim = MaskTable(tok, limit=2)
    lim.id_for("a"), lim.id_for("b"), lim.id_for("a")
    with pytest.raises(ValueError):
        lim.id_for("c")


def test_argument_forms(tok):
    # one str for the whole call
    c = LineConstraints(tok, "01", None, 3, [2, 0, 1])
    assert c.per_image == [0, 0, 0] and c.line_ids([2, 0, 1]) == [0, 0, 0] and len(c.table) == 1
    # per image: None / str / per line; a blocklist beside it where the allowlist is None
    c = LineConstraints(tok, [None, "01", ["ab", None, "10"]], [None, None, [None, "x", None]], 3, [1, 2, 3])
    assert c.per_image[0] == -1 and c.per_image[1] == 0
    assert c.per_image[2] == [1, 2, 0]                                    # "10" is the set "01"
    assert c.line_ids([1, 2, 3]) == [-1, 0, 0, 1, 2, 0]
    # all None: no table at all
    assert not LineConstraints(tok, [None, None], None, 2, [1, 1])
    # the detector paths know no line counts: per call and per image work, per line raises
    assert LineConstraints(tok, ["01", None], None, 2, None).line_ids([4, 2]) == [0, 0, 0, 0, -1, -1]
    with pytest.raises(ValueError, match="not known yet"):
        LineConstraints(tok, [["01"], None], None, 2, None)
    with pytest.raises(ValueError):
        LineConstraints(tok, "01", "23", 1, [1])                          # both for one line
    with pytest.raises(ValueError):
        LineConstraints(tok, [["01", None]], [[None, "2"], ], 1, [3])     # per-line list of the wrong length
    with pytest.raises(ValueError):
        LineConstraints(tok, ["01"], None, 2, [1, 1])                     # one entry per image
    with pytest.raises(TypeError):
        LineConstraints(tok, 5, None, 1, [1])
    with pytest.raises(TypeError):
        LineConstraints(tok, [[5]], None, 1, [1])


def test_predictor_call_validates_before_any_device_work():
    """The keywords sit after the reference's own arguments; malformed lists raise before a line is sliced or a kernel launched."""
    import inspect
    from PIL import Image
    from surya_amd.recognition.predictor import RecognitionPredictor
    params = list(inspect.signature(RecognitionPredictor.__call__).parameters)
    assert params[-2:] == ["allowlist", "blocklist"] and params.index("drop_repeated_text") == len(params) - 3
    pred = object.__new__(RecognitionPredictor)
    pred.processor = RecognitionModelLoader({"config": rec_config("REC-TINY"), "state_dict": {}}).processor()
    pred.model = None
    img = Image.new("RGB", (64, 32))
    with pytest.raises(ValueError, match="not known yet"):
        pred([img], det_predictor=object(), allowlist=[["01"]])
    with pytest.raises(ValueError):
        pred([img], bboxes=[[[0, 0, 10, 10]]], allowlist="01", blocklist="2")
    with pytest.raises(ValueError):
        pred([img], bboxes=[[[0, 0, 10, 10]]], allowlist=[["01", "23"]])


class MaskFakeModel(FakeModel):
    """The scheduler test's fake plus the mask entry points, with their contracts: one table per loop, uploaded before the first prefill
    and switched off at the end; slot ids only for slots that are free, naming rows of the table, set before the prefill that uses them."""

    def __init__(self, max_slots):
        super().__init__(max_slots)
        self.tables, self.slot_mask, self.line_mask_seen, self.pending = [], {}, {}, {}

    def set_token_masks(self, masks):
        assert not self.inflight and self.prefill_out is None
        self.tables.append(None if masks is None else np.array(masks))
        self.slot_mask = {}                                     # a new table sets every slot back to unconstrained

    def set_slot_masks(self, slots, ids):
        assert self.tables and self.tables[-1] is not None, "SA_ERR_STATE: slot ids without a table"
        assert not self.inflight and len(slots) == len(ids)
        for s, i in zip(slots, ids):
            assert s not in self.active and -1 <= i < len(self.tables[-1])
            self.slot_mask[s] = i
            self.pending[s] = True

    def prefill(self, tiles, grid_hw, input_ids, slot_ids):
        if self.tables and self.tables[-1] is not None:
            for s in slot_ids:
                assert self.pending.pop(s, False), "a slot was prefilled without its mask id being set first"
        super().prefill(tiles, grid_hw, input_ids, slot_ids)
        for ids, s in zip(input_ids, slot_ids):
            self.line_mask_seen[ids[0] - 1000] = self.slot_mask.get(s, -1)


@pytest.mark.parametrize("n_lines,max_tokens,slots,sps,ahead", [(23, 12, 4, 4, True), (40, 6, 7, 1, False), (30, 20, 8, 4, True)])
def test_mask_ids_reach_the_slots_and_survive_slot_reuse(n_lines, max_tokens, slots, sps, ahead):
    old = (settings.RECOGNITION_STEPS_PER_SYNC, settings.RECOGNITION_ENCODE_AHEAD)
    settings.RECOGNITION_STEPS_PER_SYNC, settings.RECOGNITION_ENCODE_AHEAD = sps, ahead
    try:
        pred, prep = make(n_lines, max_tokens, slots)
        pred.model = MaskFakeModel(slots)
        table = np.arange(3 * 5, dtype=np.uint32).reshape(3, 5) + 1
        want = [(i % 4) - 1 for i in range(n_lines)]           # -1, 0, 1, 2: unconstrained lines take over slots of masked ones and back
        prep.update(token_masks=table, mask_ids=want)
        toks, _, _ = pred.generate(prep, slots)
    finally:
        settings.RECOGNITION_STEPS_PER_SYNC, settings.RECOGNITION_ENCODE_AHEAD = old
    m = pred.model
    assert len(m.tables) == 2 and np.array_equal(m.tables[0], table) and m.tables[1] is None      # uploaded once, switched off at the end
    assert [m.line_mask_seen[i] for i in range(n_lines)] == want
    assert n_lines > slots                                      # slots were reused
    for i in range(n_lines):
        assert toks[i] == expected(i, prep["max_tokens"][i])    # scheduling is what it was


def test_fed_chunks_carry_their_mask_ids():
    from surya_amd.recognition.loop import FEED_END
    from test_scheduler_cpu import _chunks
    pred, prep = make(20, 8, 4)
    pred.model = MaskFakeModel(4)
    want = [(i % 3) - 1 for i in range(20)]
    chunks = _chunks(prep, [0, 7, 12, 20])
    for ch in chunks:
        ch["mask_ids"] = [want[p.id] for p in ch["prompts"]]
    feed_items = chunks + [FEED_END]
    first = {"prompts": [], "max_tokens": {}, "overall_max_tokens": 8, "token_masks": np.ones((2, 4), np.uint32)}
    pred.generate(first, 4, feed=lambda block: feed_items.pop(0))
    assert [pred.model.line_mask_seen[i] for i in range(20)] == want
    assert len(pred.model.tables) == 2 and pred.model.tables[1] is None


def test_a_call_without_lists_never_touches_the_mask_entry_points():
    pred, prep = make(12, 6, 4)                                # the plain FakeModel has neither set_token_masks nor set_slot_masks
    toks, _, _ = pred.generate(prep, 4)
    assert all(toks[i] == expected(i, prep["max_tokens"][i]) for i in range(12))
    pred, prep = make(5, 6, 4)
    prep["mask_ids"] = [0, -1, 0, -1, 0]                       # ids without a table are a caller's bug
    with pytest.raises(AssertionError):
        pred.generate(prep, 4)


def test_a_failed_loop_still_switches_the_masks_off():
    pred, prep = make(6, 6, 4)
    pred.model = MaskFakeModel(4)

    def boom(n, ring):
        raise RuntimeError("device lost")
    pred.model.decode_async = boom
    prep.update(token_masks=np.ones((1, 4), np.uint32), mask_ids=[0] * 6)
    with pytest.raises(RuntimeError):
        pred.generate(prep, 4)
    assert pred.model.tables[-1] is None


@pytest.mark.parametrize("rank", [0, 1])
def test_shard_lines_deals_the_mask_ids_with_the_lines(monkeypatch, rank):
    """sharded_prediction_loop with two (faked) ranks: the rank's own loop sees the whole table and the ids of exactly its lines."""
    import torch
    from surya_amd import dist as sdist
    from surya_amd.recognition.predictor import RecognitionPredictor
    n, world = 7, 2
    monkeypatch.setattr(sdist, "collectives_on", lambda group=None: True)
    monkeypatch.setattr(sdist, "world_info", lambda group=None: (rank, world))
    monkeypatch.setattr(sdist, "collective_device", lambda dev, group=None: "cpu")
    monkeypatch.setattr(sdist, "assert_same_inputs", lambda *a, **k: None)
    monkeypatch.setattr(sdist, "gather_line_outputs", lambda toks, scores, boxes, mine, n_total, max_tokens, **k: (toks, scores, boxes))
    pred = object.__new__(RecognitionPredictor)
    pred.model = SimpleNamespace(device="cpu")
    pred.process_group = None
    seen = {}

    def loop(local, rbs, math_mode):
        seen.update(local)
        m = len(local["slices"])
        return [[5]] * m, torch.zeros((m, 6, 6)), [[0.5]] * m
    pred.prediction_loop = loop
    table = np.arange(2 * 3, dtype=np.uint32).reshape(2, 3) + 1
    ids = [(i % 3) - 1 for i in range(n)]
    flat = {"slices": [np.zeros((4, 10 + i, 3), np.float32) for i in range(n)], "input_text": [None] * n, "task_names": ["ocr_with_boxes"] * n,
            "token_masks": table, "mask_ids": ids}
    pred.sharded_prediction_loop(flat, 4, True)
    mine = list(range(rank, n, world))
    assert seen["mask_ids"] == [ids[i] for i in mine] and seen["token_masks"] is table
    assert [s.shape[1] for s in seen["slices"]] == [10 + i for i in mine]
    # a call without lists hands its rank's loop no mask keys at all
    seen.clear()
    del flat["token_masks"], flat["mask_ids"]
    pred.sharded_prediction_loop(flat, 4, True)
    assert "mask_ids" not in seen and "token_masks" not in seen


def test_page_sharded_call_slices_per_image_lists(monkeypatch):
    """_call_page_sharded: rank r of 2 runs the single-rank call on pages r, r + 2, ... with THEIR entries of a per-image list (a str is
    every page's entry); without lists the rank's call is reached positionally, as before."""
    from PIL import Image
    from surya_amd import dist as sdist
    from surya_amd.recognition.predictor import RecognitionPredictor
    from surya_amd.recognition.schema import OCRResult
    monkeypatch.setattr(sdist, "world_info", lambda group=None: (1, 2))
    monkeypatch.setattr(sdist, "collective_device", lambda dev, group=None: "cpu")
    monkeypatch.setattr(sdist, "assert_same_inputs", lambda *a, **k: None)
    monkeypatch.setattr(sdist, "gather_objects", lambda local, mine, n, group=None: list(local))
    pred = object.__new__(RecognitionPredictor)
    pred.model = SimpleNamespace(device="cpu")
    pred.process_group, pred.shard_pages, pred.shard_lines = None, True, False
    got = {}

    def rank_call(images, *a, **kw):
        got["n"], got["kw"] = len(images), kw
        return [OCRResult(text_lines=[], image_bbox=[0, 0, 1, 1]) for _ in images]
    pred._call = rank_call
    pages = [Image.new("RGB", (8 + i, 8)) for i in range(5)]
    args = (pages, ["ocr_with_boxes"] * 5, SimpleNamespace(), None, None, [None] * 5, False, True, False, False)
    pred._call_page_sharded(*args, allowlist=["a", None, "c", "d", None], blocklist=None)
    assert got["n"] == 2 and got["kw"] == {"allowlist": [None, "d"], "blocklist": [None, None]}
    pred._call_page_sharded(*args, allowlist=None, blocklist="xy")
    assert got["kw"] == {"allowlist": [None, None], "blocklist": ["xy", "xy"]}
    pred._call_page_sharded(*args)
    assert got["kw"] == {}
