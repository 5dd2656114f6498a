"""GPU: constrained output through the recognition engine (surya_rec_set_token_masks / surya_rec_set_slot_masks) and through
RecognitionPredictor(allowlist=, blocklist=), on REC-SMALL (vocabulary 69 632: the 256 x 320 lm_head tile with a partial last tile).

The reference for a token and its score is the engine's own UNMASKED logits of that step (surya_rec_copy_last_logits recomputes them with
the plain-bias epilogue of the same GEMM), masked in torch: first argmax and max softmax of logits.masked_fill(~allowed, -inf), which is
what the reference's process_outputs computes on masked next_token_logits. Tokens must be equal, scores within the rtol = 2e-3 of
test_full_vocab_fused_argmax_equals_recomputed_logits. Rows whose slot is unconstrained must be BIT-identical to a run of an engine
that never saw a mask table.
"""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch
from PIL import Image

from surya_amd import _lib as L
from surya_amd.config import rec_config
from surya_amd.settings import settings
from surya_amd.synth import make_line_crops, make_rec_weights

from util import make_prompts

pytestmark = pytest.mark.gpu
DIGITS = "0123456789.,-"
VOWELS = "aeiouAEIOU 0"
N_LINES = 6
GRIDS = [(2, 2 + 2 * (i % 5)) for i in range(N_LINES)]


@functools.lru_cache(maxsize=None)
def _cfg_sd(name="REC-SMALL"):
    cfg = rec_config(name)
    return cfg, make_rec_weights(cfg, 0)


@functools.lru_cache(maxsize=None)
def _tokenizer(name="REC-SMALL"):
    from surya_amd.recognition.loader import RecognitionModelLoader
    return RecognitionModelLoader({"config": _cfg_sd(name)[0], "state_dict": {}}).processor().ocr_tokenizer


def _model(dtype, max_slots=8, **kw):
    from surya_amd.recognition.model import HipRecModel
    cfg, sd = _cfg_sd()
    return HipRecModel(cfg, sd, image_token_id=cfg.image_token_id, pad_token_id=cfg.pad_token_id, eos_token_id=cfg.eos_token_id, dtype=dtype,
                       max_slots=max_slots, max_kv_len=64, max_patches=max(4096, max_slots * 48), max_prefill_tokens=max(1024, max_slots * 16), **kw)


def _table():
    tk, V = _tokenizer(), _cfg_sd()[0].decoder.vocab_size
    return np.stack([tk.token_mask(allow=DIGITS, vocab_size=V), tk.token_mask(block=VOWELS, vocab_size=V)])


def _allowed_rows(table, ids, V):
    """bool [len(ids), V] on the GPU: the allowed set of every row (-1 = everything)."""
    bits = np.unpackbits(np.ascontiguousarray(table).view(np.uint8), axis=1, bitorder="little")[:, :V].astype(bool)
    rows = np.ones((len(ids), V), bool)
    for r, i in enumerate(ids):
        if i >= 0:
            rows[r] = bits[i]
    return torch.from_numpy(rows).cuda()


def _check_step(m, cfg, tok, score, slots, allowed, what):
    """tok / score [max_slots] of one step against the masked recomputation from that step's unmasked logits (row r = slots[r])."""
    lg = m.last_logits()
    assert lg.shape == (len(slots), cfg.decoder.vocab_size)
    ml = lg.double().masked_fill(~allowed, float("-inf"))
    best = ml.max(1, keepdim=True).values
    cols = torch.arange(ml.shape[1], device=ml.device).expand_as(ml)
    ref_tok = torch.where(ml == best, cols, torch.full_like(cols, 2 ** 31 - 1)).min(1).values.cpu().numpy()
    ref_score = (1.0 / torch.exp(ml - best).sum(1)).cpu().numpy()
    got_tok, got_score = np.asarray(tok)[slots], np.asarray(score)[slots]
    assert np.array_equal(got_tok, ref_tok), (what, got_tok.tolist(), ref_tok.tolist())
    assert allowed[torch.arange(len(slots)), torch.from_numpy(got_tok).long()].all(), (what, "an id outside the allowed set")
    live = ~np.isin(ref_tok, [cfg.eos_token_id, cfg.pad_token_id])              # finished rows report score 0
    rel = np.abs(got_score[live] - ref_score[live]) / ref_score[live]
    print(f"{what}: max relative score error {rel.max() if rel.size else 0.0:.3e}")
    assert (rel <= 2e-3).all(), (what, rel.max())
    assert (got_score[~live] == 0).all()


@functools.lru_cache(maxsize=None)
def _line(i):
    """Tiles and prompt of line i: a function of i alone, whatever other lines a run holds."""
    tiles, seqs = make_prompts(_cfg_sd()[0], [GRIDS[i % N_LINES]], seed=100 + i)
    return tiles, seqs[0]


def _run(m, slots, steps, single=False, lines=None):
    """Prefill lines (default: line i into slots[i]) and decode `steps` steps; (tokens, scores, boxes) [1 + steps, len(slots)(, 6)]."""
    lines = list(range(len(slots))) if lines is None else lines
    tiles, seqs = torch.cat([_line(i)[0] for i in lines]), [_line(i)[1] for i in lines]
    m.prefill(tiles.cuda(), [GRIDS[i % N_LINES] for i in lines], seqs, slots)
    t, s, b = m.read_outputs(1)
    out = [(t[0, slots].copy(), s[0, slots].copy(), b[0, slots].copy())]
    m.set_active(sorted(slots))
    if single:
        for _ in range(steps):
            m.decode(1)
            t, s, b = m.read_outputs(1)
            out.append((t[0, slots].copy(), s[0, slots].copy(), b[0, slots].copy()))
    elif steps:
        m.decode(steps)
        t, s, b = m.read_outputs(steps)
        out += [(t[k, slots].copy(), s[k, slots].copy(), b[k, slots].copy()) for k in range(steps)]
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_every_step_equals_the_masked_recomputation(hip_lib, dtype):
    """decode(1) at a time: after the prefill (the first token is constrained too) and after each of 6 steps, token and score of every
    slot -- digits, blocklist, unconstrained -- equal the recomputation, and every emitted id is in its slot's set."""
    cfg = _cfg_sd()[0]
    m = _model(dtype)
    table = _table()
    slots, ids = [0, 1, 2, 3, 4, 5], [0, 1, -1, 0, 1, -1]
    allowed = _allowed_rows(table, ids, cfg.decoder.vocab_size)
    m.set_token_masks(table)
    m.set_slot_masks(slots, ids)
    tiles, seqs = make_prompts(cfg, GRIDS, seed=9)
    m.prefill(tiles.cuda(), GRIDS, seqs, slots)
    t, s, _ = m.read_outputs(1)
    _check_step(m, cfg, t[0], s[0], slots, allowed, f"{dtype} prefill")
    m.set_active(slots)
    seen = [set() for _ in slots]
    for step in range(6):
        m.decode(1)
        t, s, _ = m.read_outputs(1)
        _check_step(m, cfg, t[0], s[0], slots, allowed, f"{dtype} step {step}")
        for r, sl in enumerate(slots):
            seen[r].add(int(t[0, sl]))
    digit_ids = set(np.flatnonzero(allowed[0].cpu().numpy()).tolist())
    assert seen[0] <= digit_ids and seen[3] <= digit_ids


def test_unconstrained_rows_and_masks_off_are_bit_identical_to_an_engine_without_masks(hip_lib):
    """Mixed slots (digits / blocklist / none): the -1 rows equal, bit for bit in tokens, scores and boxes, the run of an engine that never
    had a table; the constrained rows differ from it; switching the table off restores every row exactly."""
    m = _model(torch.bfloat16)
    slots, ids = [0, 1, 2, 3, 4, 5], [0, 1, -1, 0, 1, -1]
    plain = _run(m, slots, 6)
    m.set_token_masks(_table())
    m.set_slot_masks(slots, ids)
    mixed = _run(m, slots, 6)
    free = [r for r, i in enumerate(ids) if i < 0]
    for a, b in zip(plain, mixed):
        assert np.array_equal(a[:, free].view(np.int32), b[:, free].view(np.int32))
    assert not np.array_equal(plain[0][:, [0, 3]], mixed[0][:, [0, 3]]), "the digit rows were not constrained at all"
    m.set_token_masks(None)
    again = _run(m, slots, 6)
    for a, b in zip(plain, again):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_eight_steps_in_one_call_equal_eight_calls(hip_lib):
    """decode(8) (the head also writes the next step's embedding) against 8 x decode(1), masks on."""
    m = _model(torch.bfloat16)
    slots, ids = [0, 1, 2, 3, 4, 5], [0, 1, -1, 0, 1, -1]
    m.set_token_masks(_table())
    m.set_slot_masks(slots, ids)
    one = _run(m, slots, 8, single=True)
    m.set_slot_masks(slots, ids)
    eight = _run(m, slots, 8)
    for a, b in zip(one, eight):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_streams_do_not_depend_on_the_slot_count(hip_lib):
    """The same 64 lines alone and as the first 64 of 320 active slots (the grouped 256 x 320 launch above 256 rows): identical streams."""
    m = _model(torch.bfloat16, max_slots=320)
    table = _table()
    ids64 = [(i % 3) - 1 for i in range(64)]
    m.set_token_masks(table)
    m.set_slot_masks(list(range(64)), ids64)
    few = _run(m, list(range(64)), 5)
    m.set_slot_masks(list(range(320)), [(i % 3) - 1 for i in range(320)])
    many = _run(m, list(range(320)), 5)
    for a, b in zip(few, many):
        assert np.array_equal(a.view(np.int32), b[:, :64].view(np.int32))
    dig = set(np.flatnonzero(_allowed_rows(table, [0], _cfg_sd()[0].decoder.vocab_size)[0].cpu().numpy()).tolist())
    rows = [i for i in range(320) if (i % 3) - 1 == 0]
    assert set(many[0][:, rows].reshape(-1).tolist()) <= dig


def test_a_reused_slot_takes_its_new_lines_mask(hip_lib):
    """Slot 0 decodes a digits-only line, then an unconstrained one: the second line equals its run on an engine without masks; slot 1 the
    other way round."""
    m = _model(torch.bfloat16)
    plain = _run(m, [0, 1], 4, lines=[2, 3])
    table = _table()
    m.set_token_masks(table)
    m.set_slot_masks([0, 1], [0, -1])
    _run(m, [0, 1], 3, lines=[0, 1])
    m.set_slot_masks([0, 1], [-1, 0])
    second = _run(m, [0, 1], 4, lines=[2, 3])
    for a, b in zip(plain, second):
        assert np.array_equal(a[:, 0].view(np.int32), b[:, 0].view(np.int32))
    dig = set(np.flatnonzero(_allowed_rows(table, [0], _cfg_sd()[0].decoder.vocab_size)[0].cpu().numpy()).tolist())
    assert set(second[0][:, 1].tolist()) <= dig


def test_mxfp8_head_with_masks(hip_lib):
    """bf16 engine on MXFP8 decode weights: the decode steps' tokens lie in the set and equal the masked recomputation from the MXFP8 head's
    own logits."""
    cfg = _cfg_sd()[0]
    m = _model(torch.bfloat16, decode_fp8=True)
    table = _table()
    slots, ids = [0, 1, 2, 3, 4, 5], [0, 1, -1, 0, 1, -1]
    allowed = _allowed_rows(table, ids, cfg.decoder.vocab_size)
    m.set_token_masks(table)
    m.set_slot_masks(slots, ids)
    tiles, seqs = make_prompts(cfg, GRIDS, seed=9)
    m.prefill(tiles.cuda(), GRIDS, seqs, slots)
    t, s, _ = m.read_outputs(1)
    _check_step(m, cfg, t[0], s[0], slots, allowed, "mxfp8 prefill (bf16 head)")
    m.set_active(slots)
    for step in range(4):
        m.decode(1)
        t, s, _ = m.read_outputs(1)
        _check_step(m, cfg, t[0], s[0], slots, allowed, f"mxfp8 step {step}")


def test_captured_steps_follow_the_tables_contents(hip_lib):
    """hipGraph replay on: the table lives at a fixed address, so steps captured under one table obey the next one's contents."""
    cfg = _cfg_sd()[0]
    tk, V = _tokenizer(), cfg.decoder.vocab_size
    m = _model(torch.bfloat16)
    slots = [0, 1, 2, 3]
    L.check(m.lib.surya_set_tuning(b"graph", C.c_int(1)), "surya_set_tuning(graph)")
    try:
        streams = []
        for chars in (DIGITS, DIGITS, DIGITS, "xyz"):                       # eager, capture, replay, replay under new contents
            t1 = tk.token_mask(allow=chars, vocab_size=V)[None]
            m.set_token_masks(t1)
            m.set_slot_masks(slots, [0] * 4)
            toks = _run(m, slots, 4)[0]
            assert set(toks.reshape(-1).tolist()) <= set(np.flatnonzero(_allowed_rows(t1, [0], V)[0].cpu().numpy()).tolist()), chars
            streams.append(toks)
        assert np.array_equal(streams[0], streams[1]) and np.array_equal(streams[0], streams[2])
    finally:
        L.check(m.lib.surya_set_tuning(b"graph", C.c_int(0)), "surya_set_tuning(graph)")


def test_entry_points_refuse_bad_tables_and_ids(hip_lib):
    cfg = _cfg_sd()[0]
    m = _model(torch.bfloat16)
    words = (cfg.decoder.vocab_size + 31) // 32
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.set_slot_masks([0], [0])                                           # no table yet
    good = _table()
    empty = good.copy()
    empty[1] = 0
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
        m.set_token_masks(empty)                                             # a mask without an allowed id
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
        m.set_token_masks(np.repeat(good[:1], L.SA_MAX_TOKEN_MASKS + 1, axis=0))
    with pytest.raises(ValueError):
        m.set_token_masks(np.ones((1, words + 1), np.uint32))
    m.set_token_masks(good)
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
        m.set_slot_masks([0], [2])                                           # row 2 of a two-row table
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
        m.set_slot_masks([8], [0])                                           # slot 8 of 8
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
        m.set_slot_masks([3, 3], [0, 1])                                     # a slot named twice
    m.set_slot_masks([0, 1], [1, -1])
    m.set_token_masks(None)


# ------------------------------------------------------------------------------------------------------------------ the predictor
def _predictor(max_slots=16, max_tokens=10):
    from surya_amd.recognition.predictor import RecognitionModelLoader, RecognitionPredictor
    cfg, sd = _cfg_sd()

    class Loader(RecognitionModelLoader):
        def model(self, device=None, dtype_=None, **caps):
            return super().model("cuda:0", torch.bfloat16, max_slots=max_slots, max_kv_len=512, max_patches=8192, max_prefill_tokens=2048)

    class Pred(RecognitionPredictor):
        model_loader_cls = Loader
        batch_size = max_slots

    settings.RECOGNITION_MAX_TOKENS = max_tokens
    return Pred(checkpoint={"config": cfg, "state_dict": sd})


@pytest.fixture()
def _max_tokens():
    old = settings.RECOGNITION_MAX_TOKENS
    yield
    settings.RECOGNITION_MAX_TOKENS = old


def _lines_of(results):
    return [ln for r in results for ln in r.text_lines]


def test_predictor_allowlist_forms(hip_lib, _max_tokens):
    pred = _predictor()
    crops = make_line_crops(8, seed=4)
    imgs = [Image.fromarray(c) for c in crops[:4]]
    boxes = [[[0, 0, im.size[0], im.size[1]], [0, 0, im.size[0] // 2, im.size[1]]] for im in imgs]        # two lines per image
    plain = pred(imgs, bboxes=boxes)
    # allowlist=None is the call without the keyword
    assert [r.model_dump() for r in pred(imgs, bboxes=boxes, allowlist=None, blocklist=None)] == [r.model_dump() for r in plain]
    assert pred.model.n_token_masks == 0
    # one str for every line of the call
    out = pred(imgs, bboxes=boxes, allowlist=DIGITS)
    lines = _lines_of(out)
    assert len(lines) == 8 and all(set(ln.text) <= set(DIGITS) for ln in lines)
    assert any(ln.text for ln in lines), "every constrained line came out empty"
    assert all(0 <= (ln.confidence or 0) <= 1 for ln in lines)
    assert pred.model.n_token_masks == 0                                     # the call switched the masks off on its way out
    # per image: unconstrained / digits / per line (digits, none) / blocklist
    out = pred(imgs, bboxes=boxes, allowlist=[None, DIGITS, [DIGITS, None], None], blocklist=[None, None, None, VOWELS])
    assert [r.model_dump() for r in out[:1]] == [r.model_dump() for r in plain[:1]]
    assert all(set(ln.text) <= set(DIGITS) for ln in out[1].text_lines)
    assert set(out[2].text_lines[0].text) <= set(DIGITS)
    assert out[2].text_lines[1].model_dump() == plain[2].text_lines[1].model_dump()
    # (tags such as <i> are ids of their own, not characters: a blocklist does not concern them)
    assert all(not (set(re.sub(r"<[^>]+>", "", ln.text)) & set(VOWELS)) for ln in out[3].text_lines)
    # a constrained line equals itself whatever is constrained beside it
    assert out[1].model_dump() == pred(imgs, bboxes=boxes, allowlist=DIGITS)[1].model_dump()
    # malformed arguments raise
    with pytest.raises(ValueError):
        pred(imgs, bboxes=boxes, allowlist=DIGITS, blocklist="x")
    with pytest.raises(ValueError):
        pred(imgs, bboxes=boxes, allowlist=[DIGITS])
    with pytest.raises(ValueError):
        pred(imgs, bboxes=boxes, allowlist=[[DIGITS], None, None, None])
    with pytest.raises(TypeError):
        pred(imgs, bboxes=boxes, allowlist=7)
    assert [r.model_dump() for r in pred(imgs, bboxes=boxes)] == [r.model_dump() for r in plain]


def test_streamed_call_with_a_list_equals_the_serial_one(hip_lib, _max_tokens):
    from surya_amd.synth import make_pages_with_lines
    from test_gpu_predictors import _det_with_drawn_rows
    size = 256
    pages_np, rows = make_pages_with_lines(5, size, seed=99)
    pages = [Image.fromarray(p) for p in pages_np]
    det = _det_with_drawn_rows(pages, rows, size, 2)
    pred = _predictor(max_slots=8, max_tokens=7)
    per_image = [DIGITS, None, DIGITS, "xyz", None]
    for kw in (dict(allowlist=DIGITS), dict(allowlist=per_image)):
        pred.stream_detection = False
        serial = pred(pages, det_predictor=det, **kw)
        assert "streamed" not in pred.last_timing
        pred.stream_detection = True
        streamed = pred(pages, det_predictor=det, **kw)
        assert pred.last_timing.get("streamed") == 1.0
        assert [r.model_dump() for r in serial] == [r.model_dump() for r in streamed] and len(streamed) == 5
        assert sum(len(r.text_lines) for r in streamed) > 8
        assert all(set(ln.text) <= set(DIGITS) for ln in streamed[0].text_lines)
    with pytest.raises(ValueError, match="not known yet"):
        pred(pages, det_predictor=det, allowlist=[[DIGITS], None, None, None, None])
