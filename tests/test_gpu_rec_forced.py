"""GPU: forced decoding through the recognition engine (surya_rec_set_forced / set_forced_tokens / read_forced / wait_forced) and through
RecognitionPredictor.align, on REC-SMALL (vocabulary 69 632: the 256 x 320 lm_head tile with a partial last tile), six slots.

References: (a) the slow host route that exists without the feature -- prefill, then surya_rec_set_next_tokens + decode(1) per step on the
same model with forcing off -- which a forced run must equal BIT for bit in boxes, greedy tokens and greedy probabilities; (b) the engine's
own logits of a step (surya_rec_copy_last_logits) in float64: the forced token's probability within the recognition tests' rtol = 2e-3, its
log-probability within 2e-3 absolute (the same bound through the logarithm).
"""
import ctypes as C

import numpy as np
import pytest
import torch
from PIL import Image

from surya_amd import _lib as L
from surya_amd.settings import settings
from surya_amd.synth import make_line_crops

from test_gpu_rec_allowlist import GRIDS, N_LINES, _cfg_sd, _line, _max_tokens, _model, _predictor, _run   # noqa: F401
from util import make_prompts

pytestmark = pytest.mark.gpu
SLOTS = [0, 1, 2, 3, 4, 5]
LENS = [5, 7, 0, 3, 7, 6]                   # forced ids per slot: mixed, one slot free-running from the start
ARITH = [(torch.float32, False), (torch.bfloat16, False), (torch.float16, False), (torch.bfloat16, True)]


def _ids(line, n, end_eos=False):
    """n forced ids of line `line`: a function of the line alone; plain ids (never eos / pad) unless the last is asked to be eos."""
    cfg = _cfg_sd()[0]
    g = np.random.default_rng(500 + line)
    ids = g.integers(0, cfg.decoder.vocab_size, size=n).tolist()
    stop = (cfg.eos_token_id, cfg.pad_token_id)
    ids = [i if i not in stop else 17 for i in ids]
    if end_eos and n:
        ids[-1] = cfg.eos_token_id
    return ids


def _seqs(lens, eos_on=(1,)):
    return [_ids(i, n, end_eos=i in eos_on) for i, n in enumerate(lens)]


def _prefill(m, slots, ids=None):
    lines = list(range(len(slots)))
    tiles, seqs = torch.cat([_line(i)[0] for i in lines]), [_line(i)[1] for i in lines]
    if ids is not None:
        m.set_forced_tokens(slots, ids)
    m.prefill(tiles.cuda(), [GRIDS[i % N_LINES] for i in lines], seqs, slots)


def _run_forced(m, slots, steps, ids, single=False):
    """Line i into slots[i] with ids[i] forced; (tokens, scores, boxes, greedy tokens, greedy probabilities, log-probabilities), each
    [1 + steps, len(slots)(, 6)]."""
    _prefill(m, slots, ids)
    t, s, b = m.read_outputs(1)
    f = m.read_forced(1)
    out = [(t[0, slots].copy(), s[0, slots].copy(), b[0, slots].copy()) + tuple(a[0, slots].copy() for a in f)]
    m.set_active(sorted(slots))
    for _ in range(steps if single else 1 if steps else 0):
        n = 1 if single else steps
        m.decode(n)
        t, s, b = m.read_outputs(n)
        f = m.read_forced(n)
        out += [(t[j, slots].copy(), s[j, slots].copy(), b[j, slots].copy()) + tuple(a[j, slots].copy() for a in f) for j in range(n)]
    return tuple(np.stack([o[i] for o in out]) for i in range(6))


def _slow_route(m, slots, steps, ids, free_tail=0):
    """Forcing off: prefill, then per step set_next_tokens(the forced id of the position just emitted, pad after eos / pad) + decode(1); a
    slot past its ids keeps the engine's own next token. `free_tail`: the last steps run as ONE decode call (nothing left to force).
    -> (tokens, scores, boxes) [1 + steps, len(slots)(, 6)] as the ENGINE chose them (the greedy stream under teacher forcing)."""
    cfg = _cfg_sd()[0]
    stop = (cfg.eos_token_id, cfg.pad_token_id)
    _prefill(m, slots)
    t, s, b = m.read_outputs(1)
    out = [(t[0, slots].copy(), s[0, slots].copy(), b[0, slots].copy())]
    m.set_active(sorted(slots))

    def feed(pos):
        pairs = [(sl, cfg.pad_token_id if seq[pos] in stop else seq[pos]) for sl, seq in zip(slots, ids) if pos < len(seq)]
        if pairs:
            m.set_next_tokens([p[0] for p in pairs], [p[1] for p in pairs])

    for k in range(steps - free_tail):
        feed(k)
        m.decode(1)
        t, s, b = m.read_outputs(1)
        out.append((t[0, slots].copy(), s[0, slots].copy(), b[0, slots].copy()))
    if free_tail:
        feed(steps - free_tail)
        assert all(len(seq) <= steps - free_tail + 1 for seq in ids)
        m.decode(free_tail)
        t, s, b = m.read_outputs(free_tail)
        out += [(t[j, slots].copy(), s[j, slots].copy(), b[j, slots].copy()) for j in range(free_tail)]
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _forced_mask(ids, steps):
    """bool [1 + steps, len(ids)]: position k of slot r is forced; and the ids there."""
    on = np.zeros((1 + steps, len(ids)), bool)
    val = np.zeros((1 + steps, len(ids)), np.int64)
    for r, seq in enumerate(ids):
        n = min(len(seq), 1 + steps)
        on[:n, r], val[:n, r] = True, seq[:n]
    return on, val


@pytest.mark.parametrize("dtype,fp8", ARITH)
def test_forced_equals_host_teacher_forcing_bit_for_bit(hip_lib, dtype, fp8):
    cfg = _cfg_sd()[0]
    m = _model(dtype, decode_fp8=True) if fp8 else _model(dtype)
    ids, steps = _seqs(LENS), 7
    m.set_forced(True)
    tok, sc, bb, gt, gp, lp = _run_forced(m, SLOTS, steps, ids, single=True)
    m.set_forced(False)
    s_tok, s_sc, s_bb = _slow_route(m, SLOTS, steps, ids)
    on, val = _forced_mask(ids, steps)
    assert on.any() and (~on).any() and not on[:, 2].any()
    assert np.array_equal(bb, s_bb), "boxes under forcing differ from the host route's"
    assert np.array_equal(gt, s_tok), "greedy tokens under forcing differ from the host route's tokens"
    live = s_sc != 0                                             # rows that go on report 1 / total as their score
    assert live.any() and np.array_equal(_bits(gp)[live], _bits(s_sc)[live])
    assert np.array_equal(tok[on], val[on]), "a forced position did not emit its id"
    assert np.array_equal(tok[~on], s_tok[~on]) and np.array_equal(_bits(sc)[~on], _bits(s_sc)[~on]), "free positions differ"
    done = np.isin(tok, [cfg.eos_token_id, cfg.pad_token_id])
    assert (sc[done] == 0).all() and (sc[on & ~done] > 0).all() and (sc <= 1).all()
    # where the model agrees with the forced id, the score is the greedy score's bits and the log-probability the greedy token's
    agree = on & (gt == tok) & ~done
    assert np.array_equal(_bits(sc)[agree], _bits(gp)[agree])
    assert (lp <= 0).all() and np.isfinite(lp).all()
    assert np.allclose(np.exp(lp.astype(np.float64))[on & ~done], sc[on & ~done], rtol=1e-5, atol=0)      # two fp32 routes to one number


@pytest.mark.parametrize("dtype,fp8", ARITH)
def test_every_step_against_the_logits(hip_lib, dtype, fp8):
    cfg = _cfg_sd()[0]
    m = _model(dtype, decode_fp8=True) if fp8 else _model(dtype)
    m.set_forced(True)
    ids = _seqs([7, 7, 0, 7, 4, 7], eos_on=())
    tiles, seqs = make_prompts(cfg, GRIDS, seed=9)
    m.set_forced_tokens(SLOTS, ids)
    m.prefill(tiles.cuda(), GRIDS, seqs, SLOTS)
    m.set_active(SLOTS)
    worst_p = worst_l = 0.0
    for step in range(7):
        if step:
            m.decode(1)
        t, s, _ = m.read_outputs(1)
        gt, gp, lp = m.read_forced(1)
        lg = m.last_logits().double()
        assert lg.shape == (len(SLOTS), cfg.decoder.vocab_size)
        logp = torch.log_softmax(lg, 1)
        tok = torch.from_numpy(t[0, SLOTS].astype(np.int64)).cuda()
        want = [seq[step] if step < len(seq) else None for seq in ids]
        for r, w in enumerate(want):
            assert w is None or int(tok[r]) == w, (step, r)
        ref_lp = logp[torch.arange(len(SLOTS)), tok].cpu().numpy()
        ref_arg = lg.argmax(1).cpu().numpy()
        assert np.array_equal(gt[0, SLOTS], ref_arg), (step, gt[0, SLOTS].tolist(), ref_arg.tolist())
        for r, w in enumerate(want):
            if w is None:
                assert int(tok[r]) == ref_arg[r]                 # a free-running slot emits the argmax
        live = ~np.isin(t[0, SLOTS], [cfg.eos_token_id, cfg.pad_token_id])
        rel = np.abs(s[0, SLOTS].astype(np.float64) - np.exp(ref_lp))[live] / np.exp(ref_lp)[live]
        dl = np.abs(lp[0, SLOTS].astype(np.float64) - ref_lp)
        worst_p, worst_l = max(worst_p, rel.max()), max(worst_l, dl.max())
        assert (rel <= 2e-3).all(), (step, rel.max())
        assert (dl <= 2e-3).all(), (step, dl.max())
        ref_gp = np.exp(logp.max(1).values.cpu().numpy())
        assert (np.abs(gp[0, SLOTS] - ref_gp) / ref_gp <= 2e-3).all()
    print(f"{dtype} fp8={fp8}: max relative probability error {worst_p:.3e}, max log-probability error {worst_l:.3e}")


def test_forcing_the_greedy_stream_reproduces_it(hip_lib):
    m = _model(torch.bfloat16)
    free = _run(m, SLOTS, 6)
    ids = [free[0][:, r].tolist() for r in range(len(SLOTS))]
    m.set_forced(True)
    got = _run_forced(m, SLOTS, 6, ids)
    for a, b in zip(free, got[:3]):
        assert np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(got[3], got[0])                        # greedy_token == token everywhere
    m.set_forced(False)
    again = _run(m, SLOTS, 6)
    for a, b in zip(free, again):
        assert np.array_equal(_bits(a), _bits(b))


def test_a_slot_past_its_ids_free_runs_with_the_bits_of_a_slot_never_forced(hip_lib):
    m = _model(torch.bfloat16)
    ids = _seqs([3, 3, 1, 3, 2, 0], eos_on=())
    m.set_forced(True)
    got = _run_forced(m, SLOTS, 6, ids)                          # one decode call: the cursor runs past the end inside it
    m.set_forced(False)
    slow = _slow_route(m, SLOTS, 6, ids, free_tail=4)            # forcing off: positions 3.. come from a plain decode(4)
    for a, b in zip(slow, got[:3]):
        assert np.array_equal(_bits(a[3:]), _bits(b[3:]))
    assert np.array_equal(got[3][3:], got[0][3:])                # free-running: the emitted token is the greedy one
    live = got[1][3:] != 0
    assert np.array_equal(_bits(got[4][3:])[live], _bits(got[1][3:])[live])


def test_eight_steps_in_one_call_equal_eight_calls(hip_lib):
    m = _model(torch.bfloat16)
    m.set_forced(True)
    ids = _seqs([9, 4, 0, 9, 6, 9])
    one = _run_forced(m, SLOTS, 8, ids, single=True)
    eight = _run_forced(m, SLOTS, 8, ids)
    for a, b in zip(one, eight):
        assert np.array_equal(_bits(a), _bits(b))


def test_forced_outputs_do_not_depend_on_the_slot_count(hip_lib):
    """The same 64 lines alone and as the first 64 of 320 active slots (the grouped 256 x 320 launch above 256 rows)."""
    m = _model(torch.bfloat16, max_slots=320)
    m.set_forced(True)
    ids = [_ids(i, 5 if i % 3 else 2) for i in range(320)]
    few = _run_forced(m, list(range(64)), 4, ids[:64])
    many = _run_forced(m, list(range(320)), 4, ids)
    for a, b in zip(few, many):
        assert np.array_equal(_bits(a), _bits(b[:, :64]))
    on, val = _forced_mask(ids, 4)
    assert np.array_equal(many[0][on], val[on])


def test_decode_async_ring_equals_read(hip_lib):
    m = _model(torch.bfloat16)
    m.set_forced(True)
    ids = _seqs([9, 4, 0, 9, 6, 9])
    ref = _run_forced(m, SLOTS, 8, ids)
    _prefill(m, SLOTS, ids)
    m.read_outputs(1)
    m.set_active(SLOTS)
    m.decode_async(4, 0)
    m.decode_async(4, 1)
    got = [[], [], [], []]
    waited = []
    for ring in (0, 1):
        t, _, _ = m.wait_outputs(4, ring)
        f = m.wait_forced(4, ring)
        for dst, a in zip(got, (t,) + tuple(f)):
            dst.append(a[:, SLOTS].copy())
        waited.append([a.copy() for a in f])
    for a, b in zip(got, (ref[0], ref[3], ref[4], ref[5])):
        assert np.array_equal(_bits(np.concatenate(a)), _bits(b[1:]))
    # the synchronous read of all 16 steps shows the bytes the waits returned in rows 0-3 and 8-11: mirror, wait and read agree on where
    # a step lives
    read = [a.copy() for a in m.read_forced(16)]
    for ring in (0, 1):
        for r, w in zip(read, waited[ring]):
            assert r[8 * ring: 8 * ring + 4].tobytes() == w.tobytes()


def test_a_ring_half_filled_while_off_is_refused(hip_lib):
    m = _model(torch.bfloat16)
    _run(m, SLOTS, 0)
    m.decode_async(2, 0)
    m.wait_outputs(2, 0)
    m.set_forced(True)
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.wait_forced(2, 0)
    m.decode_async(2, 1)
    m.wait_outputs(2, 1)
    gt, gp, _ = m.wait_forced(2, 1)
    assert (gt[:, SLOTS] >= 0).all() and (gp[:, SLOTS] > 0).all()


def test_captured_steps_toggled_off_on_off(hip_lib):
    """hipGraph replay on: switching drops the captured steps, so off / on / off give the arrays the eager runs give."""
    m = _model(torch.bfloat16)
    ids = _seqs([5, 2, 0, 5, 4, 5])
    eager_off = _run(m, SLOTS, 4)
    m.set_forced(True)
    eager_on = _run_forced(m, SLOTS, 4, ids)
    m.set_forced(False)
    L.check(m.lib.surya_set_tuning(b"graph", C.c_int(1)), "surya_set_tuning(graph)")
    try:
        for rnd in range(2):
            for rep in range(3):                                                # eager, capture, replay
                got = _run(m, SLOTS, 4)
                for a, b in zip(eager_off, got):
                    assert np.array_equal(_bits(a), _bits(b)), (rnd, rep)
            m.set_forced(True)
            for rep in range(3):
                got = _run_forced(m, SLOTS, 4, ids)
                for a, b in zip(eager_on, got):
                    assert np.array_equal(_bits(a), _bits(b)), (rnd, rep)
            m.set_forced(False)
    finally:
        L.check(m.lib.surya_set_tuning(b"graph", C.c_int(0)), "surya_set_tuning(graph)")


def test_the_fallback_head_forces_too(hip_lib):
    """Tuning ghead = 1 runs greedy_head_kernel<T, true> (no fused embedding): the same tokens and greedy tokens as the default head;
    boxes, scores and log-probabilities within the bound test_head2_and_fused_embedding_equal_round3_kernels sets for the two heads' totals (the same
    sum in another tree: rtol 1e-5), which reaches a log-probability as 1e-5 absolute plus its own fp32 rounding at |log p| ~ 11."""
    m = _model(torch.bfloat16)
    m.set_forced(True)
    ids = _seqs([5, 2, 0, 5, 4, 5])
    ref = _run_forced(m, SLOTS, 4, ids)

    def tune(**kw):
        for k, v in kw.items():
            L.check(m.lib.surya_set_tuning(k.encode(), C.c_int(v)), f"surya_set_tuning({k})")

    tune(ghead=1, fuse_embed=0)
    try:
        got = _run_forced(m, SLOTS, 4, ids)
    finally:
        tune(ghead=2, fuse_embed=1)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[3], ref[3])
    diff = np.abs(got[2].astype(np.int64) - ref[2].astype(np.int64))          # (the two heads' bbox dot products: that test's bound)
    assert diff.max() <= 1 and (diff > 0).mean() <= 0.02, (diff.max(), (diff > 0).mean())
    assert np.allclose(got[1], ref[1], rtol=1e-5, atol=1e-7) and np.allclose(got[4], ref[4], rtol=1e-5, atol=1e-7)
    assert np.abs(got[5].astype(np.float64) - ref[5]).max() <= 2e-5
    on, val = _forced_mask(ids, 4)
    assert np.array_equal(got[0][on], val[on])


def test_refusals(hip_lib):
    from test_gpu_rec_allowlist import _table
    m = _model(torch.bfloat16)
    V = _cfg_sd()[0].decoder.vocab_size
    lib, h = m.lib, m.handle
    assert lib.surya_rec_set_forced(h, C.c_int(2)) == L.SA_ERR_ARG and lib.surya_rec_set_forced(h, C.c_int(-1)) == L.SA_ERR_ARG
    for call in (lambda: m.read_forced(1), lambda: m.wait_forced(1, 0), lambda: m.set_forced_tokens([0], [[1, 2]])):
        with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
            call()                                                              # everything is refused while off
    # mutual exclusion with masks and alternatives, both ways
    m.set_token_masks(_table())
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.set_forced(True)
    m.set_token_masks(None)
    m.set_alternatives(True)
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.set_forced(True)
    m.set_alternatives(False)
    m.set_forced(True)
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.set_token_masks(_table())
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.set_alternatives(True)
    m.set_token_masks(None)                                                     # (n_masks = 0 and alternatives off stay what they were)
    m.set_alternatives(False)
    # set_forced_tokens: bad arguments change nothing
    ids = _seqs([4, 4, 4, 4, 4, 4], eos_on=())
    good = _run_forced(m, SLOTS, 3, ids)
    m.set_forced_tokens(SLOTS, ids)
    for slots, seqs in (([0, 0], [[1], [2]]), ([8], [[1]]), ([-1], [[1]]), ([0], [[V]]), ([0], [[-1]]), ([0], [[5] * (L.SA_MAX_FORCED_TOKENS + 1)])):
        with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
            m.set_forced_tokens(slots, seqs)
    _prefill(m, SLOTS)                                                          # the ids set before the refused calls are still in place
    t, _, _ = m.read_outputs(1)
    assert np.array_equal(t[0, SLOTS], good[0][0])
    m.set_forced_tokens([0], [[5] * L.SA_MAX_FORCED_TOKENS])                    # the longest list is fine, and so is an empty one
    m.set_forced_tokens([1, 2], [[], [3]])
    # switch-off resets the table: the next switch-on starts with every slot free-running
    m.set_forced(False)
    free = _run(m, SLOTS, 3)
    m.set_forced(True)
    _prefill(m, SLOTS)
    t, s, b = m.read_outputs(1)
    assert np.array_equal(t[0, SLOTS], free[0][0]) and np.array_equal(_bits(s[0, SLOTS]), _bits(free[1][0]))


# ------------------------------------------------------------------------------------------------------------------ the predictor
def _lines_of(results):
    return [ln for r in results for ln in r.text_lines]


def test_call_before_and_after_align_is_unchanged(hip_lib, _max_tokens):
    pred = _predictor(max_tokens=10)
    imgs = [Image.fromarray(c) for c in make_line_crops(4, seed=4)]
    boxes = [[[0, 0, im.size[0], im.size[1]]] for im in imgs]
    before = pred(imgs, bboxes=boxes)
    settings.RECOGNITION_MAX_TOKENS = 16
    aligned = pred.align(imgs, [["abc"], ["hello world"], [""], ["1234"]], bboxes=boxes)
    assert not pred.model.forced and [ln.text for ln in _lines_of(aligned)] == ["abc", "hello world", "", "1234"]
    settings.RECOGNITION_MAX_TOKENS = 10
    after = pred(imgs, bboxes=boxes)
    assert before == after and [r.model_dump() for r in before] == [r.model_dump() for r in after]
    assert [r.model_dump_json() for r in before] == [r.model_dump_json() for r in after]
    assert all("log_prob" not in ln for r in after for ln in r.model_dump()["text_lines"])
    assert all(ln.log_prob is None and all(c.greedy is None for c in ln.chars) for ln in _lines_of(after))


def test_predictor_align(hip_lib, _max_tokens):
    pred = _predictor(max_tokens=48)
    crops = make_line_crops(6, seed=4)
    imgs = [Image.fromarray(c) for c in crops[:3]]
    boxes = [[[0, 0, im.size[0], im.size[1]], [0, 0, im.size[0] // 2, im.size[1]]] for im in imgs]        # two lines per image
    texts = [["Forced decoding", "-" * 40], ["", "a \U0001F600 b"], ["x", "The quick brown fox, 1234567890."]]
    out = pred.align(imgs, texts, bboxes=boxes)
    assert not pred.model.forced and len(out) == 3
    forced = pred.last_forced
    stream_of = {tuple(pred.last_packed[0][k]): k for k in range(len(pred.last_packed[0]))}
    for r, tx in zip(out, texts):
        assert len(r.text_lines) == len(tx)
        for ln, text in zip(r.text_lines, tx):
            assert ln.text == text                                               # read back through the tokenizer
            ids = pred.forced_ids(text, "ocr_with_boxes")
            k = stream_of[tuple(ids)]                                            # forty dashes did not stop early: the whole list was emitted
            want = float(np.sum(np.asarray(forced[2][k], np.float64)))
            assert ln.log_prob == want and ln.log_prob < 0 and "log_prob" in ln.model_dump()
            assert len(ln.chars) == len(text), (text, [c.text for c in ln.chars])      # one char per character (a non-BMP one is two tokens)
            assert [c.text for c in ln.chars] == list(text)
            for c in ln.chars:
                assert len(c.polygon) == 4 and 0 < c.confidence <= 1
                assert c.greedy is not None and 0 < c.greedy.confidence <= 1 and c.greedy.token_id >= 0
                assert c.greedy.confidence >= c.confidence * (1 - 1e-6)          # the model's own reading is at least as likely
                assert "greedy" in c.model_dump()
            if text:
                assert abs(ln.confidence - float(np.mean([c.confidence for c in ln.chars]))) < 1e-12
    # aligning a line to __call__'s own output for it gives __call__'s characters, confidences and polygons
    settings.RECOGNITION_MAX_TOKENS = 10
    imgs = [Image.fromarray(c) for c in make_line_crops(12, seed=7)]
    boxes = [[[0, 0, im.size[0], im.size[1]]] for im in imgs]
    plain = pred(imgs, bboxes=boxes)
    plain_streams = {tuple(pred.last_packed[0][k]) for k in range(len(pred.last_packed[0]))}
    settings.RECOGNITION_MAX_TOKENS = 11                                        # the ids plus eos
    # (only a text that tokenizes back into the ids it came from can be compared: lone surrogates vanish from the text, the tag fixer adds
    # closing tags, math ids decode to several characters; the other lines are aligned to "")
    ids_of = [tuple(pred.forced_ids(r.text_lines[0].text, "ocr_with_boxes")) for r in plain]
    ok = [ids in plain_streams or ids[:-1] in plain_streams for ids in ids_of]
    again = pred.align(imgs, [[r.text_lines[0].text if k else ""] for r, k in zip(plain, ok)], bboxes=boxes)
    streams = {tuple(pred.last_packed[0][k]) for k in range(len(pred.last_packed[0]))}
    same = 0
    strip = lambda ln: [{k: v for k, v in c.items() if k != "greedy"} for c in ln.model_dump()["chars"]]
    for p, a, ids, k in zip(_lines_of(plain), _lines_of(again), ids_of, ok):
        if not k or not p.chars:
            continue
        assert ids in streams
        assert strip(a) == strip(p) and a.confidence == p.confidence and a.text == p.text
        assert all(c.greedy.text == c.text and c.greedy.confidence == c.confidence for c in a.chars if len(c.text) == 1 and ord(c.text) < 0x10000)
        same += 1
    print(f"aligned to its own output: {same} of {len(imgs)} lines compared")
    assert same >= 1
