"""GPU: beam search through the recognition engine (surya_rec_set_beam / read_beam / wait_beam) and through RecognitionPredictor.beam_width,
on REC-SMALL (vocabulary 69 632), six lines, at most 24 slots and 8 selections.

References: (a) the slow host route that exists without the feature -- every hypothesis prefix replayed in a slot of its own (prefill,
then surya_rec_set_next_tokens + decode(1) per token, alternatives on), selection in float64 on the host; (c) forced decoding of the final
hypotheses on the same handle. The rules themselves are checked without a GPU (tests/test_beam_cpu.py)."""
import ctypes as C

import numpy as np
import pytest
import torch
from PIL import Image

from surya_amd import _lib as L
from surya_amd.settings import settings
from surya_amd.synth import make_line_crops

from test_gpu_rec_allowlist import GRIDS, N_LINES, _cfg_sd, _line, _max_tokens, _model, _run, _tokenizer   # noqa: F401

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
LINES = list(range(N_LINES))        # line seeds 100 + i (test_gpu_rec_allowlist._line). On the reference alone they keep the B-th and the
                                    # (B + 1)-th candidate at least 2e-4 apart at all 8 selections, but for line 1 in fp32 at B = 3 and 4
                                    # (selection 1): one line of six left out there, none in bf16 / fp16 or at B = 2 (measured on MI355X)
STEPS = 7                           # decode steps behind the prefill: 8 selections
MARGIN = 2e-4                       # fp32 accumulation of <= 8 terms at magnitude <= 128 errs by at most 8 x 7.6e-6 (half an ulp of 128)
ARRAYS = ("tokens", "parents", "ranks", "probs", "logps")


def _ids():
    cfg = _cfg_sd()[0]
    return cfg.eos_token_id, cfg.pad_token_id, cfg.nop_token_id


def _prefill(m, lines, slots):
    tiles, seqs = torch.cat([_line(i)[0] for i in lines]), [_line(i)[1] for i in lines]
    m.prefill(tiles.cuda(), [GRIDS[i % N_LINES] for i in lines], seqs, slots)


def _beam_run(m, B, lines, steps, single=False):
    """Beam mode on: line i into group i. -> dict of the five beam arrays [1 + steps, groups, B] and "boxes" [1 + steps, groups, B, 6]."""
    G = len(lines)
    sl = (np.arange(G)[:, None] * B + np.arange(B)[None, :])
    _prefill(m, lines, (np.arange(G) * B).tolist())
    rows = [tuple(a[0][sl].copy() for a in m.read_beam(1)) + (m.read_outputs(1)[2][0][sl].copy(),)]
    m.set_active(sl.reshape(-1).tolist())
    for n in ([1] * steps if single else [steps] if steps else []):
        m.decode(n)
        bm, bb = m.read_beam(n), m.read_outputs(n)[2]
        rows += [tuple(a[k][sl].copy() for a in bm) + (bb[k][sl].copy(),) for k in range(n)]
    out = {k: np.stack([r[i] for r in rows]) for i, k in enumerate(ARRAYS + ("boxes",))}
    # the engine reports a step's box per slot as it was BEFORE the selection: a beam's box is the one of its parent's slot
    out["boxes"] = np.take_along_axis(out["boxes"], np.maximum(out["parents"], 0)[..., None], axis=2)
    return out


def _place(B, chosen):
    """beam_core.h's placement of a chosen SET [(parent, rank)] (rank -1 = frozen): it needs no order across parents. -> per slot or None."""
    at = [None] * B
    further = []
    for par, rk in sorted(chosen):
        if at[par] is None:
            at[par] = (par, rk)
        else:
            further.append((par, rk))
    free = [b for b in range(B) if at[b] is None]
    for c in further:
        at[free.pop(0)] = c
    return at


def _reference(m, B, lines, steps):
    """The slow route, beam mode off: at every selection each live hypothesis prefix is replayed from its prompt in slot line * B + beam
    (one prefill call per beam index, so a prefill has the rows of the beam run's), its four alternatives and its box are read back, and
    the host selects in float64. -> expected arrays like _beam_run's (logps float64), and per line the first selection whose B-th and
    (B + 1)-th candidates were closer than MARGIN (None: never)."""
    eos, pad, nop = _ids()
    G = len(lines)
    sl = (np.arange(G)[:, None] * B + np.arange(B)[None, :])
    flat = sl.reshape(-1).tolist()
    beams = [[dict(toks=[], cum=0.0, fin=True, alive=False) for _ in range(B)] for _ in range(G)]
    exp = {k: np.zeros((1 + steps, G, B), np.float64 if k in ("probs", "logps") else np.int64) for k in ARRAYS}
    exp["boxes"] = np.zeros((1 + steps, G, B, 6), np.int64)
    exp["finished"] = np.zeros((1 + steps, G, B), bool)
    close = [None] * G
    m.set_alternatives(True)
    for t in range(1 + steps):
        for b in range(B if t else 1):
            _prefill(m, lines, sl[:, b].tolist())
        if t:
            m.set_active(flat)
            for k in range(t):
                feed = [(bm["toks"][k] if k < len(bm["toks"]) and bm["toks"][k] not in (eos, pad) else pad) for g in range(G) for bm in beams[g]]
                m.set_next_tokens(flat, feed)
                m.decode(1)
        at_, ap_ = (a[0].copy() for a in m.read_alternatives(1))
        bb_ = m.read_outputs(1)[2][0].copy()
        for g in range(G):
            cands = []                                   # (score, parent, rank)
            for b, bm in enumerate(beams[g] if t else beams[g][:1]):
                if t and bm["fin"]:
                    if bm["alive"]:
                        cands.append((bm["cum"], b, -1))
                    continue
                for j in range(4):
                    if at_[sl[g, b], j] >= 0 and ap_[sl[g, b], j] > 0:
                        cands.append((bm["cum"] + float(np.log(np.float64(ap_[sl[g, b], j]))), b, j))
            cands.sort(key=lambda c: (-c[0], c[1], c[2]))
            if len(cands) > B and cands[B - 1][0] - cands[B][0] < MARGIN and close[g] is None:
                close[g] = t
            score_of = {(c[1], c[2]): c[0] for c in cands[:B]}
            new = []
            for b, c in enumerate(_place(B, list(score_of))):
                if c is None:
                    new.append(dict(toks=[], cum=-np.inf, fin=True, alive=False))
                    exp["tokens"][t, g, b], exp["parents"][t, g, b], exp["logps"][t, g, b], exp["finished"][t, g, b] = pad, -1, -np.inf, True
                    continue
                par, rk = c
                old = beams[g][par]
                exp["parents"][t, g, b], exp["logps"][t, g, b] = par, score_of[c]
                exp["boxes"][t, g, b] = bb_[sl[g, par]]
                if rk < 0:
                    new.append(dict(old))
                    exp["tokens"][t, g, b], exp["finished"][t, g, b] = pad, True
                else:
                    tok = int(at_[sl[g, par], rk])
                    fin = tok in (eos, pad) or (t == 0 and tok == nop)
                    new.append(dict(toks=old["toks"] + [tok], cum=score_of[c], fin=fin, alive=True))
                    exp["tokens"][t, g, b], exp["ranks"][t, g, b], exp["probs"][t, g, b], exp["finished"][t, g, b] = tok, rk, ap_[sl[g, par], rk], fin
            beams[g] = new
    m.set_alternatives(False)
    return exp, close, beams


def _hypotheses(run, B, g):
    """Token sequences, scores and finished flags of group g's final beams from the device arrays alone (parents followed forwards)."""
    eos, pad, nop = _ids()
    T = run["tokens"].shape[0]
    seqs = [[] for _ in range(B)]
    fin = [True] * B
    for t in range(T):
        par, tok = run["parents"][t, g], run["tokens"][t, g]
        new_s, new_f = [], []
        for b in range(B):
            if par[b] < 0:
                new_s.append(None); new_f.append(True)
            elif t and fin[par[b]]:
                new_s.append(seqs[par[b]]); new_f.append(True)
            else:
                new_s.append(seqs[par[b]] + [int(tok[b])]); new_f.append(int(tok[b]) in (eos, pad) or (t == 0 and int(tok[b]) == nop))
        seqs, fin = new_s, new_f
    return [(seqs[b], float(run["logps"][T - 1, g, b]), fin[b]) for b in range(B) if seqs[b] is not None]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [2, 3, 4])
def test_device_beam_equals_the_host_replay(hip_lib, dtype, B):
    m = _model(dtype, max_slots=24)
    eos, pad, nop = _ids()
    exp, close, _ = _reference(m, B, LINES, STEPS)
    m.set_beam(B, nop)
    got = _beam_run(m, B, LINES, STEPS)
    m.set_beam(None)
    left_out = [g for g in range(len(LINES)) if close[g] is not None]
    print(f"{dtype} B={B}: lines left out (selection closer than {MARGIN}) {left_out} at steps {[close[g] for g in left_out]}")
    assert len(left_out) <= 1, "the recorded line seeds keep the reference clear of near-ties"
    worst = 0.0
    for g in range(len(LINES)):
        if close[g] is not None:
            continue
        for k in ("tokens", "parents"):
            assert np.array_equal(got[k][:, g], exp[k][:, g]), (g, k, got[k][:, g], exp[k][:, g])
        alive = exp["parents"][:, g] >= 0
        live = alive & (exp["probs"][:, g] > 0)                                     # a beam that took a token at that step
        assert np.array_equal(got["ranks"][:, g][live], exp["ranks"][:, g][live])
        assert np.array_equal(got["boxes"][:, g][live], exp["boxes"][:, g][live]), "a child's box is its parent slot's, bit for bit"
        assert got["probs"][:, g].astype(np.float32).tobytes() == exp["probs"][:, g].astype(np.float32).tobytes()
        dev_fin = (got["probs"][:, g] == 0) | np.isin(got["tokens"][:, g], (eos, pad))
        dev_fin[0] |= got["tokens"][0, g] == nop
        assert np.array_equal(dev_fin, exp["finished"][:, g])
        err = np.abs(got["logps"][:, g][alive].astype(np.float64) - exp["logps"][:, g][alive])
        worst = max(worst, float(err.max()))
        assert (err <= 8 * 7.6e-6).all(), (g, err.max())
        assert np.isneginf(got["logps"][:, g][~alive]).all()
    print(f"{dtype} B={B}: max |device fp32 score - float64 score| = {worst:.3e}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_call_of_four_steps_equals_four_calls(hip_lib, dtype):
    m = _model(dtype, max_slots=24)
    m.set_beam(4, _ids()[2])
    one = _beam_run(m, 4, LINES, 4)
    four = _beam_run(m, 4, LINES, 4, single=True)
    for k in ARRAYS + ("boxes",):
        assert one[k].tobytes() == four[k].tobytes(), k
    assert (one["parents"][1:] != np.arange(4)[None, None, :]).any(), "no beam ever moved behind the prefill: the fork was not exercised"


def test_captured_steps_replay_the_selection_and_the_fork(hip_lib):
    """hipGraph replay on: the first call of a shape runs eagerly, the second is captured, the third replayed -- the same five arrays."""
    m = _model(torch.bfloat16, max_slots=24)
    m.set_beam(3, _ids()[2])
    L.check(m.lib.surya_set_tuning(b"graph", C.c_int(1)), "surya_set_tuning(graph)")
    try:
        runs = [_beam_run(m, 3, LINES, 4) for _ in range(3)]
    finally:
        L.check(m.lib.surya_set_tuning(b"graph", C.c_int(0)), "surya_set_tuning(graph)")
        m.set_beam(None)
    for k in ARRAYS + ("boxes",):
        assert runs[0][k].tobytes() == runs[1][k].tobytes() == runs[2][k].tobytes(), k


@pytest.mark.parametrize("dtype", DTYPES)
def test_scores_agree_with_forced_decoding(hip_lib, dtype):
    """Every final hypothesis, forced through the same handle with beam mode off: the sum of its tokens' log-probabilities equals the
    beam score within T x 2e-3 (the per-token bound of test_gpu_rec_forced.py)."""
    B = 4
    m = _model(dtype, max_slots=24)
    m.set_beam(B, _ids()[2])
    run = _beam_run(m, B, LINES, STEPS)
    m.set_beam(None)
    hyps = [(g, h) for g in range(len(LINES)) for h in _hypotheses(run, B, g)]
    assert len(hyps) == B * len(LINES)
    slots = list(range(len(hyps)))
    m.set_forced(True)
    m.set_forced_tokens(slots, [h[0] for _, h in hyps])
    _prefill(m, [LINES[g] for g, _ in hyps], slots)
    lp = [m.read_forced(1)[2][0][slots].copy()]
    m.set_active(slots)
    m.decode(STEPS)
    lp += [m.read_forced(STEPS)[2][k][slots].copy() for k in range(STEPS)]
    m.set_forced(False)
    lp = np.stack(lp).astype(np.float64)
    worst = 0.0
    for r, (g, (toks, score, fin)) in enumerate(hyps):
        T = len(toks)
        diff = abs(float(lp[:T, r].sum()) - score)
        worst = max(worst, diff / T)
        assert diff <= T * 2e-3, (dtype, g, toks, score, lp[:T, r].sum())
    print(f"{dtype}: max |forced sum - beam score| / T = {worst:.3e}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_after_switching_off_greedy_is_bit_identical_to_a_fresh_handle(hip_lib, dtype):
    slots = [0, 1, 2, 3, 4, 5]
    a = _model(dtype, max_slots=24)
    a.set_beam(3, _ids()[2])
    _beam_run(a, 3, LINES, 3)
    a.set_beam(0)
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        a.read_beam(1)
    got = _run(a, slots, 6)
    want = _run(_model(dtype, max_slots=24), slots, 6)
    for x, y in zip(got, want):
        assert x.tobytes() == y.tobytes()


def test_refusals(hip_lib):
    m = _model(torch.bfloat16, max_slots=8)
    nop = _ids()[2]
    for w in (1, 5, -1):
        with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
            m.set_beam(w, nop)
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
        m.read_beam(1)                                                       # never switched on
    for on, off in ((lambda: m.set_forced(True), lambda: m.set_forced(False)), (lambda: m.set_kv_fp8(True), lambda: m.set_kv_fp8(False)),
                    (lambda: m.set_decode_fp8(True), lambda: m.set_decode_fp8(False))):
        on()
        with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
            m.set_beam(2, nop)
        off()
        m.set_beam(2, nop)
        with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
            on()
        m.set_beam(0)
    m.set_beam(3, nop)
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
        _prefill(m, [0], [1])                                                # not a lead slot
    with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
        _prefill(m, [0], [6])                                                # a group that does not fit 8 slots
    _prefill(m, [0, 1], [0, 3])
    for bad in ([0, 1], [0, 1, 2, 3], [1, 2, 3], [3, 4, 5, 0, 1, 2], [0, 1, 2, 0, 1, 2]):
        with pytest.raises(L.SuryaAmdError, match="SA_ERR_ARG"):
            m.set_active(bad)                                                # partial, unaligned, descending, repeated groups
    m.set_active([0, 1, 2, 3, 4, 5])
    m.set_alternatives(True)                                                 # independent of beam mode
    m.decode(1)
    at, ap = m.read_alternatives(1)
    assert (at[0, :6, 0] >= 0).all() and (ap[0, :6, 0] > 0).all()
    m.set_alternatives(False)
    m.read_alternatives(1)                                                   # still served: the beams' candidates
    m.set_beam(0)
    torch.cuda.synchronize()


def test_decode_async_ring_equals_read(hip_lib):
    """Two pipelined calls of four steps: what wait_outputs / wait_beam / wait_alternatives return per ring half is the synchronous run's,
    and read_outputs / read_beam / read_alternatives of all 16 steps show the same bytes in rows 0-3 and 8-11 -- the mirror, the wait
    and the read agree on where a step of each of the three sets lives."""
    B, G = 2, len(LINES)
    m = _model(torch.bfloat16, max_slots=24)
    m.set_beam(B, _ids()[2])
    ref = _beam_run(m, B, LINES, 8)
    sl = (np.arange(G)[:, None] * B + np.arange(B)[None, :])
    _prefill(m, LINES, (np.arange(G) * B).tolist())
    m.set_active(sl.reshape(-1).tolist())
    m.decode_async(4, 0)
    m.decode_async(4, 1)
    waited = []                                                              # per ring: the nine arrays over all slots, as returned
    for ring in (0, 1):
        waited.append([a.copy() for a in m.wait_outputs(4, ring) + m.wait_beam(4, ring) + m.wait_alternatives(4, ring)])
    for i, k in enumerate(ARRAYS):
        got = np.concatenate([w[3 + i][:, sl] for w in waited])
        assert got.tobytes() == ref[k][1:].tobytes(), k
    boxes = np.concatenate([w[2][:, sl] for w in waited])
    parents = np.concatenate([w[4][:, sl] for w in waited])
    boxes = np.take_along_axis(boxes, np.maximum(parents, 0)[..., None], axis=2)
    assert boxes.tobytes() == ref["boxes"][1:].tobytes()
    read = [a.copy() for a in m.read_outputs(16) + m.read_beam(16) + m.read_alternatives(16)]
    for ring in (0, 1):
        for i, (r, w) in enumerate(zip(read, waited[ring])):
            assert r[8 * ring: 8 * ring + 4].tobytes() == w.tobytes(), (ring, i)
    m.set_beam(None)


def test_a_ring_half_filled_while_off_is_refused(hip_lib):
    """decode_async ran with beam mode off, then it is switched on: that ring half mirrored neither beam outputs nor candidates."""
    B, G = 2, len(LINES)
    m = _model(torch.bfloat16, max_slots=24)
    _run(m, list(range(G)), 0)
    m.decode_async(2, 0)
    m.wait_outputs(2, 0)
    m.set_beam(B, _ids()[2])
    for wait in (m.wait_beam, m.wait_alternatives):
        with pytest.raises(L.SuryaAmdError, match="SA_ERR_STATE"):
            wait(2, 0)
    sl = (np.arange(G)[:, None] * B + np.arange(B)[None, :])
    _prefill(m, LINES, (np.arange(G) * B).tolist())
    m.set_active(sl.reshape(-1).tolist())
    m.decode_async(2, 1)
    m.wait_outputs(2, 1)
    parents = m.wait_beam(2, 1)[1][:, sl]
    assert (parents >= -1).all() and (parents >= 0).any(axis=2).all()
    m.set_beam(None)


@pytest.mark.parametrize("dtype", DTYPES)
def test_with_a_token_mask_every_token_is_allowed(hip_lib, dtype):
    cfg = _cfg_sd()[0]
    eos, pad, nop = _ids()
    tk, V = _tokenizer(), cfg.decoder.vocab_size
    digits = tk.token_mask(allow="0123456789.,-", vocab_size=V)
    two, ends = np.zeros_like(digits), np.zeros_like(digits)
    for mask, pair in ((two, (eos, 5000)), (ends, (eos, pad))):
        for i in pair:
            mask[i >> 5] |= np.uint32(1 << (i & 31))
    allowed = set(np.flatnonzero(np.unpackbits(digits.view(np.uint8), bitorder="little")[:V]).tolist())
    B = 3
    m = _model(dtype, max_slots=24)
    m.set_token_masks(np.stack([digits, two, ends]))
    ids = [0, 0, 0, 1, 1, 2]                                                 # lines 0-2 digits, 3-4 {eos, 5000}, 5 {eos, pad}
    m.set_slot_masks(list(range(6 * B)), np.repeat(ids, B).tolist())
    m.set_beam(B, nop)
    run = _beam_run(m, B, LINES, 5)
    m.set_beam(None)
    m.set_token_masks(None)
    for g in range(3):
        hyps = _hypotheses(run, B, g)
        assert len(hyps) == B and all(set(h[0]) <= allowed for h in hyps), hyps
    for g in range(3, 5):
        # two allowed ids: two first tokens, so two beams and one empty slot after the first selection ...
        assert sorted(run["parents"][0, g].tolist()) == [-1, 0, 0] and np.isneginf(run["logps"][0, g]).sum() == 1
        assert set(run["tokens"][0, g][run["parents"][0, g] >= 0].tolist()) == {eos, 5000}
        # ... and every reading is made of the two ids; the one that opened with eos stays as it is
        hyps = _hypotheses(run, B, g)
        assert all(set(h[0]) <= {eos, 5000} for h in hyps) and [eos] in [h[0] for h in hyps]
        assert sum(h[2] for h in hyps) >= 1
    # two ids that both end the line: two hypotheses, finished, and the third slot stays empty to the end
    hyps = _hypotheses(run, B, 5)
    assert sorted(h[0] for h in hyps) == sorted([[eos], [pad]]) and all(h[2] for h in hyps)
    assert (np.sort(run["parents"][:, 5], axis=1)[:, 0] == -1).all() and (run["parents"][:, 5] >= 0).sum() == 2 * run["parents"].shape[0]


# ------------------------------------------------------------------------------------------------------------------ the predictor
def _predictor(dtype, max_slots=12, max_tokens=8):
    from surya_amd.recognition.predictor import RecognitionModelLoader, RecognitionPredictor
    cfg, sd = _cfg_sd()

    class Loader(RecognitionModelLoader):
        def model(self, device=None, dtype_=None, **caps):
            return super().model("cuda:0", dtype, max_slots=max_slots, max_kv_len=512, max_patches=8192, max_prefill_tokens=2048)

    class Pred(RecognitionPredictor):
        model_loader_cls = Loader
        batch_size = max_slots

    settings.RECOGNITION_MAX_TOKENS = max_tokens
    return Pred(checkpoint={"config": cfg, "state_dict": sd})


@pytest.mark.parametrize("dtype", DTYPES)
def test_predictor_beam_width(hip_lib, _max_tokens, dtype):
    pred = _predictor(dtype)
    imgs = [Image.fromarray(c) for c in make_line_crops(3, seed=4)]
    boxes = [[[0, 0, im.size[0], im.size[1]], [0, 0, im.size[0] // 2, im.size[1]]] for im in imgs]        # six lines
    plain = [r.model_dump() for r in pred(imgs, bboxes=boxes)]
    pred.beam_width = 3
    out = pred(imgs, bboxes=boxes, recognition_batch_size=12)
    lines = [ln for r in out for ln in r.text_lines]
    assert len(lines) == 6 and pred.model.beam == 0                          # the call switched beam mode off on its way out
    for ln in lines:
        h = ln.hypotheses
        assert 1 <= len(h) <= 3 and ln.text == h[0].text and ln.log_prob == h[0].log_prob and ln.confidence == h[0].confidence
        assert [x.finished for x in h] == sorted((x.finished for x in h), reverse=True)
        for part in ([x.log_prob for x in h if x.finished], [x.log_prob for x in h if not x.finished]):
            assert part == sorted(part, reverse=True)
        assert all(x.log_prob <= 0 and 0 <= (x.confidence or 0) <= 1 for x in h)
        assert "hypotheses" in ln.model_dump() and len(ln.model_dump()["hypotheses"]) == len(h)
    assert any(len(ln.hypotheses) == 3 for ln in lines)
    if dtype == torch.float32:                                               # four groups at a time or two: the same readings
        small = pred(imgs, bboxes=boxes, recognition_batch_size=6)
        assert [r.model_dump() for r in small] == [r.model_dump() for r in out]
    dig = pred(imgs, bboxes=boxes, allowlist="0123456789.,-")
    for ln in (ln for r in dig for ln in r.text_lines):
        assert all(set(x.text) <= set("0123456789.,-") for x in ln.hypotheses)
    pred.beam_width = None
    again = pred(imgs, bboxes=boxes)
    assert [r.model_dump() for r in again] == plain and all(ln.hypotheses is None for r in again for ln in r.text_lines)
