"""GPU: the fp8 decode options above 256 slots (MXFP8 weights: csrc/gemm_mx.h; FP8 KV cache: csrc/decode_attn_kv8.h), engine and predictor.

  * REC-SMALL bf16 with 320 slots and MXFP8 decode weights: the GRIDS prompts of test_gpu_rec.py (all six of them) replicated over the
    320 slots, teacher-forced for 6 decode steps on the fp32 oracle's tokens (the logits AFTER each of the six steps are compared: all of
    them are fp8 steps; the prompt's own logits come from the unquantised prefill). Every replica of a prompt has bit-identical logits (a line's
    results do not depend on its row block or on the tile that computed it); one replica per prompt is within
    test_rec_small_fp8_decode_teacher_forced's bound of the rec_oracle.MX_DECODE emulation (2 x bf16 deviation + 0.5 x format deviation
    + 1e-2 x max|logit|; the oracle runs once, on the six lines); the fused greedy head of the MXFP8 lm_head at 320 rows agrees with
    the logits; and every mx_big_m_split x mx_big_m_gateup arm gives the bits of the default.
  * The predictor at recognition_batch_size 64 / 256 / 512 returns identical OCRResults with MXFP8 weights, with the FP8 KV cache, and
    with both (the shape of test_ocr_results_identical_across_slot_counts).
  * Switching fp8 off at 320 slots restores the bf16 tokens, scores and boxes exactly.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import rec_oracle as ro
from surya_amd.config import rec_config
from surya_amd.settings import settings
from surya_amd.synth import make_rec_weights, make_line_crops
from util import make_prompts, left_pad_batch
from test_gpu_rec import GRIDS, build, _oracle_run

pytestmark = pytest.mark.gpu

SLOTS = 320
STEPS = 6
NP = len(GRIDS)


def _set(hip_lib, **kw):
    for k, v in kw.items():
        assert hip_lib.surya_set_tuning(k.encode(), C.c_int(v)) == 0, (k, v)


@pytest.fixture(scope="module")
def small320(hip_lib):
    cfg, sd, m = build("REC-SMALL", torch.bfloat16, max_slots=SLOTS)
    tiles, seqs = make_prompts(cfg, GRIDS)
    yield cfg, sd, m, tiles, seqs, tiles.cuda().contiguous()
    m.set_decode_fp8(False)
    _set(hip_lib, mx_big_m_split=-1, mx_big_m_gateup=-1)


@functools.lru_cache(maxsize=1)
def _oracle():
    """fp32 oracle tokens / logits, the oracle's bf16 rounding model and its MXFP8 emulation, once for the six lines."""
    cfg = rec_config("REC-SMALL")
    sd = make_rec_weights(cfg, 0)
    tiles, seqs = make_prompts(cfg, GRIDS)
    toks_ref, _, _, logits_ref = _oracle_run(cfg, sd, tiles, seqs, STEPS + 1)
    ids, am, pos = left_pad_batch(cfg, seqs)
    grids = [(1, h, w) for h, w in GRIDS]
    ob = ro.OracleRecModel(cfg, {k: v.bfloat16() for k, v in sd.items()}, cfg.image_token_id)
    logits_b16 = ro.teacher_forced_logits(ob, ids, tiles, grids, am, pos, toks_ref, cfg.pad_token_id)
    ro.MX_DECODE = True
    try:
        om = ro.OracleRecModel(cfg, sd, cfg.image_token_id)
        logits_mx = ro.teacher_forced_logits(om, ids, tiles, grids, am, pos, toks_ref, cfg.pad_token_id)
    finally:
        ro.MX_DECODE = False
    return toks_ref, logits_ref, logits_b16, logits_mx


def _prefill_replicas(m, tiles_d, seqs):
    """Prompt i goes to every slot s with s % NP == i, one prefill call per replica set (the same call each time, other slots)."""
    for s0 in range(0, SLOTS, NP):
        n = min(NP, SLOTS - s0)
        P = sum(h * w for h, w in GRIDS[:n])
        m.prefill(tiles_d[:P].contiguous(), GRIDS[:n], seqs[:n], list(range(s0, s0 + n)))
    m.set_active(list(range(SLOTS)))


def _teacher_forced(cfg, m, tiles_d, seqs, toks_ref, steps):
    """`steps` decode(1) calls on the oracle's tokens; per step the logits after it [SLOTS, V] (device: entry k belongs to the oracle's
    logits k + 1), and its fused greedy head must agree with those logits."""
    _prefill_replicas(m, tiles_d, seqs)
    slots = list(range(SLOTS))
    out = []
    for step in range(steps):
        m.set_next_tokens(slots, [toks_ref[s % NP][step] if step < len(toks_ref[s % NP]) else cfg.pad_token_id for s in slots])
        m.decode(1)
        tok, score, _ = m.read_outputs(1)
        lg2 = m.last_logits()
        assert lg2.shape[0] == SLOTS
        assert np.array_equal(tok[0, :SLOTS], lg2.argmax(-1).cpu().numpy())
        p = torch.softmax(lg2.double(), -1).max(-1).values.cpu().numpy()
        assert np.allclose(score[0, :SLOTS], p, rtol=1e-4)
        out.append(lg2.clone())
    return out


def _replicas_identical(lg):
    for i in range(NP):
        rows = lg[i::NP].contiguous().view(torch.int32)
        assert torch.equal(rows, rows[:1].expand_as(rows)), i


@pytest.fixture(scope="module")
def default_arm(hip_lib, small320):
    cfg, sd, m, tiles, seqs, tiles_d = small320
    toks_ref, logits_ref, _, _ = _oracle()
    m.set_decode_fp8(True)
    _set(hip_lib, mx_big_m_split=-1, mx_big_m_gateup=-1)
    return _teacher_forced(cfg, m, tiles_d, seqs, toks_ref, min(STEPS, len(logits_ref) - 1))


def test_rec_small_fp8_decode_320_slots_teacher_forced(hip_lib, small320, default_arm):
    cfg = small320[0]
    toks_ref, logits_ref, logits_b16, logits_mx = _oracle()
    pick = [i + NP * (45 + i) for i in range(NP)]           # one replica per prompt, all above row 256
    assert max(pick) < SLOTS and [s % NP for s in pick] == list(range(NP))
    rep = []
    assert len(default_arm) >= 1
    for k, lg_all in enumerate(default_arm):
        step = k + 1                                        # index into the oracle's logits
        assert lg_all.shape[0] == SLOTS
        _replicas_identical(lg_all)
        lg = lg_all[pick].cpu()
        live = [i for i in range(NP) if step < len(toks_ref[i])]
        if not live:
            continue
        ref, emu = logits_ref[step][live], logits_mx[step][live]
        scale = ref.abs().max().item()
        b16_dev = (logits_b16[step][live] - ref).abs().max().item()
        mx_dev = (emu - ref).abs().max().item()
        err_emu = (lg[live] - emu).abs().max().item()
        rep.append((step, err_emu / scale, mx_dev / scale, b16_dev / scale))
        print("fp8 decode REC-SMALL, 320 slots (step, |gpu - emulation|, |emulation - fp32|, |bf16 ref - fp32|) / max|logit|:  %d  %.4f  %.4f  %.4f" % rep[-1])
        assert err_emu <= 2 * b16_dev + 0.5 * mx_dev + 1e-2 * scale, rep[-1]
    assert rep and max(r[2] for r in rep) > 0               # the fp8 path really ran


@pytest.mark.parametrize("gateup", [0, 1, 2])
@pytest.mark.parametrize("split", [0, 2, 3])
def test_rec_small_fp8_320_slots_same_bits_in_every_arm(hip_lib, small320, default_arm, split, gateup):
    cfg, sd, m, tiles, seqs, tiles_d = small320
    toks_ref = _oracle()[0]
    m.set_decode_fp8(True)
    _set(hip_lib, mx_big_m_split=split, mx_big_m_gateup=gateup)
    try:
        got = _teacher_forced(cfg, m, tiles_d, seqs, toks_ref, len(default_arm))
    finally:
        _set(hip_lib, mx_big_m_split=-1, mx_big_m_gateup=-1)
    for step, (a, b) in enumerate(zip(got, default_arm)):
        _replicas_identical(a)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), step


def test_fp8_switch_restores_bf16_results_at_320_slots(hip_lib, small320):
    """bf16 results taken before fp8 was switched on == bf16 results after it was switched off again, exactly -- and the bf16 greedy head
    at 320 rows agrees with the logits it was reduced from (it did not before the lm_head launch above 256 rows was fixed: with a
    column-tile count that is no multiple of 8 -- this model's 218 -- tiles stayed uncomputed and their stale partials were whatever
    ran before, so the two bf16 runs differed in 83 tokens and 1884 scores of 6 x 320)."""
    cfg, sd, m, tiles, seqs, tiles_d = small320

    def run():
        _prefill_replicas(m, tiles_d, seqs)
        m.decode(6)
        t, s, b = m.read_outputs(6)
        return t[:, :SLOTS].copy(), s[:, :SLOTS].copy(), b[:, :SLOTS].copy()

    m.set_decode_fp8(False)
    a = run()
    m.set_decode_fp8(True)
    f = run()
    m.set_decode_fp8(False)
    c = run()
    assert all(np.array_equal(x, y) for x, y in zip(a, c))
    lg = m.last_logits()                                    # of the last bf16 step
    assert lg.shape[0] == SLOTS
    assert np.array_equal(c[0][5], lg.argmax(-1).cpu().numpy())
    live = c[0][5] != cfg.eos_token_id
    live &= c[0][5] != cfg.pad_token_id
    p = torch.softmax(lg.double(), -1).max(-1).values.cpu().numpy()
    assert np.allclose(c[1][5][live], p[live], rtol=1e-4)
    assert not np.array_equal(a[1], f[1])                   # scores differ: another arithmetic ran in between
    assert np.isfinite(f[1]).all() and (f[0] >= 0).all() and (f[0] < cfg.decoder.vocab_size).all()


@pytest.mark.parametrize("mx,kv8", [(True, False), (False, True), (True, True)])
def test_ocr_results_identical_across_slot_counts_fp8(hip_lib, mx, kv8):
    """REC-TINY bf16, 400 lines, one predictor with 512 slots: the OCRResults at recognition_batch_size 64, 256 and 512 are identical field
    for field with MXFP8 decode weights, with the FP8 KV cache, and with both."""
    from surya_amd.recognition.predictor import RecognitionPredictor, RecognitionModelLoader
    n_lines, max_slots = 400, 512
    cfg = rec_config("REC-TINY")
    sd = make_rec_weights(cfg, 0)

    class Loader(RecognitionModelLoader):
        def model(self, device=None, dtype_=None, **caps):
            return super().model("cuda:0", torch.bfloat16, max_slots=max_slots, max_kv_len=192, max_patches=max_slots * 260,
                                 max_prefill_tokens=max_slots * 72)

    class Pred(RecognitionPredictor):
        model_loader_cls = Loader
        batch_size = max_slots

    settings.RECOGNITION_MAX_TOKENS = 24
    try:
        pred = Pred(checkpoint={"config": cfg, "state_dict": sd})
        if mx:
            pred.model.set_decode_fp8(True)
        if kv8:
            pred.model.set_kv_fp8(True)
        assert pred.model.decode_fp8 == mx and pred.model.kv_fp8 == kv8
        crops = make_line_crops(n_lines, seed=11)
        imgs = [Image.fromarray(c) for c in crops]
        boxes = [[[0, 0, im.size[0], im.size[1]]] for im in imgs]
        outs = {}
        for slots in (64, 256, max_slots):
            outs[slots] = [r.model_dump() for r in pred(imgs, bboxes=boxes, recognition_batch_size=slots)]
        assert len(outs[64]) == n_lines and sum(len(r["text_lines"]) for r in outs[64]) == n_lines
        assert outs[256] == outs[64]
        assert outs[max_slots] == outs[64]
        assert len({r["text_lines"][0]["text"] for r in outs[64]}) > n_lines // 4      # the streams are not degenerate
    finally:
        settings.RECOGNITION_MAX_TOKENS = None
