"""GPU: the recogniser in float16 (SA_DTYPE_F16; RecModel<fp16_t>, csrc/rec_model_f16.hip) against the real reference.

tests/golden/rec_fp16.pt (tools/make_golden_rec_fp16.py) holds the reference's OWN fp16-vs-fp32 logit deviation on the conditioned REC-FULL
weights and bench.py's crops -- the inputs of rec_full_cond8.pt / rec_full_cond256.pt, whose fp32 logits are the yardstick. The rules are
those of tests/test_gpu_bf16_parity.py with the free constants divided by 8 (fp16 has three more significand bits than bf16):

  (a) teacher-forced fp16 logits (top logits + logsumexp) within 2 x fp16_dev (worst line of the step) + (5e-3 / 8) x max|logit| at every step;
  (b) the worst fp16 error at most half the worst error of a bf16 engine on the same inputs (the reference's own ratio is 0.15);
  (c) the argmax equals the reference token wherever the reference's top-2 margin exceeds 2 x that tolerance, over >= 0.9 of the positions;
  (d) everything finite;
  free-running: a line leaves the fp32 stream only at a near-tie onto the runner-up, and no fewer lines stay on it than with bf16.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from PIL import Image

from surya_amd import _lib as L
from surya_amd.config import rec_config
from surya_amd.settings import settings
from surya_amd.synth import make_rec_weights, make_line_crops
from util import bench_line_inputs, make_prompts
from test_gpu_baseline_parity import _subset, _check_inputs
from test_gpu_rec import GRIDS

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLOOR = 5e-3 / 8
SURE_SHARE_256 = 0.9819     # 12066 of 12 288 positions; measured when tests/golden/rec_fp16.pt was recorded (tools/make_golden_rec_fp16.py prints it)


def _build(cfg_name, sd, dtype, slots, max_kv=160, prefill=None):
    from surya_amd.recognition.model import HipRecModel
    cfg = rec_config(cfg_name)
    return cfg, HipRecModel(cfg, sd, image_token_id=cfg.image_token_id, pad_token_id=cfg.pad_token_id, eos_token_id=cfg.eos_token_id,
                            dtype=dtype, device="cuda:0", max_slots=slots, max_kv_len=max_kv, max_patches=max(4096, slots * 256),
                            max_prefill_tokens=prefill or slots * 72)


@pytest.fixture(scope="module")
def cond_sd():
    return make_rec_weights(rec_config("REC-FULL"), 0, recipe="conditioned")


@pytest.fixture(scope="module")
def bench_inputs():
    return bench_line_inputs(rec_config("REC-FULL"), 256, seed=1234)


@pytest.fixture(scope="module")
def gold():
    return torch.load(os.path.join(GOLD, "rec_fp16.pt"))


@pytest.fixture(scope="module")
def engines8(hip_lib, cond_sd):
    return {dt: _build("REC-FULL", cond_sd, dt, 8)[1] for dt in (torch.float16, torch.bfloat16)}


@pytest.fixture(scope="module")
def engines256(hip_lib, cond_sd):
    return {dt: _build("REC-FULL", cond_sd, dt, 256)[1] for dt in (torch.float16, torch.bfloat16)}


# --------------------------------------------------------------------------------------------------------------------- creation
def test_fp16_engine_is_created_and_refuses_what_it_lacks(hip_lib):
    sd = make_rec_weights(rec_config("REC-TINY"), 0)
    cfg, m = _build("REC-TINY", sd, torch.float16, 8, max_kv=256, prefill=1024)
    assert m.dtype == torch.float16 and m.c.dtype == L.DTYPE_F16 and all(t.dtype in (torch.float16, torch.float32) for t in m.weights)
    with pytest.raises(ValueError, match="float32.*bfloat16.*float16"):
        _build("REC-TINY", sd, torch.float64, 8)
    with pytest.raises(ValueError, match="bfloat16 models only"):
        m.set_decode_fp8(True)
    with pytest.raises(ValueError, match="bfloat16 models only"):
        m.set_kv_fp8(True)
    # the C ABI itself: SA_ERR_UNSUPPORTED, as on an fp32 engine
    assert hip_lib.surya_rec_set_kv_fp8(m.handle, C.c_int(1)) == L.SA_ERR_UNSUPPORTED
    dummy = (C.c_void_p * 1)(C.c_void_p(m.weights[0].data_ptr()))
    assert hip_lib.surya_rec_set_mx_weights(m.handle, dummy, C.c_int(1)) == L.SA_ERR_UNSUPPORTED
    tiles, seqs = make_prompts(cfg, GRIDS)
    out = m.encode_only(tiles.cuda(), GRIDS)
    assert out.dtype == torch.float16 and torch.isfinite(out.float()).all()


# --------------------------------------------------------------------------------------------------------------- teacher-forced
def _tol(g, dev16):
    scale = g["logits_absmax"].amax(-1)
    assert float((dev16.amax(-1) / scale).max()) <= 0.05 / 8, "fixture unfit: the reference's own fp16 run deviates too far from its fp32 run"
    return 2 * dev16.amax(-1) + FLOOR * scale, scale


def _teacher_forced(m, g, tiles, grids, seqs):
    """Per-step worst |error| on the fixture's top logits and the logsumexp, the argmax of every step, finiteness."""
    n, steps = len(seqs), g["tokens"].shape[0]
    slots = list(range(n))
    m.prefill(tiles.cuda().contiguous(), grids, seqs, slots)
    m.set_active(slots)
    errs, arg, finite = [], [], True
    for step in range(steps):
        lg = m.last_logits()
        finite = finite and bool(torch.isfinite(lg).all())
        lg = lg.cpu()
        idx, val = g["logits_top"]["indices"][step], g["logits_top"]["values"][step]
        errs.append(max((torch.gather(lg, -1, idx) - val).abs().max().item(), (torch.logsumexp(lg, -1) - g["logits_lse"][step]).abs().max().item()))
        arg.append(lg.argmax(-1))
        if step + 1 < steps:
            m.set_next_tokens(slots, g["tokens"][step].tolist())
            m.decode(1)
    return torch.tensor(errs), torch.stack(arg), finite


def _check_teacher_forced(tag, engines, g, dev16, tiles, grids, seqs, coverage_floor, ratio_bound):
    tol, scale = _tol(g, dev16)
    e16, arg16, fin16 = _teacher_forced(engines[torch.float16], g, tiles, grids, seqs)
    if ratio_bound is not None:
        eb, _, finb = _teacher_forced(engines[torch.bfloat16], g, tiles, grids, seqs)
    else:
        eb, finb = torch.full_like(e16, float("nan")), True
    val = g["logits_top"]["values"]
    sure = (val[..., 0] - val[..., 1]) > 2 * tol[:, None]
    checked, positions = int(sure.sum()), sure.numel()
    mism = int((arg16[sure] != g["tokens"][sure]).sum())
    w16, wb = float((e16 / scale).max()), float((eb / scale).max())
    print(f"REC-FULL conditioned, {tag}, teacher-forced vs the reference's fp32 run: fp16 worst logit error {w16:.5f} x max (reference's own fp16 run: "
          f"{float((dev16.amax(-1) / scale).max()):.5f}), bf16 engine {wb:.5f} x max, ratio {w16 / wb:.3f}; worst error / tolerance {float((e16 / tol).max()):.3f}; "
          f"argmax checked at {checked}/{positions} positions, {mism} mismatches")
    assert fin16 and finb                                                                         # (d)
    assert (e16 <= tol).all(), [(s, float(e16[s]), float(tol[s])) for s in range(len(tol)) if e16[s] > tol[s]]     # (a)
    if ratio_bound is not None:
        assert w16 <= ratio_bound * wb, (w16, wb)                                                 # (b)
    assert checked >= coverage_floor * positions, (checked, positions)                            # (c)
    assert mism == 0, (mism, checked)


def test_cond8_fp16_teacher_forced(engines8, bench_inputs, gold):
    g = torch.load(os.path.join(GOLD, "rec_full_cond8.pt"))
    tiles, grids, seqs = _subset(bench_inputs, g["pick"])
    _check_inputs(g, tiles, grids)
    _check_teacher_forced("8 bench crops x 48 tokens", engines8, g, gold["cond8"]["fp16_dev"], tiles, grids, seqs, 0.9, 0.5)


def test_cond256_fp16_teacher_forced(engines256, bench_inputs, gold):
    """All 256 bench lines in one batch: the M = 256 tiles, split-K with 4 row tiles, the 256 x 320 lm_head. Coverage floor of the argmax check:
    the fixture alone (margins of rec_full_cond256.pt against 2 x the tolerance built on rec_fp16.pt's fp16_dev) puts 12066 of the
    12 288 positions (0.9819, SURE_SHARE_256) above 2 x tol; the floor is that minus one point."""
    g = torch.load(os.path.join(GOLD, "rec_full_cond256.pt"))
    tiles, grids, seqs = bench_inputs
    _check_inputs(g, tiles, grids)
    assert abs(gold["cond256"]["sure_share"] - SURE_SHARE_256) < 5e-4
    _check_teacher_forced("256 bench crops x 48 tokens", engines256, g, gold["cond256"]["fp16_dev"], tiles, grids, seqs, SURE_SHARE_256 - 0.01, None)


# ----------------------------------------------------------------------------------------------------------------- free-running
def _free_running(m, g, tol, tiles, grids, seqs):
    """Greedy decoding against the fixture's fp32 stream: a line may leave it only at a near-tie (top-2 margin of the reference <= 2 x tol at
    the first difference) and onto the reference's runner-up. Returns (lines identical, first differences, tokens [steps, n])."""
    n, steps = len(seqs), g["tokens"].shape[0]
    slots = list(range(n))
    m.prefill(tiles.cuda().contiguous(), grids, seqs, slots)
    tok, _, _ = m.read_outputs(1)
    got = [tok[0][slots].copy()]
    m.set_active(slots)
    done = 1
    while done < steps:
        k = min(8, steps - done)
        m.decode(k)
        tok, _, _ = m.read_outputs(k)
        got += [tok[s][slots].copy() for s in range(k)]
        done += k
    got = np.stack(got)
    same = got == g["tokens"].numpy()
    identical, first = 0, []
    for i in range(n):
        if same[:, i].all():
            identical += 1
            continue
        s = int(np.nonzero(~same[:, i])[0][0])
        first.append((i, s))
        val, idx = g["logits_top"]["values"][s, i], g["logits_top"]["indices"][s, i]
        margin = float(val[0] - val[1])
        assert margin <= 2 * float(tol[s]), f"line {i} leaves the reference stream at step {s} where its top-2 margin is {margin:.4f} > 2 tol {2 * float(tol[s]):.4f}"
        assert int(got[s, i]) == int(idx[1]), f"line {i} step {s}: token {got[s, i]} is not the reference's runner-up {int(idx[1])}"
    return identical, first, got


def _check_free_running(tag, engines, g, gd, tiles, grids, seqs):
    n, steps = len(seqs), g["tokens"].shape[0]
    tol16, _ = _tol(g, gd["fp16_dev"])
    scale = g["logits_absmax"].amax(-1)
    tolb = 2 * g["bf16_dev"].amax(-1) + 5e-3 * scale                      # the bf16 engine by its own rule (tests/test_gpu_bf16_parity.py)
    id16, first16, got16 = _free_running(engines[torch.float16], g, tol16, tiles, grids, seqs)
    idb, _, _ = _free_running(engines[torch.bfloat16], g, tolb, tiles, grids, seqs)
    ref16 = gd["fp16_free_tokens"].numpy()
    print(f"REC-FULL conditioned, {tag}, free-running over {steps} tokens: fp16 {id16}/{n} lines identical to the reference's fp32 stream "
          f"(bf16 engine: {idb}/{n}; the reference's own fp16 run: {int((ref16 == g['tokens'].numpy()).all(0).sum())}/{n}, its bf16 run: "
          f"{int((g['bf16_free_tokens'] == g['tokens']).all(0).sum())}/{n}); {int((got16 == ref16).all(0).sum())}/{n} identical to the reference's fp16 stream; "
          f"first differences (line, step): {first16}")
    assert id16 >= idb, (id16, idb)


def test_cond8_fp16_free_running(engines8, bench_inputs, gold):
    g = torch.load(os.path.join(GOLD, "rec_full_cond8.pt"))
    tiles, grids, seqs = _subset(bench_inputs, g["pick"])
    _check_free_running("8 bench crops", engines8, g, gold["cond8"], tiles, grids, seqs)


def test_cond256_fp16_free_running(engines256, bench_inputs, gold):
    g = torch.load(os.path.join(GOLD, "rec_full_cond256.pt"))
    tiles, grids, seqs = bench_inputs
    assert len(seqs) == 256 and g["tokens"].shape[0] >= 48
    _check_free_running("256 bench crops", engines256, g, gold["cond256"], tiles, grids, seqs)


# ------------------------------------------------------------------------------------------------------------ engine mechanics
def test_fp16_multi_step_decode_matches_single_steps(hip_lib):
    """decode(8) against 8 x decode(1) on REC-SMALL at 16 slots: the device-resident greedy loop (the head's fused next-step embedding) in fp16."""
    sd = make_rec_weights(rec_config("REC-SMALL"), 0)
    cfg, m = _build("REC-SMALL", sd, torch.float16, 16, max_kv=256, prefill=2048)
    grids = (GRIDS * 3)[:16]
    tiles, seqs = make_prompts(cfg, grids)
    slots = list(range(16))
    m.prefill(tiles.cuda(), grids, seqs, slots)
    m.set_active(slots)
    single = []
    for _ in range(8):
        m.decode(1)
        t, s, b = m.read_outputs(1)
        single.append((t[0].copy(), s[0].copy(), b[0].copy()))
    m.prefill(tiles.cuda(), grids, seqs, slots)
    m.set_active(slots)
    m.decode(8)
    t, s, b = m.read_outputs(8)
    for k in range(8):
        assert np.array_equal(t[k], single[k][0]) and np.array_equal(b[k], single[k][2]) and np.array_equal(s[k], single[k][1]), k
    assert np.isfinite(s[:8]).all() and len({tuple(t[:8, i]) for i in range(16)}) > 1


def _fp16_predictor(max_slots, max_tokens):
    from surya_amd.recognition.predictor import RecognitionPredictor, RecognitionModelLoader
    cfg = rec_config("REC-TINY")
    sd = make_rec_weights(cfg, 0)

    class Loader(RecognitionModelLoader):
        def model(self, device=None, dtype=None, **caps):                 # the dtype BasePredictor hands down
            return super().model("cuda:0", dtype, max_slots=max_slots, max_kv_len=192, max_patches=max_slots * 260, max_prefill_tokens=max_slots * 72)

    class Pred(RecognitionPredictor):
        model_loader_cls = Loader
        batch_size = max_slots

    settings.RECOGNITION_MAX_TOKENS = max_tokens
    assert Pred(checkpoint={"config": cfg, "state_dict": sd}).model.dtype == torch.bfloat16      # dtype=None still gives bf16
    return Pred(checkpoint={"config": cfg, "state_dict": sd}, dtype=torch.float16)


def test_fp16_ocr_results_identical_across_slot_counts(hip_lib):
    """REC-TINY, 300 synthetic lines through RecognitionPredictor(dtype=float16) -- device pre-processing, look-ahead encoding, the decode regime
    above 256 slots -- at recognition_batch_size 64 and 320: identical OCRResults, computed in fp16."""
    try:
        pred = _fp16_predictor(320, 24)
        assert pred.model.dtype == torch.float16 and pred.device_preprocess
        imgs = [Image.fromarray(c) for c in make_line_crops(300, seed=11)]
        boxes = [[[0, 0, im.size[0], im.size[1]]] for im in imgs]
        a = [r.model_dump() for r in pred(imgs, bboxes=boxes, recognition_batch_size=64)]
        b = [r.model_dump() for r in pred(imgs, bboxes=boxes, recognition_batch_size=320)]
        assert len(a) == 300 and sum(len(r["text_lines"]) for r in a) == 300
        assert a == b
        assert len({r["text_lines"][0]["text"] for r in a}) > 300 // 4          # the streams are not degenerate
        tiles, _ = make_prompts(pred.model.cfg, GRIDS)
        assert pred.model.encode_only(tiles.cuda(), GRIDS).dtype == torch.float16
    finally:
        settings.RECOGNITION_MAX_TOKENS = None


def test_fp16_streamed_detect_recognise_equals_the_serial_call(hip_lib):
    """RecognitionPredictor(dtype=float16)(images, det_predictor=...): the streamed call returns the serial call's OCRResults."""
    from surya_amd.synth import make_pages_with_lines
    from test_gpu_predictors import _det_with_drawn_rows
    try:
        pages_np, rows = make_pages_with_lines(5, 256, seed=99)
        pages = [Image.fromarray(p) for p in pages_np]
        det = _det_with_drawn_rows(pages, rows, 256, 2)
        rec = _fp16_predictor(16, 7)
        rec.stream_detection = False
        serial = rec(pages, det_predictor=det)
        rec.stream_detection = True
        streamed = rec(pages, det_predictor=det)
        assert rec.last_timing.get("streamed") == 1.0 and sum(len(r.text_lines) for r in serial) > 16
        assert [r.model_dump() for r in serial] == [r.model_dump() for r in streamed]
    finally:
        settings.RECOGNITION_MAX_TOKENS = None
