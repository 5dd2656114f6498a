"""GPU: layout and table recognition in float16 (SA_DTYPE_F16), the dtype the reference loads both models in on a GPU
(settings.MODEL_DTYPE; surya/layout/loader.py:27-32, surya/table_rec/loader.py:27-32).

Fixtures: the existing fp32 fixtures (tests/golden/layout_*.pt, table_*.pt) and tests/golden/layout_fp16.pt / table_fp16.pt, recorded by
tools/make_golden_layout_fp16.py from the reference's own modules run in fp16 and bf16 on the same inputs, teacher-forced with the fp32
fixtures' fed tokens: the reference's fp16 outputs and its own fp16 / bf16 deviations from fp32 (e_ref). The reference's fp16 run of
LAYOUT-DEFAULT and TABLE-DEFAULT takes seconds on the CPU, so BOTH are in the fp16 fixtures with e_ref, like the small configurations.

Per configuration, an fp16 engine and a bf16 engine on the same input, against the fp32 fixture:
  (a) err <= max(floor, 1.5 e_ref). floor = the bf16 tolerance of tests/test_gpu_layout.py / test_gpu_table.py divided by 8, for three more
      significand bits: 3.75e-3 x encoder_absmax, 5e-3 x the step's logit scale, 2.5e-3 on boxes. 1.5: the factor of
      tests/test_gpu_ocr_error_fp16.py. The reference's own fp16 runs sit at 1.1-1.6e-3, 1.3-2.4e-3 and 0.7-1.1e-3: inside the floors by two.
  (b) err <= 0.5 x the bf16 engine's error: the feature's point (the reference's own ratio is 0.08-0.17).
  (c) the argmax of every class / classification head equals the fp32 fixture's wherever its top-2 margin exceeds 2 x the bound of (a), and
      at least 0.85 of the positions are that clear. (TABLE-SMALL has near-ties on which the reference's own fp16 run differs from fp32.)
  (d) everything finite.
Then the device-fed decode runs in fp16 (the contract of tests/test_gpu_layout_fed.py), both predictors end to end in fp16 (no host /
device token mismatch from FedRuns; the layout results and the table's first pass equal to the same call at batch_size = 1),
load_predictors(dtype=float16), the constructor's errors and the plain engine creation."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import test_gpu_layout_fed as FED
from surya_amd import _lib as L
from surya_amd.layout.config import layout_config
from surya_amd.layout.model import FedRuns, HipLayoutModel
from surya_amd.synth import make_layout_weights, make_table_weights
from surya_amd.table_rec.config import BOX_PROPERTIES, table_config

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F16, BF16 = torch.float16, torch.bfloat16
FLOOR = {"encoder": 3e-2 / 8, "logits": 4e-2 / 8, "boxes": 2e-2 / 8}
CASES = [("layout", "LAYOUT-TINY"), ("layout", "LAYOUT-SMALL"), ("layout", "LAYOUT-PAD"), ("layout", "LAYOUT-DEFAULT"),
         ("table", "TABLE-TINY"), ("table", "TABLE-SMALL"), ("table", "TABLE-DEFAULT")]


# ------------------------------------------------------------------------------------------------ creation and errors
def test_engine_creation_accepts_f16(hip_lib):
    """surya_layout_create with SA_DTYPE_F16 returns SA_OK (HipLayoutModel raises on any other code) for both families."""
    for cfg, sd in ((layout_config("LAYOUT-TINY"), make_layout_weights), (table_config("TABLE-TINY"), make_table_weights)):
        m = HipLayoutModel(cfg, sd(cfg, 0), dtype=F16, max_batch=2, max_boxes=16)
        assert m.handle and m.c.dtype == L.DTYPE_F16 == 2 and m.dtype == F16
        assert all(w.dtype in (F16, torch.float32) for w in m.weights)


def test_constructor_still_refuses_other_dtypes(hip_lib):
    cfg = layout_config("LAYOUT-TINY")
    with pytest.raises(ValueError, match="float32.*bfloat16.*float16"):
        HipLayoutModel(cfg, make_layout_weights(cfg, 0), dtype=torch.float64)


# ------------------------------------------------------------------------------------------------ the networks
def _fixture(family, name):
    tag = name.split("-")[1].lower()
    g = torch.load(os.path.join(GOLD, f"{family}_{tag}.pt"))
    h = torch.load(os.path.join(GOLD, f"{family}_fp16.pt"))[name]
    if family == "layout":
        ref_c, ref_b = g["class_logits"], g["bbox_logits"]
    else:
        ref_c = torch.cat([g["logits"][k] for k, _, _ in BOX_PROPERTIES if k != "bbox"], -1)
        ref_b = g["logits"]["bbox"]
    return g, h, ref_c.numpy(), ref_b.numpy()


def _run(family, name, dtype, g):
    """(encoder states [B, L / stride, C] fp32, class or property logits [steps, B, n], boxes [steps, B, 6]), teacher-forced with the
    fixture's tokens; the table prompt in ONE pass (surya_layout_prefill: the prompt kernel)."""
    cfg = layout_config(name) if family == "layout" else table_config(name)
    sd = (make_layout_weights if family == "layout" else make_table_weights)(cfg, 0)
    m = HipLayoutModel(cfg, sd, dtype=dtype, max_batch=g["batch"], max_boxes=32 if family == "layout" else 64)
    px = torch.randn(g["batch"], 3, *cfg.encoder.image_size, generator=torch.Generator().manual_seed(g["seed"]))
    m.encode(px.cuda().contiguous())
    enc = m.encoder_states()
    assert enc.dtype == dtype
    enc = enc.float().cpu()[:, ::g["enc_stride"]]
    cls, box = [], []
    if family == "layout":
        tok = np.full((g["batch"], 7), cfg.decoder.bos_token_id, np.int32)
        for step in range(g["steps"]):
            c, b = m.decode_step(tok, step)
            cls.append(c); box.append(b)
            tok = g["fed_tokens"][step].numpy().astype(np.int32)
    else:
        T = g["prompt"].shape[1]
        c, b = m.prefill(g["prompt"].numpy().astype(np.int32))
        cls.append(c); box.append(b)
        for step in range(1, g["steps"]):
            c, b = m.decode_step(g["fed_tokens"][step - 1].numpy().astype(np.int32), T + step - 1)
            cls.append(c); box.append(b)
    return enc, np.stack(cls), np.stack(box), cfg


def _errors(enc, cls, box, g, ref_c, ref_b, scale):
    return {"encoder": float((enc - g["encoder_out"]).abs().max()) / g["encoder_absmax"],
            "logits": float((np.abs(cls - ref_c).max(axis=(1, 2)) / scale).max()), "boxes": float(np.abs(box - ref_b).max())}


def _heads(family, cfg):
    """[(first column, width)] of the heads whose argmax is a class: layout = all logits; table = category, merges, is_header."""
    if family == "layout":
        return [(0, cfg.decoder.label_count)]
    out, o = [], 0
    modes = {k: mode for k, _, mode in BOX_PROPERTIES}
    for k, n in cfg.decoder.head_widths():
        if k == "bbox":
            continue
        if modes[k] == "classification":
            out.append((o, n))
        o += n
    return out


@pytest.mark.parametrize("family,name", CASES, ids=[c[1] for c in CASES])
def test_fp16_engine_against_the_fp32_fixture_and_a_bf16_engine(hip_lib, family, name):
    g, h, ref_c, ref_b = _fixture(family, name)
    scale = np.maximum(1.0, np.abs(ref_c).max(axis=(1, 2)))                     # per step, as tests/test_gpu_layout.py / test_gpu_table.py
    enc, cls, box, cfg = _run(family, name, F16, g)
    assert np.isfinite(cls).all() and np.isfinite(box).all() and bool(torch.isfinite(enc).all())          # (d)
    e16 = _errors(enc, cls, box, g, ref_c, ref_b, scale)
    encb, clsb, boxb, _ = _run(family, name, BF16, g)
    eb = _errors(encb, clsb, boxb, g, ref_c, ref_b, scale)
    e_ref = {"encoder": h["fp16_dev"]["encoder"] / g["encoder_absmax"], "logits": h["fp16_dev"]["logits"], "boxes": h["fp16_dev"]["boxes"]}
    e_refb = {"encoder": h["bf16_dev"]["encoder"] / g["encoder_absmax"], "logits": h["bf16_dev"]["logits"], "boxes": h["bf16_dev"]["boxes"]}
    bound = {k: max(FLOOR[k], 1.5 * e_ref[k]) for k in FLOOR}
    for k in FLOOR:
        print(f"LAYFP16 {name} | {k} | fp16 {e16[k]:.3e} (reference's own fp16 {e_ref[k]:.3e}, bound {bound[k]:.3e}) | bf16 {eb[k]:.3e} "
              f"(reference's own bf16 {e_refb[k]:.3e}) | ratio {e16[k] / eb[k]:.3f}")
    # the engine's fp16 outputs beside the reference's own fp16 outputs (informative: two fp16 implementations, each ~e_ref from fp32)
    d = float((np.abs(cls - h["logits_fp16"].float().numpy()).max(axis=(1, 2)) / scale).max())
    print(f"LAYFP16 {name} | engine fp16 vs reference fp16 logits: {d:.3e} x scale")
    # (c) argmax where the fixture's margin is clear
    clear = agree = total = 0
    for o, n in _heads(family, cfg):
        rc_, gc_ = ref_c[..., o:o + n], cls[..., o:o + n]
        top = np.sort(rc_, -1)
        margin = top[..., -1] - top[..., -2]
        ok = margin > 2 * bound["logits"] * scale[:, None]
        same = gc_.argmax(-1) == rc_.argmax(-1)
        clear += int(ok.sum()); agree += int((same & ok).sum()); total += ok.size
    print(f"LAYFP16 {name} | argmax: {clear} of {total} positions clear ({clear / total:.3f}), {agree} agree")
    for k in FLOOR:
        assert e16[k] <= bound[k], (name, k, e16[k], bound[k])                                            # (a)
        assert e16[k] <= 0.5 * eb[k], (name, k, e16[k], eb[k])                                            # (b)
    assert agree == clear and clear >= 0.85 * total, (name, clear, agree, total)                          # (c)


# ------------------------------------------------------------------------------------------------ device-fed runs
@pytest.mark.parametrize("name", ["LAYOUT-TINY", "LAYOUT-SMALL"])
def test_layout_device_fed_runs_in_fp16(hip_lib, name):
    """tests/test_gpu_layout_fed.py's contract in fp16: records bit-identical to the host-fed loop, fed tokens equal to
    oracle.layout_oracle.fed_token_layout evaluated in torch.float16, the header / footer rule made to fire."""
    cfg = layout_config(name)
    d = cfg.decoder
    B, steps = 5, 22
    m = HipLayoutModel(cfg, make_layout_weights(cfg, 0), dtype=F16, max_batch=8, max_boxes=32)
    px = FED._pixels(cfg, B, 11).cuda().contiguous()
    first = np.full((B, 7), d.bos_token_id, np.int32)
    sizes = np.array([[612, 792], [1200, 300], [90, 2000], [1024, 1024], [777, 333]], np.int32)
    m.encode(px)
    plain = FED._host_fed(m, first, 0, steps, FED._layout_rule(d, F16, None, None))
    classes = np.concatenate([r[0].argmax(-1) for r in plain])
    ids = [int(np.bincount(classes).argmax()), int(classes[-1])]
    m.encode(px)
    want = FED._host_fed(m, first, 0, steps, FED._layout_rule(d, F16, sizes, ids))
    fired = sum(int((r[2][:, 6] != r[0].argmax(-1)).sum()) for r in want)
    assert fired > 0, "the header / footer rule never fired: the test would not cover it"
    m.encode(px)
    FED._set_feedback_with_ids(m, sizes, ids, d.skew_scaler)
    got, pos = [], 0
    for run, n in enumerate((7, 7, 8)):
        m.decode_steps(first if run == 0 else None, pos, n, run & 1)
        cls, box, tok = m.wait_steps(n, run & 1)
        got += [(cls[k], box[k], tok[k]) for k in range(n)]
        pos += n
    for k, (a, b) in enumerate(zip(want, got)):
        assert np.array_equal(a[2], b[2]), (k, a[2], b[2])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), k
    assert all(np.isfinite(r[0]).all() and np.isfinite(r[1]).all() for r in got)


def test_table_device_fed_runs_in_fp16(hip_lib):
    cfg = table_config("TABLE-TINY")
    d = cfg.decoder
    B, T, steps = 6, 3, 20
    m = HipLayoutModel(cfg, make_table_weights(cfg, 0), dtype=F16, max_batch=8, max_boxes=64)
    px = FED._pixels(cfg, 3, 5).cuda().contiguous()
    rng = np.random.default_rng(2)
    prompt = np.concatenate([rng.integers(0, 1025, (B, T, 6)), rng.integers(5, 10, (B, T, 1)), rng.integers(5, 9, (B, T, 1)),
                             rng.integers(1, 4, (B, T, 1)), rng.integers(5, 7, (B, T, 1))], -1).astype(np.int32)

    def rule(cls, box):
        return torch.stack([FED.lo.fed_token_table(torch.from_numpy(cls[j]).to(F16).float(), torch.from_numpy(box[j]).to(F16).float(), d)
                            for j in range(cls.shape[0])]).numpy().astype(np.int32)

    src = [0, 1, 2, 2, 0, 1]
    m.encode(px)
    m.select(src)
    cls, box = m.prefill(prompt)
    first = rule(cls, box)
    want = FED._host_fed(m, first, T, steps, rule)
    m.encode(px)
    m.select(src)
    m.prefill(prompt)
    m.set_feedback()
    got, pos = [], T
    for run, n in enumerate((16, 4)):
        m.decode_steps(first if run == 0 else None, pos, n, run & 1)
        c, b, t = m.wait_steps(n, run & 1)
        got += [(c[k], b[k], t[k]) for k in range(n)]
        pos += n
    for k, (a, b) in enumerate(zip(want, got)):
        assert np.array_equal(a[2], b[2]), (k, a[2], b[2])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), k


def test_layout_graph_replay_equals_eager_in_fp16(hip_lib):
    """The same (rows, steps) shape three times: eager, capture + replay, replay -- identical records; FedRuns then serves them one step at
    a time against the host's fp16 rule."""
    cfg = layout_config("LAYOUT-SMALL")
    d = cfg.decoder
    B = 4
    m = HipLayoutModel(cfg, make_layout_weights(cfg, 0), dtype=F16, max_batch=4, max_boxes=40)
    L.check(m.lib.surya_set_tuning(b"graph", C.c_int(1)), "surya_set_tuning(graph)")
    try:
        px = FED._pixels(cfg, B, 3).cuda().contiguous()
        first = np.full((B, 7), d.bos_token_id, np.int32)
        sizes = np.array([[612, 792]] * B, np.int32)
        runs = []
        for rep in range(3):
            m.encode(px)
            m.set_feedback(sizes)
            rec = []
            for run in range(3):
                m.decode_steps(first if run == 0 else None, run * 8, 8, run & 1)
                rec.append(m.wait_steps(8, run & 1))
            runs.append(rec)
        for rep in (1, 2):
            for x, y in zip(runs[0], runs[rep]):
                assert all(np.array_equal(a, b) for a, b in zip(x, y)), rep
        m.encode(px)
        m.set_feedback(sizes)
        fr = FedRuns(m, 0, 24, 8)
        rule = FED._layout_rule(d, F16, sizes, None)
        tok = first
        flat = [(c[k], b[k], t[k]) for c, b, t in runs[0] for k in range(8)]
        for k in range(24):
            cls, box = fr.step(tok)
            assert np.array_equal(cls, flat[k][0]) and np.array_equal(box, flat[k][1])
            tok = rule(cls, box)
    finally:
        L.check(m.lib.surya_set_tuning(b"graph", C.c_int(0)), "surya_set_tuning(graph)")


# ------------------------------------------------------------------------------------------------ predictors
def test_layout_predictor_fp16_end_to_end(hip_lib):
    """LayoutPredictor(dtype=float16) on synthetic pages, one of them sliced: schema-valid results, FedRuns raises on no step (the host's
    fp16 token rule equals the device's), and the same results at batch_size = 1."""
    from PIL import Image
    from surya_amd.layout.config import ID_TO_LABEL
    from surya_amd.layout.predictor import LayoutModelLoader, LayoutPredictor
    from surya_amd.layout.schema import LayoutResult
    from surya_amd.synth import make_pages
    cfg = layout_config("LAYOUT-SMALL")

    class Loader(LayoutModelLoader):
        def model(self, device=None, dtype=None, max_batch=None):
            return super().model("cuda:0", dtype, max_batch=4)

    class Pred(LayoutPredictor):
        model_loader_cls = Loader
        batch_size = 4

    pred = Pred(checkpoint={"config": cfg, "state_dict": make_layout_weights(cfg, 0)}, dtype=F16)
    assert pred.model.dtype == F16
    pages = [Image.fromarray(p) for p in make_pages(3, 512, seed=3)]
    pages.append(Image.fromarray(np.vstack(make_pages(2, 1024, seed=5))[:1800]))          # 1024 x 1800: two slices of 1200 / 600 rows
    out = pred(pages, top_k=3)
    assert len(out) == 4 and all(isinstance(r, LayoutResult) for r in out)
    assert out[3].sliced and out[3].image_bbox == [0, 0, 1024, 1800] and not out[0].sliced
    labels = set(ID_TO_LABEL.values())
    for r in out:
        for b in r.bboxes:
            assert b.label in labels and len(b.polygon) == 4 and 0 <= b.confidence <= 1 and len(b.top_k) <= 3
            assert np.isfinite(np.array(b.polygon)).all()
    assert sum(len(r.bboxes) for r in out) > 0
    one = pred(pages, batch_size=1, top_k=3)
    assert [r.model_dump() for r in one] == [r.model_dump() for r in out]


def test_table_predictor_fp16_end_to_end(hip_lib):
    """TableRecPredictor(dtype=float16), both passes (rows / columns, then cells): schema-valid, no host / device token mismatch, and the
    first pass of every table equal to the same call at batch_size = 1. (The second pass cannot be compared across batch sizes in any
    dtype: as in the reference, every row prompt carries the columns of ALL tables of its batch, surya/table_rec/__init__.py:190-230.)"""
    from PIL import Image
    from surya_amd.table_rec import predictor as tp
    from surya_amd.table_rec.schema import TableResult
    cfg = table_config("TABLE-TINY")
    sd = make_table_weights(cfg, 0)
    sd["decoder.box_property_heads.category.weight"][5 + 1] *= 3.0      # rows and columns must appear for the second pass to run
    sd["decoder.box_property_heads.category.weight"][5 + 2] *= 2.5
    rng = np.random.default_rng(3)
    pages = [Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)) for h, w in ((200, 320), (128, 128), (90, 400))]
    first_pass = []
    orig = tp.TableRecPredictor.decode_batch_predictions

    def logged(self, rowcol, *a, **k):
        first_pass[-1].extend(rowcol)
        return orig(self, rowcol, *a, **k)

    old = tp.TABLE_REC_MAX_BOXES
    tp.TABLE_REC_MAX_BOXES = 14
    tp.TableRecPredictor.decode_batch_predictions = logged
    try:
        pred = tp.TableRecPredictor(checkpoint={"config": cfg, "state_dict": sd}, dtype=F16)
        assert pred.model.dtype == F16
        first_pass.append([])
        out = pred(pages, batch_size=2)
        first_pass.append([])
        one = pred(pages, batch_size=1)
    finally:
        tp.TABLE_REC_MAX_BOXES = old
        tp.TableRecPredictor.decode_batch_predictions = orig
    for res in (out, one):
        assert len(res) == len(pages) and all(isinstance(r, TableResult) for r in res)
        assert sum(len(r.rows) for r in res) > 0 and sum(len(r.cols) for r in res) > 0 and sum(len(r.cells) for r in res) > 0
        for r, im in zip(res, pages):
            assert r.image_bbox == [0, 0, im.width, im.height] and len(r.unmerged_cells) >= len(r.cells)
            for c in r.cells:
                assert 0 <= c.row_id < max(1, len(r.rows)) and c.colspan >= 1 and np.isfinite(np.array(c.polygon)).all()
    assert len(first_pass[0]) == len(first_pass[1]) == len(pages) and sum(len(p) for p in first_pass[0]) > 0
    assert first_pass[0] == first_pass[1]
    for a, b in zip(out, one):
        assert [x.model_dump() for x in a.rows] == [x.model_dump() for x in b.rows]
        assert [x.model_dump() for x in a.cols] == [x.model_dump() for x in b.cols]


def test_load_predictors_in_float16_constructs_all_five(hip_lib, monkeypatch):
    """load_predictors(dtype=torch.float16) on the smallest configuration of every family: layout, OCR-error, detection and table
    recognition run fp16, the recogniser (which has no fp16 mode; the reference runs it in bf16 on such a GPU) bf16."""
    import surya_amd.models as M
    small = {"LayoutPredictor": "LAYOUT-TINY", "OCRErrorPredictor": "OCRERR-TINY", "RecognitionPredictor": "REC-TINY",
             "DetectionPredictor": "DET-TINY", "TableRecPredictor": "TABLE-TINY"}
    for nm, ck in small.items():
        cls = getattr(M, nm)
        monkeypatch.setattr(M, nm, lambda device=None, dtype=None, _c=cls, _k=ck: _c(_k, device=device, dtype=dtype))
    out = M.load_predictors(device="cuda", dtype=torch.float16)
    assert list(out) == ["layout", "ocr_error", "recognition", "detection", "table_rec"]
    assert {k: p.model.dtype for k, p in out.items()} == {"layout": F16, "ocr_error": F16, "recognition": BF16, "detection": F16, "table_rec": F16}
