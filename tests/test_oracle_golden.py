"""CPU: pin the oracle restatements against fixtures produced by the REAL reference modules
(oracle/make_golden.py, run in the build container where /root/reference exists; fixtures travel to the GPU box)."""
import os

import numpy as np
import pytest
import torch

from oracle import rec_oracle as ro
from oracle import det_oracle as do
from surya_amd.config import rec_config, det_config
from surya_amd.synth import make_rec_weights, make_det_weights, make_pages
from util import make_prompts, left_pad_batch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("attn", ["eager", "sdpa"])
def test_rec_oracle_matches_reference(attn):
    g = torch.load(os.path.join(GOLD, f"rec_tiny_{attn}.pt"))
    cfg = rec_config(g["config"])
    sd = make_rec_weights(cfg, 0)
    grids = [tuple(x) for x in g["grids"]]
    tiles, seqs = make_prompts(cfg, grids, seed=g["seed"])
    thw = [(1, h, w) for h, w in grids]
    emb = ro.image_embeddings(sd, cfg, tiles, thw)
    assert (emb - g["image_embeddings"]).abs().max().item() <= 2e-5 * g["image_embeddings"].abs().max().item()
    ids, am, pos = left_pad_batch(cfg, seqs)
    om = ro.OracleRecModel(cfg, sd, cfg.image_token_id)
    steps = g["tokens"].shape[0]
    logits = ro.teacher_forced_logits(om, ids, tiles, thw, am, pos, [g["tokens"][:, b].tolist() for b in range(len(seqs))],
                                      cfg.pad_token_id)
    # the fixture's streams are free-running greedy: forcing them reproduces the reference's own logits
    for s in range(steps):
        ref = g["logits"][s]
        assert (logits[s] - ref).abs().max().item() <= 1e-4 * ref.abs().max().item(), s
        assert torch.equal(logits[s].argmax(-1), g["tokens"][s])          # token ids bit-exact


def test_rec_small_oracle_matches_reference():
    """REC-SMALL (FULL's op mix: encoder head_dim 80, GQA 5:1, odd MLP width): image embeddings, the reference's top-32
    logits per step (values at the same vocabulary indices), logsumexp and greedy tokens."""
    g = torch.load(os.path.join(GOLD, "rec_small_eager.pt"))
    cfg = rec_config(g["config"])
    sd = make_rec_weights(cfg, 0)
    grids = [tuple(x) for x in g["grids"]]
    tiles, seqs = make_prompts(cfg, grids, seed=g["seed"])
    thw = [(1, h, w) for h, w in grids]
    emb = ro.image_embeddings(sd, cfg, tiles, thw)
    assert (emb - g["image_embeddings"]).abs().max().item() <= 2e-5 * g["image_embeddings"].abs().max().item()
    ids, am, pos = left_pad_batch(cfg, seqs)
    om = ro.OracleRecModel(cfg, sd, cfg.image_token_id)
    steps = g["tokens"].shape[0]
    logits = ro.teacher_forced_logits(om, ids, tiles, thw, am, pos, [g["tokens"][:, b].tolist() for b in range(len(seqs))],
                                      cfg.pad_token_id)
    for s in range(steps):
        tol = 1e-4 * float(g["logits_absmax"][s].max())
        got_top = torch.gather(logits[s], -1, g["logits_top"]["indices"][s])
        assert (got_top - g["logits_top"]["values"][s]).abs().max().item() <= tol, s
        assert (torch.logsumexp(logits[s], -1) - g["logits_lse"][s]).abs().max().item() <= tol, s
        assert torch.equal(logits[s].argmax(-1), g["tokens"][s])          # token ids bit-exact


def test_rec_oracle_greedy_loop_and_boxes_match_reference():
    g = torch.load(os.path.join(GOLD, "rec_tiny_eager.pt"))
    cfg = rec_config(g["config"])
    sd = make_rec_weights(cfg, 0)
    grids = [tuple(x) for x in g["grids"]]
    tiles, seqs = make_prompts(cfg, grids, seed=g["seed"])
    ids, am, pos = left_pad_batch(cfg, seqs)
    om = ro.OracleRecModel(cfg, sd, cfg.image_token_id)
    steps = g["tokens"].shape[0]
    toks, boxes, _, _ = ro.generate(om, ids, tiles, [(1, h, w) for h, w in grids], am, pos, steps, cfg.eos_token_id,
                                    cfg.pad_token_id, cfg.nop_token_id)
    for b in range(len(seqs)):
        n = len(toks[b])
        assert toks[b] == g["tokens"][:n, b].tolist()
        got, ref = np.asarray(boxes[b]), g["bbox_ints"][:n, b].numpy()
        assert np.abs(got - ref).max() <= 1 and (got != ref).mean() < 0.02     # trunc-boundary flips only


def test_det_oracle_matches_reference_bit_for_bit():
    g = torch.load(os.path.join(GOLD, "det_tiny.pt"))
    cfg = det_config(g["config"])
    sd = make_det_weights(cfg, 0)
    x = do.normalise_pages(make_pages(g["n"], g["size"], seed=g["page_seed"]))
    out = do.forward(sd, cfg, x)
    assert torch.equal(out, g["logits"])
    up = do.heatmaps(sd, cfg, x)
    assert torch.equal(up[:, :, ::8, ::8], g["upsampled_sample"])
    assert 0.05 < float(out.std()) and float(out.min()) >= 0 and float(out.max()) <= 1


def test_processor_tiles_match_reference():
    from surya_amd.recognition.processor import SuryaOCRProcessor
    from surya_amd.recognition.tokenizer import OCRTokenizer, ByteMathTokenizer
    g = torch.load(os.path.join(GOLD, "processor_tiles.pt"))
    proc = SuryaOCRProcessor(OCRTokenizer(None, ByteMathTokenizer(256), reserve_special=64))
    tiles, grid = proc.process_and_tile(g["image"].numpy())
    assert (1,) + tuple(grid) == tuple(g["grid_thw"])
    assert np.array_equal(tiles, g["tiles"].numpy())          # fp64 rescale + fp32 normalise + patch order: bit-exact


# ------------------------------------------------------------------ BASELINE-configuration fixtures (make_golden_full.py)
def _subset_rows(g, rows):
    return {k: (v[:, rows] if torch.is_tensor(v) and v.dim() >= 2 and v.shape[1] == g["tokens"].shape[1] else v)
            for k, v in g.items() if k != "logits_top"} | {
        "logits_top": {k: v[:, rows] for k, v in g["logits_top"].items()}}


def _check_teacher_forced(cfg, sd, g, tiles, grids, seqs, steps, tol_rel=1e-4):
    ids, am, pos = left_pad_batch(cfg, seqs)
    om = ro.OracleRecModel(cfg, sd, cfg.image_token_id)
    thw = [(1, h, w) for h, w in grids]
    forced = [g["tokens"][:steps, b].tolist() for b in range(len(seqs))]
    logits = ro.teacher_forced_logits(om, ids, tiles, thw, am, pos, forced, cfg.pad_token_id)
    for s in range(steps):
        tol = tol_rel * float(g["logits_absmax"][s].max())
        got_top = torch.gather(logits[s], -1, g["logits_top"]["indices"][s])
        assert (got_top - g["logits_top"]["values"][s]).abs().max().item() <= tol, s
        assert (torch.logsumexp(logits[s], -1) - g["logits_lse"][s]).abs().max().item() <= tol, s
        assert torch.equal(logits[s].argmax(-1), g["tokens"][s])          # token ids bit-exact


def test_rec_full_bench_lines_oracle_matches_reference():
    """REC-FULL on two of bench.py's own crops (the widest and the narrowest of the 8-line fixture), prefill + 3 steps:
    the oracle reproduces the reference's top-32 logits, logsumexp and greedy tokens on the benchmark configuration."""
    from util import bench_line_inputs
    g = torch.load(os.path.join(GOLD, "rec_full_bench8.pt"))
    cfg = rec_config("REC-FULL")
    sd = make_rec_weights(cfg, 0)
    rows = [0, 7]
    tiles, grids, seqs = bench_line_inputs(cfg, g["lines"], seed=g["line_seed"], pick=[g["pick"][r] for r in rows])
    assert [tuple(x) for x in grids] == [tuple(g["grids"][r]) for r in rows]
    _check_teacher_forced(cfg, sd, _subset_rows(g, rows), tiles, grids, seqs, 4)


def test_rec_full_conditioned_fixture_premise_and_oracle():
    """The conditioned REC-FULL fixture (make_golden_full.py rec8c; used by tests/test_gpu_bf16_parity.py): (1) its premise -- the
    REFERENCE's own bf16 run stays within 2 % of max|logit| of its fp32 run at every step, and the argmax check at margin > 2 tol
    covers >= 90 % of the positions; (2) the oracle reproduces the reference on this weight set too (2 lines, prefill + 3 steps)."""
    from util import bench_line_inputs
    g = torch.load(os.path.join(GOLD, "rec_full_cond8.pt"))
    scale = g["logits_absmax"].amax(-1)
    dev = g["bf16_dev"].amax(-1)
    assert float((dev / scale).max()) <= 0.02
    tol = 2 * dev + 5e-3 * scale
    val = g["logits_top"]["values"]
    covered = ((val[..., 0] - val[..., 1]) > 2 * tol[:, None]).float().mean().item()
    assert covered >= 0.9, covered
    assert int((g["bf16_free_tokens"] == g["tokens"]).all(0).sum()) >= 4        # the reference's own bf16 greedy stream mostly holds
    cfg = rec_config("REC-FULL")
    sd = make_rec_weights(cfg, 0, recipe="conditioned")
    rows = [0, 7]
    tiles, grids, seqs = bench_line_inputs(cfg, g["lines"], seed=g["line_seed"], pick=[g["pick"][r] for r in rows])
    _check_teacher_forced(cfg, sd, _subset_rows(g, rows), tiles, grids, seqs, 4)


def test_rec_small_256_oracle_matches_reference():
    g = torch.load(os.path.join(GOLD, "rec_small_256.pt"))
    cfg = rec_config("REC-SMALL")
    sd = make_rec_weights(cfg, 0)
    grids = [tuple(x) for x in g["grids"]]
    tiles, seqs = make_prompts(cfg, grids, seed=g["seed"])
    rows = list(range(0, 256, 32))                      # lines are independent: 8 of the 256 pin the oracle
    offs = np.cumsum([0] + [h * w for h, w in grids])
    t = torch.cat([tiles[offs[i]:offs[i + 1]] for i in rows])
    _check_teacher_forced(cfg, sd, _subset_rows(g, rows), t, [grids[i] for i in rows], [seqs[i] for i in rows], 6)


def test_det_default_1024_oracle_matches_reference():
    """DET-DEFAULT on page 0 of bench.py's detection leg at 1024^2: the oracle's output is bit-identical to the module's."""
    g = torch.load(os.path.join(GOLD, "det_default_1024.pt"))
    cfg = det_config(g["config"])
    sd = make_det_weights(cfg, 0)
    x = do.normalise_pages(make_pages(g["pages"], g["size"], seed=g["page_seed"])[g["page"]:g["page"] + 1])
    out = do.forward(sd, cfg, x)
    up = do.heatmaps(sd, cfg, x)
    # bit-identical where the CPU runs the fixture's convolution kernels; another CPU's oneDNN kernels sum the 1024^2
    # convolutions in another order, a few float32 ulp on the [0, 1] maps (1.3e-6 with AVX2 kernels instead of AVX-512)
    if not (torch.equal(out, g["logits"]) and torch.equal(up[:, :, ::4, ::4], g["upsampled_sample"])):
        torch.testing.assert_close(out, g["logits"], rtol=0, atol=1e-5)
        torch.testing.assert_close(up[:, :, ::4, ::4], g["upsampled_sample"], rtol=0, atol=1e-5)


def test_host_assembly_and_tokenizer_match_reference_vectors():
    """tests/golden/host_reference.json (oracle/make_golden_host.py: the REAL reference's get_bboxes_text + __call__ tail and
    InnerOCRTokenizer, recorded in the build container) against our batched output assembly and tokenizer -- the travelling form
    of the live cross-checks in tests/test_oracle_vs_reference.py: runs wherever the repo goes."""
    import json
    import math
    import numpy as np
    from surya_amd.recognition.predictor import RecognitionPredictor
    from surya_amd.recognition.processor import SuryaOCRProcessor
    from surya_amd.recognition.tokenizer import ByteMathTokenizer, OCRTokenizer, DEFAULT_SPECIAL_TOKENS
    with open(os.path.join(GOLD, "host_reference.json"), encoding="utf-8") as f:
        g = json.load(f)
    a = g["assembly"]
    tok = OCRTokenizer(None, ByteMathTokenizer(a["tokenizer"]["math_size"]), reserve_special=a["tokenizer"]["reserve_special"])
    pred = object.__new__(RecognitionPredictor)
    pred.processor = SuryaOCRProcessor(tok)
    for words in (False, True):
        idx = [i for i, ln in enumerate(a["lines"]) if ln["return_words"] == words]
        flat = {"polygons": [a["lines"][i]["polygon"] for i in idx], "res_scales": [tuple(a["lines"][i]["res_scale"]) for i in idx],
                "slices": [np.zeros(a["lines"][i]["slice_shape"], np.uint8) for i in idx]}
        items = [(k, k, a["lines"][i]["tokens"], a["lines"][i]["scores"], np.asarray(a["lines"][i]["rows"], np.float32))
                 for k, i in enumerate(idx)]
        got = pred._assemble_batch(flat, items, False, words, a["bbox_size"])
        for k, i in enumerate(idx):
            assert json.loads(json.dumps(got[k].model_dump())) == a["lines"][i]["expected"], i
    t = g["tokenizer"]
    ours = OCRTokenizer(DEFAULT_SPECIAL_TOKENS, ByteMathTokenizer(t["math_size"]))
    for e in t["encode"]:
        assert ours._tokenize_ocr(e["text"]) == e["ids"], e["text"]
    for d in t["decode"]:
        assert ours._decode_ocr(d["ids"]) == d["text"], d["ids"]


# ------------------------------------------------------------------------------------------ layout model family
@pytest.mark.parametrize("name,fixture", [("LAYOUT-TINY", "layout_tiny.pt"), ("LAYOUT-SMALL", "layout_small.pt"), ("LAYOUT-DEFAULT", "layout_default.pt"),
                                          ("LAYOUT-PAD", "layout_pad.pt")])
def test_layout_oracle_matches_reference(name, fixture):
    """oracle/layout_oracle.py (Donut-Swin encoder + ADETR decoder with cross / self attention) against fixtures recorded from the
    reference's own DonutSwinLayoutModel / SuryaLayoutDecoder (oracle/make_golden_layout.py): encoder output, and -- teacher-forced on
    the recorded fed-back tokens -- class logits and sigmoid box outputs of every decode step; the argmax classes are bit-exact."""
    from oracle import layout_oracle as lo
    from oracle.make_golden_layout import layout_pixels
    from surya_amd.layout.config import layout_config
    from surya_amd.synth import make_layout_weights
    g = torch.load(os.path.join(GOLD, fixture))
    cfg = layout_config(name)
    d = cfg.decoder
    sd = make_layout_weights(cfg, 0)
    x = layout_pixels(cfg, g["batch"], g["seed"])
    with torch.inference_mode():
        enc = lo.encoder_forward(sd, cfg.encoder, x)
        assert (enc[:, ::g["enc_stride"]] - g["encoder_out"]).abs().max().item() <= 1e-4 * g["encoder_absmax"]
        st = lo.LayoutDecoderState(d.num_hidden_layers)
        boxes = torch.tensor([[[d.bos_token_id] * 7]] * g["batch"], dtype=torch.long)
        for step in range(g["steps"]):
            box, cls = lo.decoder_forward(sd, d, boxes, enc, step, st)
            ref_c, ref_b = g["class_logits"][step], g["bbox_logits"][step]
            assert (cls[:, -1] - ref_c).abs().max().item() <= 1e-4 * max(1.0, ref_c.abs().max().item()), step
            assert (box[:, -1] - ref_b).abs().max().item() <= 1e-5, step
            assert torch.equal(cls[:, -1].argmax(-1), ref_c.argmax(-1))
            boxes = g["fed_tokens"][step].unsqueeze(1)


# ------------------------------------------------------------------------------------------ table recognition (second caller of the family)
@pytest.mark.parametrize("name,fixture", [("TABLE-TINY", "table_tiny.pt"), ("TABLE-SMALL", "table_small.pt"), ("TABLE-DEFAULT", "table_default.pt")])
def test_table_oracle_matches_reference(name, fixture):
    """oracle/layout_oracle.py with a table_rec config (LabelEmbedding, plain residual flow, one head per box property) against
    fixtures recorded from the reference's own table_rec DonutSwinModel / SuryaTableRecDecoder driven the way its inference loop drives
    them (oracle/make_golden_table.py): encoder output; the multi-token prompt prefill both in ONE call and token by token (what the
    HIP path does -- a causal prefill is the same arithmetic); then teacher-forced single steps. Classification argmaxes are bit-exact."""
    from oracle import layout_oracle as lo
    from oracle.make_golden_table import table_pixels
    from surya_amd.table_rec.config import table_config, BOX_PROPERTIES
    from surya_amd.synth import make_table_weights
    g = torch.load(os.path.join(GOLD, fixture))
    cfg = table_config(name)
    d = cfg.decoder
    sd = make_table_weights(cfg, 0)
    x = table_pixels(cfg, g["batch"], g["seed"])
    with torch.inference_mode():
        enc = lo.encoder_forward(sd, cfg.encoder, x)
        assert (enc[:, ::g["enc_stride"]] - g["encoder_out"]).abs().max().item() <= 1e-4 * g["encoder_absmax"]
        T = g["prompt"].shape[1]
        for token_by_token in (False, True):
            st = lo.LayoutDecoderState(d.num_hidden_layers)
            if token_by_token:
                for t in range(T):
                    box, props = lo.decoder_forward(sd, d, g["prompt"][:, t:t + 1], enc, t, st)
            else:
                box, props = lo.decoder_forward(sd, d, g["prompt"], enc, 0, st)
            pos = T
            for step in range(g["steps"]):
                if step > 0:
                    box, props = lo.decoder_forward(sd, d, g["fed_tokens"][step - 1].unsqueeze(1), enc, pos, st)
                    pos += 1
                for k, _, mode in BOX_PROPERTIES:
                    got = box[:, -1] if k == "bbox" else props[k][:, -1]
                    ref = g["logits"][k][step]
                    assert (got - ref).abs().max().item() <= (1e-5 if k == "bbox" else 1e-4 * max(1.0, ref.abs().max().item())), (k, step)
                    if mode == "classification":
                        assert torch.equal(got.argmax(-1), ref.argmax(-1)), (k, step)


def test_family_host_logic_matches_reference_vectors():
    """tests/golden/family_host_reference.json (oracle/make_golden_family_host.py: the REAL reference's table LabelShaper, processor
    prompts, TableRecPredictor.decode_batch_predictions, layout prediction_to_polygon and ImageSlicer, recorded in the build container)
    against surya_amd.table_rec / surya_amd.layout -- the travelling form of the live cross-checks in tests/test_oracle_vs_reference.py."""
    import copy
    import json
    from types import SimpleNamespace
    import numpy as np
    from PIL import Image
    from surya_amd.layout import predictor as lp, slicer as ls
    from surya_amd.table_rec import predictor as tp
    from surya_amd.table_rec.processor import TableRecProcessor
    from surya_amd.table_rec.shaper import LabelShaper
    with open(os.path.join(GOLD, "family_host_reference.json"), encoding="utf-8") as f:
        g = json.load(f)
    sh = LabelShaper()
    s = g["shaper"]
    conv = sh.convert_polygons_to_bboxes(copy.deepcopy(s["items"]))
    assert [[float(v) for v in c["bbox"]] for c in conv] == s["bboxes"]
    assert sh.dict_to_labels(conv) == s["labels"]
    for e in s["box_to_polygon"]:
        assert sh.convert_bbox_to_polygon(list(e["box"])) == e["polygon"]
    assert {k: list(v) for k, v in sh.component_idx_dict().items()} == s["component_idx"]
    p = g["processor"]
    proc = TableRecProcessor({"height": 128, "width": 128})
    got = proc(images=None, query_items=copy.deepcopy(p["rows"]), columns=copy.deepcopy(p["columns"]), convert_images=False)["input_ids"]
    assert got.tolist() == p["ids_with_columns"]
    got = proc(images=None, query_items=copy.deepcopy(p["rows"]), columns=None, convert_images=False)["input_ids"]
    assert got.tolist() == p["ids_without_columns"]
    proc.image_processor = lambda images: {"pixel_values": []}
    q = [{"polygon": [[0, 0], [w, 0], [w, h], [0, h]], "category": 4, "colspan": 0, "merges": 0, "is_header": 0} for w, h in p["image_sizes"]]
    got = proc(images=[Image.new("RGB", tuple(sz)) for sz in p["image_sizes"]], query_items=q)["input_ids"]
    assert got.tolist() == p["ids_table_queries"]
    o_self = SimpleNamespace(processor=proc)
    for a in g["assembly"]:
        res = tp.TableRecPredictor.decode_batch_predictions(o_self, [copy.deepcopy(a["rowcol"])], copy.deepcopy(a["cells"]), [tuple(a["size"])],
                                                            [0] * len(a["cells"]), sh)
        assert json.loads(json.dumps(res[0].model_dump())) == a["expected"]
    for e in g["layout"]["prediction_to_polygon"]:
        assert lp.prediction_to_polygon(np.asarray(e["token"], np.float32), tuple(e["size"]), 1024, 512) == e["polygon"]
    sl = ls.ImageSlicer({"height": 1500, "width": 1500}, {"height": 1200, "width": 1200})
    for e in g["layout"]["slicer"]:
        im = Image.new("RGB", tuple(e["size"]))
        pieces, positions = sl.slice([im])
        assert sl.slice_count(im) == e["count"] and [list(x) for x in positions] == e["positions"] and [list(x.size) for x in pieces] == e["piece_sizes"]
