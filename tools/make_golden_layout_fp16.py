"""Record the layout / table-recognition fp16 fixtures from the REAL reference modules (build container only; half a minute on the CPU).

    python tools/make_golden_layout_fp16.py

Imports VikParuchuri/surya @ v0.14.6's DonutSwinLayoutModel / SuryaLayoutDecoder and table_rec's DonutSwinModel / SuryaTableRecDecoder
through oracle/ref_shim and the builders of oracle/make_golden_layout.py / make_golden_table.py, loads the seeded synthetic weights
into them and runs them in fp32, fp16 (the reference's GPU dtype, settings.MODEL_DTYPE) and bf16 on the inputs of the existing fp32
fixtures (tests/golden/layout_*.pt, table_*.pt), TEACHER-FORCED with those fixtures' fed_tokens: every dtype sees the same token stream,
so the outputs differ by arithmetic alone.

Per configuration (LAYOUT-TINY / SMALL / PAD / DEFAULT, TABLE-TINY / SMALL / DEFAULT): the reference's own fp16 class / property logits and
boxes (kept in fp16, the modules' output dtype) and, for fp16 and bf16, the deviation from the fp32 run in the units of
tests/test_gpu_layout.py / test_gpu_table.py -- encoder: max |d| (the fixture's encoder_absmax scales it), logits: max over steps of
max |d| / scale of the step, boxes: max |d|. The fp32 run must reproduce the existing fixture (asserted). No weights, no encoder tensors:
about ten kilobytes each.
-> tests/golden/layout_fp16.pt, tests/golden/table_fp16.pt."""
from __future__ import annotations

import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch

GOLD = os.path.join(ROOT, "tests", "golden")
DTYPES = (("fp32", torch.float32), ("fp16", torch.float16), ("bf16", torch.bfloat16))


def _load(enc, dec, sd):
    """The fp32 weights every time: a round trip through a 16-bit dtype would round them."""
    enc.float().load_state_dict({k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}, strict=False)
    dec.float().load_state_dict({k[len("decoder."):]: v for k, v in sd.items() if k.startswith("decoder.")}, strict=False)


def run_layout(enc, dec, dec_cfg, cfg, g, x, dt):
    """make_golden_layout.record's loop with the fixture's tokens fed instead of the run's own."""
    d = cfg.decoder
    B = g["batch"]
    with torch.inference_mode():
        h = enc(pixel_values=x.to(dt))[0]
        dec.model._setup_cache(dec_cfg, B, "cpu", dt)
        boxes = torch.tensor([[[d.bos_token_id] * 7] + [[d.pause_token_id] * 7] * d.pause_token_count] * B, dtype=torch.long)
        pos = torch.ones_like(boxes[0, :, 0]).cumsum(0) - 1
        cls, box = [], []
        for step in range(g["steps"]):
            out = dec(input_boxes=boxes, encoder_hidden_states=h, cache_position=pos, use_cache=True, prefill=(step == 0))
            pos = pos[-1:] + 1
            cls.append(out.class_logits[:, -1, :].clone())
            box.append(out.bbox_logits[:, -1, :].clone())
            boxes = g["fed_tokens"][step].unsqueeze(1).to(torch.long)
    return h, torch.stack(cls), torch.stack(box)


def run_table(enc, dec, dec_cfg, cfg, g, x, dt):
    from surya_amd.table_rec.config import BOX_PROPERTIES
    B = g["batch"]
    heads = [k for k, _, _ in BOX_PROPERTIES if k != "bbox"]
    with torch.inference_mode():
        h = enc(pixel_values=x.to(dt)).last_hidden_state
        dec.model._setup_cache(dec_cfg, B, "cpu", dt)
        cur = g["prompt"]
        pos = torch.ones_like(cur[0, :, 0], dtype=torch.int64).cumsum(0) - 1
        cls, box = [], []
        for step in range(g["steps"]):
            out = dec(input_ids=cur, encoder_hidden_states=h, cache_position=pos, use_cache=True, prefill=(step == 0))
            pos = pos[-1:] + 1
            last = out["box_property_logits"]
            cls.append(torch.cat([last[k][:, -1, :] for k in heads], -1).clone())          # category | merges | colspan | is_header
            box.append(last["bbox"][:, -1, :].clone())
            cur = g["fed_tokens"][step].unsqueeze(1).to(torch.long)
    return h, torch.stack(cls), torch.stack(box)


def fixture_outputs(family, g):
    """(class or property logits [steps, B, n], boxes [steps, B, 6]) of an fp32 fixture, stacked as the engine's head slot stacks them."""
    if family == "layout":
        return g["class_logits"], g["bbox_logits"]
    from surya_amd.table_rec.config import BOX_PROPERTIES
    return torch.cat([g["logits"][k] for k, _, _ in BOX_PROPERTIES if k != "bbox"], -1), g["logits"]["bbox"]


def record(family, name):
    from oracle import make_golden_layout as ML, make_golden_table as MT
    if family == "layout":
        from surya_amd.layout.config import layout_config as config
        from surya_amd.synth import make_layout_weights as weights
        build, run, pixels = ML.build_reference_layout, run_layout, ML.layout_pixels
    else:
        from surya_amd.table_rec.config import table_config as config
        from surya_amd.synth import make_table_weights as weights
        build, run, pixels = MT.build_reference_table, run_table, MT.table_pixels
    g = torch.load(os.path.join(GOLD, f"{family}_{name.split('-')[1].lower()}.pt"))
    cfg = config(name)
    sd = weights(cfg, 0)
    enc, dec, dec_cfg = build(cfg, sd)
    x = pixels(cfg, g["batch"], g["seed"])
    ref_c, ref_b = fixture_outputs(family, g)
    scale = ref_c.abs().amax((1, 2)).clamp(min=1.0)                  # per step: max(1, max |fp32 logits|), the tests' logit scale
    out = {"config": name, "steps": g["steps"], "batch": g["batch"]}
    f32 = None
    for tag, dt in DTYPES:
        _load(enc, dec, sd)
        enc.to(dt), dec.to(dt)
        t0 = time.time()
        h, c, b = run(enc, dec, dec_cfg, cfg, g, x, dt)
        print(f"{name} {tag}: reference encoder + {g['steps']} teacher-forced steps, batch {g['batch']}: {time.time() - t0:.1f}s", flush=True)
        assert torch.isfinite(h.float()).all() and torch.isfinite(c.float()).all() and torch.isfinite(b.float()).all(), (name, tag)
        if tag == "fp32":
            f32 = (h, c, b)
            assert torch.allclose(h[:, ::g["enc_stride"]], g["encoder_out"], atol=1e-5 * g["encoder_absmax"]), "fp32 run != fixture (encoder)"
            assert torch.allclose(c, ref_c, atol=1e-4) and torch.allclose(b, ref_b, atol=1e-5), "fp32 run != fixture (decoder)"
            continue
        dev = {"encoder": float((h.float() - f32[0]).abs().max()),
               "logits": float(((c.float() - f32[1]).abs().amax((1, 2)) / scale).max()),
               "boxes": float((b.float() - f32[2]).abs().max())}
        out[tag + "_dev"] = dev
        print(f"{name} {tag}: encoder {dev['encoder'] / g['encoder_absmax']:.2e} x absmax, logits {dev['logits']:.2e} x scale, "
              f"boxes {dev['boxes']:.2e}", flush=True)
        if tag == "fp16":
            out["logits_fp16"], out["boxes_fp16"] = c.clone(), b.clone()
    return out


def main():
    from oracle import ref_shim
    ref_shim.install_layout()
    lay = {n: record("layout", n) for n in ("LAYOUT-TINY", "LAYOUT-SMALL", "LAYOUT-PAD", "LAYOUT-DEFAULT")}
    tab = {n: record("table", n) for n in ("TABLE-TINY", "TABLE-SMALL", "TABLE-DEFAULT")}
    for fname, g in (("layout_fp16.pt", lay), ("table_fp16.pt", tab)):
        path = os.path.join(GOLD, fname)
        torch.save(g, path)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
