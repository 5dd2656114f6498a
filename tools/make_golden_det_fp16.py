"""Record the text detector's fp16 fixture from the REAL reference module (build container only; takes minutes on the CPU).

    python tools/make_golden_det_fp16.py

Imports VikParuchuri/surya @ v0.14.6's EfficientViTForSemanticSegmentation through oracle/ref_shim, loads the seeded synthetic
DET-DEFAULT weights (surya_amd.synth.make_det_weights(cfg, 0)) into it and runs it in fp32, fp16 (the reference's GPU default
dtype, settings.MODEL_DTYPE) and bf16 on two inputs:

  1024^2  page 0 of make_pages(16, 1024, seed=1234): the input of det_default_1024.pt (bench.py's detection leg);
  256^2   both pages of make_pages(2, 256, seed=5).

Per input it stores the fp32 logits, the fp16 logits (kept in fp16: the module's output dtype, so nothing is lost) and the reference's
own deviations from fp32: fp16_dev / fp16_dev_mean (max / mean |fp16 - fp32|) and bf16_dev / bf16_dev_mean; the maps up-sampled x4 are
F.interpolate of the stored logits (detection/__init__.py:121-129), which a test recomputes. -> tests/golden/det_fp16.pt (no weights,
~0.85 MiB: the 1024^2 fp32 logits must stay fp32, they equal det_default_1024.pt's).
"""
from __future__ import annotations

import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch

GOLD = os.path.join(ROOT, "tests", "golden")


def reference_module(cfg):
    from surya.detection.model.config import EfficientViTConfig
    from surya.detection.model.encoderdecoder import EfficientViTForSemanticSegmentation
    from surya_amd.synth import make_det_weights
    rc = EfficientViTConfig(widths=cfg.widths, depths=cfg.depths, head_dim=cfg.head_dim,
                            decoder_layer_hidden_size=cfg.decoder_layer_hidden_size, decoder_hidden_size=cfg.decoder_hidden_size,
                            num_labels=cfg.num_labels)
    m = EfficientViTForSemanticSegmentation(rc).eval()
    m.load_state_dict(make_det_weights(cfg, 0), strict=True)
    return m, make_det_weights(cfg, 0)


def record(m, sd, pages, size):
    from oracle.det_oracle import normalise_pages
    from surya.detection.processor import SegformerImageProcessor            # the reference's own rescale + normalise
    x = normalise_pages(pages)
    rp = SegformerImageProcessor(size={"height": size, "width": size})
    for i, p in enumerate(pages):
        assert np.array_equal(rp(p)["pixel_values"][0], x[i].numpy()), "normalise_pages != reference processor"
    out = {}
    with torch.inference_mode():
        for name, dt in (("fp32", torch.float32), ("fp16", torch.float16), ("bf16", torch.bfloat16)):
            m.float().load_state_dict(sd, strict=True)           # the fp32 weights every time: a bf16 round trip would round them
            t0 = time.time()
            out[name] = m.to(dt)(pixel_values=x.to(dt)).logits
            print(f"{size}^2 x {len(pages)} {name} reference: {time.time() - t0:.1f}s", flush=True)
        ref = out["fp32"]
    d16 = (out["fp16"].float() - ref).abs()
    db = (out["bf16"].float() - ref).abs()
    assert torch.isfinite(out["fp16"]).all()
    g = {"size": size, "n_pages": len(pages), "logits": ref.clone(), "logits_fp16": out["fp16"].clone(),
         "fp16_dev": float(d16.max()), "fp16_dev_mean": float(d16.mean()),
         "bf16_dev": float(db.max()), "bf16_dev_mean": float(db.mean())}
    print(f"{size}^2: fp16 dev {g['fp16_dev']:.3e} / {g['fp16_dev_mean']:.3e}, bf16 dev {g['bf16_dev']:.3e} / {g['bf16_dev_mean']:.3e}",
          flush=True)
    return g


def main():
    from oracle import ref_shim
    ref_shim.install()
    from surya_amd.config import det_config
    from surya_amd.synth import make_pages
    cfg = det_config("DET-DEFAULT")
    m, sd = reference_module(cfg)
    g = {"config": "DET-DEFAULT",
         "p1024": {**record(m, sd, make_pages(16, 1024, seed=1234)[:1], 1024), "pages": 16, "page_seed": 1234, "page": 0},
         "p256": {**record(m, sd, make_pages(2, 256, seed=5), 256), "pages": 2, "page_seed": 5, "page": 0}}
    path = os.path.join(GOLD, "det_fp16.pt")
    torch.save(g, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
