"""CPU: the fp16 detector's fixture (tests/golden/det_fp16.pt, tools/make_golden_det_fp16.py) and the fp16 dtype code of the C ABI."""
import os
import re

import torch

from surya_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def test_det_fp16_fixture_describes_the_det_default_1024_input():
    """The 1024^2 fp32 output of det_fp16.pt is det_default_1024.pt's: same page, same weights, same module."""
    g = torch.load(os.path.join(GOLD, "det_fp16.pt"))
    d = torch.load(os.path.join(GOLD, "det_default_1024.pt"))
    p = g["p1024"]
    assert (p["size"], p["pages"], p["page_seed"], p["page"]) == (d["size"], d["pages"], d["page_seed"], d["page"])
    assert torch.equal(p["logits"], d["logits"])


def test_reference_fp16_is_closer_than_bf16():
    """The reference's own fp16 run deviates from its fp32 run by less than a quarter of its bf16 run's deviation, at both sizes."""
    g = torch.load(os.path.join(GOLD, "det_fp16.pt"))
    for key in ("p1024", "p256"):
        p = g[key]
        assert p["logits_fp16"].dtype == torch.float16 and torch.isfinite(p["logits_fp16"]).all()
        dev = (p["logits_fp16"].float() - p["logits"]).abs()
        assert abs(dev.max().item() - p["fp16_dev"]) < 1e-7 and abs(dev.mean().item() - p["fp16_dev_mean"]) < 1e-7
        assert p["fp16_dev"] < p["bf16_dev"] / 4 and p["fp16_dev_mean"] < p["bf16_dev_mean"] / 4, key


def test_dtype_f16_code_matches_header():
    with open(os.path.join(ROOT, "include", "surya_amd.h")) as f:
        hdr = f.read()
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define SA_DTYPE_(\w+) (\d+)", hdr)}
    assert codes == {"F32": L.DTYPE_F32, "BF16": L.DTYPE_BF16, "F16": L.DTYPE_F16}
    assert L.DTYPE_F16 == 2
