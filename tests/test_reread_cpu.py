"""CPU: re-reading doubtful lines (RecognitionPredictor.reread, recognition/reread.py) and the host side of the contrast adjustment,
without a GPU: autocontrast_crop against Pillow's own function, the choice rule and the gate on hand-made readings, variant construction
(rolled quads, np.rot90), validation and every refusal, the second pass's admission on the fake model of the encoded / rank tests, the
serialised form with `reread = None`, and the new entry's bindings against the header."""
import os
import re

import numpy as np
import pytest
from PIL import Image, ImageOps

from surya_amd import _lib as L
from surya_amd.common.imageops import autocontrast_crop, fill_poly_mask, quad_homography, quad_ok, quad_size, warp_quad
from surya_amd.recognition import reread as rr
from surya_amd.recognition.reread import Reread
from surya_amd.recognition.schema import LineReading, OCRResult, TextLine
from test_encoded_cpu import BOXES3, IMAGES, _enc_pred, _stream_of
from test_rank_cpu import fake_loop_settings, proc  # noqa: F401

POLY = [[0, 0], [4, 0], [4, 2], [0, 2]]


# --------------------------------------------------------------------------------------------------- the contrast adjustment
def pillow(crop, mask, cutoff):
    m = None if mask is None else Image.fromarray((np.asarray(mask) != 0).astype(np.uint8) * 255)
    return np.asarray(ImageOps.autocontrast(Image.fromarray(crop), cutoff=cutoff, mask=m, preserve_tone=True))


def test_autocontrast_crop_equals_pillow():
    rng = np.random.default_rng(27)
    crops = []
    for t in range(320):
        h, w = int(rng.integers(1, 41)), int(rng.integers(1, 81))
        a = int(rng.integers(0, 256))
        b = int(rng.integers(a, 256))
        crop = rng.integers(a, b + 1, size=(h, w, 3)).astype(np.uint8)
        if t % 5 == 0:                                        # grey: the luma is the value, bounds are hit exactly
            crop[..., 1] = crop[..., 2] = crop[..., 0]
        mask = (rng.random((h, w)) < rng.random()).astype(np.uint8) if t % 2 else None
        crops.append((crop, mask))
    flat = np.full((7, 9, 3), 93, np.uint8)
    two = np.where(rng.random((12, 30, 1)) < 0.3, 0, 25).astype(np.uint8).repeat(3, axis=2)
    one_in = np.zeros((9, 11), np.uint8)
    one_in[4, 5] = 1
    none_in = np.zeros((5, 5), np.uint8)
    full = rng.integers(0, 256, size=(40, 80, 3)).astype(np.uint8)
    crops += [(flat, None), (two, None), (full, None), (rng.integers(0, 256, (9, 11, 3)).astype(np.uint8), one_in),
              (rng.integers(0, 256, (5, 5, 3)).astype(np.uint8), none_in), (np.zeros((1, 1, 3), np.uint8), None)]
    n = 0
    for crop, mask in crops:
        for cutoff in (0, 1, 10, 25, 49):
            got, (lo, hi) = autocontrast_crop(crop, mask, cutoff, with_bounds=True)
            assert got.dtype == np.uint8 and np.array_equal(got, pillow(crop, mask, cutoff)), (crop.shape, mask is not None, cutoff, lo, hi)
            n += 1
    assert n >= 300 * 5
    assert np.array_equal(autocontrast_crop(flat, None, 10), flat)                       # an all-equal crop: the identity
    got, bounds = autocontrast_crop(two, None, 0, with_bounds=True)
    assert bounds == (0, 25) and set(got[two == 25].tolist()) == {254}                   # the (0, 25) LUT stops at 254, as Pillow's
    for bad in (50, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            autocontrast_crop(flat, None, bad)


# ------------------------------------------------------------------------------------------------------ gate and choice rule
def line(text, conf, **more):
    return TextLine(text=text, confidence=conf, polygon=POLY, chars=[], **more)


def test_gate():
    assert rr.doubtful(line("abc", 0.59), 0.6) and not rr.doubtful(line("abc", 0.6), 0.6) and not rr.doubtful(line("abc", 0.9), 0.6)
    assert not rr.doubtful(line("", 1.0), 1.1) and not rr.doubtful(line("", 0.0), 0.6)   # an empty line is not doubtful
    assert not rr.doubtful(line("abc", 0.0), 0.0) and rr.doubtful(line("abc", 1.0), 1.1)
    # an unmet constraint is doubtful whatever the confidence, an empty text included
    assert rr.doubtful(line("12", 0.99, pattern_matched=False), 0.0) and rr.doubtful(line("", 1.0, pattern_matched=False), 0.0)
    assert rr.doubtful(line("Ala", 0.99, lexicon_index=-1), 0.0) and not rr.doubtful(line("Alabama", 0.99, lexicon_index=0), 0.5)
    assert not rr.doubtful(line("12", 0.99, pattern_matched=True), 0.5) and rr.doubtful(line("12", 0.4, pattern_matched=True), 0.5)


def test_choice_rule():
    pick = lambda *c: rr.choose(list(c))
    assert pick(line("a", 0.5), line("b", 0.7), line("c", 0.6)) == 1
    assert pick(line("a", 0.5), line("b", 0.5), line("c", 0.5)) == 0                     # the original wins exact ties
    assert pick(line("a", 0.5), line("b", 0.7), line("c", 0.7)) == 1                     # ... and the earlier variant the others
    assert pick(line("a", 0.2), line("", 1.0)) == 0                                      # a non-empty text beats an empty one's confidence of 1
    assert pick(line("", 1.0), line("a", 0.1)) == 1
    assert pick(line("", 1.0), line("", 1.0)) == 0
    # a met constraint beats everything else
    assert pick(line("12", 0.9, pattern_matched=False), line("7", 0.2, pattern_matched=True), line("8", 0.1, pattern_matched=True)) == 1
    assert pick(line("12", 0.9, pattern_matched=False), line("13", 0.95, pattern_matched=False)) == 1
    assert pick(line("12", 0.9, pattern_matched=False), line("", 1.0, pattern_matched=False)) == 0
    assert pick(line("Al", 0.9, lexicon_index=-1), line("Alabama", 0.3, lexicon_index=0)) == 1
    assert pick(line("Alabama", 0.3, lexicon_index=0), line("Alaska", 0.3, lexicon_index=1)) == 0
    assert pick(line("a", None), line("b", 0.1)) == 1                                    # no confidence counts as 0


# ------------------------------------------------------------------------------------------------------------- variants
def test_rolled_quads_and_rot90():
    q = ((3.0, 5.0), (23.0, 5.0), (23.0, 12.0), (3.0, 12.0))
    assert rr.rolled(q, 0) == q and rr.rolled(q, 1) == (q[1], q[2], q[3], q[0]) and rr.rolled(q, 2) == (q[2], q[3], q[0], q[1])
    assert rr.rolled(q, 3) == (q[3], q[0], q[1], q[2]) and all(quad_ok(rr.rolled(q, k)) for k in range(4))
    page = np.random.default_rng(3).integers(0, 256, size=(20, 30, 3), dtype=np.uint8)
    crop = page[5:12, 3:23]
    for k in range(4):
        turned = rr.rolled(q, k)
        w, h = quad_size(turned)
        assert (w, h) == ((20, 7) if k % 2 == 0 else (7, 20))
        assert np.array_equal(warp_quad(page, quad_homography(turned, w, h), w, h), np.rot90(crop, k)), k
    s = Reread(below=0.5, contrast=3, rotations=(270, 90))
    assert s.variants == ("contrast", "rot90", "rot270")
    v = rr.line_variants(s, q)
    assert [n for n, _ in v] == ["contrast", "rot90", "rot270"] and v[0][1] == ("adjust", 3)
    assert v[1][1] == ("quad", rr.rolled(q, 1)) and v[2][1] == ("quad", rr.rolled(q, 3))
    assert [n for n, _ in rr.line_variants(s, None)] == ["contrast"]                     # no quad: no turns
    assert rr.line_variants(Reread(below=0.5, rotations=(180,)), None) == []


def test_base_quad():
    assert rr.base_quad("bbox", None, None, (2, 3, 60, 14)) == ((2.0, 3.0), (60.0, 3.0), (60.0, 14.0), (2.0, 14.0))
    assert rr.clip_bbox([-4, 3, 90, 14], 64, 40) == (0, 3, 64, 14) and rr.clip_bbox([5, 9, 5, 9], 64, 40) == (5, 9, 6, 10)
    tilted = [[10, 10], [50, 14], [49, 24], [9, 20]]
    assert rr.base_quad("poly", tilted, None) == tuple((float(x), float(y)) for x, y in tilted)
    first = ((1.5, 2.0), (9.0, 2.5), (9.0, 5.0), (1.0, 5.0))
    assert rr.base_quad("poly", tilted, first) == first                                  # the quad the first pass warped the line from
    for bad in ([[0, 0], [10, 0], [10, 10]], [[0, 0], [10, 10], [10, 0], [0, 10]], [[0, 0], [0, 10], [10, 10], [10, 0]],
                [[0, 0], [10, 0], [10, 5], [5, 5], [0, 5]], [[0, 0], [10, 0], [10, 0], [0, 0]]):
        assert rr.base_quad("poly", bad, None) is None                                   # not quad_ok: no turned variants
    assert rr.base_quad("bbox", None, None, (5, 5, 5, 9)) is None                        # an empty rectangle
    assert rr.source_polygon(tilted, (1, 1)) is tilted and rr.source_polygon([[3, 5]], (2.0, 1.5)) == [[6, 7]]


def test_host_contrast_masks_polygon_lines():
    rng = np.random.default_rng(5)
    page = rng.integers(60, 140, size=(40, 64, 3)).astype(np.float32)
    poly = [[10, 8], [50, 12], [48, 30], [8, 26]]
    from surya_amd.recognition.predictor import slice_and_pad_poly, slice_bboxes_from_image
    crop = slice_and_pad_poly(page, poly)
    mask = fill_poly_mask(crop.shape[0], crop.shape[1], [(x - 8, y - 8) for x, y in poly])
    got = rr.host_contrast(crop, "poly", poly, None, 2)
    assert got.dtype == np.float32 and np.array_equal(got, pillow(crop.astype(np.uint8), mask, 2).astype(np.float32))
    assert not np.array_equal(got, pillow(crop.astype(np.uint8), None, 2).astype(np.float32))      # the pad is not counted
    box = slice_bboxes_from_image(page, [[2, 3, 60, 14]])[0]
    assert np.array_equal(rr.host_contrast(box, "bbox", None, None, 2), pillow(box.astype(np.uint8), None, 2).astype(np.float32))
    assert np.array_equal(rr.host_contrast(crop, "poly", poly, ((0.0, 0.0),) * 4, 2), pillow(crop.astype(np.uint8), None, 2).astype(np.float32))
    assert rr.host_contrast(np.zeros((0, 5, 3), np.float32), "bbox", None, None, 2).size == 0


# ------------------------------------------------------------------------------------------------ validation and refusals
def test_reread_values():
    s = Reread(below=0.6, contrast=2, rotations=(180,))
    assert (s.below, s.contrast, s.rotations) == (0.6, 2, (180,)) and Reread(1, rotations=[90, 270]).rotations == (90, 270)
    assert Reread(below=0.5, contrast=0).variants == ("contrast",) and Reread(below=0.5, contrast=49).contrast == 49
    with pytest.raises(TypeError):
        Reread()                                              # `below` has no default
    for kw in (dict(below="0.5", contrast=2), dict(below=None, contrast=2), dict(below=True, contrast=2), dict(below=0.5, contrast=2.0),
               dict(below=0.5, contrast=True), dict(below=0.5, rotations=180), dict(below=0.5, rotations="90"), dict(below=0.5, rotations=(90.0,)),
               dict(below=0.5, rotations=(True,))):
        with pytest.raises(TypeError):
            Reread(**kw)
    for kw in (dict(below=0.5), dict(below=0.5, contrast=None, rotations=()), dict(below=0.5, contrast=50), dict(below=0.5, contrast=-1),
               dict(below=0.5, rotations=(45,)), dict(below=0.5, rotations=(0,)), dict(below=0.5, rotations=(360,)), dict(below=0.5, rotations=(90, 90)),
               dict(below=float("nan"), contrast=2)):
        with pytest.raises(ValueError):
            Reread(**kw)
    assert rr.checked(None) is None and rr.checked(s).contrast == 2
    with pytest.raises(TypeError):
        rr.checked({"below": 0.5})
    s.contrast = 77                                           # assigned after construction: checked again per call
    with pytest.raises(ValueError):
        rr.checked(s)


def test_refusals_come_before_any_model_call(proc, fake_loop_settings):
    pred = _enc_pred(proc)
    enc = pred.encode(IMAGES, bboxes=BOXES3, recognition_batch_size=8)
    calls = len(pred.model.log)
    pred.reread = Reread(below=0.5, contrast=2)
    texts = [["a"] * len(p) for p in BOXES3]
    for what, call in (("align", lambda: pred.align(IMAGES, texts, bboxes=BOXES3)), ("rank", lambda: pred.rank(IMAGES, [[["a"]] * len(p) for p in BOXES3], bboxes=BOXES3)),
                       ("encode", lambda: pred.encode(IMAGES, bboxes=BOXES3)), ("read", lambda: enc.read()),
                       ("rank", lambda: enc.rank([[["a"]] * len(p) for p in BOXES3])), ("align", lambda: enc.align(texts))):
        with pytest.raises(ValueError, match=r"reread does not apply to " + what):
            call()
    for attr, value in (("shard_lines", True), ("shard_pages", True), ("process_group", object())):
        setattr(pred, attr, value)
        with pytest.raises(NotImplementedError, match="a call with reread runs on one rank"):
            pred(IMAGES, bboxes=BOXES3)
        setattr(pred, attr, None if attr == "process_group" else False)
    for bad, exc in (("contrast", TypeError), (0.5, TypeError), ({"below": 0.5}, TypeError)):
        pred.reread = bad
        with pytest.raises(exc):
            pred(IMAGES, bboxes=BOXES3)
    pred.reread = Reread(below=0.5, contrast=2)
    pred.reread.rotations = (45,)
    with pytest.raises(ValueError):
        pred(IMAGES, bboxes=BOXES3)
    assert len(pred.model.log) == calls and pred._reread is None
    pred.reread = None
    enc.release()


# ------------------------------------------------------------------------------------------------- admission on a fake model
def _conf_pred(proc, conf_of):
    """The fake predictor of the encoded tests whose assembled lines carry conf_of(text), with the lines handed to pre-processing and
    the slot masks recorded."""
    pred = _enc_pred(proc)
    seen = []
    inner = pred.preprocess_prompts_device

    def recording(prompts, pages):
        seen.append(([p.image for p in prompts], [pg.shape for pg in pages]))
        return inner(prompts, pages)
    pred.preprocess_prompts_device = recording

    def assemble(flat, items, drop_repeated_text, return_words, bbox_size):
        return [TextLine(text=",".join(map(str, it[2])), polygon=flat["polygons"][it[1]], confidence=conf_of(",".join(map(str, it[2]))), chars=[])
                for it in items]
    pred._assemble_batch = assemble
    return pred, seen


def test_second_pass_admits_doubtful_lines_times_variants(proc, fake_loop_settings):
    texts = [[_stream_of(b) for b in page] for page in BOXES3]
    low = {texts[0][1], texts[1][0]}                          # the doubtful lines: the second of page 0, the only one of page 1
    pred, seen = _conf_pred(proc, lambda t: 0.3 if t in low else 0.9)
    plain = pred(IMAGES, bboxes=BOXES3, recognition_batch_size=8, allowlist=[["ab", None, "abc"], "xy"])
    masks_plain = [c for c in pred.model.log if c[0] == "set_slot_masks"]
    del seen[:]
    pred.model.log.clear()
    pred.reread = Reread(below=0.5, contrast=4, rotations=(180, 90))
    got = pred(IMAGES, bboxes=BOXES3, recognition_batch_size=8, allowlist=[["ab", None, "abc"], "xy"])
    assert pred._reread is None and pred.last_timing["reread_lines"] == 2.0 and pred.last_timing["reread_ms"] > 0.0
    assert len(seen) == 2                                     # the first pass, then ONE more run
    refs, pages = seen[1]
    # 2 doubtful lines x (contrast, rot90, rot180), widest first; every page holds a doubtful line here, so both travel again
    assert len(refs) == 6 and sorted(p[:2] for p in pages) == [(32, 48), (40, 64)]
    by_box = {}
    for r in refs:
        by_box.setdefault((r.page, r.x0, r.y0), []).append(r)
    assert len(by_box) == 2
    for (pg, x0, y0), rs in by_box.items():
        box = next(b for b in (BOXES3[0][1], BOXES3[1][0]) if (b[0], b[1]) == (x0, y0))
        adj = [r for r in rs if r.adjust is not None]
        assert len(adj) == 1 and adj[0].adjust == 4 and adj[0].quad is None and (adj[0].x1, adj[0].y1) == (box[2], box[3])
        quads = sorted(r.quad for r in rs if r.quad is not None)
        rect = ((float(box[0]), float(box[1])), (float(box[2]), float(box[1])), (float(box[2]), float(box[3])), (float(box[0]), float(box[3])))
        assert quads == sorted([rr.rolled(rect, 1), rr.rolled(rect, 2)]) and all(r.adjust is None for r in rs if r.quad is not None)
    # each re-read line went in under ITS OWN mask id: three slots each for the ids of lines (0, 1) and (1, 0) of the first pass
    runs = [c for c in pred.model.log if c[0] == "set_slot_masks"]
    n_first = sum(len(c[1]) for c in masks_plain)
    first = [i for c in runs for i in c[2]][:n_first]
    second = [i for c in runs for i in c[2]][n_first:]
    assert n_first == 4 and sorted(first) == sorted(i for c in masks_plain for i in c[2]) and len(second) == 6
    assert sorted(first) == [-1, 0, 1, 2]                     # "ab", no list, "abc", "xy"
    assert sorted(second) == [-1] * 3 + [2] * 3               # line (0, 1) has no list, line (1, 0) has "xy": so have their variants
    # results: lines that were not doubtful are the plain call's plus variant = "original"; re-read ones list four candidates
    strip = lambda ln: {k: v for k, v in ln.model_dump().items() if k not in ("variant", "readings")}
    for page_got, page_plain in zip(got, plain):
        for a, b in zip(page_got.text_lines, page_plain.text_lines):
            assert strip(a) == strip(b) and a.variant == "original"          # (the fake reads every variant as the line itself: ties -> original)
            if b.text in low:
                assert [r.variant for r in a.readings] == ["original", "contrast", "rot90", "rot180"]
                assert all(isinstance(r, LineReading) and r.text == b.text and r.confidence == 0.3 for r in a.readings)
            else:
                assert a.readings is None and "readings" not in a.model_dump()
    # the gate at 0: nothing is re-read, no second run
    del seen[:]
    pred.reread = Reread(below=0.0, contrast=4)
    again = pred(IMAGES, bboxes=BOXES3, recognition_batch_size=8)
    assert len(seen) == 1 and pred.last_timing["reread_lines"] == 0.0
    assert all(ln.variant == "original" and ln.readings is None for r in again for ln in r.text_lines)
    pred.reread = None


def test_a_better_variant_takes_the_lines_place(proc, fake_loop_settings):
    """The fake reads a line by the corner of its crop; a stand-in pre-processing moves the corner of turned lines, so that a turned
    reading differs and can win."""
    state = {"second": False}
    pred, seen = _conf_pred(proc, lambda t: 0.8 if state["second"] else 0.4)
    inner = pred.preprocess_prompts_device

    def pre(prompts, pages):
        state["second"] = any(p.image.quad is not None or p.image.adjust is not None for p in prompts)
        return inner(prompts, pages)
    pred.preprocess_prompts_device = pre
    plain = pred(IMAGES, bboxes=BOXES3, recognition_batch_size=8)
    pred.reread = Reread(below=0.5, rotations=(180,), contrast=1)
    got = pred(IMAGES, bboxes=BOXES3, recognition_batch_size=8)
    for a, b in zip([l for r in got for l in r.text_lines], [l for r in plain for l in r.text_lines]):
        assert a.variant == "contrast" and a.polygon == b.polygon and a.text == b.text and a.confidence == 0.8      # the first of the two better ones
        assert [(r.variant, r.confidence) for r in a.readings] == [("original", 0.4), ("contrast", 0.8), ("rot180", 0.8)]
        assert a.model_dump()["variant"] == "contrast" and len(a.model_dump()["readings"]) == 3
    pred.reread = None
    state["second"] = False
    assert [r.model_dump() for r in pred(IMAGES, bboxes=BOXES3, recognition_batch_size=8)] == [r.model_dump() for r in plain]


# --------------------------------------------------------------------------------------------------- schema and bindings
def test_serialised_form_without_reread_is_unchanged(proc, fake_loop_settings):
    ln = line("abc", 0.5)
    d = ln.model_dump()
    assert "variant" not in d and "readings" not in d and ln.variant is None and ln.readings is None
    assert "variant" not in ln.model_dump_json() and "readings" not in ln.model_dump_json()
    ln.variant, ln.readings = "rot180", [LineReading(variant="original", text="abc", confidence=0.5)]
    d = ln.model_dump()
    assert d["variant"] == "rot180" and d["readings"] == [{"variant": "original", "text": "abc", "confidence": 0.5}]
    pred = _enc_pred(proc)
    res = pred(IMAGES, bboxes=BOXES3, recognition_batch_size=8)
    assert all("variant" not in l and "readings" not in l for r in res for l in r.model_dump()["text_lines"])
    assert "reread_ms" not in pred.last_timing and "reread_lines" not in pred.last_timing
    assert OCRResult(**res[0].model_dump()).model_dump() == res[0].model_dump()


def test_bindings_and_header_agree():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "surya_amd.h")).read()
    m = re.search(r"\bint surya_rec_adjust_contrast\(([^;]*)\);", hdr)
    assert m and len(m.group(1).split(",")) == 9
    args = [a.strip() for a in m.group(1).split(",")]
    assert args[1] == "const void* descs" and args[2] == "int n" and args[6] == "int32_t* lo_hi" and args[7] == "int pixel_stride"
    if os.path.exists(L.LIB_PATH):
        fn = L.lib().surya_rec_adjust_contrast
        assert len(fn.argtypes) == 9 and fn.restype is not None
    from surya_amd.recognition.preprocess_gpu import ADJUST_DESC, ADJUST_WORK_BYTES, LineRef
    assert ADJUST_DESC.itemsize == 88 and "88 bytes" in hdr and ADJUST_WORK_BYTES == 1280 and "n * 1280 bytes" in hdr
    offsets = {n: ADJUST_DESC.fields[n][1] for n in ADJUST_DESC.names}
    assert offsets == {"src_off": 0, "src_w": 8, "src_h": 12, "x0": 16, "y0": 20, "w": 24, "h": 28, "cutoff": 32, "has_poly": 36, "poly": 40,
                       "out_off": 72, "mask_off": 80}
    core = open(os.path.join(os.path.dirname(L.HERE), "surya_amd", "csrc", "adjust_core.h")).read()
    assert "sizeof(AdjustDesc) == 88" in core
    assert LineRef(0, 0, 0, 4, 4).adjust is None


# ------------------------------------------------------------------------------------------------------- the host check
def test_adjust_hostcheck_is_clean_under_the_host_sanitizers(tmp_path):
    """tools/hostcheck/adjust_check.cpp -- the cut / lo / hi / LUT arithmetic of csrc/adjust_core.h and the descriptor validation of
    surya_rec_adjust_contrast -- built as a stand-alone program under the address and undefined-behaviour sanitizers, by the command of
    its header comment, and run. Nothing is loaded into Python."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, flags = os.path.join("tools", "hostcheck", "adjust_check.cpp"), "-std=c++17 -O1 -g -Iinclude -fsanitize=address,undefined"
    with open(os.path.join(root, src)) as f:
        head = " ".join(line.strip("/ \\\n") for line in f.read().split("#include")[0].splitlines())
    assert f"clang++ {flags} {src}" in head                                    # the command below is the one the program documents
    cxx = next((c for c in (shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++", shutil.which("g++"),
                            shutil.which("c++")) if c and os.path.exists(c)), None)
    assert cxx is not None, "no C++ compiler"
    exe = str(tmp_path / "adjust_check")
    subprocess.run([cxx, *flags.split(), src, "-o", exe], cwd=root, check=True, timeout=600)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "adjust_check: all passed" in run.stdout.splitlines()
