"""GPU: re-reading doubtful lines (RecognitionPredictor.reread) and the `adjust` lines of DevicePreprocessor.

  * DevicePreprocessor: tiles of `adjust` lines (bbox, polygon, rectified) == the host chain on Pillow's adjusted padded crop within
    test_gpu_prep.py's 2e-5 (whether they are identical is printed), their bounds == Pillow's; lines without `adjust` in the same call are
    bit-identical to a call without the feature; a call without an `adjust` line never reaches the new entry point;
  * the predictor on REC-SMALL with below = 1.1 (every non-empty line is re-read): readings[0] is the plain call's reading; the "contrast"
    candidate equals, field for field, the plain reading of a page whose boxes were overwritten with Pillow's adjusted crops; the turned
    candidates equal, character polygons included, pred(polygons=[rolled quad]) with rectify = True; the line returned is the one the
    choice rule names; the host pre-processing path agrees; below = 0 re-reads nothing; an unmet pattern triggers a re-read whatever the
    confidence; streamed == serial; top_k and beam_width survive into the winner; reread = None gives back the plain call."""
import numpy as np
import pytest
import torch
from PIL import Image, ImageOps

from surya_amd.common.imageops import autocontrast_bounds, fill_poly_mask, quad_homography, quad_size, warp_quad
from surya_amd.config import rec_config
from surya_amd.recognition import reread as rr
from surya_amd.recognition.reread import Reread
from surya_amd.synth import make_pages

pytestmark = pytest.mark.gpu


def pillow_adjust(crop, mask, cutoff):
    im = Image.fromarray(np.ascontiguousarray(crop))
    m = None if mask is None else Image.fromarray((mask != 0).astype(np.uint8) * 255)
    return np.asarray(ImageOps.autocontrast(im, cutoff=cutoff, mask=m, preserve_tone=True)), autocontrast_bounds(im.convert("L").histogram(m), cutoff)


def faint(pages):
    """Low-contrast, grainy copies of synthetic pages (values 60..162): no crop is flat, so every adjustment changes pixels."""
    rng = np.random.default_rng(31)
    return [(p // 4 + 60 + rng.integers(0, 40, size=p.shape)).astype(np.uint8) for p in pages]


# ------------------------------------------------------------------------------------------------------ DevicePreprocessor
class CountingLib:
    """The library with the calls of one symbol counted."""

    def __init__(self, lib, name):
        self._lib, self._name, self.calls = lib, name, 0

    def __getattr__(self, key):
        fn = getattr(self._lib, key)
        if key != self._name:
            return fn

        def counted(*a):
            self.calls += 1
            return fn(*a)
        return counted


@pytest.mark.parametrize("pix", [3, 4])
def test_device_preprocessor_adjusts_in_front_of_the_ordinary_chain(hip_lib, pix):
    from surya_amd.recognition.predictor import RecognitionModelLoader
    from surya_amd.recognition.preprocess_gpu import DevicePreprocessor, bbox_ref, poly_ref, quad_ref
    proc = RecognitionModelLoader({"config": rec_config("REC-TINY"), "state_dict": {}}).processor()
    page = faint(make_pages(1, 256, seed=5))[0]
    other = np.random.default_rng(4).integers(70, 180, size=(90, 131, 3), dtype=np.uint8)
    pages = [page, other]
    if pix == 4:
        pages = [np.concatenate([p, np.full(p.shape[:2] + (1,), 77, np.uint8)], axis=2) for p in pages]
    pre = DevicePreprocessor("cuda:0")
    pre.lib = CountingLib(pre.lib, "surya_rec_adjust_contrast")
    sizes = lambda n: [(1024, 256)] * n
    poly = [[20, 120], [230, 128], [228, 170], [18, 160]]
    quad = [(30.0, 30.0), (220.0, 44.0), (214.0, 92.0), (26.0, 70.0)]
    plain = [bbox_ref(0, 256, 256, [10, 20, 240, 60]), poly_ref(0, 256, 256, poly), bbox_ref(1, 131, 90, [3, 5, 120, 47]), quad_ref(0, 256, 256, quad)]
    t0, o0, g0 = pre(pages, plain, sizes(4))
    assert pre.lib.calls == 0                                                 # no adjusted line: the new entry point is not reached
    import dataclasses
    adj = [dataclasses.replace(plain[0], adjust=2), dataclasses.replace(plain[1], adjust=10), dataclasses.replace(plain[2], adjust=0),
           dataclasses.replace(plain[3], adjust=5)]
    lines = [adj[0], plain[1], adj[1], plain[0], adj[2], plain[3], adj[3], plain[2]]
    t1, o1, g1 = pre(pages, lines, sizes(len(lines)))
    assert pre.lib.calls == 1
    rows = lambda t, o, i: t[int(o[i]):int(o[i + 1])]
    for at, k in ((1, 1), (3, 0), (5, 3), (7, 2)):                            # the lines without `adjust` do not notice their neighbours
        assert g1[at] == g0[k] and torch.equal(rows(t1, o1, at), rows(t0, o0, k))
    # the adjusted lines: the host chain on Pillow's adjusted padded crop
    x0, y0, x1, y1 = plain[1].x0, plain[1].y0, plain[1].x1, plain[1].y1
    mask = fill_poly_mask(y1 - y0, x1 - x0, [(x - x0, y - y0) for x, y in poly])
    padded = pages[0][y0:y1, x0:x1, :3].copy()
    padded[mask == 0] = 255
    W, H = quad_size(quad)
    refs = [(pages[0][20:60, 10:240, :3], None, 2), (padded, mask, 10), (pages[1][5:47, 3:120, :3], None, 0),
            (warp_quad(pages[0], quad_homography(quad, W, H), W, H)[..., :3], None, 5)]
    bounds = pre.last_adjust_bounds.cpu().numpy().tolist()
    worst, same = 0.0, True
    for k, (at, (crop, m, c)) in enumerate(zip((0, 2, 4, 6), refs)):
        want, lohi = pillow_adjust(crop, m, c)
        assert tuple(bounds[k]) == lohi and lohi != (0, 255), (k, bounds[k], lohi)
        ref, grid = proc.process_and_tile(proc.scale_to_fit(want.astype(np.float32), (1024, 256)))
        got = rows(t1, o1, at).cpu().numpy()
        assert g1[at] == grid and got.shape == ref.shape
        worst = max(worst, float(np.abs(got - ref).max()))
        same = same and np.array_equal(got, ref)
        assert not torch.equal(rows(t1, o1, at), rows(t0, o0, k))             # ... which are not the unadjusted line's
    print(f"adjusted tiles vs host chain on Pillow's crop: worst |diff| = {worst}, identical = {same}")
    assert worst <= 2e-5, worst
    t2, o2, g2 = pre(pages, plain, sizes(4))                                  # the plain call again: what it returned before
    assert pre.lib.calls == 1 and g2 == g0 and np.array_equal(o2, o0) and torch.equal(t2, t0)


# ------------------------------------------------------------------------------------------------------------ the predictor
BOXES = [[[12, 20, 236, 58], [30, 90, 200, 122], [8, 150, 120, 176], [140, 190, 250, 240]], [[20, 30, 230, 70], [40, 120, 180, 150]]]
SKIP = ("variant", "readings")


@pytest.fixture(scope="module")
def small(hip_lib):
    from surya_amd.settings import settings
    from test_gpu_predictors import make_rec_predictor
    old = settings.RECOGNITION_MAX_TOKENS
    cfg, sd, pred = make_rec_predictor("REC-SMALL", max_slots=16, max_tokens=8)
    pages = [Image.fromarray(p) for p in faint(make_pages(2, 256, seed=8))]
    plain = pred(pages, bboxes=BOXES)
    yield pred, pages, plain
    settings.RECOGNITION_MAX_TOKENS = old


def strip(line, *more):
    return {k: v for k, v in line.model_dump().items() if k not in SKIP + more}


def lines_of(results):
    return [l for r in results for l in r.text_lines]


def adjusted_pages(pages, cutoff):
    out = []
    for im, boxes in zip(pages, BOXES):
        a = np.asarray(im).copy()
        src = a.copy()
        for x0, y0, x1, y1 in boxes:
            a[y0:y1, x0:x1] = pillow_adjust(src[y0:y1, x0:x1], None, cutoff)[0]
        out.append(Image.fromarray(a))
    return out


def rect(b):
    return ((float(b[0]), float(b[1])), (float(b[2]), float(b[1])), (float(b[2]), float(b[3])), (float(b[0]), float(b[3])))


def test_every_candidate_is_the_plain_reading_of_its_picture(small):
    pred, pages, plain = small
    try:
        pred.reread = Reread(below=1.1, contrast=2, rotations=(180, 90))
        got = pred(pages, bboxes=BOXES)
        cands = dict(pred.last_reread_candidates)
        timing = dict(pred.last_timing)
        pred.device_preprocess = False
        host = pred(pages, bboxes=BOXES)
    finally:
        pred.reread, pred.device_preprocess = None, True
    base = lines_of(plain)
    nonempty = [i for i, l in enumerate(base) if l.text != ""]
    assert len(nonempty) >= 3 and sorted(cands) == nonempty and timing["reread_lines"] == len(nonempty) and timing["reread_ms"] > 0
    # the references: Pillow's crops pasted into the pages; the rolled rectangles as polygons under rectify
    contrast = lines_of(pred(adjusted_pages(pages, 2), bboxes=BOXES))
    try:
        pred.rectify = True
        turned = {k: lines_of(pred(pages, polygons=[[[[int(x), int(y)] for x, y in rr.rolled(rect(b), k)] for b in page] for page in BOXES]))
                  for k in (1, 2)}
    finally:
        pred.rectify = None
    for i, line in enumerate(lines_of(got)):
        if i not in cands:
            assert strip(line) == strip(base[i]) and line.variant == "original" and line.readings is None
            continue
        c = cands[i]
        assert [x.variant for x in c] == ["original", "contrast", "rot90", "rot180"]
        assert [(r.variant, r.text, r.confidence) for r in line.readings] == [(x.variant, x.text, x.confidence) for x in c]
        assert (line.readings[0].text, line.readings[0].confidence) == (base[i].text, base[i].confidence)
        assert strip(c[0]) == strip(base[i])
        assert strip(c[1]) == strip(contrast[i]), (i, "contrast")
        assert strip(c[2], "polygon", "bbox") == strip(turned[1][i], "polygon", "bbox") and c[2].rectified is True, (i, "rot90")
        assert strip(c[3], "polygon", "bbox") == strip(turned[2][i], "polygon", "bbox") and c[3].rectified is True, (i, "rot180")
        assert [ch.polygon for ch in c[3].chars] == [ch.polygon for ch in turned[2][i].chars]
        win = c[rr.choose(c)]
        assert line is win or strip(line) == strip(win)
        assert line.variant == win.variant and line.polygon == base[i].polygon       # the polygon that came in
    assert any(c[1].text != c[0].text or c[1].confidence != c[0].confidence for c in cands.values())      # the adjustment changed a reading
    assert len({l.variant for l in lines_of(got)}) >= 2                                # ... and some variant won somewhere
    # the host pre-processing path: the same candidates, the same winners
    assert [(l.variant, l.text, [(r.variant, r.text) for r in l.readings or []]) for l in lines_of(host)] == \
           [(l.variant, l.text, [(r.variant, r.text) for r in l.readings or []]) for l in lines_of(got)]


def test_gate_constraint_trigger_and_back_to_default(small):
    pred, pages, plain = small
    dump = lambda rs: [r.model_dump() for r in rs]
    try:
        pred.reread = Reread(below=0.0, contrast=2, rotations=(180,))
        got = pred(pages, bboxes=BOXES)
        assert pred.last_timing["reread_lines"] == 0 and pred.last_reread_candidates == {}
        assert [strip(l) for l in lines_of(got)] == [strip(l) for l in lines_of(plain)]
        assert all(l.variant == "original" and l.readings is None and "readings" not in l.model_dump() for l in lines_of(got))
        # a pattern no line can finish within its token budget: pattern_matched is False, so every line is re-read at below = 0
        pred.pattern = r"\d{40}"
        got = lines_of(pred(pages, bboxes=BOXES))
        assert pred.last_timing["reread_lines"] == len(got) == 6
        for l in got:
            assert l.pattern_matched is False and [r.variant for r in l.readings] == ["original", "contrast", "rot180"]
            assert all(ch.isdigit() for ch in l.text)                          # (\d is re's: every Unicode decimal digit)
            best = max(range(3), key=lambda k: (l.readings[k].text != "", l.readings[k].confidence, -k))
            assert l.variant == l.readings[best].variant
    finally:
        pred.reread = pred.pattern = None
    assert dump(pred(pages, bboxes=BOXES)) == dump(plain)                              # back to default: what it returned before
    assert all("variant" not in l and "readings" not in l for r in dump(plain) for l in r["text_lines"])


@pytest.mark.parametrize("mode", ["top_k", "beam_width"])
def test_decoding_options_survive_into_the_winner(small, mode):
    pred, pages, plain = small
    try:
        setattr(pred, mode, 2)
        first = lines_of(pred(pages, bboxes=BOXES))
        pred.reread = Reread(below=1.1, rotations=(180,))
        got = lines_of(pred(pages, bboxes=BOXES))
        cands = dict(pred.last_reread_candidates)
    finally:
        setattr(pred, mode, None)
        pred.reread = None
    assert len(cands) >= 3
    for i, l in enumerate(got):
        if mode == "beam_width":
            assert l.hypotheses is not None and 1 <= len(l.hypotheses) <= 2 and l.log_prob is not None
        if i not in cands:
            assert strip(l) == strip(first[i])
            continue
        assert strip(cands[i][0]) == strip(first[i]) and l.variant == cands[i][rr.choose(cands[i])].variant
        for c in cands[i]:                                                     # every candidate was read under the call's option
            if mode == "beam_width":
                assert c.hypotheses is not None and c.hypotheses[0].text == c.text
            else:
                assert not c.chars or any(ch.alternatives is not None and len(ch.alternatives) == 2 for ch in c.chars)
    assert any(ch.alternatives for l in got for ch in l.chars) if mode == "top_k" else all(l.log_prob is not None for l in got)


def test_streamed_detect_recognise_with_reread_equals_the_serial_call(hip_lib):
    from surya_amd.synth import make_pages_with_lines
    from test_gpu_predictors import _det_with_drawn_rows, make_rec_predictor
    size = 256
    pages_np, rows = make_pages_with_lines(3, size, seed=99)
    pages = [Image.fromarray(p) for p in faint(pages_np)]
    det = _det_with_drawn_rows(pages, rows, size, 2)
    cfg, sd, pred = make_rec_predictor(max_slots=8, max_tokens=7)
    try:
        pred.reread = Reread(below=1.1, contrast=3, rotations=(180,))
        pred.stream_detection = False
        serial = pred(pages, det_predictor=det)
        n_serial = pred.last_timing["reread_lines"]
        pred.stream_detection = True
        streamed = pred(pages, det_predictor=det)
        assert pred.last_timing.get("streamed") == 1.0 and pred.last_timing["reread_lines"] == n_serial > 0
    finally:
        pred.reread = None
    assert [r.model_dump() for r in serial] == [r.model_dump() for r in streamed] and len(streamed) == 3
    lines = lines_of(streamed)
    assert sum(l.readings is not None for l in lines) == n_serial and all(l.variant is not None for l in lines)
    assert all([r.variant for r in l.readings] == ["original", "contrast", "rot180"] for l in lines if l.readings is not None)
