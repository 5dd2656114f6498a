"""GPU: rectification of rotated line quadrilaterals on the device (surya_rec_rectify, csrc/rec_rectify.h).

  * the entry point alone against warp_quad (common/imageops.py): uint8-EQUAL everywhere -- same taps, same float64 association, no
    contraction; RGB and RGBX pages, partial tiles, a grid sized by another line, `out` inside the pages' allocation and outside it;
  * every argument refusal leaves `out` untouched;
  * through DevicePreprocessor: an axis-aligned quad forced through the warp gives bbox_ref's tiles bit for bit, tilted quads the host
    chain's within test_gpu_prep.py's 2e-5, and a call without a quad never reaches the new entry point;
  * the predictor on REC-TINY: device path == host path, `rectified` per line, off again == a fresh predictor, streamed == serial,
    and one run together with a pattern."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
from PIL import Image

from surya_amd import _lib as L
from surya_amd.common.imageops import fill_poly_mask, quad_homography, quad_size, warp_quad
from surya_amd.config import det_config, rec_config
from surya_amd.synth import make_det_weights, make_pages

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


def tilted(cx, cy, w, h, deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return [(cx + c * x - s * y, cy + s * x + c * y) for x, y in ((-w / 2, -h / 2), (w / 2, -h / 2), (w / 2, h / 2), (-w / 2, h / 2))]


ONE_PIXEL = [(10.2, 7.1), (11.1, 7.3), (10.9, 8.2), (10.0, 8.0)]
TRAPEZOID = [(8.0, 10.0), (150.0, 14.0), (140.0, 40.0), (12.0, 30.0)]
# (page, quad): mixed sizes in one call -- 1 x 1, 65 x 5 and 3 x 130 are partial 16 x 16 tiles under a grid that another line sizes
SEVEN = [(0, tilted(100.0, 60.0, 150.0, 22.0, 17.0)), (1, ONE_PIXEL), (0, tilted(90.0, 80.0, 65.0, 5.0, -33.0)),
         (1, tilted(70.0, 75.0, 3.0, 130.0, 8.0)), (0, TRAPEZOID), (1, tilted(132.0, 140.0, 48.0, 20.0, 25.0)),       # over two edges of page 1
         (1, tilted(60.0, 40.0, 33.0, 17.0, -150.0))]


def _pages(pix):
    rng = np.random.default_rng(21)
    return [rng.integers(0, 256, size=(120, 200, pix), dtype=np.uint8), rng.integers(0, 256, size=(150, 140, pix), dtype=np.uint8)]


def _plan(pages, jobs, pix, base):
    """Page offsets, the descriptors of `jobs` with their crops from byte `base` of `out` on (4-byte aligned each), the end."""
    from surya_amd.recognition.preprocess_gpu import RECTIFY_DESC
    offs, total = [], 0
    for pg in pages:
        offs.append(total)
        total += pg.size
    desc = np.zeros(len(jobs), RECTIFY_DESC)
    at = (base + 3) & ~3
    for d, (pi, quad) in zip(desc, jobs):
        W, H = quad_size(quad)
        d["page_off"], d["page_w"], d["page_h"], d["out_w"], d["out_h"], d["out_off"] = offs[pi], pages[pi].shape[1], pages[pi].shape[0], W, H, at
        d["h"] = quad_homography(quad, W, H)
        at += (W * H * pix + 3) & ~3
    return offs, total, desc, at


def _call(lib, d_pages, desc, n, d_out, pix, max_w, max_h):
    rc = lib.surya_rec_rectify(L.ptr(d_pages), desc.ctypes.data_as(C.c_void_p), n, L.ptr(d_out), pix, max_w, max_h,
                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("same_allocation", [True, False])
@pytest.mark.parametrize("jobs", [SEVEN[:1], SEVEN], ids=["one", "seven"])
@pytest.mark.parametrize("pix", [3, 4])
def test_entry_point_equals_warp_quad(hip_lib, pix, jobs, same_allocation):
    lib = L.lib()
    pages = _pages(pix)
    page_bytes = sum(pg.size for pg in pages)
    offs, total, desc, end = _plan(pages, jobs, pix, page_bytes if same_allocation else 0)
    host = np.full(end if same_allocation else total, SENTINEL, np.uint8)
    for pg, o in zip(pages, offs):
        host[o:o + pg.size] = pg.reshape(-1)
    d_pages = torch.from_numpy(host).cuda()
    d_out = d_pages if same_allocation else torch.full((end,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert _call(lib, d_pages, desc, len(jobs), d_out, pix, int(desc["out_w"].max()), int(desc["out_h"].max())) == 0
    out = d_out.cpu().numpy()
    if same_allocation:
        assert np.array_equal(out[:total], host[:total])                   # the pages are read only
    written = np.zeros(out.size, bool)
    for d, (pi, quad) in zip(desc, jobs):
        W, H = int(d["out_w"]), int(d["out_h"])
        want = warp_quad(pages[pi], d["h"], W, H)
        a = int(d["out_off"])
        got = out[a:a + W * H * pix].reshape(H, W, pix)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (quad_size(quad), len(bad), bad[:4].tolist())
        written[a:a + W * H * pix] = True
    rest = ~written
    if same_allocation:
        rest[:total] = False
    assert (out[rest] == SENTINEL).all()                                   # nothing beside the crops, padding bytes included
    shapes = {(int(d["out_w"]), int(d["out_h"])) for d in desc}
    assert len(jobs) == 1 or {(1, 1), (65, 5), (3, 130)} <= shapes


def test_refusals_leave_out_untouched(hip_lib):
    lib = L.lib()
    for pix in (3, 4):
        pages = _pages(pix)
        offs, total, desc, end = _plan(pages, SEVEN[:2], pix, 0)
        d_pages = torch.from_numpy(np.concatenate([pg.reshape(-1) for pg in pages])).cuda()
        d_out = torch.full((end,), SENTINEL, dtype=torch.uint8, device="cuda")
        mw, mh = int(desc["out_w"].max()), int(desc["out_h"].max())

        def edited(field, value, i=1):
            d = desc.copy()
            d[field][i] = value
            return d
        cases = [(desc, 2, 5, mw, mh), (desc, 2, 0, mw, mh), (desc, 2, pix, 0, mh), (desc, 2, pix, mw, -1), (desc, -1, pix, mw, mh),
                 (edited("out_w", 0), 2, pix, mw, mh), (edited("out_h", -3), 2, pix, mw, mh), (edited("page_w", 0), 2, pix, mw, mh),
                 (desc, 2, pix, mw - 1, mh)]                                # a crop larger than the grid covers
        if pix == 4:
            cases += [(edited("out_off", int(desc["out_off"][1]) + 2), 2, 4, mw, mh), (edited("page_off", 2, 0), 2, 4, mw, mh)]
        for d, n, px, w, h in cases:
            assert _call(lib, d_pages, d, n, d_out, px, w, h) == L.SA_ERR_ARG, (n, px, w, h)
            assert bool((d_out == SENTINEL).all())
        assert _call(lib, d_pages, desc, 0, d_out, pix, mw, mh) == 0 and bool((d_out == SENTINEL).all())     # n == 0 launches nothing
        assert _call(lib, d_pages, desc, 2, d_out, pix, mw, mh) == 0 and not bool((d_out == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------ DevicePreprocessor
def _processor():
    from surya_amd.recognition.predictor import RecognitionModelLoader
    return RecognitionModelLoader({"config": rec_config("REC-TINY"), "state_dict": {}}).processor()


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
def test_device_preprocessor_rectifies_in_front_of_the_ordinary_chain(hip_lib, pix):
    from surya_amd.recognition.preprocess_gpu import DevicePreprocessor, bbox_ref, poly_ref, quad_ref
    proc = _processor()
    page = make_pages(1, 256, seed=5)[0]
    other = np.random.default_rng(4).integers(0, 256, size=(90, 131, 3), dtype=np.uint8)
    pages = [page, other]
    if pix == 4:
        pages = [np.concatenate([p, np.full(p.shape[:2] + (1,), 77, np.uint8)], axis=2) for p in pages]
    pre = DevicePreprocessor("cuda:0")
    pre.lib = CountingLib(pre.lib, "surya_rec_rectify")
    sizes = lambda n: [(1024, 256)] * n
    # 1. a call without a quad: the parent's call -- the new entry point is not reached
    plain = [bbox_ref(0, 256, 256, [10, 20, 240, 60]), poly_ref(0, 256, 256, [[20, 120], [230, 128], [228, 170], [18, 160]]),
             bbox_ref(1, 131, 90, [3, 5, 120, 47])]
    t0, o0, g0 = pre(pages, plain, sizes(3))
    assert pre.lib.calls == 0
    # 2. an axis-aligned rectangle forced through the warp: bbox_ref's tiles, bit for bit
    forced = bbox_ref(0, 256, 256, [10, 20, 240, 60])
    forced.quad = ((10.0, 20.0), (240.0, 20.0), (240.0, 60.0), (10.0, 60.0))
    odd = bbox_ref(1, 131, 90, [3, 5, 120, 47])                              # a size that takes both resampling stages
    odd.quad = ((3.0, 5.0), (120.0, 5.0), (120.0, 47.0), (3.0, 47.0))
    quads = [tilted(128.0, 100.0, 200.0, 30.0, 12.0), tilted(120.0, 180.0, 90.0, 14.0, -27.0), [(30.0, 30.0), (220.0, 40.0), (210.0, 90.0), (35.0, 70.0)],
             tilted(110.0, 70.0, 60.0, 16.0, 20.0)]
    qpage = [0, 0, 0, 1]                                                     # the last one hangs over page 1's right edge
    lines = [forced, plain[1], odd] + [quad_ref(pi, pages[pi].shape[1], pages[pi].shape[0], q) for pi, q in zip(qpage, quads)] + [plain[0], plain[2]]
    t1, o1, g1 = pre(pages, lines, sizes(len(lines)))
    assert pre.lib.calls == 1
    rows = lambda t, o, i: t[int(o[i]):int(o[i + 1])]
    assert g1[0] == g0[0] and torch.equal(rows(t1, o1, 0), rows(t0, o0, 0))
    assert g1[2] == g0[2] and torch.equal(rows(t1, o1, 2), rows(t0, o0, 2))
    # ... and the lines without a quad do not notice their neighbours
    assert torch.equal(rows(t1, o1, 1), rows(t0, o0, 1)) and torch.equal(rows(t1, o1, 7), rows(t0, o0, 0)) and torch.equal(rows(t1, o1, 8), rows(t0, o0, 2))
    # 3. tilted quads: the host chain on warp_quad's pixels
    worst = 0.0
    for k, (pi, q) in enumerate(zip(qpage, quads)):
        W, H = quad_size(q)
        assert lines[3 + k].shape == (H, W, 3)
        crop = warp_quad(pages[pi], quad_homography(q, W, H), W, H)[..., :3].astype(np.float32)
        ref, grid = proc.process_and_tile(proc.scale_to_fit(crop, (1024, 256)))
        got = rows(t1, o1, 3 + k).cpu().numpy()
        assert g1[3 + k] == grid and got.shape == ref.shape
        worst = max(worst, float(np.abs(got - ref).max()))
    print("rectified tiles vs host chain: worst |diff| =", worst)
    assert worst <= 2e-5, worst
    # 4. the plain call again: what it returned before
    t2, o2, g2 = pre(pages, plain, sizes(3))
    assert pre.lib.calls == 1 and g2 == g0 and np.array_equal(o2, o0) and torch.equal(t2, t0)


# ------------------------------------------------------------------------------------------------------------ the predictor
def _five_lines():
    """Two 256^2 pages, five polygon lines in page order: three tilted ones, then two axis-aligned rectangles."""
    pages = [Image.fromarray(p) for p in make_pages(2, 256, seed=8)]
    ints = lambda q: [[int(round(x)), int(round(y))] for x, y in q]
    polys = [[ints(tilted(128, 50, 200, 28, 9.0)), ints(tilted(120, 130, 150, 24, -14.0)), ints(tilted(130, 205, 180, 26, 21.0))],
             [[[30, 30], [220, 30], [220, 60], [30, 60]], [[10, 200], [240, 200], [240, 240], [10, 240]]]]
    return pages, polys


def _dump(results):
    return [r.model_dump() for r in results]


def test_predictor_rectifies_on_both_paths_and_switches_off_cleanly(hip_lib):
    from test_gpu_predictors import make_rec_predictor
    pages, polys = _five_lines()
    cfg, sd, fresh = make_rec_predictor(max_slots=8, max_tokens=8)
    baseline = fresh(pages, polygons=polys)
    cfg, sd, pred = make_rec_predictor(max_slots=8, max_tokens=8)
    out = {}
    try:
        pred.rectify = True
        for dev in (True, False):
            pred.device_preprocess = dev
            out[dev] = pred(pages, polygons=polys)
        for a, b in zip(out[True], out[False]):
            assert [l.text for l in a.text_lines] == [l.text for l in b.text_lines]
            assert [l.polygon for l in a.text_lines] == [l.polygon for l in b.text_lines]
            for la, lb in zip(a.text_lines, b.text_lines):
                assert [c.polygon for c in la.chars] == [c.polygon for c in lb.chars] and la.rectified is lb.rectified
        lines = [l for r in out[True] for l in r.text_lines]
        assert [l.rectified for l in lines] == [True, True, True, False, False]
        assert [l.polygon for l in lines] == [[[float(x), float(y)] for x, y in p] for pg in polys for p in pg]     # the polygon that came in
        assert sum(len(l.chars) for l in lines[:3]) > 0
        # the two lines that were not warped are the parent's, field for field
        strip = lambda d: {k: v for k, v in d.items() if k != "rectified"}
        assert [strip(l.model_dump()) for l in out[True][1].text_lines] == [l.model_dump() for l in baseline[1].text_lines]
        # a threshold between the tilts: only the steeper lines are warped
        pred.device_preprocess, pred.rectify = True, 12.0
        assert [l.rectified for r in pred(pages, polygons=polys) for l in r.text_lines] == [False, True, True, False, False]
        # together with a pattern: both fields are reported
        pred.rectify, pred.pattern = True, r"\d+"
        both = [l for r in pred(pages, polygons=polys) for l in r.text_lines]
        assert [l.rectified for l in both] == [True, True, True, False, False] and all(l.pattern_matched is not None for l in both)
        assert all(set(l.text) <= set("0123456789") for l in both)
    finally:
        pred.rectify = pred.pattern = None
        pred.device_preprocess = True
    again = pred(pages, polygons=polys)
    assert _dump(again) == _dump(baseline) and all(l.rectified is None and "rectified" not in l.model_dump() for r in again for l in r.text_lines)


def _det_with_masks(pages, masks, size, batch):
    """A detector whose text map is replaced by `masks` (one per page), as test_gpu_predictors._det_with_drawn_rows does for
    upright rows: here the rows are tilted quadrilaterals."""
    from surya_amd.detection.predictor import DetectionPredictor
    cfg_d = det_config("DET-TINY")
    masks_d = torch.from_numpy(masks).to("cuda:0")
    page_of = {id(im): i for i, im in enumerate(pages)}

    class Det(DetectionPredictor):
        batch_size = batch

        def batch_heatmaps(self, images, batch_size=None):
            off = 0
            for heat, split_index, split_heights, sizes in super().batch_heatmaps(images, batch_size):
                n = split_index[-1] + 1
                idx = torch.tensor([page_of[id(im)] for im in images[off:off + n]], device=heat.device)
                heat[:, 0] = masks_d[idx].float() * 0.9 + 0.03
                off += n
                yield heat, split_index, split_heights, sizes

    return Det(checkpoint={"config": cfg_d, "state_dict": make_det_weights(cfg_d, 0), "size": size}, dtype=torch.float32)


def test_streamed_detect_recognise_with_rectify_equals_the_serial_call(hip_lib):
    from test_gpu_predictors import make_rec_predictor
    size = 256
    pages = [Image.fromarray(p) for p in make_pages(3, size, seed=11)]
    masks = np.zeros((3, size, size), np.uint8)
    rows = [[tilted(128, 60, 180, 22, 10.0), tilted(128, 170, 170, 24, -12.0)], [tilted(128, 128, 190, 26, 7.0)],
            [tilted(120, 70, 150, 20, 0.0), tilted(130, 190, 160, 24, 15.0)]]
    for i, rr in enumerate(rows):
        for q in rr:
            masks[i] |= fill_poly_mask(size, size, [(int(round(x)), int(round(y))) for x, y in q])
    det = _det_with_masks(pages, masks, size, 2)
    cfg, sd, pred = make_rec_predictor(max_slots=8, max_tokens=7)
    try:
        pred.rectify = True
        pred.stream_detection = False
        serial = pred(pages, det_predictor=det)
        pred.stream_detection = True
        streamed = pred(pages, det_predictor=det)
        assert pred.last_timing.get("streamed") == 1.0
        assert _dump(serial) == _dump(streamed) and len(streamed) == 3
        flags = [l.rectified for r in streamed for l in r.text_lines]
        assert len(flags) >= 5 and all(f is not None for f in flags) and sum(flags) >= 3      # the tilted rows come back as tilted quads
    finally:
        pred.rectify = None
