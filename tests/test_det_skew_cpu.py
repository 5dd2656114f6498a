"""CPU: page skew from the heat map (surya_amd/detection/skew.py states the rule in plain numpy). The host build of csrc/det_skew_core.h --
the arithmetic the kernels run -- against that reference, scores EQUAL; invariances of the reference; planted angles on synthetic maps
(bound: 0.5 degrees = two steps of the default grid, set by the issue; the rule measured at most 0.25 on these maps); the choice rule;
every refusal; the serialised form; the host path of `straighten`; header, binding and core header against each other."""
import math
import os
import re

import numpy as np
import pytest
from PIL import Image

import det_skew_ref as R
from surya_amd.detection import skew as sk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = 0.35


def _same_as_host(heat, cs, thr=THR):
    want, n = sk.skew_scores(heat, thr, cs)
    got, gn = R.host_scores(heat, thr, cs)
    assert gn == n and got.dtype == want.dtype == np.uint64 and np.array_equal(got, want), (heat.shape, got, want)
    return want, n


def test_host_build_equals_numpy_on_random_masks():
    rng = np.random.default_rng(11)
    fixed = sk.coeffs([-45.0, 0.0, 45.0])
    assert fixed.tolist() == [[46341, -46341], [65536, 0], [46341, 46341]]
    for k in range(12):
        H, W = (int(v) for v in rng.integers(8, 301, 2))
        m = R.random_mask(rng, H, W, density=(0.02, 0.2, 0.6)[k % 3])
        _same_as_host(m, np.concatenate([fixed, R.random_table(rng, 9)]))


def test_host_build_equals_numpy_on_full_empty_and_extreme_maps():
    rng = np.random.default_rng(12)
    table = np.concatenate([sk.coeffs([-45.0, 0.0, 45.0]), R.random_table(rng, 5)])
    full, n = _same_as_host(np.full((40, 52), R.TEXT, np.float32), table)
    assert n == 40 * 52 and full[1] == 52 * 52                                    # 0 degrees: one step of a row's 52 pixels
    empty, n = _same_as_host(np.full((40, 52), R.BLANK, np.float32), table)
    assert n == 0 and not empty.any()
    for H, W in ((8, 8192), (8192, 8)):                                            # the int32 bound and the bin bound
        m = R.corner_map(H, W)
        sc, n = _same_as_host(m, table)
        assert n == 4
        for c, s in table[:3]:                                                     # the corners' bins are the rule's, first and last included
            off = (W - 1) * max(int(s), 0)
            r = [(y * int(c) - x * int(s) + off) >> 16 for y in (0, H - 1) for x in (0, W - 1)]
            assert min(r) == 0 and max(r) < H + W and (max(r) << 16) < 2 ** 31


def test_threshold_is_strict_and_pad_columns_never_count():
    m = np.zeros((16, 24), np.float32)
    m[4:6, 2:18] = THR                                                             # AT the threshold: not text
    m[9, 3:12] = np.nextafter(np.float32(THR), np.float32(1))
    sc, n = _same_as_host(m, sk.coeffs([0.0, 3.0]))
    assert n == 9 and sc[0] == 2 * 81
    assert sk.skew_scores(m, 0.0, sk.coeffs([0.0]))[1] == 32 + 9                   # threshold 0: zeros (a stitched map's pad) stay out


def test_shift_invariance_at_zero_degrees():
    """Moving the mask inside the map leaves score(0) unchanged (blank rows stay above and below it, as in every placement here)."""
    rng = np.random.default_rng(3)
    core = R.random_mask(rng, 40, 50)
    cs = sk.coeffs([0.0])
    scores = []
    for dy, dx in ((5, 5), (1, 0), (23, 31), (70, 46), (79, 0)):
        m = np.full((120, 96), R.BLANK, np.float32)
        m[dy: dy + 40, dx: dx + 50] = core
        scores.append(sk.skew_scores(m, THR, cs)[0][0])
    assert len(set(scores)) == 1 and scores[0] > 0


def test_left_right_flip_swaps_the_sign_of_the_angle():
    rng = np.random.default_rng(4)
    m = R.random_mask(rng, 70, 90, 0.3)
    cs = R.random_table(rng, 16)
    neg = cs * np.array([1, -1], np.int32)
    assert np.array_equal(sk.skew_scores(m, THR, cs)[0], sk.skew_scores(m[:, ::-1], THR, neg)[0])
    band = R.band_map(7.5)
    est = sk.SkewEstimate()
    a, _, _ = sk.estimate(band, est, (256, 256), THR)
    b, _, _ = sk.estimate(np.ascontiguousarray(band[:, ::-1]), est, (256, 256), THR)
    assert a == -b


@pytest.fixture(scope="module")
def planted():
    return {a: R.band_map(a) for a in R.PLANTS}


@pytest.mark.parametrize("plant", R.PLANTS)
def test_planted_angles(planted, plant):
    est = sk.SkewEstimate()
    angle, conf, n = sk.estimate(planted[plant], est, (256, 256), THR)
    print(f"plant {plant}: estimate {angle}, confidence {conf}, {n} text pixels")
    assert angle is not None and abs(angle - plant) <= 0.5
    assert 0.5 < conf <= 1.0 and n > 5000
    # the same map as a 2 : 1 page: the reported angle is the page-space one, atan(tan(theta_map) * sy / sx)
    a2, _, _ = sk.estimate(planted[plant], est, (512, 256), THR)
    want = math.degrees(math.atan(math.tan(math.radians(plant)) * (256 / 256) / (512 / 256)))
    print(f"  as a 512 x 256 page: estimate {a2}, page-space plant {want}")
    assert abs(a2 - want) <= 0.5
    assert abs(sk.page_angle(plant, (512, 256), (256, 256)) - want) < 1e-12


def test_map_angles_and_tables_follow_the_page():
    ang = sk.candidate_angles(sk.SkewEstimate())
    assert len(ang) == 121 and ang[0] == -15.0 and ang[60] == 0.0 and ang[-1] == 15.0 and ang[61] == 0.25
    assert np.array_equal(sk.coeff_table(ang, (300, 300), (128, 128)), sk.coeffs(ang))          # isotropic: the map angle is the page angle
    th = sk.map_angles([10.0], (200, 100), (128, 128))[0]                                         # sx = 1.5625, sy = 0.78125
    assert abs(math.tan(math.radians(th)) - 2.0 * math.tan(math.radians(10.0))) < 1e-12
    t = sk.coeff_table([10.0], (200, 100), (128, 128))[0]
    assert t.tolist() == [round(math.cos(math.radians(th)) * 65536), round(math.sin(math.radians(th)) * 65536)]


def test_choice_rule():
    ang = np.arange(-2, 3) * 0.25
    assert sk.choose([1, 1, 1, 1, 1], 1000, ang, 0.25, 256) == (None, None)                     # all scores equal
    assert sk.choose([1, 5, 9, 5, 1], 255, ang, 0.25, 256) == (None, None)                      # fewer than min_pixels
    a, c = sk.choose([1, 5, 9, 5, 1], 256, ang, 0.25, 256)
    assert a == 0.0 and c == 1 - 5 / 9                                                         # symmetric neighbours: no shift
    a, _ = sk.choose([1, 5, 9, 7, 1], 999, ang, 0.25, 0)
    assert a == 0.5 * (5 - 7) / (5 - 18 + 7) * 0.25                                            # the parabola's vertex, towards the larger neighbour
    a, _ = sk.choose([0, 0, 9, 9, 0], 999, ang, 0.25, 0)                                       # first maximum; vertex at +step / 2: the clamp's edge
    assert a == 0.125
    a, _ = sk.choose([9, 9, 9, 10, 9.999], 999, ang, 0.25, 0)
    assert a == 0.25 + 0.125 * (9 - 9.999) / (9 - 20 + 9.999) and abs(a - 0.25) <= 0.125
    # a plateau: the FIRST maximum, pulled half a step towards the plateau; a border maximum is not refined
    assert sk.choose([1, 9, 9, 9, 1], 999, ang, 0.25, 0)[0] == -0.125
    assert sk.choose([9, 5, 1, 1, 1], 999, ang, 0.25, 0)[0] == -0.5 and sk.choose([1, 1, 1, 5, 9], 999, ang, 0.25, 0)[0] == 0.5
    # the clamp itself: float64 scores whose vertex lies beyond half a step (cannot come from a true maximum, the rule holds all the same)
    s = np.array([0.0, 10.0, 10.0 + 1e-9, 0.0, 0.0])
    a, _ = sk.choose(s, 999, ang, 0.25, 0)
    assert -0.125 <= a - 0.0 <= 0.125
    # uint64 scores beyond 2^53 go through float64 without an error
    big = np.array([2 ** 60, 2 ** 62, 2 ** 61], np.uint64)
    a, c = sk.choose(big, 999, ang[:3], 0.25, 0)
    assert abs(a + 0.25) <= 0.125 and c == 0.5


def test_min_pixels_and_blank_maps_give_none():
    est = sk.SkewEstimate(min_pixels=256)
    m = np.full((64, 64), R.BLANK, np.float32)
    assert sk.estimate(m, est, (64, 64), THR) == (None, None, 0)
    m[10:12, 5:60] = R.TEXT                                                                    # 110 text pixels
    assert sk.estimate(m, est, (64, 64), THR)[:2] == (None, None)
    a, c, n = sk.estimate(m, sk.SkewEstimate(min_pixels=100), (64, 64), THR)
    assert n == 110 and a is not None and abs(a) <= 1.0 and 0 < c <= 1


def test_every_refusal():
    ok = sk.check_skew(sk.SkewEstimate())
    assert ok.max_angle == 15.0 and ok.step == 0.25 and ok.min_pixels == 256 and ok.threshold is None
    assert sk.check_skew(sk.SkewEstimate(max_angle=45, step=0.1)).max_angle == 45                # 901 candidates
    for bad in (0, -1.0, 45.01, float("nan"), float("inf"), "15", None, True):
        with pytest.raises(ValueError):
            sk.check_skew(sk.SkewEstimate(max_angle=bad))
    for bad in (0, -0.25, float("nan"), "0.25", None, True):
        with pytest.raises(ValueError):
            sk.check_skew(sk.SkewEstimate(step=bad))
    for bad in (-1, 2.5, "3", None, True):
        with pytest.raises(ValueError):
            sk.check_skew(sk.SkewEstimate(min_pixels=bad))
    for bad in (-0.1, float("nan"), "0.3", True):
        with pytest.raises(ValueError):
            sk.check_skew(sk.SkewEstimate(threshold=bad))
    with pytest.raises(ValueError, match="1025 candidates"):
        sk.check_skew(sk.SkewEstimate(max_angle=45.0, step=45.0 / 512))
    assert len(sk.candidate_angles(sk.check_skew(sk.SkewEstimate(max_angle=25.575, step=0.05)))) == 1023
    for bad in ((15.0, 0.25), {"max_angle": 15}, 15.0, "skew"):
        with pytest.raises(ValueError):
            sk.check_skew(bad)
    # a page whose map angle would leave +-45 degrees is named: 15 degrees on a 4 : 1 page squeezed onto a square is atan(4 tan 15) = 47
    pages = [((1000, 1000), (128, 128)), ((4000, 1000), (128, 128))]
    sk.check_skew(sk.SkewEstimate(max_angle=14.0), pages)
    with pytest.raises(ValueError, match="page 1 "):
        sk.check_skew(sk.SkewEstimate(), pages)
    with pytest.raises(ValueError):
        sk.coeffs([45.5])


def test_predictor_refuses_before_any_device_work():
    from surya_amd.detection.predictor import DetectionPredictor, SegformerImageProcessor, SkewEstimate
    pred = DetectionPredictor.__new__(DetectionPredictor)
    pred.processor = SegformerImageProcessor({"height": 64, "width": 64})
    assert pred.skew is None and SkewEstimate is sk.SkewEstimate and DetectionPredictor.last_skew == []
    wide = Image.new("RGB", (400, 100), (255, 255, 255))
    for bad, ims in (((15.0, 0.25), []), (SkewEstimate(max_angle=50), []), (SkewEstimate(step=0.01), []), (SkewEstimate(), [wide])):
        pred.skew = bad
        with pytest.raises(ValueError):
            pred._detect(ims)
        with pytest.raises(ValueError):
            list(pred._iter_detect_device(ims))


def test_serialised_keys_unchanged_while_none():
    from surya_amd.detection.heatmap import TextDetectionResult, result_from_device_boxes
    r = result_from_device_boxes(np.zeros((0, 4, 2), np.float32), np.zeros(0, np.float32), [64, 64], (100, 80))
    assert r.skew is None and r.skew_confidence is None
    assert list(r.model_dump()) == ["bboxes", "vertical_lines", "heatmap", "affinity_map", "image_bbox"]
    assert "skew" not in r.model_dump_json()
    r.skew, r.skew_confidence = 1.25, 0.5
    d = r.model_dump()
    assert list(d)[-2:] == ["skew", "skew_confidence"] and d["skew"] == 1.25 and d["skew_confidence"] == 0.5
    assert {"skew", "skew_confidence"} <= set(TextDetectionResult.model_fields)


def _page(w, h, pix=3, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, pix), dtype=np.uint8)


@pytest.mark.parametrize("phi", [0.0, 3.0, -3.0, 15.0])
def test_straighten_host_path(phi):
    from surya_amd.common.imageops import warp_quad
    page = _page(80, 60)
    im = Image.fromarray(page)
    (st,) = sk.straighten([im], [phi])
    c, s = abs(math.cos(math.radians(phi))), abs(math.sin(math.radians(phi)))
    W, H = math.ceil(80 * c + 60 * s - 1e-9), math.ceil(80 * s + 60 * c - 1e-9)
    assert st.image.size == (W, H) and sk.straighten_size(80, 60, phi) == (W, H)
    pts = np.array([[0.0, 0.0], [W, 0.0], [W / 2, H / 2], [12.5, 40.25]])
    assert np.abs(st.to_page(st.from_page(pts)) - pts).max() <= 1e-9 and np.abs(st.from_page(st.to_page(pts)) - pts).max() <= 1e-9
    if phi == 0.0:
        assert st.image is im and st.angle == 0.0 and np.array_equal(st.to_page(pts), pts)     # the page's own pixels, identity transform
        return
    assert st.angle == phi
    h9 = sk.straighten_matrix(80, 60, phi)
    assert h9[6] == 0 and h9[7] == 0 and h9[8] == 1 and np.array_equal(st.matrix, h9)
    assert np.array_equal(np.asarray(st.image), warp_quad(page, h9, W, H))                     # ONE matrix: the warp's and to_page's
    assert np.abs(st.to_page([[W / 2, H / 2]]) - [[40.0, 30.0]]).max() <= 1e-12                  # centre to centre
    # the output's horizontal direction is the page's baseline direction: down to the right for a positive angle
    d = st.to_page([[1.0, 0.0]]) - st.to_page([[0.0, 0.0]])
    assert abs(math.degrees(math.atan2(d[0, 1], d[0, 0])) - phi) < 1e-9
    # nothing is cut off: the page's corners land inside the output
    corners = st.from_page([[0, 0], [80, 0], [80, 60], [0, 60]])
    assert corners.min() >= -1e-6 and (corners[:, 0] <= W + 1e-6).all() and (corners[:, 1] <= H + 1e-6).all()


def test_straighten_straightens_and_leaves_small_angles_alone():
    band = R.band_map(7.5)
    page = np.repeat(((band < 0.5) * 255).astype(np.uint8)[..., None], 3, 2)                    # dark text on white
    a, b, c = sk.straighten([Image.fromarray(page)] * 3, [7.5, None, 0.05])
    assert b.angle == 0.0 and c.angle == 0.0 and b.image.size == (256, 256) and np.array_equal(np.asarray(c.image), page)
    up = (np.asarray(a.image)[..., 0] < 128).astype(np.float32)
    angle, _, _ = sk.estimate(up, sk.SkewEstimate(), a.image.size, 0.5)
    assert abs(angle) <= 0.5
    x = sk.straighten([page[..., :3], np.dstack([page, page[..., :1]])], [2.0, 2.0])              # arrays, RGB and RGBX: the same pixels
    assert np.array_equal(np.asarray(x[0].image), np.asarray(x[1].image))
    with pytest.raises(ValueError):
        sk.straighten([page], [1.0, 2.0])
    with pytest.raises(ValueError):
        sk.straighten([page], [90.0])


def test_header_bindings_and_core_agree():
    from surya_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "surya_amd.h")).read()
    ws = re.search(r"\bsize_t surya_det_skew_workspace_bytes\(([^;]*)\);", hdr)
    run = re.search(r"\bint surya_det_skew\(([^;]*)\);", hdr)
    assert ws and run
    assert [a.strip() for a in ws.group(1).split(",")] == ["int batch", "int height", "int width"]
    args = [" ".join(a.split()) for a in run.group(1).split(",")]
    assert args == ["const float* heat", "long page_stride", "int batch", "int height", "int width", "float threshold", "const int32_t* cs",
                    "int n_angles", "uint64_t* scores", "int32_t* n_text", "void* workspace", "size_t workspace_bytes", "void* stream"]
    src = open(os.path.join(ROOT, "surya_amd", "_lib.py")).read()
    assert "def bind_det_skew" in src
    if os.path.exists(L.LIB_PATH):
        import ctypes as C
        lib = L.bind_det_skew(L.lib())
        i, p = C.c_int, C.c_void_p
        assert lib.surya_det_skew.argtypes == [p, C.c_long, i, i, i, C.c_float, p, i, p, p, p, C.c_size_t, p] and lib.surya_det_skew.restype is C.c_int
        assert lib.surya_det_skew_workspace_bytes.argtypes == [i, i, i] and lib.surya_det_skew_workspace_bytes.restype is C.c_size_t
        assert lib.surya_det_skew_workspace_bytes(3, 96, 160) == 3 * 96 * 160 * 4 and lib.surya_det_skew_workspace_bytes(0, 96, 160) == 0
    core = open(os.path.join(ROOT, "surya_amd", "csrc", "det_skew_core.h")).read()
    assert f"SKEW_MAX_DIM = {sk.MAX_DIM};" in core and f"SKEW_MAX_ANGLES = {sk.MAX_ANGLES};" in core and "SKEW_FRAC_BITS = 16;" in core
    assert sk.FRAC == 1 << 16
    model = open(os.path.join(ROOT, "surya_amd", "csrc", "det_model.hip")).read()
    assert '#include "det_skew.h"' in model and "int surya_det_skew(" in model
