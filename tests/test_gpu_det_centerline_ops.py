"""GPU: surya_det_centerlines alone, on caller-owned buffers, behind a surya_det_boxes call of the same maps, against the numpy reference
(surya_amd/detection/centerline.py): cnt, sum, lo, hi and axis EQUAL. Every case poisons the five output arrays (which are longer than the
call writes) and checks that their tails stay poisoned, and that the boxes workspace is byte-identical before and after the call; every
refusal returns its code with the outputs untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

import det_centerline_ref as R
from surya_amd import _lib as L
from surya_amd.detection import centerline as cl

pytestmark = pytest.mark.gpu
POISON64, POISON32, TAIL = -0x0123456789ABCDEF, -0x1234567, 5


@pytest.fixture(scope="module")
def lib(hip_lib):
    return L.bind_det_centerlines(L.lib())


def _run(lib, maps, knots, max_boxes=512):
    """maps: list of fp32 [H, W] of one shape. surya_det_boxes, then surya_det_centerlines on its workspace. Returns (count [B], outputs)
    after the tail and workspace checks."""
    B, (H, W) = len(maps), maps[0].shape
    heat = torch.from_numpy(np.stack(maps)).cuda()
    need = int(lib.surya_det_boxes_workspace_bytes(B, H, W, max_boxes))
    ws = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    boxes = torch.zeros((B, max_boxes, 4, 2), dtype=torch.float32, device="cuda")
    conf = torch.zeros((B, max_boxes), dtype=torch.float32, device="cuda")
    count = torch.zeros((B,), dtype=torch.int32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.surya_det_boxes(L.ptr(heat), C.c_long(H * W), C.c_int(B), C.c_int(H), C.c_int(W), C.c_float(R.TEXT_T), C.c_float(R.LOW_T),
                             C.c_int(max_boxes), L.ptr(boxes), L.ptr(conf), L.ptr(count), L.ptr(ws), C.c_size_t(need), stream)
    assert rc == 0
    torch.cuda.synchronize()
    before = ws.clone()
    n = B * max_boxes * knots
    cnt = torch.full((n + TAIL,), POISON32, dtype=torch.int32, device="cuda")
    sm = torch.full((n + TAIL,), POISON64, dtype=torch.int64, device="cuda")
    lo = torch.full((n + TAIL,), POISON32, dtype=torch.int32, device="cuda")
    hi = torch.full((n + TAIL,), POISON32, dtype=torch.int32, device="cuda")
    axis = torch.full((B * max_boxes + TAIL,), POISON32, dtype=torch.int32, device="cuda")
    rc = lib.surya_det_centerlines(B, H, W, max_boxes, knots, L.ptr(ws), need, L.ptr(cnt), L.ptr(sm), L.ptr(lo), L.ptr(hi), L.ptr(axis), stream)
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(ws, before), "surya_det_centerlines wrote to the boxes workspace"
    out = {}
    for name, t, m, poison in (("cnt", cnt, n, POISON32), ("sum", sm, n, POISON64), ("lo", lo, n, POISON32), ("hi", hi, n, POISON32),
                               ("axis", axis, B * max_boxes, POISON32)):
        h = t.cpu().numpy()
        assert (h[m:] == poison).all(), f"{name}: the tail behind the array was written"
        out[name] = h[:m].reshape((B, max_boxes, knots) if name != "axis" else (B, max_boxes))
    out["cnt"], out["sum"] = out["cnt"].view(np.uint32), out["sum"].view(np.uint64)
    return count.cpu().numpy(), out


def _check(lib, maps, knots, max_boxes=512):
    count, out = _run(lib, maps, knots, max_boxes)
    for b, m in enumerate(maps):
        want = cl.profile_page(m, R.TEXT_T, R.LOW_T, knots)
        n = len(want["axis"])
        if n > max_boxes:
            assert count[b] == -1
            n = 0                                                      # an overflowed page: every bin empty, every axis -1
        else:
            assert count[b] == n, (b, count[b], n)
            for k in ("cnt", "sum", "lo", "hi", "axis"):
                assert out[k][b, :n].dtype == want[k].dtype and np.array_equal(out[k][b, :n], want[k]), (b, m.shape, knots, k)
        e = cl.empty_profile(max_boxes - n, knots)
        for k in ("cnt", "sum", "lo", "hi", "axis"):
            assert np.array_equal(out[k][b, n:], e[k]), (b, m.shape, knots, k, "beyond the page's count")
    return count, out


@pytest.mark.parametrize("name", R.ADVERSARIAL)
def test_adversarial_pages(lib, name):
    count, _ = _check(lib, [R.adversarial(name)], 16)
    assert count[0] >= 1


@pytest.mark.parametrize("shape", [(8, 8), (40, 68), (300, 260)])
def test_random_masks_with_runs_across_wave_segments(lib, shape):
    rng = np.random.default_rng(shape[1])
    for density in (0.2, 0.6):
        _check(lib, [R.random_mask(rng, *shape, density=density)], 16)
    full = np.full(shape, R.TEXT, np.float32)                           # one component: every lane of every wave in a run
    full[0, 0] = R.BLANK
    _check(lib, [full], 16)


@pytest.mark.parametrize("case", R.BANDS[:3])
def test_planted_bands(lib, case):
    _check(lib, [R.band_map(*case)[0]], 16)
    _check(lib, [np.ascontiguousarray(R.band_map(*case)[0].T[:, : (case[0] // 4) * 4])], 16)      # upright: axis 1, runs sum x


@pytest.mark.parametrize("shape", [(8, 8192), (8192, 8)])
def test_extreme_shapes(lib, shape):
    rng = np.random.default_rng(5)
    m = np.full(shape, R.BLANK, np.float32)
    if shape[0] < shape[1]:
        m[2:5, :] = R.TEXT                                              # extent 8192 along x
        m[6, 100:8000] = R.TEXT
    else:
        m[:, 2:5] = R.TEXT                                              # extent 8192 along y
        m[100:8000, 6] = R.TEXT
    m[rng.random(shape) < 0.001] = R.BLANK
    count, out = _check(lib, [m], 64)
    assert count[0] >= 2


def test_a_full_8192_by_1024_map_and_a_sum_beyond_32_bits(lib):
    m = np.full((8192, 1024), R.TEXT, np.float32)
    count, out = _check(lib, [m], 4, max_boxes=8)
    assert count[0] == 1 and out["axis"][0, 0] == 1 and out["cnt"][0, 0].tolist() == [2048 * 1024] * 4
    assert out["sum"][0, 0].tolist() == [2048 * (1023 * 1024 // 2)] * 4
    # (no bin of THAT map passes 2^32: 2048 * 523776 = 1.07e9.) A block of 1100 x 1100 at the bottom of an 8192-row map does, at 2 knots:
    m = np.full((8192, 1100), R.BLANK, np.float32)
    m[8192 - 1100:, :] = R.TEXT
    count, out = _check(lib, [m], 2, max_boxes=8)
    assert count[0] == 1 and out["axis"][0, 0] == 0 and int(out["sum"][0, 0, 0]) == 550 * sum(range(8192 - 1100, 8192)) > 2 ** 32


def test_three_pages_one_blank_one_over_max_boxes(lib):
    maps = [R.adversarial("many_a"), np.full((64, 128), R.BLANK, np.float32), R.adversarial("segments_a")]
    count, out = _check(lib, maps, 16, max_boxes=32)
    assert count[0] == -1 and count[1] == 0 and count[2] == 31         # 320, 0 and 31 kept components
    assert (out["axis"][0] == -1).all() and (out["axis"][1] == -1).all()
    count, _ = _check(lib, maps, 16, max_boxes=512)                     # with room: all three pages counted
    assert count[0] == 320


@pytest.mark.parametrize("knots", [2, 16, 64])
def test_knot_counts(lib, knots):
    rng = np.random.default_rng(knots)
    _check(lib, [R.random_mask(rng, 72, 100, 0.3), R.band_map(72, 100, 12, 5)[0]], knots)


def test_refusals_leave_the_outputs_untouched(lib):
    B, H, W, MB, K = 2, 32, 32, 64, 16
    need = int(lib.surya_det_boxes_workspace_bytes(B, H, W, MB))
    ws = torch.zeros(need + 16, dtype=torch.uint8, device="cuda")
    outs = [torch.full((B * MB * K,), POISON32, dtype=torch.int32, device="cuda"), torch.full((B * MB * K,), POISON64, dtype=torch.int64, device="cuda"),
            torch.full((B * MB * K,), POISON32, dtype=torch.int32, device="cuda"), torch.full((B * MB * K,), POISON32, dtype=torch.int32, device="cuda"),
            torch.full((B * MB,), POISON32, dtype=torch.int32, device="cuda")]
    good = dict(B=B, H=H, W=W, MB=MB, K=K, ws=L.ptr(ws), ws_bytes=need, cnt=L.ptr(outs[0]), sum=L.ptr(outs[1]), lo=L.ptr(outs[2]), hi=L.ptr(outs[3]),
                axis=L.ptr(outs[4]))
    null = C.c_void_p(0)
    cases = [({k: null}, L.SA_ERR_ARG) for k in ("ws", "cnt", "sum", "lo", "hi", "axis")]
    cases += [({"K": 1}, L.SA_ERR_ARG), ({"K": 65}, L.SA_ERR_ARG), ({"K": 0}, L.SA_ERR_ARG), ({"K": -16}, L.SA_ERR_ARG), ({"B": -1}, L.SA_ERR_ARG),
              ({"H": 0}, L.SA_ERR_ARG), ({"W": 0}, L.SA_ERR_ARG), ({"W": -4}, L.SA_ERR_ARG), ({"MB": 0}, L.SA_ERR_ARG), ({"MB": -1}, L.SA_ERR_ARG),
              ({"ws_bytes": need - 1}, L.SA_ERR_ARG), ({"ws_bytes": 0}, L.SA_ERR_ARG), ({"ws": C.c_void_p(ws.data_ptr() + 4)}, L.SA_ERR_ARG),
              ({"W": 30}, L.SA_ERR_SHAPE), ({"W": 31}, L.SA_ERR_SHAPE), ({"H": 8193, "ws_bytes": 1 << 40}, L.SA_ERR_SHAPE),
              ({"W": 8196, "ws_bytes": 1 << 40}, L.SA_ERR_SHAPE)]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    keys = ("B", "H", "W", "MB", "K", "ws", "ws_bytes", "cnt", "sum", "lo", "hi", "axis")
    for change, code in cases:
        a = {**good, **change}
        rc = lib.surya_det_centerlines(*[a[k] for k in keys], stream)
        assert rc == code, (change, rc)
    a = {**good, "B": 0, "ws_bytes": 0}                                 # batch 0: fine, and launches nothing
    assert lib.surya_det_centerlines(*[a[k] for k in keys], stream) == 0
    torch.cuda.synchronize()
    for t, poison in zip(outs, (POISON32, POISON64, POISON32, POISON32, POISON32)):
        assert (t.cpu().numpy() == poison).all()
    # a workspace no surya_det_boxes call filled (zeros: a blank page state) is read without harm: every bin empty
    assert lib.surya_det_centerlines(*[good[k] for k in keys], stream) == 0
    torch.cuda.synchronize()
    assert (outs[0].cpu().numpy() == 0).all() and (outs[4].cpu().numpy() == -1).all()


def test_hip_det_centerlines_wrapper(hip_lib):
    from surya_amd.detection.model import HipDetCenterlines, HipDetPost
    post, op = HipDetPost("cuda:0", max_boxes=64), HipDetCenterlines("cuda:0")
    op.HEAD = 4                                                         # pages with more components fetch their rows at collect
    maps = [R.band_map(64, 128, 15, 5)[0], R.adversarial("many_a"), R.adversarial("segments_a")]
    heat = torch.from_numpy(np.stack(maps)).cuda()
    for arr in (heat, torch.stack([heat, torch.ones_like(heat)], 1).contiguous()):      # [B, H, W] and [B, labels, H, W]
        pending = post.launch(arr, R.TEXT_T, R.LOW_T)
        cp = op.launch(post, arr, 16)
        got = post.collect(pending)
        profs = op.collect(cp, [len(bx) for bx, _ in got], (R.TEXT_T, R.LOW_T))
        for m, prof in zip(maps, profs):                                # many_a has more than 64 components: run again with room
            assert R.same(prof, cl.profile_page(m, R.TEXT_T, R.LOW_T, 16))
