"""GPU: surya_det_skew alone, on caller-owned buffers, against the numpy reference (surya_amd/detection/skew.py): scores and n_text EQUAL.
Every case poisons the workspace and the two output arrays (which are longer than [batch][n_angles] / [batch]) before the call and checks
that nothing beyond them changed; every refusal returns its code with the outputs untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

import det_skew_ref as R
from surya_amd import _lib as L
from surya_amd.detection import skew as sk

pytestmark = pytest.mark.gpu
THR = 0.35
POISON64, POISON32, TAIL = -0x0123456789ABCDEF, -0x1234567, 5


@pytest.fixture(scope="module")
def lib(hip_lib):
    return L.bind_det_skew(L.lib())


def _run(lib, maps, tables, thr=THR, stride=None, fill=7.5):
    """maps: list of fp32 [H, W]; tables: int32 [B, n, 2]. Returns (rc, scores uint64 [B, n], n_text [B]) after the tail checks."""
    B, (H, W) = len(maps), maps[0].shape
    tables = np.ascontiguousarray(tables, np.int32)
    n = tables.shape[1]
    stride = H * W if stride is None else stride
    host = np.full((B, stride), fill, np.float32)                      # what lies between the pages is text-valued poison
    for b, m in enumerate(maps):
        host[b, : H * W] = m.reshape(-1)
    heat = torch.from_numpy(host).cuda()
    cs = torch.from_numpy(tables).cuda()
    scores = torch.full((B * n + TAIL,), POISON64, dtype=torch.int64, device="cuda")
    n_text = torch.full((B + TAIL,), POISON32, dtype=torch.int32, device="cuda")
    need = int(lib.surya_det_skew_workspace_bytes(B, H, W))
    assert need == B * H * W * 4
    ws = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = lib.surya_det_skew(L.ptr(heat), stride, B, H, W, thr, L.ptr(cs), n, L.ptr(scores), L.ptr(n_text), L.ptr(ws), need,
                            C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    s, t = scores.cpu().numpy(), n_text.cpu().numpy()
    assert (s[B * n:] == POISON64).all() and (t[B:] == POISON32).all() and (ws[need:].cpu().numpy() == 0xA5).all()
    return rc, s[: B * n].view(np.uint64).reshape(B, n), t[:B]


def _check(lib, maps, tables, thr=THR, stride=None):
    rc, s, t = _run(lib, maps, tables, thr, stride)
    assert rc == 0
    for b, m in enumerate(maps):
        want, n = sk.skew_scores(m, thr, tables[b])
        assert t[b] == n and np.array_equal(s[b], want), (b, m.shape, t[b], n, s[b][:4], want[:4])
    return s, t


@pytest.fixture(scope="module")
def table121():
    return sk.coeffs(sk.candidate_angles(sk.SkewEstimate()))


@pytest.mark.parametrize("shape", [(64, 64), (96, 160), (256, 256)])
def test_one_page(lib, table121, shape):
    rng = np.random.default_rng(shape[0])
    m = R.band_map(3.0, 256)[: shape[0], : shape[1]].copy()
    m[rng.random(shape) < 0.01] = R.TEXT                                # specks off the bands
    s, t = _check(lib, [m], table121[None])
    assert t[0] > 200 and len(set(s[0].tolist())) > 10


def test_three_pages_each_with_its_own_table(lib):
    rng = np.random.default_rng(2)
    maps = [R.random_mask(rng, 72, 100, 0.15), np.full((72, 100), R.BLANK, np.float32), np.full((72, 100), R.TEXT, np.float32)]
    tables = np.stack([R.random_table(rng, 33), R.random_table(rng, 33), sk.coeffs(np.linspace(-45, 45, 33))])
    s, t = _check(lib, maps, tables)
    assert t.tolist()[1:] == [0, 7200] and not s[1].any() and s[2].all()


def test_page_stride_with_poison_between_the_pages(lib):
    rng = np.random.default_rng(3)
    maps = [R.random_mask(rng, 40, 52, 0.2), R.random_mask(rng, 40, 52, 0.4)]
    _check(lib, maps, np.stack([R.random_table(rng, 17)] * 2), stride=40 * 52 + 1000)


def test_zero_pad_columns_and_values_at_the_threshold(lib, table121):
    rng = np.random.default_rng(4)
    m = R.random_mask(rng, 50, 64, 0.25)
    m[:, 61:] = 0.0                                                     # a stitched map's pad: W = 64, 61 valid columns
    m[10:14, :30] = THR                                                 # exactly at the threshold: excluded
    m[20, :30] = np.nextafter(np.float32(THR), np.float32(1))
    _, t = _check(lib, [m], table121[None])
    assert t[0] == int((m > np.float32(THR)).sum())
    _, t0 = _check(lib, [m], table121[None], thr=0.0)                   # threshold 0: the pad columns still never count
    assert t0[0] == int((m[:, :61] > 0).sum()) == 50 * 61


@pytest.mark.parametrize("shape", [(8, 8192), (8192, 8)])
def test_extreme_shapes(lib, shape):
    rng = np.random.default_rng(5)
    m = R.corner_map(*shape)
    m[rng.random(shape) < 0.02] = R.TEXT
    tab = np.concatenate([sk.coeffs([-45.0, 0.0, 45.0]), R.random_table(rng, 5)])
    _check(lib, [m], tab[None])


@pytest.mark.parametrize("n", [1, 121, 1024])
def test_angle_counts(lib, n):
    rng = np.random.default_rng(n)
    m = R.random_mask(rng, 36, 44, 0.3)
    _check(lib, [m], sk.coeffs(np.linspace(-45.0, 45.0, n) if n > 1 else [2.0])[None])


def test_a_table_outside_the_contract_counts_no_bin_outside_the_histogram(lib):
    """Coefficients beyond |theta| <= 45 degrees: most bins fall outside [0, nb) and are dropped, as the reference drops them."""
    rng = np.random.default_rng(6)
    m = R.random_mask(rng, 64, 64, 0.3)
    tab = np.array([[65536, 200000], [65536, -200000], [-65536, 0], [1 << 20, 1 << 20]], np.int32)
    _check(lib, [m], tab[None])


def test_refusals_leave_the_outputs_untouched(lib):
    m = torch.full((2, 32, 32), 0.9, dtype=torch.float32, device="cuda")
    cs = torch.from_numpy(np.stack([sk.coeffs([0.0, 1.0])] * 2)).cuda()
    scores = torch.full((4,), POISON64, dtype=torch.int64, device="cuda")
    n_text = torch.full((2,), POISON32, dtype=torch.int32, device="cuda")
    ws = torch.empty(2 * 32 * 32 * 4, dtype=torch.uint8, device="cuda")
    good = dict(heat=L.ptr(m), stride=1024, B=2, H=32, W=32, thr=0.35, cs=L.ptr(cs), n=2, scores=L.ptr(scores), n_text=L.ptr(n_text), ws=L.ptr(ws),
                ws_bytes=ws.numel())
    null = C.c_void_p(0)
    cases = [({"heat": null}, L.SA_ERR_ARG), ({"cs": null}, L.SA_ERR_ARG), ({"scores": null}, L.SA_ERR_ARG), ({"n_text": null}, L.SA_ERR_ARG),
             ({"ws": null}, L.SA_ERR_ARG), ({"B": -1}, L.SA_ERR_ARG), ({"H": 0}, L.SA_ERR_ARG), ({"W": 0}, L.SA_ERR_ARG), ({"W": -4}, L.SA_ERR_ARG),
             ({"n": 0}, L.SA_ERR_ARG), ({"n": 1025}, L.SA_ERR_ARG), ({"thr": -0.01}, L.SA_ERR_ARG), ({"thr": float("nan")}, L.SA_ERR_ARG),
             ({"ws_bytes": 2 * 32 * 32 * 4 - 1}, L.SA_ERR_ARG), ({"H": 8193}, L.SA_ERR_SHAPE), ({"W": 8196}, L.SA_ERR_SHAPE),
             ({"W": 30}, L.SA_ERR_SHAPE), ({"W": 31}, L.SA_ERR_SHAPE)]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for change, code in cases:
        a = {**good, **change}
        rc = lib.surya_det_skew(a["heat"], a["stride"], a["B"], a["H"], a["W"], a["thr"], a["cs"], a["n"], a["scores"], a["n_text"], a["ws"],
                                a["ws_bytes"], stream)
        assert rc == code, (change, rc)
    a = {**good, "B": 0}                                                # batch 0: fine, and launches nothing
    assert lib.surya_det_skew(a["heat"], a["stride"], 0, a["H"], a["W"], a["thr"], a["cs"], a["n"], a["scores"], a["n_text"], a["ws"], 0, stream) == 0
    torch.cuda.synchronize()
    assert (scores.cpu().numpy() == POISON64).all() and (n_text.cpu().numpy() == POISON32).all()
    assert lib.surya_det_skew_workspace_bytes(0, 32, 32) == 0 and lib.surya_det_skew_workspace_bytes(2, 0, 32) == 0
    rc = lib.surya_det_skew(*[good[k] for k in ("heat", "stride", "B", "H", "W", "thr", "cs", "n", "scores", "n_text", "ws", "ws_bytes")], stream)
    torch.cuda.synchronize()
    assert rc == 0 and n_text.cpu().tolist() == [1024, 1024] and scores.cpu().tolist()[0] == 32 * 32


def test_hip_det_skew_wrapper(hip_lib, table121):
    from surya_amd.detection.model import HipDetSkew
    op = HipDetSkew("cuda:0")
    maps = np.stack([R.band_map(2.0, 128), R.band_map(-7.5, 128)])
    four = np.stack([maps, np.ones_like(maps)], 1)                      # [B, labels, H, W]: plane 0 is the text map
    tables = np.stack([table121] * 2)
    for arr in (maps, four):
        s, t = op(torch.from_numpy(np.ascontiguousarray(arr)).cuda(), tables, THR)
        assert s.dtype == np.uint64 and s.shape == (2, 121)
        for b in range(2):
            want, n = sk.skew_scores(maps[b], THR, table121)
            assert t[b] == n and np.array_equal(s[b], want)
