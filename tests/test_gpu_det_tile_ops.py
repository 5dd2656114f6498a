"""GPU: the two copies of tiled detection alone (surya_det_cut_tiles_u8, surya_det_stitch_tiles; csrc/det_tile.h) against the plain-numpy
statement of tests/det_tile_ref.py, byte for byte and bit for bit, on hand-made data at P = 64; a line across three seams through the
stitch and surya_det_boxes; the refusals. The descriptor tables are built here from det_tile_ref's spans, not by the predictor."""
import ctypes as C

import numpy as np
import pytest
import torch

import det_tile_ref as tr
from surya_amd.detection import heatmap as hm

pytestmark = pytest.mark.gpu
P = 64
SOURCES = [(1, 1), (63, 65), (64, 64), (200, 130), (131, 257)]                      # (w, h)


def _windows(w, h):
    """Inside the page (where it is large enough), flush with each edge, odd origins, hanging over the right / bottom / both edges, and
    over the left / top edge (negative origin)."""
    return [(0, 0), (w - P, h - P), (3, 5), (w - 40, h - 23), (w - 17, 0), (0, h - 9), (-5, -7), ((w - P) // 2, (h - P) // 2), (w + 3, 2)]


@pytest.fixture(scope="module")
def tiler(hip_lib):
    from surya_amd.detection.model import HipDetTiler
    return HipDetTiler()


@pytest.mark.parametrize("shift", [0, 4, 1])          # the pages' addresses: 16-byte aligned, 4-byte aligned only, odd
@pytest.mark.parametrize("dst_pix", [4, 3])
@pytest.mark.parametrize("src_pix", [4, 3])
def test_cut_is_byte_equal(tiler, src_pix, dst_pix, shift):
    from surya_amd.detection.model import CUT_DESC
    rng = np.random.default_rng(src_pix * 16 + dst_pix * 4 + shift)
    pages = [rng.integers(0, 256, (h, w, src_pix), dtype=np.uint8) for w, h in SOURCES]     # (RGBX: junk in the fourth byte)
    offs, total = [], 0
    for pg in pages:
        offs.append(total + shift)
        total = (total + shift + pg.nbytes + 255) & ~255
    buf = np.zeros(total, np.uint8)
    for pg, o in zip(pages, offs):
        buf[o: o + pg.nbytes] = pg.ravel()
    dbuf = torch.from_numpy(buf).cuda()
    jobs = [(k, x0, y0) for k, (w, h) in enumerate(SOURCES) for x0, y0 in _windows(w, h)]
    n = len(jobs)
    order = rng.permutation(n + 2)[:n]                  # a descriptor's tile is not its position; two tiles of the batch stay unwritten
    descs = np.zeros(n, CUT_DESC)
    ref = np.full((n + 2, P, P, dst_pix), 0x5A, np.uint8)
    for i, (k, x0, y0) in enumerate(jobs):
        w, h = SOURCES[k]
        descs[i] = (dbuf.data_ptr() + offs[k], w, h, src_pix, x0, y0, order[i])
        ref[order[i]] = tr.cut_window(pages[k], x0, y0, P, dst_pix)
    dst = torch.full((n + 2, P, P, dst_pix), 0x5A, dtype=torch.uint8, device="cuda")
    tiler.cut(tiler.table(descs), n, dst)
    assert np.array_equal(dst.cpu().numpy(), ref)


@pytest.mark.parametrize("size,dst_pix,off", [(64, 4, 4), (64, 3, 2), (30, 4, 0), (30, 3, 0), (7, 3, 0)])
def test_cut_one_pixel_per_lane_path(tiler, size, dst_pix, off):
    """A tile side that is no multiple of 4, or a batch that is not aligned for the wide store: the byte-store kernel."""
    from surya_amd.detection.model import CUT_DESC
    rng = np.random.default_rng(size + dst_pix + off)
    page = rng.integers(0, 256, (45, 70, 3), dtype=np.uint8)
    dpage = torch.from_numpy(page).cuda()
    wins = [(0, 0), (70 - size, 45 - size), (50, 30), (-3, -2)]
    descs = np.zeros(len(wins), CUT_DESC)
    for i, (x0, y0) in enumerate(wins):
        descs[i] = (dpage.data_ptr(), 70, 45, 3, x0, y0, i)
    nbytes = len(wins) * size * size * dst_pix
    raw = torch.full((nbytes + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    dst = raw[off: off + nbytes].view(len(wins), size, size, dst_pix)
    tiler.cut(tiler.table(descs), len(wins), dst)
    assert np.array_equal(dst.cpu().numpy(), np.stack([tr.cut_window(page, x0, y0, size, dst_pix) for x0, y0 in wins]))
    got = raw.cpu().numpy()
    assert (got[:off] == 0x5A).all() and (got[off + nbytes:] == 0x5A).all()


def _stitch_descs(map_t, mw, mh, overlap, planes, tile0):
    """STITCH_DESC records of one page whose tiles are heat[tile0 ...] in row-major order; map_t: cuda fp32 [planes, mh, pitch]."""
    from surya_amd.detection.model import STITCH_DESC
    pitch = map_t.shape[2]
    assert pitch == (mw + 3) & ~3 and map_t.shape[1] == mh and map_t.is_contiguous()
    out = []
    for y0, ya, yb in tr.spans(mh, P, overlap):
        for x0, xa, xb in tr.spans(mw, P, overlap):
            out.append((map_t.data_ptr(), pitch, mh * pitch, tile0 + len(out), xa - x0, ya - y0, xb - xa, yb - ya, xa, ya, planes,
                        pitch - mw if xb == mw else 0, 0))
    return np.array(out, STITCH_DESC)


GRIDS = [(50, 40, (1, 1)), (200, 61, (4, 1)), (61, 65, (1, 2)), (131, 100, (3, 2))]         # (mw, mh, (columns, rows))
SENTINEL = -3.0


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("overlap", [0, 1, 16])
def test_stitch_is_bit_equal(tiler, overlap, planes):
    rng = np.random.default_rng(overlap * 2 + planes)
    for mw, mh, grid in GRIDS:
        assert (len(tr.offsets(mw, P, overlap)), len(tr.offsets(mh, P, overlap))) == grid
        n = grid[0] * grid[1]
        tiles = rng.random((n + 1, 2, P, P), dtype=np.float32)                    # every tile its own values: a wrong owner shows
        heat = torch.from_numpy(tiles).cuda()
        pitch = (mw + 3) & ~3
        ref = tr.stitch(tiles[1:], mw, mh, P, overlap, planes=planes, out=np.full((planes, mh, pitch), SENTINEL, np.float32))
        assert not (ref == SENTINEL).any() and (pitch == mw or not ref[:, :, mw:].any())
        # a guard row in front of and behind the map: nothing is written outside it
        raw = torch.full((planes * mh * pitch + 2 * pitch,), SENTINEL, dtype=torch.float32, device="cuda")
        m = raw[pitch: pitch + planes * mh * pitch].view(planes, mh, pitch)
        descs = _stitch_descs(m, mw, mh, overlap, planes, 1)
        tiler.stitch(heat, tiler.table(descs[rng.permutation(n)]), n)
        got = raw.cpu().numpy()
        assert np.array_equal(got[pitch: -pitch].reshape(planes, mh, pitch).view(np.int32), ref.view(np.int32)), (mw, mh)
        assert (got[:pitch] == SENTINEL).all() and (got[-pitch:] == SENTINEL).all()


def test_stitch_unaligned_map_rows(tiler):
    """A map whose rows do not start on 16 bytes (a pitch that is no multiple of 4, a map 4 bytes into its allocation) and a tile whose owned
    rectangle starts at an odd column: the lanes in front of the first 16-byte boundary and the four-load form of the wide store."""
    from surya_amd.detection.model import STITCH_DESC
    rng = np.random.default_rng(3)
    tiles = rng.random((2, 1, P, P), dtype=np.float32)
    heat = torch.from_numpy(tiles).cuda()
    pitch, rows = 75, 50
    raw = torch.full((rows * pitch + 1,), SENTINEL, dtype=torch.float32, device="cuda")
    m = raw[1:]
    descs = np.array([(m.data_ptr(), pitch, rows * pitch, 0, 3, 2, 37, 40, 1, 5, 1, 3, 0),
                      (m.data_ptr(), pitch, rows * pitch, 1, 0, 0, 30, 45, 41, 5, 1, 0, 0)], STITCH_DESC)
    ref = np.full((rows, pitch), SENTINEL, np.float32)
    ref[5:45, 1:38] = tiles[0, 0, 2:42, 3:40]
    ref[5:45, 38:41] = 0
    ref[5:50, 41:71] = tiles[1, 0, 0:45, 0:30]
    tiler.stitch(heat, tiler.table(descs), 2)
    assert np.array_equal(m.cpu().numpy().reshape(rows, pitch).view(np.int32), ref.view(np.int32))


def test_stitch_two_pages_one_launch_and_one_page_two_launches(tiler):
    rng = np.random.default_rng(11)
    (mwa, mha), (mwb, mhb), overlap = (131, 100), (61, 65), 16
    na, nb = 6, 2
    tiles = rng.random((na + nb, 2, P, P), dtype=np.float32)
    heat = torch.from_numpy(tiles).cuda()

    def fresh(mw, mh):
        return torch.full((2, mh, (mw + 3) & ~3), SENTINEL, dtype=torch.float32, device="cuda")
    ma, mb_ = fresh(mwa, mha), fresh(mwb, mhb)
    da, db = _stitch_descs(ma, mwa, mha, overlap, 2, 0), _stitch_descs(mb_, mwb, mhb, overlap, 2, na)
    both = np.concatenate([da, db])[rng.permutation(na + nb)]
    tiler.stitch(heat, tiler.table(both), na + nb)
    ref_a, ref_b = tr.stitch(tiles[:na], mwa, mha, P, overlap), tr.stitch(tiles[na:], mwb, mhb, P, overlap)
    assert np.array_equal(ma.cpu().numpy().view(np.int32), ref_a.view(np.int32))
    assert np.array_equal(mb_.cpu().numpy().view(np.int32), ref_b.view(np.int32))
    # page A again, its tiles in two forwards of three: tile indices restart, the second launch completes the first
    m2 = fresh(mwa, mha)
    d2 = _stitch_descs(m2, mwa, mha, overlap, 2, 0)
    d2["tile"] %= 3
    first, second = torch.from_numpy(tiles[:3]).cuda(), torch.from_numpy(tiles[3:6]).cuda()
    tiler.stitch(first, tiler.table(d2[:3]), 3)
    part = tr.stitch(tiles[:na], mwa, mha, P, overlap, out=np.full(ref_a.shape, SENTINEL, np.float32), only={0, 1, 2})
    assert (part == SENTINEL).any()
    assert np.array_equal(m2.cpu().numpy().view(np.int32), part.view(np.int32))                     # cells no tile owns yet: untouched
    tiler.stitch(second, tiler.table(d2[3:]), 3)
    assert np.array_equal(m2.cpu().numpy().view(np.int32), ref_a.view(np.int32))


def test_a_line_across_three_seams_is_one_box_on_the_device(tiler):
    from surya_amd.detection.model import HipDetPost
    m = tr.bar_map()
    tiles = tr.cut_map(m[None], P, 16)                                                  # cut on the host: [12, 1, 64, 64]
    heat = torch.from_numpy(tiles).cuda()
    page = torch.full((1, 160, 200), SENTINEL, dtype=torch.float32, device="cuda")
    tiler.stitch(heat, tiler.table(_stitch_descs(page, 200, 160, 16, 1, 0)), len(tiles))
    assert np.array_equal(page.cpu().numpy()[0], m)
    (boxes, conf), = HipDetPost()(page, 0.6, 0.35)
    ref_boxes, ref_conf = hm.detect_boxes(m, 0.6, 0.35)
    assert len(boxes) == len(ref_boxes) == 1
    assert np.abs(boxes[0] - np.asarray(ref_boxes[0], np.float32)).max() <= 1e-3
    assert np.allclose(conf, np.asarray(ref_conf, np.float32), rtol=0, atol=1e-7)


def test_refusals(tiler):
    from surya_amd import _lib as L
    from surya_amd.detection.model import CUT_DESC, STITCH_DESC
    page = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    dst = torch.full((2, P, P, 4), 0x5A, dtype=torch.uint8, device="cuda")
    heat = torch.ones((2, 2, P, P), dtype=torch.float32, device="cuda")
    m = torch.full((1, 8, 8), SENTINEL, dtype=torch.float32, device="cuda")
    good_cut = np.array([(page.data_ptr(), 8, 8, 3, 0, 0, 0)], CUT_DESC)
    good_st = np.array([(m.data_ptr(), 8, 64, 0, 0, 0, 8, 8, 0, 0, 1, 0, 0)], STITCH_DESC)
    ct, stt = tiler.table(good_cut), tiler.table(good_st)
    cut, st = tiler.lib.surya_det_cut_tiles_u8, tiler.lib.surya_det_stitch_tiles
    z = C.c_void_p(0)
    for args in ((z, 1, L.ptr(dst), 2, P, 4), (L.ptr(ct), 1, z, 2, P, 4), (L.ptr(ct), -1, L.ptr(dst), 2, P, 4), (L.ptr(ct), 1, L.ptr(dst), 0, P, 4),
                 (L.ptr(ct), 1, L.ptr(dst), 2, 0, 4), (L.ptr(ct), 1, L.ptr(dst), 2, -P, 4), (L.ptr(ct), 1, L.ptr(dst), 2, P, 5),
                 (L.ptr(ct), 1, L.ptr(dst), 2, P, 2), (L.ptr(ct), 65536, L.ptr(dst), 2, P, 4)):
        assert cut(*args, z) == L.SA_ERR_ARG, args
    for args in ((z, 2, 2, P, L.ptr(stt), 1), (L.ptr(heat), 2, 2, P, z, 1), (L.ptr(heat), 2, 2, P, L.ptr(stt), -1), (L.ptr(heat), 0, 2, P, L.ptr(stt), 1),
                 (L.ptr(heat), 2, 0, P, L.ptr(stt), 1), (L.ptr(heat), 2, 2, 0, L.ptr(stt), 1), (L.ptr(heat), 2, 2, P, L.ptr(stt), 65536)):
        assert st(*args, z) == L.SA_ERR_ARG, args
    assert cut(L.ptr(ct), 0, L.ptr(dst), 2, P, 4, z) == 0 and st(L.ptr(heat), 2, 2, P, L.ptr(stt), 0, z) == 0       # n == 0: nothing launched
    torch.cuda.synchronize()
    assert (dst == 0x5A).all() and (m == SENTINEL).all()                           # nothing was launched by any of them
    # what the device table itself says is checked on the device: such a descriptor writes nothing
    bad_cut = np.concatenate([good_cut] * 5)
    bad_cut["pix"][0], bad_cut["tile"][1], bad_cut["tile"][2], bad_cut["w"][3], bad_cut["src"][4] = 5, 2, -1, 0, 0
    tiler.cut(tiler.table(bad_cut), 5, dst)
    bad_st = np.concatenate([good_st] * 7)
    bad_st["tile"][0], bad_st["tw"][1], bad_st["tx0"][2], bad_st["planes"][3], bad_st["pad_cols"][4], bad_st["dst"][5], bad_st["dy0"][6] = 2, 0, 60, 3, 4, 0, -1
    tiler.stitch(heat, tiler.table(bad_st), 7)
    torch.cuda.synchronize()
    assert (dst == 0x5A).all() and (m == SENTINEL).all()
    tiler.cut(ct, 1, dst)
    tiler.stitch(heat, stt, 1)
    assert (dst[0, :8, :8, :3] == 0).all() and (dst[0, 8:, :, :3] == 255).all() and (dst[1] == 0x5A).all() and (m == 1.0).all()
