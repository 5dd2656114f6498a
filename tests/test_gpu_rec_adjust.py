"""GPU: contrast adjustment of line crops on the device (surya_rec_adjust_contrast, csrc/rec_adjust.h), the entry alone on caller-owned
buffers. The reference for every byte is Pillow's ImageOps.autocontrast(crop, cutoff, preserve_tone=True, mask); (lo, hi) are held to
Pillow's own histogram run through Pillow's loops (common/imageops.py::autocontrast_bounds, which tests/test_reread_cpu.py holds to
Pillow end to end).

  * RGB and RGBX pages; crops of 1 x 1, 1 x 7, 3 x 1, 37 x 301, 64 x 512 (several workgroups) and 256 x 1024; crops on every page edge;
    odd byte offsets with 3-byte pixels; cutoffs 0, 1, 10, 49; a flat crop (identity); lo = 0, hi = 25 (lut[hi] = 254);
  * every one of the 32 640 (lo, hi) pairs with its whole LUT;
  * 4-point polygon lines against fill_poly_mask, a sliver among them; 1, 33 and 300 lines per call;
  * a rectified-then-adjusted line; canary bytes around every output range, mask, work area and bounds row; every refusal."""
import ctypes as C

import numpy as np
import pytest
import torch
from PIL import Image, ImageOps

from surya_amd import _lib as L
from surya_amd.common.imageops import autocontrast_bounds, fill_poly_mask, quad_homography, quad_size, warp_quad

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
WORK = 1280


def pillow_adjust(crop, mask, cutoff):
    """(Pillow's adjusted crop, (lo, hi) of Pillow's histogram) of a padded uint8 [h, w, 3] crop; mask [h, w] of 0 / 1 or None."""
    im = Image.fromarray(np.ascontiguousarray(crop))
    m = None if mask is None else Image.fromarray((mask != 0).astype(np.uint8) * 255)
    out = np.asarray(ImageOps.autocontrast(im, cutoff=cutoff, mask=m, preserve_tone=True))
    return out, autocontrast_bounds(im.convert("L").histogram(m), cutoff)


def banded_page(h, w, pix, seed):
    """A page whose 32 x 32 blocks each hold random values of a range of their own: crops of low, mixed and full contrast."""
    rng = np.random.default_rng(seed)
    bh, bw = (h + 31) // 32, (w + 31) // 32
    a = rng.integers(0, 200, size=(bh, bw, 1))
    span = rng.integers(1, 120, size=(bh, bw, 1))
    lo = np.kron(a, np.ones((32, 32, 1), np.int64))[:h, :w]
    sp = np.kron(span, np.ones((32, 32, 1), np.int64))[:h, :w]
    page = (lo + rng.integers(0, 1 << 30, size=(h, w, 3)) % sp).clip(0, 255).astype(np.uint8)
    if pix == 4:
        page = np.concatenate([page, np.full((h, w, 1), 77, np.uint8)], axis=2)
    return page


def make_pages(pix):
    p0, p1 = banded_page(120, 200, pix, 3), banded_page(300, 1100, pix, 4)
    p0[10:20, 10:40, :3] = (90, 140, 31)                                       # a flat crop: one luma level
    ramp = np.random.default_rng(5).integers(0, 26, size=(12, 30, 1))
    ramp[0, 0], ramp[0, 1] = 0, 25
    p0[40:52, 100:130, :3] = ramp                                              # lo = 0, hi = 25
    return [p0, p1]


# (page, x0, y0, w, h, cutoff, polygon relative to the crop origin or None)
SPECIAL = [
    (1, 50, 20, 301, 37, 10, None),
    (0, 10, 10, 30, 10, 10, None),                                             # flat: the identity
    (0, 100, 40, 30, 12, 0, None),                                             # (0, 25)
    (0, 7, 9, 1, 1, 1, None), (0, 11, 3, 7, 1, 49, None), (0, 199, 50, 1, 3, 0, None),
    (1, 500, 100, 512, 64, 1, None),
    (0, 0, 30, 40, 20, 10, None), (0, 60, 0, 50, 16, 49, None), (0, 150, 60, 50, 30, 1, None), (0, 20, 100, 90, 20, 10, None),     # the four edges
    (0, 0, 0, 200, 120, 10, None),                                             # the whole page
    (1, 100, 150, 220, 40, 10, [(3, 6), (216, 0), (219, 33), (0, 39)]),
    (1, 400, 200, 120, 30, 1, [(0, 0), (119, 14), (119, 16), (0, 2)]),         # a sliver
    (0, 30, 60, 64, 24, 49, [(10, 0), (63, 8), (50, 23), (0, 12)]),
    (1, 900, 10, 150, 60, 0, [(0, 0), (150, 0), (150, 60), (0, 60)]),          # the polygon is the crop
    (1, 700, 250, 9, 9, 10, [(4, 4), (5, 4), (5, 5), (4, 5)]),                 # a few pixels inside
    (1, 60, 30, 1024, 256, 10, None),                                          # the largest task size
    (1, 10, 5, 1024, 256, 1, [(0, 20), (1000, 0), (1023, 230), (30, 255)]),
]


def jobs_for(n):
    if n == 1:
        return SPECIAL[:1]
    extra = n - len(SPECIAL)
    rng = np.random.default_rng(n)
    jobs = list(SPECIAL)
    for k in range(extra):
        pi = int(rng.integers(0, 2))
        H, W = (120, 200) if pi == 0 else (300, 1100)
        w, h = int(rng.integers(1, 90)), int(rng.integers(1, 30))
        x0, y0 = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
        poly = None
        if k % 3 == 0 and w > 4 and h > 4:
            poly = [(int(rng.integers(0, w // 2)), int(rng.integers(0, h // 2))), (int(rng.integers(w // 2, w)), int(rng.integers(0, h // 2))),
                    (int(rng.integers(w // 2, w)), int(rng.integers(h // 2, h))), (int(rng.integers(0, w // 2)), int(rng.integers(h // 2, h)))]
        jobs.append((pi, x0, y0, w, h, (0, 1, 10, 49)[k % 4], poly))
    return jobs


def plan(pages, jobs, pix, out_base, lead):
    """Page offsets (the first page `lead` bytes in), descriptors with their outputs from `out_base` on with canary gaps between them,
    the page bytes' end, the outputs' end, the masks' end."""
    from surya_amd.recognition.preprocess_gpu import ADJUST_DESC
    offs, total = [], lead
    for pg in pages:
        offs.append(total)
        total += pg.size
    desc = np.zeros(len(jobs), ADJUST_DESC)
    at, mask_at = out_base, 3
    for k, (d, (pi, x0, y0, w, h, c, poly)) in enumerate(zip(desc, jobs)):
        at += 4 if pix == 4 else 1 + k % 4                                     # a gap in front of every output; odd offsets with 3-byte pixels
        if pix == 4:
            at = (at + 3) & ~3
        d["src_off"], d["src_w"], d["src_h"] = offs[pi], pages[pi].shape[1], pages[pi].shape[0]
        d["x0"], d["y0"], d["w"], d["h"], d["cutoff"], d["out_off"] = x0, y0, w, h, c, at
        at += w * h * pix
        if poly is not None:
            d["has_poly"], d["poly"], d["mask_off"] = 1, np.asarray(poly, np.float32).reshape(-1), mask_at
            mask_at += w * h + 2
    return offs, total, desc, at + 8, mask_at + 8


def call(lib, d_pages, desc, n, d_out, d_mask, d_work, d_lohi, pix):
    rc = lib.surya_rec_adjust_contrast(L.ptr(d_pages), desc.ctypes.data_as(C.c_void_p), n, L.ptr(d_out), L.ptr(d_mask), L.ptr(d_work),
                                       L.ptr(d_lohi), pix, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def sentinel(n, dtype=torch.uint8):
    return torch.full((n,), SENTINEL, dtype=dtype, device="cuda")


def check_outputs(pages, jobs, desc, out, mask, lohi, pix, keep=None):
    """Every output crop, bounds pair and mask against Pillow / fill_poly_mask; -> which bytes of `out` and `mask` the call owned."""
    written, mwritten = np.zeros(out.size, bool), np.zeros(mask.size, bool)
    for k, (d, (pi, x0, y0, w, h, c, poly)) in enumerate(zip(desc, jobs)):
        crop = pages[pi][y0:y0 + h, x0:x0 + w, :3].copy()
        m = None
        if poly is not None:
            m = fill_poly_mask(h, w, poly)
            crop[m == 0] = 255
            a = int(d["mask_off"])
            assert np.array_equal(mask[a:a + w * h].reshape(h, w), m), (k, "mask")
            mwritten[a:a + w * h] = True
        want, (lo, hi) = pillow_adjust(crop, m, c)
        a = int(d["out_off"])
        got = out[a:a + w * h * pix].reshape(h, w, pix)
        assert (int(lohi[k, 0]), int(lohi[k, 1])) == (lo, hi), (k, jobs[k][:6], lohi[k].tolist(), (lo, hi))
        bad = np.argwhere(got[..., :3] != want)
        assert len(bad) == 0, (k, jobs[k][:6], len(bad), bad[:4].tolist())
        assert pix == 3 or not got[..., 3].any()                               # X is written as 0
        written[a:a + w * h * pix] = True
        if keep is not None:
            keep[k] = (lo, hi)
    return written, mwritten


@pytest.mark.parametrize("n", [1, 33, 300])
@pytest.mark.parametrize("pix", [3, 4])
def test_entry_equals_pillow_at_every_byte(hip_lib, pix, n):
    lib = L.lib()
    pages, jobs = make_pages(pix), jobs_for(n)
    assert len(jobs) == n
    same = pix == 4                                                            # RGBX: the outputs lie behind the pages, in their allocation
    page_bytes = sum(pg.size for pg in pages)
    lead = 0 if pix == 4 else 1                                                # RGB: the pages start at an odd byte
    offs, total, desc, end, mask_end = plan(pages, jobs, pix, ((lead + page_bytes + 3) & ~3) if same else 0, lead)
    host = np.full(end if same else total, SENTINEL, np.uint8)
    for pg, o in zip(pages, offs):
        host[o:o + pg.size] = pg.reshape(-1)
    d_pages = torch.from_numpy(host).cuda()
    d_out = d_pages if same else sentinel(end)
    d_mask, d_work, d_lohi = sentinel(mask_end), sentinel(n * WORK + 16), sentinel(2 * n + 2, torch.int32)
    assert call(lib, d_pages, desc, n, d_out, d_mask, d_work, d_lohi, pix) == 0
    out, mask, lohi = d_out.cpu().numpy(), d_mask.cpu().numpy(), d_lohi.cpu().numpy()
    if same:
        assert np.array_equal(out[:total], host[:total])                      # the pages are read only
    bounds = {}
    written, mwritten = check_outputs(pages, jobs, desc, out, mask, lohi[:2 * n].reshape(n, 2), pix, bounds)
    if same:
        written[:total] = True
    assert (out[~written] == SENTINEL).all() and (mask[~mwritten] == SENTINEL).all()      # nothing beside the crops and the masks
    assert bool((d_work[n * WORK:] == SENTINEL).all()) and (lohi[2 * n:] == SENTINEL).all()      # ... the work area and the bounds rows
    if n > 1:
        assert bounds[1][0] == bounds[1][1]                                    # the flat crop: hi <= lo, and its output is its input
        d, (pi, x0, y0, w, h, c, _) = desc[1], jobs[1]
        a = int(d["out_off"])
        assert np.array_equal(out[a:a + w * h * pix].reshape(h, w, pix)[..., :3], pages[pi][y0:y0 + h, x0:x0 + w, :3])
        assert bounds[2] == (0, 25)
        d, (pi, x0, y0, w, h, c, _) = desc[2], jobs[2]
        a = int(d["out_off"])
        got, src = out[a:a + w * h * pix].reshape(h, w, pix)[..., 0], pages[pi][y0:y0 + h, x0:x0 + w, 0]
        assert set(got[src == 25].tolist()) == {254} and set(got[src == 0].tolist()) == {0}


PAIRS = [(lo, hi) for lo in range(256) for hi in range(lo + 1, 256)]


@pytest.mark.parametrize("part", range(4))
def test_every_bounds_pair_with_its_whole_lut(hip_lib, part):
    """A crop per (lo, hi): the grey ramp 0..255 once, 382 pixels of `lo` and 382 of `hi`, cutoff 25. Of its 1020 counts 255 go at each
    end: every ramp value outside [lo, hi] and a part of the two big bins, so the bounds are (lo, hi) and all 256 values pass the LUT."""
    from surya_amd.recognition.preprocess_gpu import ADJUST_DESC
    assert len(PAIRS) == 32640
    lib = L.lib()
    pairs = PAIRS[part::4]
    n, w = len(pairs), 1020
    rows = np.empty((n, w), np.uint8)
    rows[:, :256] = np.arange(256, dtype=np.uint8)
    rows[:, 256:638] = np.asarray([p[0] for p in pairs], np.uint8)[:, None]
    rows[:, 638:] = np.asarray([p[1] for p in pairs], np.uint8)[:, None]
    page = np.repeat(rows[:, :, None], 3, axis=2)                              # one page, a crop per row
    desc = np.zeros(n, ADJUST_DESC)
    desc["src_w"], desc["src_h"], desc["w"], desc["h"], desc["cutoff"] = w, n, w, 1, 25
    desc["y0"] = np.arange(n)
    desc["out_off"] = np.arange(n, dtype=np.int64) * (w * 3)
    d_pages, d_out = torch.from_numpy(page.reshape(-1)).cuda(), sentinel(n * w * 3 + 8)
    d_work, d_lohi = sentinel(n * WORK), sentinel(2 * n, torch.int32)
    assert call(lib, d_pages, desc, n, d_out, None, d_work, d_lohi, 3) == 0
    assert np.array_equal(d_lohi.cpu().numpy().reshape(n, 2), np.asarray(pairs, np.int32))
    out = d_out.cpu().numpy()
    assert (out[n * w * 3:] == SENTINEL).all()
    out = out[:n * w * 3].reshape(n, w, 3)
    short = 0
    for k in range(n):
        want = np.asarray(ImageOps.autocontrast(Image.fromarray(page[k:k + 1]), cutoff=25, preserve_tone=True))
        assert np.array_equal(out[k:k + 1], want), pairs[k]
        short += int(want[0, pairs[k][1], 0] == 254)
    assert short > 0                                                           # some of the 4852 pairs whose lut[hi] is 254 are in every part


@pytest.mark.parametrize("pix", [3, 4])
def test_rectified_then_adjusted(hip_lib, pix):
    """surya_rec_rectify writes an upright crop behind the pages; the adjustment reads that crop as its source (no mask) and writes
    its copy behind it, on the same stream."""
    from surya_amd.recognition.preprocess_gpu import ADJUST_DESC, RECTIFY_DESC
    lib = L.lib()
    page = banded_page(120, 200, pix, 9)
    quad = [(30.0, 20.0), (170.0, 44.0), (164.0, 78.0), (24.0, 52.0)]
    W, H = quad_size(quad)
    base = (page.size + 3) & ~3
    crop_bytes = (W * H * pix + 3) & ~3
    rd = np.zeros(1, RECTIFY_DESC)
    rd["page_off"], rd["page_w"], rd["page_h"], rd["out_w"], rd["out_h"], rd["out_off"] = 0, 200, 120, W, H, base
    rd["h"] = quad_homography(quad, W, H)
    ad = np.zeros(1, ADJUST_DESC)
    ad["src_off"], ad["src_w"], ad["src_h"], ad["w"], ad["h"], ad["cutoff"], ad["out_off"] = base, W, H, W, H, 2, base + crop_bytes
    host = np.full(base + 2 * crop_bytes + 8, SENTINEL, np.uint8)
    host[:page.size] = page.reshape(-1)
    d_pages = torch.from_numpy(host).cuda()
    d_work, d_lohi = sentinel(WORK), sentinel(2, torch.int32)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.surya_rec_rectify(L.ptr(d_pages), rd.ctypes.data_as(C.c_void_p), 1, L.ptr(d_pages), pix, W, H, stream) == 0
    assert call(lib, d_pages, ad, 1, d_pages, None, d_work, d_lohi, pix) == 0
    out = d_pages.cpu().numpy()
    upright = warp_quad(page, rd["h"][0], W, H)
    assert np.array_equal(out[base:base + W * H * pix].reshape(H, W, pix), upright)
    want, (lo, hi) = pillow_adjust(upright[..., :3], None, 2)
    got = out[base + crop_bytes:base + crop_bytes + W * H * pix].reshape(H, W, pix)
    assert np.array_equal(got[..., :3], want) and d_lohi.tolist() == [lo, hi] and (lo, hi) != (0, 255)
    assert (out[base + crop_bytes + W * H * pix:] == SENTINEL).all() and np.array_equal(out[:page.size], page.reshape(-1))
    # the adjusted copy may not land on the crop it reads
    ad["out_off"] = base + crop_bytes - 4
    before = d_pages.clone()
    assert call(lib, d_pages, ad, 1, d_pages, None, d_work, d_lohi, pix) == L.SA_ERR_ARG and torch.equal(before, d_pages)


def test_refusals_leave_every_buffer_unchanged(hip_lib):
    lib = L.lib()
    for pix in (3, 4):
        pages = make_pages(pix)
        jobs = [SPECIAL[0], SPECIAL[12], SPECIAL[7]]
        offs, total, desc, end, mask_end = plan(pages, jobs, pix, 0, 0)
        d_pages = torch.from_numpy(np.concatenate([pg.reshape(-1) for pg in pages])).cuda()
        bufs = dict(out=sentinel(end), mask=sentinel(mask_end), work=sentinel(3 * WORK), lohi=sentinel(6, torch.int32))
        keep = {k: v.clone() for k, v in bufs.items()}
        pages_before = d_pages.clone()

        def edited(field, value, i=1):
            d = desc.copy()
            d[field][i] = value
            return d

        def refused(d, n=3, px=pix, out="out", mask="mask", work="work", lohi="lohi", src=d_pages):
            rc = call(lib, src, d, n, bufs.get(out), bufs.get(mask), bufs.get(work), bufs.get(lohi), px)
            return rc == L.SA_ERR_ARG and all(torch.equal(bufs[k], keep[k]) for k in bufs) and torch.equal(d_pages, pages_before)

        assert refused(desc, px=5) and refused(desc, px=0) and refused(desc, n=-1)
        assert refused(desc, out=None) and refused(desc, work=None) and refused(desc, lohi=None) and refused(desc, mask=None)     # a polygon line without a mask arena
        for field, value in (("w", 0), ("h", -2), ("src_w", 0), ("src_h", 0), ("x0", -1), ("y0", -1), ("cutoff", 50), ("cutoff", -1),
                             ("has_poly", 2), ("mask_off", -1), ("out_off", -1), ("src_off", -3)):
            assert refused(edited(field, value)), (field, value)
        assert refused(edited("x0", 1100 - 220 + 1)) and refused(edited("y0", 300 - 40 + 1))      # one pixel over the source's edge
        assert refused(edited("out_off", int(desc["out_off"][0]) + 5))          # two outputs on the same bytes
        assert refused(edited("out_off", int(desc["out_off"][2]) - 1))          # ... by one byte
        assert refused(edited("has_poly", 1, 0))                                # a second mask, at offset 0 over the one at offset 3
        if pix == 4:
            assert refused(edited("out_off", int(desc["out_off"][1]) + 2)) and refused(edited("src_off", 2, 0))
        # outputs inside the pages' allocation, on a source page
        assert call(lib, d_pages, desc, 3, d_pages, bufs["mask"], bufs["work"], bufs["lohi"], pix) == L.SA_ERR_ARG
        assert torch.equal(d_pages, pages_before) and all(torch.equal(bufs[k], keep[k]) for k in bufs)
        # n == 0 launches nothing; the plain call then writes
        assert call(lib, d_pages, desc, 0, bufs["out"], bufs["mask"], bufs["work"], bufs["lohi"], pix) == 0
        assert all(torch.equal(bufs[k], keep[k]) for k in bufs)
        assert call(lib, d_pages, desc, 3, bufs["out"], bufs["mask"], bufs["work"], bufs["lohi"], pix) == 0
        assert not torch.equal(bufs["out"], keep["out"]) and torch.equal(d_pages, pages_before)
