"""GPU: surya_rec_unroll alone (csrc/rec_unroll.h) against warp_columns (common/imageops.py): uint8-EQUAL everywhere -- the same taps, the
same float64 association, no contraction. RGB and RGBX pages; crops of 1 x 1, 17 x 5, 33 x 16 and 300 x 40 under one grid; curves that
leave the page on every side; n = 0 and n = 33 (two launches); `out` inside the pages' allocation and outside it; every refusal leaves
`out` untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

from surya_amd import _lib as L
from surya_amd.common.imageops import curve_table, warp_columns
from surya_amd.recognition.preprocess_gpu import UNROLL_DESC

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


def arc(x0, y0, length, sag, n=9, thickness=16.0):
    """A centre line of about `length` from (x0, y0) to the right, sagging by `sag`; (points, thickness)."""
    xs = np.linspace(0.0, length, n)
    return np.stack([x0 + xs, y0 + sag * np.sin(np.pi * xs / max(length, 1e-9))], 1), thickness


# (page, (points, thickness)): 1 x 1, 17 x 5, 33 x 16, 300 x 40, then curves across the left, top, right and bottom edges and one far outside
CURVES = [(0, ([(10.2, 7.1), (11.1, 7.3)], 0.9)), (1, ([(20.0, 30.0), (27.15, 36.0), (33.0, 31.0)], 5.0)), (0, arc(40.0, 50.0, 30.0, 6.0)),
          (0, arc(5.0, 80.0, 295.0, 25.0, n=17, thickness=40.0)),
          (1, arc(-30.0, 60.0, 90.0, 12.0)), (1, ([(50.0, -12.0), (90.0, 4.0), (130.0, -9.0)], 24.0)), (1, arc(100.0, 70.0, 120.0, -15.0)),
          (1, ([(20.0, 140.0), (70.0, 158.0), (120.0, 146.0)], 30.0)), (0, ([(500.0, 400.0), (560.0, 430.0)], 12.0)),
          (0, ([(150.0, 20.0), (150.0, 100.0)], 14.0)), (0, ([(200.0, 60.0), (120.0, 70.0), (60.0, 40.0)], 10.0))]      # downwards; right to left


def _pages(pix):
    rng = np.random.default_rng(31)
    return [rng.integers(0, 256, size=(130, 320, pix), dtype=np.uint8), rng.integers(0, 256, size=(150, 140, pix), dtype=np.uint8)]


def _plan(pages, jobs, pix, base):
    """Page offsets, their total, the descriptors of `jobs` with their crops from byte `base` of `out` on (4-byte aligned each), the end,
    and the stacked tables."""
    offs, total = [], 0
    for pg in pages:
        offs.append(total)
        total += pg.size
    desc = np.zeros(len(jobs), UNROLL_DESC)
    tables, at, t_at = [], (base + 3) & ~3, 0
    for d, (pi, (points, thickness)) in zip(desc, jobs):
        table, W, H = curve_table(points, thickness)
        d["page_off"], d["page_w"], d["page_h"], d["out_w"], d["out_h"], d["out_off"] = offs[pi], pages[pi].shape[1], pages[pi].shape[0], W, H, at
        d["table_off"] = t_at
        tables.append(table)
        at += (W * H * pix + 3) & ~3
        t_at += table.size
    return offs, total, desc, at, tables


def _call(lib, d_pages, desc, n, d_tables, d_out, pix, max_w, max_h):
    rc = lib.surya_rec_unroll(L.ptr(d_pages), desc.ctypes.data_as(C.c_void_p), n, L.ptr(d_tables) if d_tables is not None else None, L.ptr(d_out),
                              pix, max_w, max_h, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def _tables_on_device(tables):
    return torch.from_numpy(np.concatenate([t.reshape(-1) for t in tables])).cuda()


@pytest.mark.parametrize("same_allocation", [True, False])
@pytest.mark.parametrize("jobs", [CURVES[:1], CURVES, (CURVES * 3)[:33]], ids=["one", "eleven", "thirty_three"])
@pytest.mark.parametrize("pix", [3, 4])
def test_entry_point_equals_warp_columns(hip_lib, pix, jobs, same_allocation):
    lib = L.lib()
    pages = _pages(pix)
    page_bytes = sum(pg.size for pg in pages)
    offs, total, desc, end, tables = _plan(pages, jobs, pix, page_bytes if same_allocation else 0)
    host = np.full(end if same_allocation else total, SENTINEL, np.uint8)
    for pg, o in zip(pages, offs):
        host[o:o + pg.size] = pg.reshape(-1)
    d_pages = torch.from_numpy(host).cuda()
    d_out = d_pages if same_allocation else torch.full((end,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert _call(lib, d_pages, desc, len(jobs), _tables_on_device(tables), d_out, pix, int(desc["out_w"].max()), int(desc["out_h"].max())) == 0
    out = d_out.cpu().numpy()
    if same_allocation:
        assert np.array_equal(out[:total], host[:total])                   # the pages are read only
    written = np.zeros(out.size, bool)
    for d, (pi, _), table in zip(desc, jobs, tables):
        W, H = int(d["out_w"]), int(d["out_h"])
        want = warp_columns(pages[pi], table, H)
        a = int(d["out_off"])
        got = out[a:a + W * H * pix].reshape(H, W, pix)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, ((W, H), len(bad), bad[:4].tolist())
        written[a:a + W * H * pix] = True
    rest = ~written
    if same_allocation:
        rest[:total] = False
    assert (out[rest] == SENTINEL).all()                                   # nothing beside the crops, padding bytes included
    shapes = {(int(d["out_w"]), int(d["out_h"])) for d in desc}
    assert len(jobs) == 1 or {(1, 1), (17, 5), (33, 16), (300, 40)} <= shapes, shapes


def test_refusals_leave_out_untouched(hip_lib):
    lib = L.lib()
    for pix in (3, 4):
        pages = _pages(pix)
        offs, total, desc, end, tables = _plan(pages, CURVES[1:3], pix, 0)
        d_pages = torch.from_numpy(np.concatenate([pg.reshape(-1) for pg in pages])).cuda()
        d_tab = _tables_on_device(tables)
        d_out = torch.full((end,), SENTINEL, dtype=torch.uint8, device="cuda")
        mw, mh = int(desc["out_w"].max()), int(desc["out_h"].max())

        def edited(field, value, i=1):
            d = desc.copy()
            d[field][i] = value
            return d
        cases = [(desc, 2, d_tab, 5, mw, mh), (desc, 2, d_tab, 0, mw, mh), (desc, 2, d_tab, pix, 0, mh), (desc, 2, d_tab, pix, mw, -1),
                 (desc, -1, d_tab, pix, mw, mh), (edited("out_w", 0), 2, d_tab, pix, mw, mh), (edited("out_h", -3), 2, d_tab, pix, mw, mh),
                 (edited("page_w", 0), 2, d_tab, pix, mw, mh), (edited("page_h", 0), 2, d_tab, pix, mw, mh), (desc, 2, d_tab, pix, mw - 1, mh),
                 (desc, 2, d_tab, pix, mw, mh - 1), (desc, 2, None, pix, mw, mh), (edited("table_off", -4), 2, d_tab, pix, mw, mh),
                 (edited("table_off", 3), 2, d_tab, pix, mw, mh), (edited("page_off", -4, 0), 2, d_tab, pix, mw, mh),
                 (edited("out_off", -4), 2, d_tab, pix, mw, mh), (desc, 2, d_tab[1:], pix, mw, mh)]          # tables not 16-byte aligned
        if pix == 4:
            cases += [(edited("out_off", int(desc["out_off"][1]) + 2), 2, d_tab, 4, mw, mh), (edited("page_off", 2, 0), 2, d_tab, 4, mw, mh)]
        for d, n, tab, px, w, h in cases:
            assert _call(lib, d_pages, d, n, tab, d_out, px, w, h) == L.SA_ERR_ARG, (n, px, w, h)
            assert bool((d_out == SENTINEL).all())
        assert _call(lib, d_pages, desc, 0, d_tab, d_out, pix, mw, mh) == 0 and bool((d_out == SENTINEL).all())     # n == 0 launches nothing
        assert _call(lib, d_pages, desc, 2, d_tab, d_out, pix, mw, mh) == 0 and not bool((d_out == SENTINEL).all())
