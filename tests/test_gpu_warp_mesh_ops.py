"""GPU: surya_warp_mesh alone (csrc/page_warp.h) against warp_mesh (common/imageops.py): uint8-EQUAL everywhere -- the same bilinear form,
the same taps, the same float64 association, no contraction. RGB and RGBX pages of 1 x 1, 17 x 5, 33 x 16, 131 x 97 and 300 x 200 under one
grid; cells of 16, 32 and 64 (the last cell partial in every case but 33 x 16 at 16 along y); meshes: zero, an integer shift, random
valid, every edge pushed off the page, +-1e12; n = 0, 1 and 33 (two launches); `out` inside the pages' allocation and outside it; the
pages stay as they were and every byte beside the outputs keeps its sentinel; every refusal leaves `out` untouched."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dewarp_ref as R
from surya_amd import _lib as L
from surya_amd.common.imageops import warp_mesh
from surya_amd.recognition.preprocess_gpu import MESH_DESC

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
SIZES = R.PAGES + [(300, 200)]
MESHES = [R.zero_mesh, R.shift_mesh, lambda W, H, c: R.random_mesh(W, H, c, seed=W + c), R.off_page_mesh, R.huge_mesh]
JOBS = [(p, m) for m in range(len(MESHES)) for p in range(len(SIZES))]          # 25 (page, mesh) pairs
JOBS33 = (JOBS + JOBS[5:])[:33]


@functools.lru_cache(maxsize=None)
def _page(p, pix):
    pg = R.page(*SIZES[p], pix)
    pg.setflags(write=False)
    return pg


@functools.lru_cache(maxsize=None)
def _mesh(p, m, cell):
    mesh = MESHES[m](*SIZES[p], cell)
    mesh.setflags(write=False)
    return mesh


@functools.lru_cache(maxsize=None)
def _want(p, m, cell, pix):
    """The host rule's output, computed once per case and shared."""
    out = warp_mesh(_page(p, pix), _mesh(p, m, cell), cell)
    out.setflags(write=False)
    return out


def _plan(jobs, cell, pix, base):
    """Page offsets, their total, the descriptors of `jobs` with their outputs from byte `base` of `out` on (4-byte aligned each), the
    end, and the stacked meshes."""
    offs, total = [], 0
    for p in range(len(SIZES)):
        offs.append(total)
        total += (_page(p, pix).size + 3) & ~3
    desc = np.zeros(len(jobs), MESH_DESC)
    meshes, at, m_at = [], (base + 3) & ~3, 0
    for d, (p, m) in zip(desc, jobs):
        W, H = SIZES[p]
        mesh = _mesh(p, m, cell)
        d["page_off"], d["w"], d["h"], d["cell"], d["out_off"], d["mesh_off"] = offs[p], W, H, cell, at, m_at
        meshes.append(mesh.reshape(-1))
        at += (W * H * pix + 3) & ~3
        m_at += mesh.size
    return offs, total, desc, at, np.concatenate(meshes)


def _call(lib, d_pages, desc, n, d_meshes, d_out, pix, max_w, max_h):
    rc = lib.surya_warp_mesh(L.ptr(d_pages) if d_pages is not None else None, desc.ctypes.data_as(C.c_void_p) if desc is not None else None, n,
                             L.ptr(d_meshes) if d_meshes is not None else None, L.ptr(d_out) if d_out is not None else None, pix, max_w, max_h,
                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def _host_pages(pix, offs, size):
    host = np.full(size, SENTINEL, np.uint8)
    for p, o in enumerate(offs):
        host[o:o + _page(p, pix).size] = _page(p, pix).reshape(-1)
    return host


@pytest.mark.parametrize("same_allocation", [True, False])
@pytest.mark.parametrize("jobs", [JOBS[14:15], JOBS33], ids=["one", "thirty_three"])
@pytest.mark.parametrize("cell", [16, 32, 64])
@pytest.mark.parametrize("pix", [3, 4])
def test_entry_point_equals_warp_mesh(hip_lib, pix, cell, jobs, same_allocation):
    lib = L.lib()
    page_bytes = sum((_page(p, pix).size + 3) & ~3 for p in range(len(SIZES)))
    offs, total, desc, end, meshes = _plan(jobs, cell, pix, page_bytes if same_allocation else 0)
    host = _host_pages(pix, offs, end if same_allocation else total)
    d_pages = torch.from_numpy(host).cuda()
    d_out = d_pages if same_allocation else torch.full((end,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert _call(lib, d_pages, desc, len(jobs), torch.from_numpy(meshes).cuda(), d_out, pix, int(desc["w"].max()), int(desc["h"].max())) == 0
    out = d_out.cpu().numpy()
    if same_allocation:
        assert np.array_equal(out[:total], host[:total])                   # the pages are read only
    else:
        assert np.array_equal(d_pages.cpu().numpy(), host)
    written = np.zeros(out.size, bool)
    for d, (p, m) in zip(desc, jobs):
        W, H = SIZES[p]
        want = _want(p, m, cell, pix)
        a = int(d["out_off"])
        got = out[a:a + W * H * pix].reshape(H, W, pix)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, ((W, H), m, len(bad), bad[:4].tolist())
        written[a:a + W * H * pix] = True
    rest = ~written
    if same_allocation:
        rest[:total] = False
    assert (out[rest] == SENTINEL).all()                                   # nothing beside the outputs, padding bytes included


def test_refusals_leave_out_untouched(hip_lib):
    lib = L.lib()
    for pix in (3, 4):
        jobs = [(1, 2), (3, 2)]
        offs, total, desc, end, meshes = _plan(jobs, 32, pix, 0)
        d_pages = torch.from_numpy(_host_pages(pix, offs, total)).cuda()
        d_mesh = torch.from_numpy(np.concatenate([meshes, np.zeros(2)])).cuda()
        d_out = torch.full((end + 4,), SENTINEL, dtype=torch.uint8, device="cuda")
        mw, mh = int(desc["w"].max()), int(desc["h"].max())

        def edited(field, value, i=1):
            d = desc.copy()
            d[field][i] = value
            return d
        ok = (d_pages, desc, 2, d_mesh, d_out, pix, mw, mh)

        def but(**kw):
            names = ("pages", "desc", "n", "mesh", "out", "pix", "mw", "mh")
            return tuple(kw.get(k, v) for k, v in zip(names, ok))
        cases = [but(pix=5), but(pix=0), but(pix=2), but(mw=0), but(mh=-1), but(n=-1), but(mw=mw - 1), but(mh=mh - 1),
                 but(pages=None), but(desc=None), but(mesh=None), but(out=None), but(mesh=d_mesh[1:]),               # meshes not 16-byte aligned
                 but(desc=edited("w", 0)), but(desc=edited("h", -3)), but(desc=edited("w", mw + 1)), but(desc=edited("h", mh + 1, 0)),
                 but(desc=edited("cell", 0)), but(desc=edited("cell", 8)), but(desc=edited("cell", 24)),
                 but(desc=edited("cell", 1040)), but(desc=edited("cell", -32)), but(desc=edited("reserved", 1, 0)),
                 but(desc=edited("page_off", -4, 0)), but(desc=edited("out_off", -4)), but(desc=edited("mesh_off", -2)),
                 but(desc=edited("mesh_off", 3)), but(mh=16 * 65535 + 1)]                                               # more tile rows than a grid holds
        if pix == 4:
            cases += [but(desc=edited("out_off", int(desc["out_off"][1]) + 2)), but(desc=edited("page_off", 2, 0)), but(pages=d_pages[2:]),
                      but(out=d_out[1:])]
        for k, case in enumerate(cases):
            assert _call(lib, *case) == L.SA_ERR_ARG, (pix, k)
            assert bool((d_out == SENTINEL).all()), (pix, k)
        assert _call(lib, *but(n=0)) == 0 and bool((d_out == SENTINEL).all())                     # n == 0 launches nothing
        assert _call(lib, *ok) == 0 and not bool((d_out == SENTINEL).all())
