"""GPU: `dewarp(..., device="cuda")` (surya_amd/detection/dewarp.py): byte-equal to the host arm on the field-B page (1024 x 1400, RGB,
the mesh fitted from its planted lines) and on a mixed batch -- a PIL page with a mesh, one with None, an RGBX array with a mesh, one with
an all-zero mesh; pages returned untouched are the same objects; one surya_warp_mesh call per `dewarp` call."""
import numpy as np
import pytest
from PIL import Image

import dewarp_ref as R
from surya_amd import _lib as L
from surya_amd.detection import dewarp as dw

pytestmark = pytest.mark.gpu


class CountingLib:
    """The library with one entry point's calls counted."""

    def __init__(self, lib, name):
        self._lib, self._name, self.calls = lib, name, 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != self._name:
            return fn

        def counted(*a):
            self.calls += 1
            return fn(*a)
        return counted


def test_field_b_page_on_the_device_equals_the_host_arm(hip_lib, monkeypatch):
    page, mesh = R.field_b_page()
    counting = CountingLib(L.lib(), "surya_warp_mesh")
    monkeypatch.setattr(L, "lib", lambda: counting)
    im = Image.fromarray(page)
    (host,) = dw.dewarp([im], meshes=[mesh])
    assert counting.calls == 0
    (dev,) = dw.dewarp([im], meshes=[mesh], device="cuda")
    assert counting.calls == 1
    a, b = np.asarray(host.image), np.asarray(dev.image)
    assert a.shape == b.shape == (1400, 1024, 3) and dev.image.size == im.size
    bad = np.argwhere(a != b)
    assert len(bad) == 0, (len(bad), bad[:4].tolist())
    assert not np.array_equal(a, page) and dev.mesh is mesh and dev.cell == 64 and dev.max_shift == host.max_shift > 10.0
    pts = np.array([[100.5, 300.0], [900.0, 1200.25]])
    assert np.abs(dev.from_page(dev.to_page(pts)) - pts).max() <= 1e-6


def test_mixed_batch_on_the_device_equals_the_host_arm(hip_lib):
    W, H, cell = 300, 200, 32
    pg = R.page(W, H, 3)
    other = R.page(131, 97, 3)
    m1, m2 = R.random_mesh(W, H, cell, 21), R.random_mesh(131, 97, cell, 22)
    im = Image.fromarray(pg)
    rgbx = np.dstack([other, other[..., :1]])
    images = [im, im, rgbx, pg]
    meshes = [m1, None, m2, R.zero_mesh(W, H, cell)]
    host = dw.dewarp(images, meshes=meshes, options=dw.Dewarp(cell=cell))
    dev = dw.dewarp(images, meshes=meshes, options=dw.Dewarp(cell=cell), device="cuda:0")
    for k in (0, 2):
        a, b = np.asarray(host[k].image), np.asarray(dev[k].image)
        assert a.shape == b.shape and np.array_equal(a, b), k
        assert dev[k].mesh is meshes[k]
    assert np.asarray(dev[2].image).shape == (97, 131, 3)
    for k in (1, 3):
        assert dev[k].image is images[k] and host[k].image is images[k] and dev[k].mesh is None
    # a batch of RGBX arrays alone travels with stride 4
    (h4,), (d4,) = dw.dewarp([rgbx], meshes=[m2], options=dw.Dewarp(cell=cell)), dw.dewarp([rgbx], meshes=[m2], options=dw.Dewarp(cell=cell), device="cuda")
    assert np.array_equal(np.asarray(h4.image), np.asarray(d4.image)) and np.array_equal(np.asarray(h4.image), np.asarray(host[2].image))
