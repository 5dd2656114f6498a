"""Host side of the layout-family device pre-processing (surya_amd/layout/preprocess_gpu.py, csrc/layout_prep.h): the slicer's strips
by reference, the descriptor layout, the library's argument checks, and when the device path engages. No GPU needed."""
import ctypes as C

import numpy as np
import pytest
from PIL import Image

from surya_amd.layout.predictor import LAYOUT_SLICE_MIN, LAYOUT_SLICE_SIZE, LayoutImageProcessor, LayoutPredictor
from surya_amd.layout.preprocess_gpu import PAGE_DESC, device_preprocessor, page_descriptors
from surya_amd.layout.slicer import ImageSlicer

# (width, height): below, at and above the 1500-px thresholds, tall and wide, and a page whose long side gives a step above the slice size
PAGE_SIZES = [(816, 1056), (1500, 1500), (1500, 1501), (1501, 1500), (1024, 1800), (3200, 1000), (1632, 2112), (600, 7000),
              (7000, 40), (1, 1), (1501, 1)]


@pytest.mark.parametrize("size", PAGE_SIZES)
def test_strip_rectangles_equal_the_slicer_crops(size):
    rng = np.random.default_rng(size[0] * 7 + size[1])
    w, h = size
    pages = [Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)),
             Image.fromarray(rng.integers(0, 256, size=(300, 200, 3), dtype=np.uint8))]
    sl = ImageSlicer(LAYOUT_SLICE_MIN, LAYOUT_SLICE_SIZE)
    pieces, positions = sl.slice(pages)
    rects, positions_r = sl.slice_rects(pages)
    assert positions_r == positions
    assert len(rects) == len(pieces) == sum(sl.slice_count(p) if max(p.size) > 1500 else 1 for p in pages)
    for (p, (x0, y0, x1, y1)), piece in zip(rects, pieces):
        assert 0 <= x0 < x1 <= pages[p].width and 0 <= y0 < y1 <= pages[p].height
        assert piece.size == (x1 - x0, y1 - y0)
        assert np.array_equal(np.asarray(piece), np.asarray(pages[p])[y0:y1, x0:x1])
    if max(size) > 1500:                                 # the strips tile the page along its long side
        assert len([r for r in rects if r[0] == 0]) > 1


class _PageDescC(C.Structure):
    """sa::lprep::PageDesc as a C compiler lays it out (csrc/layout_prep.h, include/surya_amd.h)."""
    _fields_ = [("page_off", C.c_int64), ("page_w", C.c_int32), ("page_h", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32),
                ("cw", C.c_int32), ("ch", C.c_int32)]


def test_descriptor_dtype_matches_the_c_layout():
    assert PAGE_DESC.itemsize == C.sizeof(_PageDescC) == 32
    for name, _ in _PageDescC._fields_:
        assert PAGE_DESC.fields[name][1] == getattr(_PageDescC, name).offset, name
    d = page_descriptors([(20, 30), (5, 7)], [0, 1800], [(1, (2, 1, 7, 5)), (0, (0, 0, 30, 20))])
    c = (_PageDescC * 2).from_buffer_copy(d.tobytes())
    assert (c[0].page_off, c[0].page_w, c[0].page_h, c[0].x0, c[0].y0, c[0].cw, c[0].ch) == (1800, 7, 5, 2, 1, 5, 4)
    assert (c[1].page_off, c[1].page_w, c[1].page_h, c[1].x0, c[1].y0, c[1].cw, c[1].ch) == (0, 30, 20, 0, 0, 30, 20)
    for bad in [(0, (0, 0, 31, 20)), (0, (3, 0, 3, 20)), (0, (-1, 0, 4, 4)), (1, (0, 0, 7, 6))]:
        with pytest.raises(ValueError):
            page_descriptors([(20, 30), (5, 7)], [0, 1800], [bad])


def test_library_rejects_bad_arguments_without_touching_memory(hip_lib):
    """Every check runs on the host before anything is enqueued: the pointers below are never dereferenced."""
    f = hip_lib.surya_layout_preprocess
    fake = C.c_void_p(0x1000)
    mean = (C.c_float * 3)(0.5, 0.5, 0.5)
    std = (C.c_float * 3)(0.5, 0.5, 0.5)

    def call(desc, n=None, pix=3, pages=fake, nbytes=30 * 20 * 3, out=fake, oh=16, ow=16, m=mean):
        d = np.asarray(desc, PAGE_DESC)
        return f(pages, C.c_size_t(nbytes), d.ctypes.data_as(C.c_void_p), C.c_int(len(d) if n is None else n), C.c_int(pix), m, std,
                 C.c_int(oh), C.c_int(ow), out, None)

    ok = [(0, 30, 20, 0, 0, 30, 20)]
    assert call(ok, pages=C.c_void_p(0)) == -1                      # SA_ERR_ARG
    assert call(ok, out=C.c_void_p(0)) == -1
    assert call(ok, m=None) == -1
    assert call(ok, pix=2) == -1
    assert call(ok, n=-1) == -1
    assert call(ok, oh=0) == -2                                      # SA_ERR_SHAPE
    assert call([(0, 30, 20, 1, 0, 30, 20)]) == -2                   # crop beyond the page's right edge
    assert call([(0, 30, 20, 0, 5, 30, 16)]) == -2                   # ... bottom edge
    assert call([(0, 30, 20, 0, 0, 0, 20)]) == -2                    # empty crop
    assert call([(0, 30, 20, -1, 0, 10, 10)]) == -2
    assert call([(3, 30, 20, 0, 0, 30, 20)]) == -2                   # page beyond pages_bytes
    assert call(ok, pix=4) == -2                                     # the same page at 4 bytes per pixel does not fit
    assert call(ok + [(0, 30, 20, 0, 0, 30, 21)]) == -2              # the second descriptor is checked as well


class _StandIn:
    device = "cpu"


def test_device_path_engages_only_for_the_engine_and_the_familys_processor():
    pred = object.__new__(LayoutPredictor)
    pred.model = _StandIn()
    pred.processor = LayoutImageProcessor({"height": 64, "width": 64})
    pred.device_preprocess = True
    assert device_preprocessor(pred, pred.processor) is None          # not a HipLayoutModel
    pred.device_preprocess = False
    assert device_preprocessor(pred, pred.processor) is None


def test_layout_preprocess_host_setting_selects_the_host_chain():
    """LAYOUT_PREPROCESS_HOST=1 turns the device path off for both predictors (a fresh interpreter: settings are read at import)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("from surya_amd.layout.predictor import LayoutPredictor; from surya_amd.table_rec.predictor import TableRecPredictor; "
            "print(LayoutPredictor.device_preprocess, TableRecPredictor.device_preprocess)")
    for value, want in (("1", "False False"), ("0", "True True")):
        env = dict(os.environ, LAYOUT_PREPROCESS_HOST=value)
        out = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, check=True)
        assert out.stdout.strip().splitlines()[-1] == want, out.stdout
