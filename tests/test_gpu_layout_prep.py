"""GPU: page pre-processing of the layout family on the device (surya_layout_preprocess, csrc/layout_prep.h) against the host chain it
replaces (LayoutImageProcessor), with zero tolerance, and the layout / table predictors end to end on both paths."""
import numpy as np
import pytest
import torch
from PIL import Image

from surya_amd.layout.predictor import LAYOUT_SLICE_MIN, LAYOUT_SLICE_SIZE, LayoutImageProcessor
from surya_amd.layout.slicer import ImageSlicer

pytestmark = pytest.mark.gpu

MEAN_STD = [None, ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))]     # the processor's 0.5 / 0.5, and a table checkpoint's own values


def _pages_and_rects(rng):
    """(w, h) pages and the crop boxes the kernel test takes from them: every size of the issue, several in one launch."""
    sl = ImageSlicer(LAYOUT_SLICE_MIN, LAYOUT_SLICE_SIZE)
    sizes = [(768, 768), (816, 1056), (1632, 2112), (500, 300), (768, 1000), (1, 1), (3000, 5), (1024, 1800), (3200, 1000)]
    pages = [rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8) for w, h in sizes]
    rects = []
    for i, (w, h) in enumerate(sizes):
        if (w, h) in ((1024, 1800), (3200, 1000)):                 # both height strips / the three width strips, by the slicer
            strips = sl._strips((w, h))
            assert len(strips) == (2 if w == 1024 else 3)
            rects += [(i, box) for box, _ in strips]
        else:
            rects.append((i, (0, 0, w, h)))
    return pages, rects


def _host(pages, rects, size, mean_std):
    proc = LayoutImageProcessor({"height": size[0], "width": size[1]}, *(mean_std or (None, None)))
    crops = [pages[p][y0:y1, x0:x1, :3] for p, (x0, y0, x1, y1) in rects]
    return torch.from_numpy(np.stack(proc(crops)["pixel_values"])), proc


@pytest.mark.parametrize("mean_std", MEAN_STD, ids=["default", "imagenet"])
@pytest.mark.parametrize("stride", [3, 4, "mixed"])
def test_device_pixel_values_equal_the_host_chain(hip_lib, stride, mean_std):
    from surya_amd.layout.preprocess_gpu import LayoutDevicePreprocessor
    rng = np.random.default_rng(11)
    pages, rects = _pages_and_rects(rng)
    want, proc = _host(pages, rects, (768, 768), mean_std)
    if stride == 3:
        dev_pages = [np.ascontiguousarray(pg[..., :3]) for pg in pages]
    elif stride == 4:
        dev_pages = pages                                            # the fourth byte is noise: it must be ignored
    else:
        dev_pages = [pg if i % 2 else np.ascontiguousarray(pg[..., :3]) for i, pg in enumerate(pages)]
    prep = LayoutDevicePreprocessor("cuda:0")
    got = prep.run(dev_pages, rects, (768, 768), proc.image_mean, proc.image_std)
    torch.cuda.synchronize()
    got = got.cpu()
    assert got.shape == want.shape == (len(rects), 3, 768, 768)
    for i in range(len(rects)):
        bad = (got[i] != want[i]).sum().item()
        print(f"image {i} rect {rects[i]}: {bad} differing values, max |diff| {(got[i] - want[i]).abs().max().item():.3g}")
    assert torch.equal(got, want)


def test_more_images_than_one_launch_and_a_non_square_output(hip_lib):
    """70 crops (two launches of at most 64 descriptors), an output of 64 x 96, the staging buffer reused by a second call."""
    from surya_amd.layout.preprocess_gpu import LayoutDevicePreprocessor
    rng = np.random.default_rng(5)
    pages = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for w, h in ((300, 200), (64, 96), (97, 31))]
    rects = []
    for k in range(70):
        p = k % 3
        h, w = pages[p].shape[:2]
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        rects.append((p, (x0, y0, int(rng.integers(x0 + 1, w + 1)), int(rng.integers(y0 + 1, h + 1)))))
    want, proc = _host(pages, rects, (64, 96), None)
    prep = LayoutDevicePreprocessor("cuda:0")
    first = prep.run(pages, rects[:5], (64, 96), proc.image_mean, proc.image_std)
    got = prep.run(pages, rects, (64, 96), proc.image_mean, proc.image_std)
    torch.cuda.synchronize()
    assert torch.equal(first.cpu(), want[:5])
    assert torch.equal(got.cpu(), want)


def _pages(rng, sizes):
    return [Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)) for w, h in sizes]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_layout_predictor_device_path_equals_the_host_path(hip_lib, dtype):
    """LayoutPredictor on the same pages through both pre-processing paths in one process (device_preprocess False is what
    LAYOUT_PREPROCESS_HOST=1 sets): a sliced page, a call of more slices than the model's batch, identical results."""
    from surya_amd.layout import predictor as lp
    old = lp.LAYOUT_MAX_BOXES
    lp.LAYOUT_MAX_BOXES = 12
    try:
        loader = lp.LayoutModelLoader("LAYOUT-PAD")
        pred = lp.LayoutPredictor(checkpoint="LAYOUT-PAD", dtype=dtype)
        pred.model = loader.model(dtype=dtype, max_batch=4)
        rng = np.random.default_rng(21)
        pages = _pages(rng, [(816, 1056), (1024, 1800), (300, 500), (176, 208), (3200, 1000), (40, 30)])    # 9 slices
        assert pred.device_preprocess
        got = pred(pages)
        prep = pred.device_prep
        assert prep is not None and prep._host is not None              # the device path ran
        prep.timing = True
        pred.device_preprocess = False
        want = pred(pages)
        assert prep.timings == []                                       # ... and the checker did not
    finally:
        lp.LAYOUT_MAX_BOXES = old
    assert len(got) == len(want) == len(pages)
    assert any(r.sliced for r in want)
    assert sum(len(r.bboxes) for r in want) > 0
    for a, b in zip(got, want):
        assert a.model_dump() == b.model_dump()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_table_predictor_device_path_equals_the_host_path(hip_lib, dtype):
    """TableRecPredictor, both passes, through both pre-processing paths in one process: identical results."""
    from surya_amd.synth import make_table_weights
    from surya_amd.table_rec import predictor as tp
    from surya_amd.table_rec.config import table_config
    cfg = table_config("TABLE-TINY")
    sd = make_table_weights(cfg, 0)
    sd["decoder.box_property_heads.category.weight"][5 + 1] *= 3.0      # rows and columns must appear for the second pass to run
    sd["decoder.box_property_heads.category.weight"][5 + 2] *= 2.5
    old = tp.TABLE_REC_MAX_BOXES
    tp.TABLE_REC_MAX_BOXES = 14
    try:
        pred = tp.TableRecPredictor(checkpoint={"config": cfg, "state_dict": sd}, dtype=dtype)
        rng = np.random.default_rng(3)
        pages = _pages(rng, [(320, 200), (128, 128), (400, 90), (500, 300), (60, 700)])
        got = pred(pages, batch_size=3)
        prep = pred.device_prep
        assert prep is not None and prep._host is not None
        prep.timing = True
        pred.device_preprocess = False
        want = pred(pages, batch_size=3)
        assert prep.timings == []
    finally:
        tp.TABLE_REC_MAX_BOXES = old
    assert sum(len(r.rows) for r in want) > 0 and sum(len(r.cols) for r in want) > 0
    assert len(got) == len(want) == len(pages)
    for a, b in zip(got, want):
        assert a.model_dump() == b.model_dump()
