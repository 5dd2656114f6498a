"""CPU: the restatement of what Pillow's `thumbnail(size, LANCZOS)` does to a page that shrinks an axis by 4x or more
(surya_amd/common/pil_resample.py: `plan_chain`, `reduce_reference`, the boxed `lanczos_coeffs`) against Pillow itself, bit for
bit: the integer box reduction alone on images that hold every block sum, the boxed tables, and the whole chain."""
import numpy as np
import pytest
from PIL import Image

from surya_amd.common import pil_resample as pr
from reduce_cases import CHAIN_64, CHAIN_FACTORS, FACTORS, RAGGED, exhaustive_sum_image


def pil_chain(a, size):
    im = Image.fromarray(a)
    im.thumbnail(size, Image.Resampling.LANCZOS)
    return np.asarray(im.resize(size, Image.Resampling.LANCZOS))


def run_chain(a, steps, reduce=pr.reduce_reference, resize=pr.resample_reference):
    cur = a
    for st in steps:
        cur = reduce(cur, st[1], st[2]) if st[0] == "reduce" else resize(cur, st[1][0], st[1][1], st[2])
    return cur


@pytest.mark.parametrize("fx,fy", FACTORS)
def test_reduce_reference_equals_pillow_on_every_block_sum(fx, fy):
    a = exhaustive_sum_image(fx, fy)
    ref = np.asarray(Image.fromarray(a).reduce((fx, fy)))
    got = pr.reduce_reference(a, fx, fy)
    assert got.shape == ref.shape and np.array_equal(got, ref)
    if fx * fy & (fx * fy - 1):                    # the image does reach the sums a rounded division gets wrong
        n = fx * fy
        s = a.astype(np.int64).reshape(a.shape[0] // fy, fy, a.shape[1] // fx, fx, 3).sum((1, 3))
        assert ((s + n // 2) // n != ref).any()


@pytest.mark.parametrize("w,h,fx,fy", RAGGED)
def test_reduce_reference_equals_pillow_on_ragged_images(w, h, fx, fy):
    a = np.random.default_rng(w * 31 + h + fx * 7 + fy).integers(0, 256, (h, w, 3), dtype=np.uint8)
    ref = np.asarray(Image.fromarray(a).reduce((fx, fy)))
    got = pr.reduce_reference(a, fx, fy)
    assert got.shape == ref.shape == (-(-h // fy), -(-w // fx), 3) and np.array_equal(got, ref)


def test_whole_image_box_gives_the_unboxed_tables():
    for n_in, n_out in [(2200, 1024), (791, 1024), (500, 171), (171, 1024), (64, 64)]:
        b0, k0, s0 = pr.lanczos_coeffs(n_in, n_out)
        b1, k1, s1 = pr.lanczos_coeffs(n_in, n_out, 0.0, float(n_in))
        assert s0 == s1 and np.array_equal(b0, b1) and np.array_equal(k0, k1)
    b, kk, _ = pr.lanczos_coeffs(162, 64, 0.0, 161.5)                         # a fractional right edge moves the centres ...
    assert not np.array_equal(kk, pr.lanczos_coeffs(162, 64)[1])
    assert (b[:, 0] + b[:, 1]).max() == 162                                   # ... and the taps still reach the last (ragged) pixel


@pytest.mark.parametrize("w,h,size", [(w, h, (64, 64)) for w, h in CHAIN_64] + [(5000, 1100, (1024, 1024))])
def test_chain_with_reduce_equals_pillow(w, h, size):
    a = np.random.default_rng(w * 7 + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    steps = pr.plan_chain(w, h, size)
    assert steps is not None and steps[-1][0] == "resize" and steps[-1][1] == size
    if (w, h) in CHAIN_FACTORS:
        assert steps[0] == ("reduce",) + CHAIN_FACTORS[(w, h)]
        fx, fy = CHAIN_FACTORS[(w, h)]
        assert steps[1][2] == (0.0, 0.0, w / fx, h / fy)
    assert np.array_equal(run_chain(a, steps), pil_chain(a, size))


def test_planners_agree_where_no_reduce_is_needed_and_keep_their_limits():
    for w, h, size in [(1700, 2200, (1024, 1024)), (640, 480, (512, 512)), (100, 90, (256, 256)), (1024, 1024, (1024, 1024))]:
        assert [s[1] for s in pr.plan_chain(w, h, size)] == pr.plan(w, h, size)
        assert all(s[0] == "resize" and s[2] is None for s in pr.plan_chain(w, h, size))
    assert pr.plan(5000, 6000, (1024, 1024)) is None and pr.plan_chain(5000, 6000, (1024, 1024))[0] == ("reduce", 2, 2)
    assert pr.plan_chain(10, 2000, (1024, 1024)) is None                       # very tall image: left to Pillow in both planners
