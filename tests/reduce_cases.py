"""Cases shared by the CPU and GPU tests of thumbnail's box reduction (test_pil_reduce_cpu.py, test_gpu_resample_reduce.py)."""
import numpy as np

FACTORS = [(2, 2), (3, 3), (4, 4), (5, 5), (2, 3), (3, 2), (6, 6), (7, 7), (5, 2), (1, 6), (6, 1), (3, 5)]
RAGGED = [(37, 23, 3, 3), (41, 19, 5, 2), (50, 31, 4, 4), (53, 29, 6, 7), (33, 17, 2, 1), (33, 17, 1, 3)]
# (w, h) -> the factors Image.resize(reducing_gap=2.0) picks at size (64, 64): int(w / tw / 2) or 1, int(h / th / 2) or 1
CHAIN_64 = [(320, 64), (323, 64), (256, 64), (257, 7), (581, 129), (64, 258), (385, 389), (839, 192), (255, 64)]
CHAIN_FACTORS = {(320, 64): (2, 2), (323, 64): (2, 2), (257, 7): (2, 1), (581, 129): (4, 4), (385, 389): (3, 3), (839, 192): (6, 6),
                 (64, 258): (2, 2)}


def exhaustive_sum_image(fx, fy, channels=3):
    """One fx x fy block per block sum 0 .. 255 * n, each filled with sum // n and sum % n pixels one higher: every tie of the
    rounded mean, for every output level. Blocks side by side in rows of 64; the channels hold the same sums in shifted order."""
    n = fx * fy
    sums = np.arange(255 * n + 1)
    per_row = 64
    rows = -(-len(sums) // per_row)
    img = np.zeros((rows * fy, per_row * fx, channels), np.uint8)
    for c in range(channels):
        for i, s in enumerate(np.roll(sums, 97 * c)):
            blk = np.full(n, s // n, np.uint8)
            blk[: s % n] += 1
            r, q = divmod(i, per_row)
            img[r * fy:(r + 1) * fy, q * fx:(q + 1) * fx, c] = np.roll(blk, c).reshape(fy, fx)
    return img
