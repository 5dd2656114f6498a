"""Test infrastructure: tiled detection in plain numpy -- the grid, the seams, the cut and the stitch, restated from the rules of
surya_amd/detection/tiling.py without importing it (the CPU test holds the two statements against each other and against the table of
worked cases; the GPU tests hold the kernels of csrc/det_tile.h and the predictor path against this file, bit for bit)."""
import numpy as np


def offsets(M, P, overlap):
    if M <= P:
        return [0]
    step = P - overlap
    n = (M - P + step - 1) // step + 1
    return [min(i * step, M - P) for i in range(n)]


def seams(M, P, overlap):
    """The inner seams s_0 .. s_{n-2}: the middle of each pair of neighbours' overlap."""
    u = offsets(M, P, overlap)
    return [(u[i + 1] + u[i] + P) // 2 for i in range(len(u) - 1)]


def spans(M, P, overlap):
    """Per tile of the axis: (offset, first owned pixel, one past the last owned pixel)."""
    u = offsets(M, P, overlap)
    s = [0] + seams(M, P, overlap) + [M]
    return [(u[i], s[i], s[i + 1]) for i in range(len(u))]


def cut_window(page, x0, y0, P, dst_pix):
    """The P x P window at (x0, y0) of a uint8 [h, w, 3 | 4] page as [P, P, dst_pix]: white outside the page, fourth byte 0."""
    h, w = page.shape[:2]
    out = np.full((P, P, dst_pix), 255, np.uint8)
    if dst_pix == 4:
        out[..., 3] = 0
    ya, yb, xa, xb = max(y0, 0), min(y0 + P, h), max(x0, 0), min(x0 + P, w)
    if ya < yb and xa < xb:
        out[ya - y0: yb - y0, xa - x0: xb - x0, :3] = page[ya:yb, xa:xb, :3]
    return out


def cut_grid(page, P, overlap, dst_pix=4):
    """Every tile of a page (which IS its scaled page), row-major: [rows * columns, P, P, dst_pix]."""
    h, w = page.shape[:2]
    return np.stack([cut_window(page, x0, y0, P, dst_pix) for y0 in offsets(h, P, overlap) for x0 in offsets(w, P, overlap)])


def cut_map(m, P, overlap, fill=0.0):
    """A float [planes, mh, mw] map cut the same way (what a network that reproduced its input would return per tile): row-major
    [tiles, planes, P, P], `fill` outside the map."""
    planes, mh, mw = m.shape
    out = []
    for y0 in offsets(mh, P, overlap):
        for x0 in offsets(mw, P, overlap):
            t = np.full((planes, P, P), fill, m.dtype)
            yb, xb = min(y0 + P, mh), min(x0 + P, mw)
            t[:, : yb - y0, : xb - x0] = m[:, y0:yb, x0:xb]
            out.append(t)
    return np.stack(out)


def stitch(tiles, mw, mh, P, overlap, planes=None, out=None, only=None):
    """tiles float32 [rows * columns, labels, P, P] (row-major) -> the page map [planes, mh, round_up(mw, 4)], pad columns 0: every pixel
    from the one tile that owns it. `out`: stitch into this array (cells no tile owns stay); `only`: the tile indices to stitch."""
    planes = tiles.shape[1] if planes is None else planes
    pitch = (mw + 3) & ~3
    if out is None:
        out = np.zeros((planes, mh, pitch), np.float32)
    xs, ys = spans(mw, P, overlap), spans(mh, P, overlap)
    t = 0
    for y0, ya, yb in ys:
        for x0, xa, xb in xs:
            if only is None or t in only:
                out[:, ya:yb, xa:xb] = tiles[t, :planes, ya - y0: yb - y0, xa - x0: xb - x0]
                if xb == mw:
                    out[:, ya:yb, mw:] = 0
            t += 1
    return out


def bar_map():
    """The seam-crossing bar: 160 rows x 200 columns of 0.02 with one 160-pixel line across all three vertical seams of P = 64, overlap 16."""
    yy, xx = np.mgrid[0:160, 0:200].astype(np.float32)
    bar = np.exp(-np.maximum(np.abs(xx - 100) / 80, np.abs(yy - 70) / 6) ** 4) * 0.9
    return np.ascontiguousarray(np.maximum(np.float32(0.02), bar).astype(np.float32))
