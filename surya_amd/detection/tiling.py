"""Tiled detection: the rules, stated once (DetectionPredictor.tiling; kernels: csrc/det_tile.h; numpy checker: tests/det_tile_ref.py).

P is the processor size, a page is W x H.

1. Scaled page S, size (mw, mh) = (max(1, ceil(W * scale)), max(1, ceil(H * scale))). With scale == 1, S is the page's own pixels;
   otherwise S is the page after `thumbnail((mw, mh), LANCZOS)` + `resize((mw, mh), LANCZOS)`: the reference's double resize, to this
   target instead of the processor's square. A tiled page is never cut by split_image: the grid replaces the strips.
2. Tile grid, per axis with map length M: one tile at offset 0 if M <= P, else n = ceil((M - P) / (P - overlap)) + 1 tiles at
   u_i = min(i * (P - overlap), M - P). Tiles are P x P windows of S; what lies outside S is white (255), as split_image pads a last strip.
3. Ownership. The seam between tiles i and i + 1 of an axis is s_i = (u_{i+1} + u_i + P) // 2, the middle of their overlap; s_{-1} = 0
   and s_{n-1} = M. Map pixel x belongs to tile i iff s_{i-1} <= x < s_i, the two axes independently. Every pixel of the page map is
   copied from exactly one tile -- the one in which it lies farthest from a cut border, where the network had the most context. No
   blending, no max: the stitched map is a pure gather.
4. Page map: fp32 [planes][mh][round_up(mw, 4)], pad columns 0. surya_det_boxes runs on plane 0 of it; boxes are rescaled from
   (mw, mh) to (W, H).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Tuple


@dataclass(frozen=True)
class DetTiling:
    """scale in (0, 1]: the page is detected at `scale` times its own resolution. overlap: map pixels two neighbouring tiles share at
    least, 0 <= overlap <= P // 2 (the upper bound is checked against the predictor's processor size: `check`)."""
    scale: float = 1.0
    overlap: int = 128

    def __post_init__(self):
        if isinstance(self.scale, bool) or not isinstance(self.scale, (int, float)) or not (0.0 < float(self.scale) <= 1.0):
            raise ValueError(f"DetTiling.scale must be in (0, 1], got {self.scale!r}")
        if isinstance(self.overlap, bool) or not isinstance(self.overlap, int) or self.overlap < 0:
            raise ValueError(f"DetTiling.overlap must be an integer >= 0, got {self.overlap!r}")

    def check(self, P: int) -> "DetTiling":
        if self.overlap > P // 2:
            raise ValueError(f"DetTiling.overlap must be in 0..{P // 2} for processor size {P}, got {self.overlap}")
        return self


def check_tiling(tiling, P: int) -> DetTiling:
    """The refusals of DetectionPredictor.tiling, before any device work."""
    if not isinstance(tiling, DetTiling):
        raise ValueError(f"DetectionPredictor.tiling must be None or a DetTiling, got {type(tiling).__name__}")
    return tiling.check(P)


def scaled_size(w: int, h: int, scale: float) -> Tuple[int, int]:
    return max(1, math.ceil(w * scale)), max(1, math.ceil(h * scale))


def axis_offsets(M: int, P: int, overlap: int) -> List[int]:
    if M <= P:
        return [0]
    n = -(-(M - P) // (P - overlap)) + 1
    return [min(i * (P - overlap), M - P) for i in range(n)]


def axis_seams(offsets: List[int], M: int, P: int) -> List[int]:
    """[s_{-1} = 0, s_0, ..., s_{n-1} = M]: tile i owns [seams[i], seams[i + 1])."""
    return [0] + [(offsets[i + 1] + offsets[i] + P) // 2 for i in range(len(offsets) - 1)] + [M]


def axis_spans(M: int, P: int, overlap: int) -> List[Tuple[int, int, int]]:
    """Per tile of an axis: (offset, first owned map pixel, one past the last)."""
    u = axis_offsets(M, P, overlap)
    s = axis_seams(u, M, P)
    return [(u[i], s[i], s[i + 1]) for i in range(len(u))]


@dataclass(frozen=True)
class PagePlan:
    """One page under a DetTiling: scaled size, the two axes' spans, and the tiles in row-major order."""
    size: Tuple[int, int]                      # (W, H) of the page
    map_size: Tuple[int, int]                  # (mw, mh) of S and of the page map's valid region
    xs: Tuple[Tuple[int, int, int], ...]
    ys: Tuple[Tuple[int, int, int], ...]

    @property
    def grid(self) -> Tuple[int, int]:         # (columns, rows)
        return len(self.xs), len(self.ys)

    @property
    def n_tiles(self) -> int:
        return len(self.xs) * len(self.ys)

    @property
    def pitch(self) -> int:
        return (self.map_size[0] + 3) & ~3

    def tiles(self):
        """Row-major: (x0, y0, owned x span, owned y span) of every tile, spans in map coordinates."""
        return [(x[0], y[0], (x[1], x[2]), (y[1], y[2])) for y in self.ys for x in self.xs]


def page_plan(w: int, h: int, P: int, tiling: DetTiling) -> PagePlan:
    mw, mh = scaled_size(w, h, tiling.scale)
    return PagePlan((w, h), (mw, mh), tuple(axis_spans(mw, P, tiling.overlap)), tuple(axis_spans(mh, P, tiling.overlap)))
