"""Overlap-tile geometry for inference on images larger than one forward pass (pure Python, no GPU).

    p = plan(h, w, tile, blend="crop", margin=None, overlap=0.25, sigma_scale=0.125) -> TilePlan

The image [C, h, w] is extended to hp x wp = the next multiples of 32 by the reflect pad to the bottom /
right that Evaluator._run_model_single applies (row r >= h reads row 2 (h - 1) - r), cut into ny x nx tiles
of th x tw = min(tile, hp) x min(tile, wp) pixels, each tile goes through the network on its own, and the
tile outputs are blended back into one [K, h, w] map.  ops.tile_gather / ops.tile_blend (tiling.hip) read
the same geometry by value; tests/_tiling_ref.py restates both in plain loops.

Along an axis of padded length L with tile extent e = min(tile, L) and stride S:

    n    = 1 if L <= tile else ceil((L - tile) / S) + 1
    o(i) = min(i S, L - tile)                     the last tile is pulled back flush with the edge

so every origin is a multiple of 32 (pool-aligned through all three 2x2 pools and the final 2H -> H mean)
and no tile reads beyond the padded image.  Tile number = iy * nx + ix.

Stride and the weight of tile-local position t (origin o, extent e); a pixel's weight in a tile is wy * wx:

    crop      S = tile - 2 margin (margin % 16 == 0, tile >= 2 margin + 32);
              1 if (margin if o > 0 else 0) <= t < e - (margin if o + e < L else 0) else 0
    constant  S = max(32, 32 floor(tile (1 - overlap) / 32));  1
    gaussian  the same S;  exp(-0.5 ((t - (e - 1) / 2) / (sigma_scale e))^2), formed in fp32 on the host

Properties (tests/test_tiling_host.py pins them):
  * every pixel of [0, hp) x [0, wp) has positive total weight: consecutive origins are at most S apart,
    S <= e for the blended modes and S = e - 2 margin for crop, whose cores [o + margin, o + e - margin)
    therefore abut or overlap, with the first and last core reaching the image edge;
  * in crop mode at most 2 cores overlap per axis (core i + 2 starts at or behind the end of core i because
    e >= 2 margin, the clamped last origin lies behind o(n - 2)), so the weight sum of a pixel is 1, 2 or 4:
    the mean of bit-equal values is exact in fp32.

Why crop is exact and not merely seamless: in eval mode every layer of the network is position independent
(conv, BatchNorm as an affine, ReLU, 2x2 pool, x2 bilinear, 1x1, the enhance head, the 2H -> H mean), so a
logit at distance >= the receptive radius from every tile edge that is not an image edge, in a tile whose
origin is pool-aligned, is the number the whole-image forward produces.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

# Receptive margin of the logits at H, in pixels.  Measured with oracle.eunet_ref.forward (the bilinear
# Enhanced-UNet: trunk, dec1, enhance head) in fp64, eval mode, base 16, perturbed formula weights, on a
# 384 x 384 image cut into 256 x 256 tiles at origins that are multiples of 8: tile and whole-image logits
# agree to rounding (1e-16) from depth 54 inwards and differ (up to 0.08) at depths 0..53 from every edge
# that is not an image edge (an edge flush with the image costs nothing: both routes zero-pad there); at an
# origin misaligned by 4 the interior differs too (3e-3).  53 rounded up to the next multiple of 16; a
# 48-pixel margin does not suffice.  The 'unet' model (no enhance head) and upsample="transpose" (a 2x2
# up-convolution reaches less far than the bilinear taps) spread no further.  tests/test_tiling_host.py
# repeats the measurement.
RECEPTIVE_MARGIN = 64

BLENDS = ("crop", "constant", "gaussian")
ALIGN = 32  # three 2x2 pools make 8; the engine wants its input a multiple of 32 (train_eval.py:397-417)


def ceil32(v: int) -> int:
    return (int(v) + ALIGN - 1) // ALIGN * ALIGN


def axis_count(L: int, e: int, S: int) -> int:
    return 1 if L <= e else -(-(L - e) // S) + 1


def axis_origin(i: int, L: int, e: int, S: int) -> int:
    return min(i * S, L - e)


@dataclass(frozen=True)
class TilePlan:
    h: int
    w: int
    hp: int
    wp: int
    tile: int
    th: int
    tw: int
    stride: int
    ny: int
    nx: int
    blend: str
    margin: int  # crop only, else 0
    sigma_scale: float  # gaussian only

    @property
    def n(self) -> int:
        return self.ny * self.nx

    @property
    def mode(self) -> int:
        """eunet_tile_blend's mode: EUNET_TILE_CROP / CONSTANT / GAUSSIAN."""
        return BLENDS.index(self.blend)

    @property
    def inflation(self) -> float:
        """Pixels pushed through the network over pixels of the padded image."""
        return self.n * self.th * self.tw / (self.hp * self.wp)

    def origins(self, axis: int) -> Tuple[int, ...]:
        """Tile origins along axis 0 (rows) or 1 (columns)."""
        L, e, n = ((self.hp, self.th, self.ny), (self.wp, self.tw, self.nx))[axis]
        return tuple(axis_origin(i, L, e, self.stride) for i in range(n))

    def origin(self, number: int) -> Tuple[int, int]:
        """(oy, ox) of tile `number` = iy * nx + ix."""
        if not 0 <= number < self.n:
            raise IndexError(f"tile {number} of {self.n}")
        return self.origins(0)[number // self.nx], self.origins(1)[number % self.nx]

    def table(self, axis: int) -> Optional[np.ndarray]:
        """The gaussian weights of the e tile-local positions along axis (fp32; the table the blend kernel
        reads), None for the other modes."""
        if self.blend != "gaussian":
            return None
        e = (self.th, self.tw)[axis]
        t = np.arange(e, dtype=np.float32)
        c, s = np.float32((e - 1) / 2), np.float32(self.sigma_scale * e)
        z = (t - c) / s
        return np.exp(np.float32(-0.5) * z * z).astype(np.float32)

    def weights(self, axis: int, i: int) -> np.ndarray:
        """fp32 weights of the e tile-local positions of tile index i along axis."""
        L, e = ((self.hp, self.th), (self.wp, self.tw))[axis]
        o = self.origins(axis)[i]
        if self.blend == "gaussian":
            return self.table(axis)
        wgt = np.ones(e, np.float32)
        if self.blend == "crop":
            if o > 0:
                wgt[:self.margin] = 0
            if o + e < L:
                wgt[e - self.margin:] = 0
        return wgt


def plan(h: int, w: int, tile: int, *, blend: str = "crop", margin: Optional[int] = None, overlap: float = 0.25,
         sigma_scale: float = 0.125) -> TilePlan:
    """The tiling of an h x w image with tiles of at most tile x tile (module docstring)."""
    h, w, tile = int(h), int(w), int(tile)
    if blend not in BLENDS:
        raise ValueError(f"blend must be one of {BLENDS}, not {blend!r}")
    if h < 1 or w < 1:
        raise ValueError(f"image must be at least 1 x 1, not {h} x {w}")
    if tile < ALIGN or tile % ALIGN:
        raise ValueError(f"tile must be a positive multiple of {ALIGN}, not {tile}")
    hp, wp = ceil32(h), ceil32(w)
    if hp - h >= h or wp - w >= w:  # F.pad(mode="reflect") refuses a pad that is not smaller than the dimension
        raise ValueError(f"a {h} x {w} image cannot be reflect-padded to {hp} x {wp}: the padding must be "
                         "smaller than the dimension")
    if blend == "crop":
        margin = RECEPTIVE_MARGIN if margin is None else int(margin)
        if margin < 0 or margin % 16:
            raise ValueError(f"margin must be a non-negative multiple of 16, not {margin}")
        if tile < 2 * margin + ALIGN:
            raise ValueError(f"tile {tile} is too small for margin {margin}: tile >= 2 margin + {ALIGN}")
        stride = tile - 2 * margin
        sigma_scale = 0.0
    else:
        if not 0.0 <= overlap < 1.0:
            raise ValueError(f"overlap must be in [0, 1), not {overlap}")
        if blend == "gaussian" and not sigma_scale > 0.0:
            raise ValueError(f"sigma_scale must be positive, not {sigma_scale}")
        margin = 0
        stride = max(ALIGN, ALIGN * int(math.floor(tile * (1.0 - overlap) / ALIGN)))
        sigma_scale = float(sigma_scale) if blend == "gaussian" else 0.0
    th, tw = min(tile, hp), min(tile, wp)
    return TilePlan(h=h, w=w, hp=hp, wp=wp, tile=tile, th=th, tw=tw, stride=stride, ny=axis_count(hp, th, stride),
                    nx=axis_count(wp, tw, stride), blend=blend, margin=margin, sigma_scale=sigma_scale)
