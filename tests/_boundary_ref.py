"""A numpy restatement of include/eunet.h's eunet_edt_sq and eunet_boundary_stats, in the project's own words: the
edges, the squared distance as the separable two-pass minimum, the three statistics buffers and the reference
rows.  tests/test_boundary_host.py holds it to an all-pairs brute force and to scipy.ndimage; the GPU tests hold
the kernels to it."""
import math

import numpy as np

NONE = 2 ** 31 - 1  # EUNET_EDT_NONE


def region(m, v):
    """R_v(M): int64 comparison in all 64 bits."""
    return np.asarray(m, np.int64) == np.int64(v)


def _shift(a, dy, dx, fill=False):
    """b[y, x] = a[y + dy, x + dx], fill outside the image."""
    h, w = a.shape
    b = np.full_like(a, fill)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    if abs(dy) < h and abs(dx) < w:
        b[yd, xd] = a[ys, xs]
    return b


def edges(r):
    """E: the pixels of the region r (bool [h, w]) with a 4-neighbour outside the image or outside r."""
    inner = r.copy()
    for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        inner &= _shift(r, dy, dx)
    return r & ~inner


def sites(m, v, mode):
    r = region(m, v)
    return {"eq": r, "ne": ~r, "edge": edges(r)}[mode]


def edt_sq(s):
    """Squared Euclidean distance to the nearest True of s (bool [h, w]), int64, NONE everywhere without one:
    g(y, x) = the squared vertical distance to the nearest site of column x, then D(y, x) = min_j g(y, j) + (x - j)^2."""
    h, w = s.shape
    if not s.any():
        return np.full((h, w), NONE, np.int64)
    if w > h:  # the distance is symmetric in the axes: let the quadratic second pass run along the shorter one
        return np.ascontiguousarray(edt_sq(np.ascontiguousarray(s.T)).T)
    big = np.int64(4 * 8192 * 8192)
    far = np.int64(3 * 8192)
    ys = np.arange(h, dtype=np.int64)[:, None]
    above = np.maximum.accumulate(np.where(s, ys, -far), axis=0)  # the last site row at or above, or -far
    below = np.minimum.accumulate(np.where(s, ys, far)[::-1], axis=0)[::-1]  # the first at or below, or far
    g = np.minimum(ys - above, below - ys) ** 2
    g[g >= far * far // 4] = big  # a column without a site
    xs = np.arange(w, dtype=np.int64)
    off = (xs[:, None] - xs[None, :]) ** 2  # [x, j]
    d = np.empty((h, w), np.int64)
    for y in range(h):
        d[y] = (g[y][None, :] + off).min(axis=1)
    assert d.max() < big
    return d


def edt_sq_maps(maps, values, mode):
    """eunet_edt_sq: maps int64 [n, h, w] -> int32 [n, nv, h, w]."""
    maps = np.asarray(maps, np.int64)
    out = np.empty((maps.shape[0], len(values)) + maps.shape[1:], np.int32)
    for i, m in enumerate(maps):
        for j, v in enumerate(values):
            out[i, j] = edt_sq(sites(m, v, mode))
    return out


def isqrt_q16(d2):
    """floor(2^16 sqrt(d2)) as the integer square root of d2 2^32."""
    return math.isqrt(int(d2) << 32)


def _diamond(radius):
    return [(dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)
            if abs(dy) + abs(dx) <= radius]


def ref_sets(r):
    """(boundary, interior) of the region r as the reference forms them: the pixels whose radius-1 L1 diamond
    holds both a pixel of r and a position outside r (or outside the image); the pixels whose whole radius-2
    diamond is inside the image and in r."""
    any1 = np.zeros_like(r)
    all1 = np.ones_like(r)
    for dy, dx in _diamond(1):
        any1 |= _shift(r, dy, dx)
        all1 &= _shift(r, dy, dx)
    all2 = np.ones_like(r)
    for dy, dx in _diamond(2):
        all2 &= _shift(r, dy, dx)
    return any1 & ~all1, all2


def boundary_stats(pred, gt, k=3, ignore_index=255, cap=64, radii=(2,)):
    """eunet_boundary_stats on zeroed buffers: (surf [k, 2, cap^2 + 5], band [k, nr, 3], refrows [n, k, 2, 3])."""
    pred, gt = np.asarray(pred, np.int64), np.asarray(gt, np.int64)
    if pred.ndim == 2:
        pred, gt = pred[None], gt[None]
    cap2 = cap * cap
    surf = np.zeros((k, 2, cap2 + 5), np.int64)
    band = np.zeros((k, len(radii), 3), np.int64)
    refrows = np.zeros((pred.shape[0], k, 2, 3), np.int64)
    for i, (p0, g) in enumerate(zip(pred, gt)):
        p = np.where(g == ignore_index, np.int64(ignore_index), p0)  # the ignore rule
        for c in range(k):
            rp, rg = region(p, c), region(g, c)
            ep, eg = edges(rp), edges(rg)
            dp, dg = edt_sq(ep), edt_sq(eg)
            for direction, (own, other) in enumerate(((ep, dg), (eg, dp))):
                s = surf[c, direction]
                for d2 in other[own]:
                    d2 = int(d2)
                    if d2 == NONE:
                        s[cap2 + 2] += 1
                        continue
                    s[d2 if d2 <= cap2 else cap2 + 1] += 1
                    s[cap2 + 3] = max(int(s[cap2 + 3]), d2)
                    s[cap2 + 4] += isqrt_q16(d2)
            for j, r in enumerate(radii):
                bp, bg = rp & (dp <= r * r), rg & (dg <= r * r)
                band[c, j] += (int(bp.sum()), int(bg.sum()), int((bp & bg).sum()))
            for row, (sp, sg) in enumerate(zip(ref_sets(region(p0, c)), ref_sets(rg))):  # the maps as they are
                refrows[i, c, row] = (int(sp.sum()), int(sg.sum()), int((sp & sg).sum()))
    return surf, band, refrows


def combine(a, b, cap):
    """Two surf buffers accumulated into one: everything adds, the maximum is the max."""
    out = a + b
    out[..., cap * cap + 3] = np.maximum(a[..., cap * cap + 3], b[..., cap * cap + 3])
    return out


def edge_distances(pred, gt, c, ignore_index=255):
    """The explicit distance lists (pixels, float64; inf without a counterpart) of class c for one image pair:
    (pred edge -> gt edge, gt edge -> pred edge).  What the metrics are defined on."""
    pred, gt = np.asarray(pred, np.int64), np.asarray(gt, np.int64)
    p = np.where(gt == ignore_index, np.int64(ignore_index), pred)
    ep, eg = edges(region(p, c)), edges(region(gt, c))
    out = []
    for own, other in ((ep, eg), (eg, ep)):
        d2 = edt_sq(other)[own].astype(np.float64)
        out.append(np.where(d2 == NONE, np.inf, np.sqrt(d2)))
    return out
