"""Restatement of the warp kernels (include/eunet.h, "elastic deformation and affine warp"): the sampling map in
fp64 with explicit loops over the 4 x 4 taps, the two gathers in numpy integers from a given float32 map.
tests/test_warp_host.py holds these to plain torch (F.interpolate, F.grid_sample)."""
import numpy as np

A = -0.75  # the cubic-convolution kernel of F.interpolate(mode="bicubic")
LIMIT = float(1 << 20)


def cubic_weights(t):
    """Weights of the taps floor(u) - 1 .. floor(u) + 2 at fraction t."""
    def near(v):   # |distance| <= 1
        return ((A + 2.0) * v - (A + 3.0)) * v * v + 1.0

    def far(v):    # 1 < |distance| < 2
        return ((A * v - 5.0 * A) * v + 8.0 * A) * v - 4.0 * A
    return [far(t + 1.0), near(t), near(1.0 - t), far(2.0 - t)]


def _pos(n, g):
    """(floor(u), u - floor(u)) of u = x (g - 1) / (n - 1) for x = 0 .. n - 1 (u = 0 when n == 1)."""
    x = np.arange(n, dtype=np.float64)
    u = np.zeros(n) if n == 1 else x * (g - 1) / (n - 1)
    i = np.floor(u)
    return i.astype(np.int64), u - i


def displacement_ref(h, w, ctrl):
    """fp64 [2, h, w]: the bicubic interpolation (align_corners=True) of ctrl [2, gh, gw]; explicit loops over
    the 4 x 4 taps, every pixel at once."""
    ctrl = np.asarray(ctrl, dtype=np.float64)
    _, gh, gw = ctrl.shape
    iy, ty = _pos(h, gh)
    ix, tx = _pos(w, gw)
    wy, wx = cubic_weights(ty), cubic_weights(tx)
    out = np.zeros((2, h, w), dtype=np.float64)
    for a in range(4):
        yy = np.clip(iy - 1 + a, 0, gh - 1)
        for b in range(4):
            xx = np.clip(ix - 1 + b, 0, gw - 1)
            out += (wy[a][:, None] * wx[b][None, :])[None] * ctrl[:, yy[:, None], xx[None, :]]
    return out


def grid_ref(h, w, ctrl, m=None):
    """fp64 [h, w, 2]: (sx, sy) = m (x, y, 1) + D(y, x); m is the 2x3 inverse map (None: identity)."""
    m = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]) if m is None else np.asarray(m, dtype=np.float64)
    d = displacement_ref(h, w, ctrl)
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    out = np.empty((h, w, 2), dtype=np.float64)
    out[..., 0] = m[0, 0] * x + m[0, 1] * y + m[0, 2] + d[0]
    out[..., 1] = m[1, 0] * x + m[1, 1] * y + m[1, 2] + d[1]
    return out


def quantise(grid):
    """float32 map -> (qx, qy int64 in 1/32 pixel, finite mask)."""
    g = np.asarray(grid)
    assert g.dtype == np.float32 and g.ndim == 3 and g.shape[2] == 2
    ok = np.isfinite(g[..., 0]) & np.isfinite(g[..., 1])
    c = np.clip(np.where(ok[..., None], g, np.float32(0)), np.float32(-LIMIT), np.float32(LIMIT))
    q = np.rint(c * np.float32(32.0)).astype(np.int64)  # exact product, round-half-even
    return q[..., 0], q[..., 1], ok


def border_index(i, n, border):
    """(index into [0, n), inside mask) of integer indices i under the border rule."""
    i = np.asarray(i, dtype=np.int64)
    if border == "constant":
        inside = (i >= 0) & (i < n)
        return np.where(inside, i, 0), inside
    assert border == "reflect"
    if n == 1:
        return np.zeros_like(i), np.ones(i.shape, dtype=bool)
    p = 2 * (n - 1)
    r = np.mod(i, p)  # non-negative
    r = np.where(r >= n, p - r, r)
    return r, np.ones(i.shape, dtype=bool)


def warp_u8_ref(src, grid, border="reflect", fill=0):
    """HWC uint8 [hi, wi, c] through a float32 map [ho, wo, 2] -> uint8 [ho, wo, c]."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3
    hi, wi, _ = src.shape
    qx, qy, ok = quantise(grid)
    ix, fx, iy, fy = qx >> 5, qx & 31, qy >> 5, qy & 31
    acc = np.zeros(qx.shape + (src.shape[2],), dtype=np.int64)
    for dy, dx, wgt in ((0, 0, (32 - fx) * (32 - fy)), (0, 1, fx * (32 - fy)), (1, 0, (32 - fx) * fy), (1, 1, fx * fy)):
        bx, inx = border_index(ix + dx, wi, border)
        by, iny = border_index(iy + dy, hi, border)
        p = np.where((inx & iny)[..., None], src[by, bx].astype(np.int64), fill)
        acc += wgt[..., None] * p
    out = (acc + 512) >> 10
    return np.where(ok[..., None], out, fill).astype(np.uint8)


def warp_labels_ref(x, grid, border="reflect", fill=0, flip_h=False, flip_v=False):
    """int64 [hi, wi] or uint8 [n, hi, wi] through a float32 map -> [ho, wo] / [n, ho, wo], mirrored by the flags."""
    x = np.asarray(x)
    g = np.asarray(grid)
    if flip_v:
        g = g[::-1]
    if flip_h:
        g = g[:, ::-1]
    qx, qy, ok = quantise(np.ascontiguousarray(g))
    hi, wi = x.shape[-2:]
    bx, inx = border_index((qx + 16) >> 5, wi, border)
    by, iny = border_index((qy + 16) >> 5, hi, border)
    take = ok & inx & iny
    if x.ndim == 2:
        return np.where(take, x[by, bx], fill).astype(x.dtype)
    return np.where(take[None], x[:, by, bx], fill).astype(x.dtype)
