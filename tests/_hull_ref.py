"""A plain-loop restatement of the per-cell convex hulls (include/eunet.h, "per-cell convex hulls"): the corner points
of a label's pixels as Python integer tuples, Andrew's monotone chain over all of them, and brute-force loops with the
header's tie rules for every column of the hull table.  Shared by tests/test_hull_host.py and tests/test_gpu_hull.py."""
import math

import numpy as np

HULL_COLS = 11


def clean(ids, n):
    """The plane as the measurement sees it: ids outside 0..n are not a label."""
    ids = np.asarray(ids).astype(np.int64)
    return np.where((ids < 0) | (ids > n), 0, ids)


def corners(plane, label):
    """The corner lattice points (x, y) of every pixel of the label, as a set of tuples of Python integers."""
    pts = set()
    ys, xs = np.nonzero(np.asarray(plane) == label)
    for y, x in zip(ys.tolist(), xs.tolist()):
        pts.update(((x, y), (x + 1, y), (x, y + 1), (x + 1, y + 1)))
    return pts


def cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def chain(points):
    """The strictly convex hull of a set of (x, y) tuples, from the point with the smallest y, then the smallest x,
    along the top edge first (y pointing down): a positive shoelace sum."""
    pts = sorted(points, key=lambda q: (q[1], q[0]))
    if len(pts) < 3:
        return pts
    halves = []
    for seq in (pts, pts[::-1]):
        half = []
        for q in seq:
            while len(half) >= 2 and cross(half[-2], half[-1], q) <= 0:
                half.pop()
            half.append(q)
        halves.append(half[:-1])
    return halves[0] + halves[1]


def hull_row(v):
    """The 11 columns of the hull table from the vertex list."""
    nv = len(v)
    row = [0] * HULL_COLS
    if nv == 0:
        return row
    row[0] = nv
    best_d, pair = -1, None
    for i in range(nv):
        for j in range(i + 1, nv):
            d = (v[j][0] - v[i][0]) ** 2 + (v[j][1] - v[i][1]) ** 2
            if d > best_d:  # strictly: the first (i, j) among equals stays
                best_d, pair = d, (i, j)
    width = None  # (c, dx, dy)
    for k in range(nv):
        a, b = v[k], v[(k + 1) % nv]
        row[1] += a[0] * b[1] - b[0] * a[1]
        dx, dy = b[0] - a[0], b[1] - a[1]
        row[2] += math.floor(65536 * math.sqrt(dx * dx + dy * dy))
        c = max(cross(a, b, q) for q in v)
        assert c >= 0
        # c^2 / |e|^2 below the best so far, in exact integers; strictly: the first edge among equals stays
        if width is None or c * c * (width[1] ** 2 + width[2] ** 2) < width[0] ** 2 * (dx * dx + dy * dy):
            width = (c, dx, dy)
    row[3] = best_d
    row[4:8] = [*v[pair[0]], *v[pair[1]]]
    row[8:11] = width
    return row


def cell_hulls(ids, n):
    """ids [p, h, w] or [h, w] -> (ext int32 [R, 2], verts int32 [2 (R + L), 2], hull int64 [p, n + 1, 11], row_off
    int64 [L + 1], vertex lists [p][n] of [(x, y)]), L = p (n + 1), in the header's layout."""
    ids = np.asarray(ids)
    if ids.ndim == 2:
        ids = ids[None]
    p, h, w = ids.shape
    L = p * (n + 1)
    hull = np.zeros((p, n + 1, HULL_COLS), np.int64)
    row_off = np.zeros(L + 1, np.int64)
    ext_rows, lists = [], [[[] for _ in range(n)] for _ in range(p)]
    for q in range(p):
        plane = clean(ids[q], n)
        for label in range(n + 1):
            r = q * (n + 1) + label
            row_off[r + 1] = row_off[r]
            if label == 0 or not (plane == label).any():
                continue
            ys, xs = np.nonzero(plane == label)
            for y in range(int(ys.min()), int(ys.max()) + 1):
                sel = xs[ys == y]
                ext_rows.append((int(sel.min()), int(sel.max())) if len(sel) else (w, -1))
            row_off[r + 1] += int(ys.max()) - int(ys.min()) + 1
            v = chain(corners(plane, label))
            lists[q][label - 1] = v
            hull[q, label] = hull_row(v)
    R = int(row_off[L])
    ext = np.asarray(ext_rows, np.int32).reshape(R, 2)
    verts = np.zeros((2 * (R + L), 2), np.int32)
    for q in range(p):
        for label in range(1, n + 1):
            r = q * (n + 1) + label
            v = lists[q][label - 1]
            assert len(v) <= 2 * (int(row_off[r + 1] - row_off[r]) + 1)
            if v:
                s = 2 * (int(row_off[r]) + r)
                verts[s:s + len(v)] = v
    return ext, verts, hull, row_off, lists


# ---- inputs -------------------------------------------------------------------------------------------------
def disc(h, w, cy, cx, r, label=1):
    yy, xx = np.mgrid[:h, :w]
    return np.where((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r, label, 0).astype(np.int64)


def ellipse(h, w, cy, cx, a, b, theta, label=1):
    yy, xx = np.mgrid[:h, :w]
    u = (xx - cx) * math.cos(theta) + (yy - cy) * math.sin(theta)
    v = -(xx - cx) * math.sin(theta) + (yy - cy) * math.cos(theta)
    return np.where((u / a) ** 2 + (v / b) ** 2 <= 1.0, label, 0).astype(np.int64)


def staircase(steps, label=1):
    """Steps of two pixels across and one down: the corners on either side lie on lines of slope 1 / 2."""
    out = np.zeros((steps + 2, 2 * steps + 2), np.int64)
    for k in range(steps):
        out[1 + k, 1 + 2 * k:3 + 2 * k] = label
    return out


def blob(rng, h, w):
    """A random walk of pixels: connected, concave, of at least two pixels (h w >= 2)."""
    assert h * w >= 2
    out = np.zeros((h, w), np.int64)
    y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
    out[y, x] = 1
    while out.sum() < 2 or rng.random() < 0.93:
        dy, dx = ((0, 1), (1, 0), (0, -1), (-1, 0))[int(rng.integers(0, 4))]
        y, x = min(max(y + dy, 0), h - 1), min(max(x + dx, 0), w - 1)
        out[y, x] = 1
    return out
