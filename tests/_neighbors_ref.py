"""Plain-loop restatements of include/eunet.h, "nearest-cell transform, label expansion and cell contacts": the
all-pairs (d^2, index) minimum, the separable two-pass formulation the kernels follow, the expansion rule and the
contact count.  tests/test_neighbors_host.py holds the first to scipy.ndimage and the second to the first; the GPU
tests hold the kernels to them.  numpy only, integers only."""
import numpy as np

NONE = 2 ** 31 - 1  # EUNET_EDT_NONE


def _planes(ids):
    ids = np.asarray(ids)
    assert ids.ndim in (2, 3)
    return ids.reshape((-1,) + ids.shape[-2:])


def nearest_site(ids):
    """ids [h, w] or [p, h, w] -> (dist int32, site int32) shaped as ids: per plane the lexicographic minimum of
    (squared distance, linear index) over the sites (id >= 1), all pairs; (NONE, -1) in a plane without a site.  The
    sites are visited in ascending index and a later one wins only when strictly nearer."""
    stack = _planes(ids)
    p, h, w = stack.shape
    dist = np.full((p, h, w), NONE, np.int64)
    site = np.full((p, h, w), -1, np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    for q in range(p):
        for s in np.flatnonzero(stack[q].reshape(-1) >= 1).tolist():
            sy, sx = divmod(s, w)
            d = (yy - sy) ** 2 + (xx - sx) ** 2
            nearer = d < dist[q]
            dist[q][nearer] = d[nearer]
            site[q][nearer] = s
    return dist.astype(np.int32).reshape(np.shape(ids)), site.astype(np.int32).reshape(np.shape(ids))


def nearest_site_separable(plane, strict=True):
    """One plane [h, w], by the two passes of the kernels, in plain loops: per column the row of the nearest site
    (the smaller row of two equally near, -1 without one); per row an outward scan from r = 0 over (g + r^2, row w +
    column) that stops at the first r with r^2 > best (strict) or, as a distance-only transform may, r^2 >= best (not
    strict: wrong for sites, kept here to show it)."""
    plane = np.asarray(plane)
    h, w = plane.shape
    rows = np.full((h, w), -1, np.int64)
    for x in range(w):
        up = -1
        for y in range(h):
            if plane[y, x] >= 1:
                up = y
            rows[y, x] = up
        dn = -1
        for y in range(h - 1, -1, -1):
            u = rows[y, x]
            if u == y:
                dn = y
            rows[y, x] = u if u >= 0 and (dn < 0 or y - u <= dn - y) else dn
    dist = np.full((h, w), NONE, np.int64)
    site = np.full((h, w), -1, np.int64)
    for y in range(h):
        for x in range(w):
            best = (NONE, -1)
            for r in range(0, max(x, w - 1 - x) + 1):
                if best[1] >= 0 and (r * r > best[0] if strict else r * r >= best[0]):
                    break
                for xx in ((x,) if r == 0 else (x - r, x + r)):
                    if 0 <= xx < w and rows[y, xx] >= 0:
                        row = int(rows[y, xx])
                        c = ((y - row) ** 2 + r * r, row * w + xx)
                        if best[1] < 0 or c < best:
                            best = c
            dist[y, x], site[y, x] = best
    return dist.astype(np.int32), site.astype(np.int32)


def expand(ids, limit2=None):
    """The expansion rule: a pixel with an id other than 0 keeps it; a pixel with id 0 takes the id of its nearest
    site when the squared distance is <= limit2 (None: always), and stays 0 otherwise."""
    stack = _planes(ids)
    dist, site = nearest_site(stack)
    out = stack.copy()
    p, h, w = stack.shape
    for q in range(p):
        for y in range(h):
            for x in range(w):
                if stack[q, y, x] == 0 and site[q, y, x] >= 0 and (limit2 is None or dist[q, y, x] <= limit2):
                    out[q, y, x] = stack[q].reshape(-1)[site[q, y, x]]
    return out.reshape(np.shape(ids))


def contacts(ids, connectivity=4):
    """int64 [m, 4] rows (plane, a, b, n), a < b, sorted: n adjacent pixel pairs of the plane carry the ids a and b,
    both >= 1.  Every pixel is paired with its right and lower neighbour, at connectivity 8 also with its lower-left
    and lower-right one."""
    stack = _planes(ids)
    p, h, w = stack.shape
    steps = [(0, 1), (1, 0)] + ([(1, -1), (1, 1)] if connectivity == 8 else [])
    table = {}
    for q in range(p):
        for y in range(h):
            for x in range(w):
                a = int(stack[q, y, x])
                for dy, dx in steps:
                    yy, xx = y + dy, x + dx
                    if a >= 1 and 0 <= yy < h and 0 <= xx < w:
                        b = int(stack[q, yy, xx])
                        if b >= 1 and b != a:
                            key = (q, min(a, b), max(a, b))
                            table[key] = table.get(key, 0) + 1
    return np.asarray([k + (n,) for k, n in sorted(table.items())], np.int64).reshape(-1, 4)


def blobs(h, w, n, seed, ignore=False):
    """A map of up to n disc-like labels on background 0 (later discs overwrite earlier ones, so labels touch), with
    a few negative "ignore" pixels if asked for.  int64 [h, w]."""
    rng = np.random.RandomState(seed)
    out = np.zeros((h, w), np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    for i in range(1, n + 1):
        cy, cx, r = rng.randint(0, h), rng.randint(0, w), rng.randint(1, 2 + max(h, w) // 8)
        out[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = i
    if ignore:
        out[rng.rand(h, w) < 0.03] = -1
    return out
