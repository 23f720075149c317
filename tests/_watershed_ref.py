"""Plain-loop restatement of the distance-transform watershed (include/eunet.h, "distance-transform watershed"):
ascent to the root of largest key, saddles between basins, the merge by depth, ids in raster order.  Nothing here
is shared with eunet.ops: the merge in particular is written again, over root pixel indices."""
import math

import numpy as np

NONE = 2 ** 31 - 1
NEIGHBOURS = tuple((dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
FORWARD = ((0, 1), (1, -1), (1, 0), (1, 1))  # E, SW, S, SE: every unordered 8-adjacent pair once


def edt_sq(fg):
    """Exact squared Euclidean distance of every pixel of the bool mask fg to the nearest pixel outside it (0 off
    the mask, NONE everywhere when the mask has no background): distance_transform_sq(mask, [1], "ne")."""
    fg = np.asarray(fg, bool)
    h, w = fg.shape
    if fg.all():
        return np.full((h, w), NONE, np.int64)
    big = 4 * (h + w) ** 2
    ys = np.arange(h)
    g = np.full((h, w), big, np.int64)  # squared vertical distance to the nearest background pixel of the column
    for x in range(w):
        bg = ys[~fg[:, x]]
        if len(bg):
            g[:, x] = ((ys[:, None] - bg[None, :]) ** 2).min(axis=1)
    xs = np.arange(w)
    dx2 = (xs[:, None] - xs[None, :]) ** 2
    out = np.empty((h, w), np.int64)
    for y in range(h):
        out[y] = (g[y][None, :] + dx2).min(axis=1)
    return out


def ascent(D):
    """root [h * w]: the linear index of every foreground pixel's root, -1 on the background."""
    h, w = D.shape
    up = np.full(h * w, -1, np.int64)
    for y in range(h):
        for x in range(w):
            if D[y, x] <= 0:
                continue
            best = (int(D[y, x]), -(y * w + x))
            for dy, dx in NEIGHBOURS:
                yy, xx = y + dy, x + dx
                if 0 <= yy < h and 0 <= xx < w and D[yy, xx] > 0:
                    k = (int(D[yy, xx]), -(yy * w + xx))
                    if k > best:
                        best = k
            up[y * w + x] = -best[1]
    root = np.full(h * w, -1, np.int64)
    for p in range(h * w):
        if up[p] < 0:
            continue
        chain, q = [], p
        while root[q] < 0 and up[q] != q:
            chain.append(q)
            q = int(up[q])
        r = q if root[q] < 0 else int(root[q])
        root[q] = r
        for c in chain:
            root[c] = r
    return root


def saddles(D, root):
    """{(a, b), a < b roots: the largest min(D[p], D[q]) over the 8-adjacent pairs p in a, q in b}."""
    h, w = D.shape
    Df = D.ravel()
    sad = {}
    for y in range(h):
        for x in range(w):
            p = y * w + x
            if root[p] < 0:
                continue
            for dy, dx in FORWARD:
                yy, xx = y + dy, x + dx
                if 0 <= yy < h and 0 <= xx < w and root[yy * w + xx] >= 0:
                    q = yy * w + xx
                    a, b = int(root[p]), int(root[q])
                    if a != b:
                        k = (min(a, b), max(a, b))
                        s = int(min(Df[p], Df[q]))
                        if sad.get(k, -1) < s:
                            sad[k] = s
    return sad


def merge(D, root, sad, depth):
    """-> (ids int32 [h, w], number of regions, areas int32 [regions])."""
    h, w = D.shape
    Df = D.ravel()
    par = {}

    def find(a):
        while par.get(a, a) != a:
            a = par[a]
        return a

    for ns, a, b in sorted((-s, a, b) for (a, b), s in sad.items()):
        ra, rb = find(a), find(b)
        if ra == rb:
            continue
        ka, kb = (int(Df[ra]), -ra), (int(Df[rb]), -rb)
        lo, hi = (ra, rb) if ka < kb else (rb, ra)
        if math.sqrt(int(Df[lo])) - math.sqrt(-ns) < depth:
            par[lo] = hi
    ids = np.zeros(h * w, np.int32)
    number = {}
    for p in range(h * w):
        if root[p] >= 0:
            rep = find(int(root[p]))
            if rep not in number:
                number[rep] = len(number) + 1
            ids[p] = number[rep]
    return ids.reshape(h, w), len(number), np.bincount(ids, minlength=len(number) + 1)[1:].astype(np.int32)


class Basins:
    """Ascent and saddles of one plane, computed once; split(depth) is then cheap."""

    def __init__(self, D):
        self.D = np.asarray(D, np.int64)
        self.root = ascent(self.D)
        self.sad = saddles(self.D, self.root)

    def split(self, depth):
        return merge(self.D, self.root, self.sad, depth)


def split(D, depth):
    return Basins(D).split(depth)


def discs(h, w, centres):
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), bool)
    for cy, cx, r in centres:
        m |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    return m
