"""A plain-loop restatement of the label-map instance metrics (include/eunet.h, "label-map instance metrics";
eunet/metrics.py, instance_stats_from_pairs), written from the definitions: dense boolean masks per id, Python ints for
every count and comparison, no table.  Also a 4-connected flood-fill labelling and the size strata as the reference's
loops (visualization.py:1762-1782).  Slow on purpose: for small maps only."""
from fractions import Fraction

import numpy as np

try:  # where scipy imports, the flood fill below is held to scipy.ndimage.label
    from scipy.ndimage import label as _scipy_label
except ImportError:
    _scipy_label = None

IOU_PERCENT = tuple(range(50, 100, 5))


def pair_table(a, b):
    """rows (plane, a, b, n) of two [p, h, w] (or [h, w]) maps with the skip rules, by np.unique over stacked keys."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    if a.ndim == 2:
        a, b = a[None], b[None]
    plane = np.broadcast_to(np.arange(a.shape[0])[:, None, None], a.shape)
    keep = (a >= 0) & (b >= 0) & ~((a == 0) & (b == 0))
    rows = np.stack([plane[keep], a[keep], b[keep]], axis=1)
    if len(rows) == 0:
        return np.zeros((0, 4), np.int64)
    uniq, n = np.unique(rows, axis=0, return_counts=True)
    return np.concatenate([uniq, n[:, None]], axis=1).astype(np.int64)


def _masks(m, valid):
    return {int(i): (m == i) & valid for i in np.unique(m[valid]).tolist() if i >= 1}


def plane_stats(pred, gt, iou_percent=IOU_PERCENT):
    """The statistics of one plane (one class) of a prediction and a ground-truth id map [h, w]: a dict of Python
    numbers and, for tp, a list per threshold.  A pixel with a negative id on either side is left out of everything."""
    pred, gt = np.asarray(pred, np.int64), np.asarray(gt, np.int64)
    valid = (pred >= 0) & (gt >= 0)
    P, G = _masks(pred, valid), _masks(gt, valid)
    area_p = {i: int(m.sum()) for i, m in P.items()}
    area_g = {j: int(m.sum()) for j, m in G.items()}
    inter = {(i, j): int((P[i] & G[j]).sum()) for i in P for j in G}
    union = {(i, j): area_p[i] + area_g[j] - n for (i, j), n in inter.items()}
    st = {"n_pred": len(P), "n_gt": len(G), "tp": [0] * len(iou_percent), "tp50": 0, "iou_sum": 0.0}
    for i in sorted(P):
        for j in sorted(G):
            n, u = inter[(i, j)], union[(i, j)]
            if n == 0:
                continue
            for k, t in enumerate(iou_percent):
                if Fraction(n, u) > Fraction(t, 100):
                    st["tp"][k] += 1
            if Fraction(n, u) > Fraction(1, 2):
                st["tp50"] += 1
                st["iou_sum"] += n / u
    # Aggregated Jaccard Index (Kumar et al. 2017)
    c = u_sum = 0
    used = set()
    for j in sorted(G):
        best = None
        for i in sorted(P):
            if inter[(i, j)] > 0 and (best is None or
                                      Fraction(inter[(i, j)], union[(i, j)]) > Fraction(inter[(best, j)], union[(best, j)])):
                best = i
        if best is None:
            u_sum += area_g[j]
        else:
            c += inter[(best, j)]
            u_sum += union[(best, j)]
            used.add(best)
    u_sum += sum(area_p[i] for i in P if i not in used)
    st["aji_c"], st["aji_u"] = c, u_sum
    # object-level Dice (GlaS): each object against the object of largest overlap on the other side
    def side(A, B, area_a, area_b, n_of):
        total = 0.0
        for x in sorted(A):
            best = None
            for y in sorted(B):
                if n_of(x, y) > 0 and (best is None or n_of(x, y) > n_of(x, best)):
                    best = y
            if best is not None:
                total += 2 * n_of(x, best) * area_a[x] / (area_a[x] + area_b[best])
        return total
    st["objdice_g"] = side(G, P, area_g, area_p, lambda j, i: inter[(i, j)])
    st["objdice_gw"] = sum(area_g.values())
    st["objdice_p"] = side(P, G, area_p, area_g, lambda i, j: inter[(i, j)])
    st["objdice_pw"] = sum(area_p.values())
    # SEG (Cell Tracking Challenge): the prediction that covers more than half of the ground truth, if any
    seg = 0.0
    for j in sorted(G):
        for i in sorted(P):
            if 2 * inter[(i, j)] > area_g[j]:
                seg += inter[(i, j)] / union[(i, j)]
    st["seg_sum"] = seg
    return st


def stats(pred, gt, iou_percent=IOU_PERCENT):
    """plane_stats of every plane of [p, h, w] maps, as arrays indexed by plane."""
    rows = [plane_stats(p, g, iou_percent) for p, g in zip(pred, gt)]
    return {k: np.asarray([r[k] for r in rows]) for k in rows[0]}


def _div(a, b):
    return float(a) / float(b) if b else float("nan")


def scores(st, iou_percent=IOU_PERCENT):
    """The scores of one row of statistics (Python numbers)."""
    tp, fp, fn = st["tp50"], st["n_pred"] - st["tp50"], st["n_gt"] - st["tp50"]
    m = {"pq": _div(st["iou_sum"], tp + fp / 2 + fn / 2), "sq": _div(st["iou_sum"], tp), "dq": _div(tp, tp + fp / 2 + fn / 2),
         "aji": _div(st["aji_c"], st["aji_u"]),
         "objdice": (_div(st["objdice_g"], st["objdice_gw"]) + _div(st["objdice_p"], st["objdice_pw"])) / 2,
         "seg": _div(st["seg_sum"], st["n_gt"])}
    sweep = []
    for k, t in enumerate(iou_percent):
        tpt = st["tp"][k]
        m[f"f1_{t}"] = _div(2 * tpt, 2 * tpt + (st["n_pred"] - tpt) + (st["n_gt"] - tpt))
        sweep.append(_div(tpt, tpt + (st["n_pred"] - tpt) + (st["n_gt"] - tpt)))
    m["ap_dsb"] = float(np.mean(sweep))
    return m


def label4(mask):
    """4-connected components by flood fill, numbered 1.. in raster order of each component's first pixel."""
    mask = np.asarray(mask) != 0
    h, w = mask.shape
    lab = np.zeros((h, w), np.int32)
    n = 0
    for y in range(h):
        for x in range(w):
            if not mask[y, x] or lab[y, x]:
                continue
            n += 1
            lab[y, x] = n
            todo = [(y, x)]
            while todo:
                cy, cx = todo.pop()
                for ny, nx in ((cy - 1, cx), (cy + 1, cx), (cy, cx - 1), (cy, cx + 1)):
                    if 0 <= ny < h and 0 <= nx < w and mask[ny, nx] and not lab[ny, nx]:
                        lab[ny, nx] = n
                        todo.append((ny, nx))
    if _scipy_label is not None:  # scipy's numbering order is no contract: canonicalise it by first pixel
        theirs, m = _scipy_label(mask)
        assert m == n
        first = {}
        for v in theirs.ravel().tolist():
            if v and v not in first:
                first[v] = len(first) + 1
        canon = np.zeros_like(lab)
        for v, k in first.items():
            canon[theirs == v] = k
        assert np.array_equal(canon, lab)
    return lab, n


def size_strata(gts, preds, num_classes=3, edges=(100, 500, 1000, 5000)):
    """The per-object coverage lists of visualization.py:1753-1817, as loops: image by image and class by class
    (background included), every 4-connected ground-truth component (label4 for scipy.ndimage.label) gives the
    fraction of its pixels that the prediction assigns to the same class, appended to the bin lo <= area < hi."""
    lows = (0,) + tuple(edges)
    highs = tuple(edges) + (float("inf"),)
    bins = [[] for _ in lows]
    for gt, pred in zip(gts, preds):
        for c in range(num_classes):
            comps, n = label4(gt == c)
            hit = (pred == c).astype(int)
            for k in range(1, n + 1):
                inside = comps == k
                area = inside.sum()
                cover = hit[inside].sum() / area  # numpy int / int: the float64 of the quotient
                for b, (lo, hi) in enumerate(zip(lows, highs)):
                    if lo <= area < hi:
                        bins[b].append(cover)
                        break
    return bins
