"""A plain-loop numpy restatement of the per-cell measurements (include/eunet.h, "per-cell measurements"): for every
label np.nonzero, then the sums, the box and the bit quads from the definition, and the descriptors by a route of
their own (the central moments directly from the coordinates about the float64 centroid).  Shared by
tests/test_cellprops_host.py and tests/test_gpu_cellprops.py."""
import math

import numpy as np

GEOM_COLS = 14


def clean(ids, n):
    """The plane as the measurement sees it: ids outside 0..n are not a label."""
    ids = np.asarray(ids).astype(np.int64)
    return np.where((ids < 0) | (ids > n), 0, ids)


def quads(plane, label):
    """(q1, q2, q3, qd, q4) of one label: over all (h + 1) (w + 1) windows of 2 x 2 pixels of the padded plane."""
    m = np.pad(np.asarray(plane) == label, 1).astype(np.int64)
    tl, tr, bl, br = m[:-1, :-1], m[:-1, 1:], m[1:, :-1], m[1:, 1:]
    cnt = tl + tr + bl + br
    diag = (cnt == 2) & (tl == br)  # two set pixels and equal diagonal ends: the two lie on one diagonal
    return (int((cnt == 1).sum()), int(((cnt == 2) & ~diag).sum()), int((cnt == 3).sum()), int(diag.sum()),
            int((cnt == 4).sum()))


def cell_stats(ids, n, image=None):
    """ids [p, h, w] or [h, w] -> (geom int64 [p, n + 1, 14], intensity int64 [p, n + 1, c, 4] or None, skipped [p])."""
    ids = np.asarray(ids)
    if ids.ndim == 2:
        ids = ids[None]
    p, h, w = ids.shape
    img = None
    if image is not None:
        img = np.asarray(image)
        img = img[:, :, None] if img.ndim == 2 else img
    c = 0 if img is None else img.shape[2]
    geom = np.zeros((p, n + 1, GEOM_COLS), np.int64)
    inten = None if img is None else np.zeros((p, n + 1, c, 4), np.int64)
    skipped = np.zeros(p, np.int64)
    for q in range(p):
        raw = ids[q].astype(np.int64)
        skipped[q] = int(((raw < 0) | (raw > n)).sum())
        plane = clean(raw, n)
        geom[q, 1:, 6:10] = (w, h, -1, -1)  # the rows of a label with no pixel
        if inten is not None:
            inten[q, 1:, :, 2] = 255
        for label in np.unique(plane[plane > 0]).tolist():  # the labels with a pixel: a large n stays cheap
            row = geom[q, label]
            ys, xs = np.nonzero(plane == label)
            ys, xs = ys.astype(np.int64), xs.astype(np.int64)
            row[0] = len(xs)
            row[1], row[2] = xs.sum(), ys.sum()
            row[3], row[4], row[5] = (xs * xs).sum(), (ys * ys).sum(), (xs * ys).sum()
            row[6:10] = (xs.min(), ys.min(), xs.max(), ys.max())
            row[10:14] = quads(plane, label)[:4]
            if inten is not None:
                v = img[ys, xs].astype(np.int64)  # [area, c]
                inten[q, label, :, 0], inten[q, label, :, 1] = v.sum(0), (v * v).sum(0)
                inten[q, label, :, 2], inten[q, label, :, 3] = v.min(0), v.max(0)
    return geom, inten, skipped


def descriptors(plane, label):
    """The float descriptors of one label of one plane, from its pixels (None when it has none)."""
    plane = np.asarray(plane)
    ys, xs = np.nonzero(plane == label)
    if len(xs) == 0:
        return None
    a = float(len(xs))
    cx, cy = xs.astype(np.float64).mean(), ys.astype(np.float64).mean()
    dx, dy = xs - cx, ys - cy
    mu20, mu02, mu11 = float((dx * dx).mean()), float((dy * dy).mean()), float((dx * dy).mean())
    lam = np.linalg.eigvalsh(np.array([[mu20, mu11], [mu11, mu02]]))
    l1, l2 = float(lam[1]), max(float(lam[0]), 0.0)
    q1, q2, q3, qd, _ = quads(plane, label)
    per = q2 + (q1 + q3 + 2 * qd) / math.sqrt(2.0)
    h, w = plane.shape
    x0, y0, x1, y1 = int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())
    euler = (q1 - q3 - 2 * qd) / 4
    return {"area": a, "centroid_x": cx, "centroid_y": cy, "bbox": (x0, y0, x1, y1),
            "extent": a / ((x1 - x0 + 1) * (y1 - y0 + 1)), "equivalent_diameter": math.sqrt(4 * a / math.pi),
            "mu20": mu20, "mu02": mu02, "mu11": mu11, "l1": l1, "l2": l2,
            "major_axis": 4 * math.sqrt(max(l1, 0.0)), "minor_axis": 4 * math.sqrt(l2),
            "eccentricity": math.sqrt(max(1 - l2 / l1, 0.0)) if l1 > 0 else 0.0,
            "orientation": 0.5 * math.atan2(2 * mu11, mu20 - mu02),
            "perimeter_crack": float(q1 + q2 + q3 + 2 * qd), "perimeter": per,
            "circularity": 4 * math.pi * a / per ** 2, "euler_number": euler, "euler_number_4": (q1 - q3 + 2 * qd) / 4,
            "holes": 1 - euler,
            "touches_border": float(x0 == 0 or y0 == 0 or x1 == w - 1 or y1 == h - 1)}


# ---- inputs -------------------------------------------------------------------------------------------------
def blobs(h, w, n, seed):
    """Up to n filled discs of ids 1..n on background, later ones over earlier ones: touching, cut and nested cells."""
    rng = np.random.default_rng(seed)
    out = np.zeros((h, w), np.int64)
    yy, xx = np.mgrid[:h, :w]
    for label in range(1, n + 1):
        cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.integers(1, max(2, min(h, w) // 3 + 2))
        out[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = label
    return out


def noise(h, w, n, seed):
    return np.random.default_rng(seed).integers(0, n + 1, (h, w)).astype(np.int64)


def rectangles(h, w):
    """Ids 1..3: a block in the corner, a full row (every chunk of it one whole run) and a full column."""
    out = np.zeros((h, w), np.int64)
    out[: max(1, h // 3), : max(1, w // 2)] = 1
    out[h // 2, :] = 2
    out[:, w - 1] = 3
    return out


def image(h, w, c, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c)).astype(np.uint8)
