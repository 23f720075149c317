"""Plain numpy restatement of the score histogram (include/eunet.h, eunet_score_hist) and of the curve
statistics built on it (eunet.metrics.curve_metrics_from_hist).  The histogram follows the stated rules pixel by
pixel; the curve statistics are restated from per-pixel (bin index, label) arrays by sorting, as sklearn forms
them, not from histograms."""
import numpy as np


def pixel_bins(p, edges):
    """p float32 [m] (all valid) -> bin index: edges[i] <= p < edges[i+1] in fp32, the last bin closed."""
    edges = np.asarray(edges, dtype=np.float32)
    b = np.searchsorted(edges, np.asarray(p, dtype=np.float32), "right") - 1
    return np.clip(b, 0, len(edges) - 2)


def pixel_conf(p):
    """The fixed-point confidence of one pixel: rint(min(p, 1) 2^24), exact in fp32, ties to even."""
    p = np.minimum(np.asarray(p, dtype=np.float32), np.float32(1))
    return np.rint(p * np.float32(2 ** 24)).astype(np.int64)


def pixels(probs, mask, c, ignore_index=255):
    """The pixels of class c that count: (p float32, positive bool, number of invalid ones)."""
    probs = np.asarray(probs, dtype=np.float32)
    mask = np.asarray(mask, dtype=np.int64)
    if probs.ndim == 3:
        probs, mask = probs[None], mask[None]
    k = probs.shape[1]
    p = probs[:, c].reshape(-1)
    m = mask.reshape(-1)
    live = m != ignore_index
    with np.errstate(invalid="ignore"):
        bad = ~(p >= 0) | np.isinf(p)
    ok = live & ~bad
    pos = (m >= 1) if k == 1 else (m == c)
    return p[ok], pos[ok], int((live & bad).sum())


def score_hist_ref(probs, mask, edges, ignore_index=255):
    """probs [K,h,w] or [N,K,h,w], mask [h,w] or [N,h,w] -> (hist int64 [K,B,3], invalid int)."""
    probs = np.asarray(probs, dtype=np.float32)
    k = probs.shape[-3]
    bins = len(edges) - 1
    hist = np.zeros((k, bins, 3), np.int64)
    invalid = 0
    for c in range(k):
        p, pos, bad = pixels(probs, mask, c, ignore_index)
        invalid += bad
        b = pixel_bins(p, edges)
        np.add.at(hist[c, :, 0], b[~pos], 1)
        np.add.at(hist[c, :, 1], b[pos], 1)
        np.add.at(hist[c, :, 2], b, pixel_conf(p))
    return hist, invalid


def exact_auc(score, y):
    """The AUC of raw scores by ranks (Mann-Whitney, ties count 1/2): nan without both classes."""
    score = np.asarray(score, dtype=np.float64)
    y = np.asarray(y, dtype=bool)
    n_pos, n_neg = int(y.sum()), int((~y).sum())
    if n_pos == 0 or n_neg == 0:
        return float("nan")
    _, inv, cnt = np.unique(score, return_inverse=True, return_counts=True)
    first = np.cumsum(cnt) - cnt  # 0-based rank of the first of each tie group
    rank = (first + (cnt + 1) / 2.0)[inv]  # 1-based average rank
    return float((rank[y].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg))


def clf_curve(score, y):
    """sklearn's _binary_clf_curve: (fps, tps, distinct scores), scores decreasing."""
    score = np.asarray(score)
    y = np.asarray(y, dtype=bool)
    order = np.argsort(-score, kind="mergesort")
    s, t = score[order], y[order]
    idx = np.r_[np.nonzero(np.diff(s))[0], len(s) - 1] if len(s) else np.zeros(0, np.int64)
    tps = np.cumsum(t)[idx].astype(np.float64)
    fps = 1 + idx - tps
    return fps, tps, s[idx]


def curve_stats_ref(p, pos, edges, n_cal=10, n_conf=50):
    """The statistics of curve_metrics_from_hist for one class from its per-pixel scores and labels."""
    p = np.asarray(p, dtype=np.float32)
    pos = np.asarray(pos, dtype=bool)
    edges = np.asarray(edges, dtype=np.float32)
    b = pixel_bins(p, edges)
    n_pos, n_neg = int(pos.sum()), int((~pos).sum())
    fps, tps, thr = clf_curve(b, pos)
    nan = float("nan")
    with np.errstate(divide="ignore", invalid="ignore"):
        tpr = np.r_[0.0, tps] / n_pos if n_pos else np.full(len(tps) + 1, nan)
        fpr = np.r_[0.0, fps] / n_neg if n_neg else np.full(len(fps) + 1, nan)
        prec = tps / (tps + fps)
        rec = tps / n_pos if n_pos else np.full(len(tps), nan)
    precision, recall = np.r_[prec[::-1], 1.0], np.r_[rec[::-1], 0.0]
    out = {"fpr": fpr, "tpr": tpr, "thresholds": np.r_[np.inf, edges[thr.astype(np.int64)].astype(np.float64)],
           "precision": precision, "recall": recall, "n_pos": n_pos, "n_neg": n_neg}
    if n_pos and n_neg:
        out["auc"] = float(np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2))
        out["ap"] = float(-np.sum(np.diff(recall) * precision[:-1]))
        tied = sum(float((b[pos] == v).sum()) * float((b[~pos] == v).sum()) for v in np.unique(b))
        out["auc_resolution"] = tied / (2.0 * n_pos * n_neg)
    else:
        out["auc"] = out["ap"] = out["auc_resolution"] = nan
    # the reliability curve of the reference (float64 np.linspace edges against the float32 scores), the last
    # bin closed and the confidence in the histogram's fixed point
    e = np.linspace(0, 1, n_cal + 1)
    conf = pixel_conf(p)
    acc_l, conf_l, cnt_l = [], [], []
    p64 = p.astype(np.float64)
    for i in range(n_cal):
        sel = (p64 >= e[i]) & ((p64 < e[i + 1]) if i < n_cal - 1 else True)
        n = int(sel.sum())
        cnt_l.append(n)
        acc_l.append(float(pos[sel].sum()) / n if n else 0.0)
        conf_l.append(float(conf[sel].sum()) / 2.0 ** 24 / n if n else (e[i] + e[i + 1]) / 2)
    out["cal_acc"], out["cal_conf"], out["cal_count"] = np.array(acc_l), np.array(conf_l), np.array(cnt_l, np.int64)
    total = len(p)
    out["ece"] = float(sum(n / total * abs(a - cf) for n, a, cf in zip(cnt_l, acc_l, conf_l))) if total else nan
    e = np.linspace(0, 1, n_conf + 1)
    out["conf_hist"] = np.array([int(((p64 >= e[i]) & ((p64 < e[i + 1]) if i < n_conf - 1 else True)).sum())
                                 for i in range(n_conf)], np.int64)
    return out
