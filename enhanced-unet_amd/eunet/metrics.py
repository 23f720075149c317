"""Drop-in metrics of reference metrics.py (metrics.py:12-194, 304-340).

    calculate_iou(mask1, mask2) -> float             # metrics.py:12-18
    calculate_dice(mask1, mask2) -> float            # metrics.py:21-26
    calculate_semantic_metrics(pred, gt) -> dict     # metrics.py:29-58 (0 bg, 1 live, 2 dead)
    calculate_instance_metrics(pred_masks, pred_labels, pred_scores,
                               gt_masks, gt_labels, iou_threshold=0.05) -> dict   # metrics.py:61-194
    calculate_viability_metrics(pred_live, pred_dead, gt_live, gt_dead) -> dict   # metrics.py:304-340

The pixel counting runs on the GPU (eunet_semantic_counts; eunet_pack_masks +
eunet_pairwise_overlap for the instance pairs -- integer, exact); inputs may be
numpy arrays (copied to the device) or device tensors.  The ratios are formed
on the host exactly as the reference forms them (int / int in float64), and so
is the greedy matching (match_from_counts, a pure function of the count
matrices).  No CPU counting path exists.

calculate_coco_metrics (metrics.py:197-301: bbox_mAP / segm_mAP) needs
pycocotools and is not built.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops

CLASS_NAMES = ("background", "live", "dead")


def _dev_long(m, device=None):
    if isinstance(m, torch.Tensor):
        t = m
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(m)))
    if not t.is_cuda:
        t = t.to(device or "cuda")
    return t.long()


def _iou(inter: int, a: int, b: int) -> float:
    union = a + b - inter
    if union == 0:
        return 1.0 if inter == 0 else 0.0
    return inter / union


def _dice(inter: int, a: int, b: int) -> float:
    if a + b == 0:
        return 1.0
    return 2 * inter / (a + b)


def _overlap(mask1, mask2):
    m1 = _dev_long(mask1)
    m2 = _dev_long(mask2, m1.device)
    if m1.shape != m2.shape:
        raise ValueError(f"mask shapes differ: {tuple(m1.shape)} vs {tuple(m2.shape)}")
    return ops.binary_overlap(m1, m2)


def calculate_iou(mask1, mask2) -> float:
    inter, union, _, _ = _overlap(mask1, mask2)
    if union == 0:
        return 1.0 if inter == 0 else 0.0
    return inter / union


def calculate_dice(mask1, mask2) -> float:
    """2 |a & b| / (sum a + sum b): the reference sums mask VALUES (metrics.py:24-26)."""
    inter, _, sa, sb = _overlap(mask1, mask2)
    return _dice(inter, sa, sb)


def semantic_counts(pred_mask, gt_mask) -> np.ndarray:
    """[3][3] int64 counts (#pred==c, #gt==c, #both==c) of one mask pair (or [n][3][3] for a batch)."""
    p = _dev_long(pred_mask)
    g = _dev_long(gt_mask, p.device)
    if p.shape != g.shape:
        raise ValueError(f"mask shapes differ: {tuple(p.shape)} vs {tuple(g.shape)}")
    if p.dim() <= 2:
        return ops.semantic_counts(p.reshape(1, -1), g.reshape(1, -1))[0].cpu().numpy()
    return ops.semantic_counts(p.reshape(p.shape[0], -1), g.reshape(g.shape[0], -1)).cpu().numpy()


def metrics_from_counts(counts) -> Dict[str, float]:
    m: Dict[str, float] = {}
    for cid, name in enumerate(CLASS_NAMES):
        a, b, inter = (int(v) for v in counts[cid])
        m[f"sem_{name}_iou"] = _iou(inter, a, b)
        m[f"sem_{name}_dice"] = _dice(inter, a, b)
    mean_iou = (m["sem_background_iou"] + m["sem_live_iou"] + m["sem_dead_iou"]) / 3
    m["sem_mean_iou"] = (m["sem_live_iou"] + m["sem_dead_iou"]) / 2
    m["sem_mean_iou_all"] = mean_iou
    m["sem_mean_dice"] = (m["sem_live_dice"] + m["sem_dead_dice"]) / 2
    return m


def calculate_semantic_metrics(pred_mask, gt_mask) -> Dict[str, float]:
    return metrics_from_counts(semantic_counts(pred_mask, gt_mask))


# ---- instance metrics (metrics.py:61-194) -----------------------------------------------------------
def match_from_counts(inter, area_p, area_g, scores, thr: float = 0.05) -> Dict[str, float]:
    """The reference's greedy matching of one class (metrics.py:88-141 / 144-192) from integer counts.

    inter [P, G] = |pred_p & gt_g|, area_p [P], area_g [G] (G > 0), scores [P].  Predictions are visited
    in a stable sort by descending score; each takes the first still unmatched ground truth with strictly
    greater IoU and matches when best_iou >= thr.  IoU = inter / (area_p + area_g - inter) as int / int
    in float64, 1.0 when the union is empty (metrics.py:12-18).  Returns the unprefixed keys iou,
    precision, recall, ap and -- under the reference's condition -- avg_iou_below_threshold."""
    inter = np.asarray(inter, dtype=np.int64).reshape(len(area_p), len(area_g))
    area_p = [int(v) for v in area_p]
    area_g = [int(v) for v in area_g]
    n_pred, n_gt = len(area_p), len(area_g)
    if n_gt == 0:
        raise ValueError("match_from_counts: the reference skips a class without ground truth")
    order = sorted(range(n_pred), key=lambda i: scores[i], reverse=True)
    matched_ious: List[float] = []
    all_pred_ious: List[float] = []
    matched_gt = set()
    for p in order:
        best_iou, best_gt = 0.0, -1
        for g in range(n_gt):
            if g in matched_gt:
                continue
            it = int(inter[p, g])
            union = area_p[p] + area_g[g] - it
            iou = 1.0 if union == 0 else it / union
            if iou > best_iou:
                best_iou, best_gt = iou, g
        all_pred_ious.append(best_iou)
        if best_iou >= thr and best_gt >= 0:
            matched_ious.append(best_iou)
            matched_gt.add(best_gt)
    m: Dict[str, float] = {}
    if matched_ious:
        m["iou"] = np.mean(matched_ious)
    elif all_pred_ious:
        m["iou"] = np.mean(all_pred_ious)
    else:
        m["iou"] = 0.0
    m["precision"] = len(matched_ious) / n_pred if n_pred else 0.0
    m["recall"] = len(matched_ious) / n_gt
    if m["precision"] == 0.0 and m["iou"] > 0.0 and n_pred:
        avg = np.mean(all_pred_ious) if all_pred_ious else 0.0
        if not avg < 0.1:
            m["avg_iou_below_threshold"] = avg
    m["ap"] = m["precision"] * m["recall"] if n_pred else 0.0
    return m


INSTANCE_CLASSES = ("live", "dead")  # instance label 0, 1


def instance_metrics_from_counts(per_class: Sequence[Optional[Tuple]], thr: float = 0.05) -> Dict[str, float]:
    """The dict of calculate_instance_metrics from per-class counts: per_class[c] = (inter, area_p, area_g,
    scores) or None for a class without ground truth (which keeps the reference's zeros)."""
    metrics: Dict[str, float] = {}
    for name in INSTANCE_CLASSES:
        for k in ("iou", "precision", "recall", "ap"):
            metrics[f"{name}_{k}"] = 0.0
    for name, counts in zip(INSTANCE_CLASSES, per_class):
        if counts is None:
            continue
        for k, v in match_from_counts(*counts, thr=thr).items():
            metrics[f"{name}_{k}"] = v
    return metrics


def _stack_masks(masks, device=None) -> torch.Tensor:
    """A list of [h, w] masks (numpy arrays or tensors) -> one uint8 [n, h, w] device tensor, non-zero = set."""
    if all(isinstance(m, torch.Tensor) for m in masks):
        t = torch.stack([m if m.is_cuda else m.to(device or "cuda") for m in masks])
    else:
        t = torch.from_numpy(np.stack([m.cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m)
                                       for m in masks])).to(device or "cuda")
    if t.dtype == torch.bool:
        return t.view(torch.uint8)
    return t if t.dtype == torch.uint8 else (t != 0).view(torch.uint8)


def instance_counts(pred_masks, gt_masks, device=None):
    """(inter [P, G], area_p [P], area_g [G]) as numpy int64: one bit-pack per side and one pairwise
    popcount "GEMM" on the device (eunet_pack_masks, eunet_pairwise_overlap)."""
    pg, ag = ops.pack_masks(_stack_masks(gt_masks, device))
    pp, ap = ops.pack_masks(_stack_masks(pred_masks, pg.device))
    inter = ops.pairwise_overlap(pp, pg)
    return inter.cpu().numpy(), ap.cpu().numpy(), ag.cpu().numpy()


def calculate_instance_metrics(pred_masks, pred_labels, pred_scores, gt_masks, gt_labels,
                               iou_threshold: float = 0.05) -> Dict[str, float]:
    """metrics.py:61-194.  Masks are [h, w] numpy arrays or device tensors (non-zero = set); labels 0 live,
    1 dead.  One pack + overlap call per class that has ground truth; a class without ground truth is
    skipped (its keys stay 0.0)."""
    device = next((m.device for m in list(pred_masks) + list(gt_masks)
                   if isinstance(m, torch.Tensor) and m.is_cuda), None)
    per_class = []
    for cid in range(len(INSTANCE_CLASSES)):
        pm = [(m, s) for m, l, s in zip(pred_masks, pred_labels, pred_scores) if l == cid]
        gm = [m for m, l in zip(gt_masks, gt_labels) if l == cid]
        if not gm:
            per_class.append(None)
            continue
        scores = [s for _, s in pm]
        if pm:
            inter, ap, ag = instance_counts([m for m, _ in pm], gm, device)
        else:
            inter, ap, ag = np.zeros((0, len(gm)), np.int64), np.zeros(0, np.int64), np.zeros(len(gm), np.int64)
        per_class.append((inter, ap, ag, scores))
    return instance_metrics_from_counts(per_class, iou_threshold)


# ---- viability (metrics.py:304-340) -----------------------------------------------------------------
def calculate_viability_metrics(pred_live_count: int, pred_dead_count: int, gt_live_count: int,
                                gt_dead_count: int) -> Dict[str, float]:
    pred_total = pred_live_count + pred_dead_count
    gt_total = gt_live_count + gt_dead_count
    pred_viability = pred_live_count / pred_total if pred_total > 0 else 0.0
    gt_viability = gt_live_count / gt_total if gt_total > 0 else 0.0
    if gt_total > 0:
        viability_accuracy = 1.0 - min(abs(pred_viability - gt_viability), 1.0)
    else:
        viability_accuracy = 1.0 if pred_total == 0 else 0.0
    return {"pred_viability": pred_viability, "gt_viability": gt_viability,
            "viability_accuracy": viability_accuracy, "pred_live_count": pred_live_count,
            "pred_dead_count": pred_dead_count, "gt_live_count": gt_live_count, "gt_dead_count": gt_dead_count}
