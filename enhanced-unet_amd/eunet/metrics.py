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

    calculate_coco_metrics(pred_annotations, gt_annotations)
        -> {'bbox_mAP', 'segm_mAP'}                  # metrics.py:197-301 (COCOeval stats[0])

calculate_coco_metrics is built natively, without pycocotools: COCOeval is a
fixed, published algorithm over IoU matrices.  Masks, boxes, IoUs and the
greedy matching of COCOeval.evaluateImg stay on the device
(eunet_pack_masks_bbox, eunet_pairwise_overlap, eunet_coco_match); only the
match tables come back, and coco_map_from_matches restates
COCOeval.accumulate + summarize for stats[0] (AP@[.50:.95], all areas, 100
detections) in numpy.  'segmentation' is a [h, w] mask where the reference
carries an RLE, and the box always comes from the mask.  The other COCO stats,
iscrowd and RLE decoding are not built.

    curve_edges(uniform=1000, per_octave=8, octaves=24) -> float32 [B + 1]
    curve_metrics_from_hist(hist, edges, class_names=None, n_cal=10, n_conf=50) -> {class: {...}}

The pixel-level ROC / PR / calibration statistics that visualization.py:1096-1199,
1819-1900 plot, from the integer score histogram of ops.score_hist (curves.hip):
numpy only, no sklearn.

    calculate_boundary_stats(pred, gt, num_classes=3, ignore_index=255, cap=64, band_radii=(2,), out=None)
    boundary_metrics_from_stats(stats, tolerances=(1, 2, 3), class_names=None) -> {class: {...}, ...}

The contour metrics (Hausdorff distance, HD95, average symmetric surface distance, surface Dice, boundary F1,
Boundary IoU) and the two lists of visualization.py:1687-1751 (plot_boundary_accuracy), from the integer
statistics of ops.boundary_stats (boundary.hip), which rest on an exact distance transform on the device.

    instance_stats_from_pairs(pairs, num_planes, iou_percent=(50, 55, ..., 95)) -> {name: array indexed by plane}
    panoptic_metrics_from_stats(stats, class_names=("live", "dead"), iou_percent=...) -> {key: float}
    calculate_panoptic_metrics(pred_ids, gt_ids, class_names=("live", "dead"), iou_percent=...) -> {key: float}
    size_strata_from_pairs(pairs, edges=(100, 500, 1000, 5000)) -> [coverages per size bin]

Instance metrics of two integer id maps (no reference counterpart; the size strata are
visualization.py:1753-1817): Panoptic Quality (Kirillov et al. 2019), the Aggregated Jaccard Index (Kumar et al.
2017), the object-level Dice of the GlaS contest (Sirinukunwattana et al. 2017), the SEG score of the Cell Tracking
Challenge and the F1 / average-precision sweep over IoU 0.5 .. 0.95 (the 2018 Data Science Bowl's score), all from
the sparse contingency table of ops.label_pairs (pairs.hip).  Every decision is taken in integers.

    cell_measurements(stats, plane=0, pixel_size=1.0) -> {descriptor: float64 [n]}
    population_summary(measurements, keys=...) -> {key: float}
    measurement_agreement(pairs, geom_pred, geom_gt, plane) -> {...};  agreement_summary(parts) -> {key: float}

Per-cell measurements (no reference counterpart): area, centroid, bounding box, second moments, axes, eccentricity,
orientation, perimeters, circularity, Euler number, holes and per-channel intensity of every label, from the integer
tables of ops.cell_stats (cellprops.hip), and how the measurements of matched predicted and ground-truth cells agree.
"""
from __future__ import annotations

import warnings
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


# ---- COCO mAP (metrics.py:197-301: COCOeval stats[0], AP@[.50:.95], all areas, 100 detections) ------
COCO_CLASSES = (0, 1)  # the categories of metrics.py:233-236 (0 live, 1 dead)
COCO_MAX_DETS = 100
# formed as pycocotools forms them (cocoeval.py, Params.setDetParams)
COCO_IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
COCO_REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)


def coco_map_from_matches(images) -> float:
    """COCOeval.accumulate + summarize for stats[0], from the per-image match tables (pure numpy).

    images: per image, in evaluation order, one entry per class of COCO_CLASSES: (scores [d] of the visited
    detections in visiting order, matches [T][d] holding the GLOBAL id of the ground truth each detection
    took or -1, number of ground truths).  A detection is a true positive when its match id is truthy:
    pycocotools tests dtm for truth and the reference numbers ground truths from 0 (metrics.py:240-242), so
    a detection matched to ground truth 0 counts as a false positive (that ground truth is still consumed).
    Returns the mean of the precision entries > -1 over [T][recall point][class], or -1 without any."""
    n_t, n_r = len(COCO_IOU_THRS), len(COCO_REC_THRS)
    n_cls = len(COCO_CLASSES)
    precision = -np.ones((n_t, n_r, n_cls))
    for k in range(n_cls):
        ev = [img[k] for img in images if len(img[k][0]) or img[k][2]]
        if not ev:
            continue
        scores = np.concatenate([np.asarray(e[0], dtype=np.float64).reshape(-1)[:COCO_MAX_DETS] for e in ev])
        inds = np.argsort(-scores, kind="mergesort")
        dtm = np.concatenate([np.asarray(e[1], dtype=np.int64).reshape(n_t, -1)[:, :COCO_MAX_DETS] for e in ev],
                             axis=1)[:, inds]
        npig = sum(int(e[2]) for e in ev)
        if npig == 0:
            continue
        tps = dtm > 0  # -1: unmatched; 0: matched to the ground truth of global id 0, falsy in pycocotools
        tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
        fp_sum = np.cumsum(~tps, axis=1).astype(dtype=float)
        for t in range(n_t):
            tp, fp = tp_sum[t], fp_sum[t]
            nd = len(tp)
            rc = tp / npig
            pr = tp / (fp + tp + np.spacing(1))
            if nd:
                pr = np.maximum.accumulate(pr[::-1])[::-1]  # the right-to-left precision envelope
            at = np.searchsorted(rc, COCO_REC_THRS, side="left")
            q = np.zeros(n_r)
            ok = at < nd  # recall points past the end keep 0 (pycocotools' try / except)
            q[ok] = pr[at[ok]]
            precision[t, :, k] = q
    s = precision[precision > -1]
    return float(np.mean(s)) if len(s) else -1.0


def _visit_order(labels, scores):
    """Per class, the detections in a stable sort by descending score, cut at COCO_MAX_DETS
    (COCOeval.computeIoU / evaluateImg); the classes one after the other."""
    scores = np.asarray(scores, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    order = []
    for c in COCO_CLASSES:
        idx = np.nonzero(labels == c)[0]
        order.append(idx[np.argsort(-scores[idx], kind="mergesort")][:COCO_MAX_DETS])
    return np.concatenate(order)


def _xywh(bbox):
    """(xmin, ymin, xmax, ymax) inclusive -> cv2.boundingRect's (x, y, w, h), on the device."""
    out = bbox.clone()
    out[:, 2:] = bbox[:, 2:] - bbox[:, :2] + 1
    return out


def coco_image_matches(pred_masks, pred_labels, pred_scores, gt_masks, gt_labels, gt_ids, device=None):
    """One image's entries for coco_map_from_matches: (bbox entry, segm entry), each a tuple over
    COCO_CLASSES of (scores, matches [T][d] of global ground-truth ids, number of ground truths).

    With detections and ground truth present: one pack_masks_bbox per side, one pairwise_overlap over the
    visited detections and one coco_match on the device; only the match table (and the areas, to refuse an
    empty mask) comes back.  Without either side there is no launch."""
    pred_labels = [int(l) for l in pred_labels]
    gt_labels = [int(l) for l in gt_labels]
    for l in pred_labels + gt_labels:
        if l not in COCO_CLASSES:
            raise ValueError(f"category_id must be one of {COCO_CLASSES}, got {l}")
    n_t = len(COCO_IOU_THRS)
    gt_ids = np.asarray(gt_ids, dtype=np.int64).reshape(-1)
    n_gt = [sum(1 for l in gt_labels if l == c) for c in COCO_CLASSES]
    scores = np.asarray([float(s) for s in pred_scores], dtype=np.float64)
    if len(pred_labels) == 0:
        entry = tuple((np.zeros(0), np.full((n_t, 0), -1, np.int64), n) for n in n_gt)
        return entry, entry
    vis = _visit_order(pred_labels, scores)
    vis_cls = np.asarray(pred_labels, dtype=np.int64)[vis]
    if len(gt_labels) == 0:
        entry = tuple((scores[vis[vis_cls == c]], np.full((n_t, int((vis_cls == c).sum())), -1, np.int64), 0)
                      for c in COCO_CLASSES)
        return entry, entry
    pg, ag, bg = ops.pack_masks_bbox(_stack_masks(gt_masks, device))
    dev = pg.device
    pp, ap, bp = ops.pack_masks_bbox(_stack_masks([pred_masks[i] for i in vis], dev))
    inter = ops.pairwise_overlap(pp, pg)
    match = ops.coco_match(inter, ap, ag, _xywh(bp), _xywh(bg), ops.upload(vis_cls.astype(np.int32), dev),
                           ops.upload(np.asarray(gt_labels, dtype=np.int32), dev), COCO_IOU_THRS)
    match = match.cpu().numpy()
    if int(ap.min().item()) == 0 or int(ag.min().item()) == 0:
        raise ValueError("calculate_coco_metrics: an empty mask has no bounding box (the reference divides 0 by 0)")
    ids = np.where(match >= 0, gt_ids[np.clip(match, 0, None)], -1)  # local index -> global ground-truth id
    out = []
    for ty in range(2):
        out.append(tuple((scores[vis[vis_cls == c]], ids[ty][:, vis_cls == c], n_gt[c]) for c in COCO_CLASSES))
    return out[0], out[1]


def calculate_coco_metrics(pred_annotations: List[Dict], gt_annotations: List[Dict]) -> Dict[str, float]:
    """metrics.py:197-301: {'bbox_mAP', 'segm_mAP'} = COCOeval stats[0] of both IoU types.

    Annotations are the reference's dicts (image_id, category_id, score for predictions) with 'segmentation'
    a [h, w] mask (numpy array or device tensor, non-zero = set) where the reference carries a pycocotools
    RLE.  A supplied 'bbox' is not read: the box is always cv2.boundingRect of the mask, as the reference's
    caller forms it (train_eval.py:959, 978).  Ground-truth ids are the positions in gt_annotations; the
    images are the sorted unique ground-truth image_ids.  Either list empty: both 0.0.  A prediction on an
    image without ground truth: both 0.0 with a warning (COCO.loadRes asserts and the reference's except
    returns the zeros).  An empty mask raises ValueError."""
    metrics = {"bbox_mAP": 0.0, "segm_mAP": 0.0}
    if not pred_annotations or not gt_annotations:
        return metrics
    image_ids = sorted({a["image_id"] for a in gt_annotations if "image_id" in a}) or [1]
    default_id = image_ids[0]
    known = set(image_ids)
    gts = {i: [] for i in image_ids}
    for pos, a in enumerate(gt_annotations):
        gts[a.get("image_id", default_id)].append((pos, a))
    preds = {i: [] for i in image_ids}
    for a in pred_annotations:
        iid = a.get("image_id", default_id)
        if iid not in known:
            warnings.warn(f"calculate_coco_metrics: a prediction on image {iid!r}, which has no ground truth; "
                          "the reference's COCO.loadRes refuses such results, so both values are 0.0")
            return metrics
        preds[iid].append(a)
    masks = [a["segmentation"] for a in list(pred_annotations) + list(gt_annotations)]
    device = next((m.device for m in masks if isinstance(m, torch.Tensor) and m.is_cuda), None)
    bbox_images, segm_images = [], []
    for iid in image_ids:
        p, g = preds[iid], [a for _, a in gts[iid]]
        eb, es = coco_image_matches([a["segmentation"] for a in p], [a.get("category_id", 0) for a in p],
                                    [a.get("score", 0.0) for a in p], [a["segmentation"] for a in g],
                                    [a["category_id"] for a in g], [pos for pos, _ in gts[iid]], device)
        bbox_images.append(eb)
        segm_images.append(es)
    metrics["bbox_mAP"] = coco_map_from_matches(bbox_images)
    metrics["segm_mAP"] = coco_map_from_matches(segm_images)
    return metrics


# ---- pixel-level ROC / PR / calibration from score histograms (visualization.py:1096-1199, 1819-1900) ----
CONF_SCALE = float(2 ** 24)  # the fixed point of the histogram's confidence sums (eunet_score_hist)


def ceil32(x) -> np.ndarray:
    """The smallest float32 >= the float64 x, elementwise.  p >= ceil32(e) in fp32 is the predicate p >= e of a
    float32 p against the float64 e, so a table of ceil32 values bins as the reference's float64 edges do."""
    x = np.asarray(x, dtype=np.float64)
    f = x.astype(np.float32)
    low = f.astype(np.float64) < x
    return np.where(low, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


def curve_edges(uniform: int = 1000, per_octave: int = 8, octaves: int = 24) -> np.ndarray:
    """The score bins of the curve statistics: float32 [B + 1], strictly increasing from 0 to 1.

    The sorted unique values of ceil32(i / uniform), i = 0..uniform, and of ceil32(2^(-j / per_octave)) and
    ceil32(1 - 2^(-j / per_octave)) for j = 1..per_octave * octaves with 2^(-j / per_octave) < 1 / uniform:
    a uniform grid with log-spaced tails towards 0 and 1, where a saturated softmax puts most pixels (on a
    synthetic saturated sigmoid a plain 1000-bin grid gave AUC 0.8225 against the exact 0.8548; with the
    tails 0.8543).  The defaults give B = 1208 and contain ceil32 of every np.linspace(0, 1, 11) and
    np.linspace(0, 1, 51) edge, which curve_metrics_from_hist's calibration bins need."""
    if uniform < 1 or per_octave < 1 or octaves < 0:
        raise ValueError("curve_edges: uniform >= 1, per_octave >= 1, octaves >= 0")
    vals = [np.arange(uniform + 1, dtype=np.float64) / uniform]
    t = 2.0 ** (-np.arange(1, per_octave * octaves + 1, dtype=np.float64) / per_octave)
    t = t[t < 1.0 / uniform]
    vals += [t, 1.0 - t]
    e = np.unique(ceil32(np.concatenate(vals)))
    if e[0] != 0.0 or e[-1] != 1.0:
        raise ValueError("curve_edges: the table does not run from 0 to 1")
    return e


def _coarse_index(edges: np.ndarray, n: int, what: str) -> np.ndarray:
    """Positions in edges of ceil32(np.linspace(0, 1, n + 1)): the coarse bins as unions of fine ones."""
    ce = ceil32(np.linspace(0, 1, n + 1))
    idx = np.searchsorted(edges, ce)
    if np.any(idx >= len(edges)) or np.any(edges[np.minimum(idx, len(edges) - 1)] != ce):
        raise ValueError(f"curve_metrics_from_hist: the {what} = {n} edges np.linspace(0, 1, {n + 1}) are not all "
                         f"in the histogram's edge table (curve_edges' uniform must be a multiple of {n})")
    return idx


def curve_metrics_from_hist(hist, edges, class_names: Optional[Sequence[str]] = None, n_cal: int = 10,
                            n_conf: int = 50) -> Dict[str, Dict]:
    """ROC, PR and calibration statistics per class from an ops.score_hist histogram (pure numpy).

    hist int64 [K, B, 3] (#negatives, #positives, confidence sum per class and bin), edges float32 [B + 1].
    Returns {class name: {...}} (default names: CLASS_NAMES[:K], or "foreground" for K = 1) with
      fpr, tpr, thresholds   sklearn's roc_curve(bin index, drop_intermediate=False): one point per occupied
                             bin from the top, after (0, 0); thresholds are the bins' lower edges (inf first):
                             the point is the classifier "p >= threshold"
      auc                    the trapezoid under (fpr, tpr)
      precision, recall      sklearn's precision_recall_curve(bin index): increasing threshold, then (1, 0)
      ap                     sum (R_n - R_{n-1}) P_n (sklearn's average_precision_score)
      auc_resolution         sum_b pos_b neg_b / (2 P N): a hard bound on |auc - AUC of the unbinned scores|
                             (only a positive and a negative tied inside one bin can differ, by at most 1/2)
      cal_acc, cal_conf, cal_count   the n_cal-bin reliability curve of visualization.py:1847-1864: fraction
                             of positives, mean confidence, pixels; an empty bin has accuracy 0 and the bin
                             centre as confidence.  Unlike the reference, the last bin holds p == 1 and
                             ignored pixels are left out (include/eunet.h)
      ece                    sum count / total |cal_acc - cal_conf| (nan without pixels)
      conf_hist              pixels per n_conf uniform bin of [0, 1]
      n_pos, n_neg
    A class without positives or without negatives has nan for auc, ap and auc_resolution."""
    if isinstance(hist, torch.Tensor):
        hist = hist.cpu().numpy()
    hist = np.asarray(hist)
    if isinstance(edges, torch.Tensor):
        edges = edges.cpu().numpy()
    edges = np.asarray(edges, dtype=np.float32)
    if hist.ndim != 3 or hist.shape[2] != 3 or hist.shape[1] != len(edges) - 1:
        raise ValueError(f"curve_metrics_from_hist: hist must be [K, {len(edges) - 1}, 3], got {hist.shape}")
    k = hist.shape[0]
    if class_names is None:
        class_names = ("foreground",) if k == 1 else CLASS_NAMES[:k]
    if len(class_names) != k:
        raise ValueError(f"curve_metrics_from_hist: {len(class_names)} class names for {k} classes")
    cal_idx = _coarse_index(edges, n_cal, "n_cal")
    conf_idx = _coarse_index(edges, n_conf, "n_conf")
    cal_edges = np.linspace(0, 1, n_cal + 1)
    centres = (cal_edges[:-1] + cal_edges[1:]) / 2
    lower = edges[:-1].astype(np.float64)
    out: Dict[str, Dict] = {}
    for c, name in enumerate(class_names):
        neg = hist[c, :, 0].astype(np.float64)
        pos = hist[c, :, 1].astype(np.float64)
        conf = hist[c, :, 2].astype(np.float64) / CONF_SCALE
        n_pos, n_neg = int(hist[c, :, 1].sum()), int(hist[c, :, 0].sum())
        occ = np.nonzero((neg + pos)[::-1] > 0)[0]  # occupied bins from the top
        occ = len(neg) - 1 - occ
        tps, fps = np.cumsum(pos[occ]), np.cumsum(neg[occ])
        with np.errstate(divide="ignore", invalid="ignore"):
            tpr = np.concatenate([[0.0], tps]) / n_pos if n_pos else np.full(len(occ) + 1, np.nan)
            fpr = np.concatenate([[0.0], fps]) / n_neg if n_neg else np.full(len(occ) + 1, np.nan)
            prec = tps / (tps + fps)
            rec = tps / n_pos if n_pos else np.full(len(occ), np.nan)
        precision = np.concatenate([prec[::-1], [1.0]])
        recall = np.concatenate([rec[::-1], [0.0]])
        if n_pos and n_neg:
            auc = float(np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2))
            ap = float(-np.sum(np.diff(recall) * precision[:-1]))
            res = float(np.sum(pos * neg) / (2.0 * n_pos * n_neg))
        else:
            auc = ap = res = float("nan")
        count = np.add.reduceat(np.concatenate([neg + pos, [0.0]]), cal_idx[:-1])
        cpos = np.add.reduceat(np.concatenate([pos, [0.0]]), cal_idx[:-1])
        cconf = np.add.reduceat(np.concatenate([conf, [0.0]]), cal_idx[:-1])
        full = count > 0
        safe = np.where(full, count, 1.0)
        cal_acc = np.where(full, cpos / safe, 0.0)
        cal_conf = np.where(full, cconf / safe, centres)
        total = count.sum()
        ece = float(np.sum(count / total * np.abs(cal_acc - cal_conf))) if total else float("nan")
        conf_hist = np.add.reduceat(np.concatenate([hist[c, :, 0] + hist[c, :, 1], [0]]), conf_idx[:-1])
        out[name] = {"fpr": fpr, "tpr": tpr, "thresholds": np.concatenate([[np.inf], lower[occ]]), "auc": auc,
                     "precision": precision, "recall": recall, "ap": ap, "auc_resolution": res,
                     "cal_acc": cal_acc, "cal_conf": cal_conf, "cal_count": count.astype(np.int64), "ece": ece,
                     "conf_hist": conf_hist.astype(np.int64), "n_pos": n_pos, "n_neg": n_neg}
    return out


# ---- viability (metrics.py:304-340) -----------------------------------------------------------------
# ---- contour metrics from the boundary statistics (visualization.py:1687-1751 and the field's metrics) ----
DIST_SCALE = float(2 ** 16)  # the fixed point of the statistics' distance sums (eunet_boundary_stats)


def calculate_boundary_stats(pred, gt, num_classes: int = 3, ignore_index: int = 255, cap: int = 64,
                             band_radii: Sequence[int] = (2,), out: Optional[Dict] = None) -> Dict:
    """The integer boundary statistics of one mask pair [h, w] or of a batch [n, h, w] (numpy arrays, copied to
    the device, or tensors), as device buffers:
      {"surf": int64 [k, 2, cap^2 + 5], "band": int64 [k, nr, 3], "refrows": int64 [images, k, 2, 3],
       "cap", "band_radii", "ignore_index"}   (ops.boundary_stats; include/eunet.h, eunet_boundary_stats).
    out: the dict of an earlier call with the same num_classes, ignore_index, cap and band_radii; surf and band
    are added to in place (the maximum combined by max) and the new images' refrows are appended -- how a
    validation set accumulates.  The same dict is returned."""
    p = _dev_long(pred).contiguous()
    g = _dev_long(gt, p.device).contiguous()
    if p.shape != g.shape:
        raise ValueError(f"mask shapes differ: {tuple(p.shape)} vs {tuple(g.shape)}")
    radii = tuple(int(r) for r in band_radii)
    if out is None:
        surf, band, refrows = ops.boundary_stats(p, g, num_classes, ignore_index, cap, radii)
        return {"surf": surf, "band": band, "refrows": refrows, "cap": int(cap), "band_radii": radii,
                "ignore_index": int(ignore_index)}
    if tuple(out["surf"].shape) != (int(num_classes), 2, int(cap) ** 2 + 5) or out["cap"] != int(cap) or \
            tuple(out["band_radii"]) != radii or out["ignore_index"] != int(ignore_index):
        raise ValueError("calculate_boundary_stats: out was made with another num_classes, ignore_index, cap or "
                         "band_radii")
    n = 1 if p.dim() == 2 else p.shape[0]
    rows = torch.zeros(n, int(num_classes), 2, 3, dtype=torch.int64, device=p.device)
    ops.boundary_stats(p, g, num_classes, ignore_index, cap, radii, out=(out["surf"], out["band"], rows))
    out["refrows"] = torch.cat([out["refrows"], rows])
    return out


def _host(a) -> np.ndarray:
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _ratio(a, b) -> float:
    return float(a) / float(b) if b else float("nan")


def _percentile_rank(n: int, q: float) -> int:
    """The 1-based rank of the nearest-rank q-quantile of n values: numpy's method="inverted_cdf"."""
    return min(max(int(np.ceil(n * q)), 1), n)


def boundary_metrics_from_stats(stats: Dict, tolerances: Sequence[int] = (1, 2, 3),
                                class_names: Optional[Sequence[str]] = None) -> Dict:
    """The contour metrics per class from calculate_boundary_stats' buffers (pure numpy; one copy to the host
    when they are device tensors).  Distances are in pixels, between the edges E_c of the two maps (the class's
    pixels with a 4-neighbour outside the class or the image: MONAI's get_mask_edges).

    Everything except the two reference rows is POOLED over the edge pixels of all accumulated images, not a
    mean of per-image values.  Returns {class name: {...}, "boundary_ious_ref", "interior_ious_ref",
    "boundary_iou_ref", "interior_iou_ref"} (default names CLASS_NAMES[:k]) with, per class,
      n_pred_edge, n_gt_edge
      nsd[t]                 surface Dice at tolerance t: (#pred edges within t of a gt edge + #gt edges within t
                             of a pred edge) / (n_pred_edge + n_gt_edge); t an integer <= cap
      boundary_precision[t], boundary_recall[t], boundary_f1[t]   the two fractions on their own, and their
                             harmonic mean (0 when both are 0)
      hd                     the Hausdorff distance: sqrt of the larger directional maximum; inf when, in some
                             image, one map has an edge of the class and the other none; nan without any edge
      hd95, hd95_exceeds_cap the larger of the two directions' nearest-rank 95th percentiles (the smallest
                             distance with at least 95 % of that direction's edge pixels at or below it, numpy's
                             method="inverted_cdf"): exact when it falls within cap pixels; otherwise nan with
                             hd95_exceeds_cap=True (cap is then a lower bound); inf when the rank falls among
                             edge pixels without a counterpart
      assd                   the average symmetric surface distance over the pairs with a counterpart: (both
                             fixed-point sums) / 2^16 / (their number), within 2^-16 px of the true mean
      boundary_iou[r]        |B_r(pred) & B_r(gt)| / |B_r(pred) | B_r(gt)| for each band radius (Cheng et al. 2021,
                             Euclidean band)
    A ratio without a denominator is nan.  boundary_ious_ref / interior_ious_ref are the lists
    visualization.py:1687-1751 builds, in its order (image, then class) and with its skip rules (a class absent
    from the image's ground truth adds nothing; a row whose ground-truth set is empty adds nothing), computed
    without the ignore rule; boundary_iou_ref / interior_iou_ref are their means (nan when empty)."""
    surf, band, refrows = _host(stats["surf"]), _host(stats["band"]), _host(stats["refrows"])
    cap, radii = int(stats["cap"]), tuple(stats["band_radii"])
    cap2 = cap * cap
    if surf.ndim != 3 or surf.shape[1:] != (2, cap2 + 5) or band.shape != (surf.shape[0], len(radii), 3) or \
            refrows.ndim != 4 or refrows.shape[1:] != (surf.shape[0], 2, 3):
        raise ValueError(f"boundary_metrics_from_stats: buffers {surf.shape}, {band.shape}, {refrows.shape} do not "
                         f"fit cap = {cap} and {len(radii)} radii")
    k = surf.shape[0]
    if class_names is None:
        class_names = CLASS_NAMES[:k]
    if len(class_names) != k:
        raise ValueError(f"boundary_metrics_from_stats: {len(class_names)} class names for {k} classes")
    tolerances = tuple(int(t) for t in tolerances)
    if any(not 0 <= t <= cap for t in tolerances):
        raise ValueError(f"boundary_metrics_from_stats: tolerances {tolerances} must lie in 0..cap = {cap}")
    d2 = np.arange(cap2 + 1)
    result: Dict = {}
    for c, name in enumerate(class_names):
        hist = [surf[c, d, :cap2 + 1].astype(np.int64) for d in (0, 1)]
        over = [int(surf[c, d, cap2 + 1]) for d in (0, 1)]
        none = [int(surf[c, d, cap2 + 2]) for d in (0, 1)]
        n = [int(hist[d].sum()) + over[d] + none[d] for d in (0, 1)]
        m: Dict = {"n_pred_edge": n[0], "n_gt_edge": n[1], "nsd": {}, "boundary_precision": {},
                   "boundary_recall": {}, "boundary_f1": {}, "boundary_iou": {}}
        for t in tolerances:
            le = [int(hist[d][:t * t + 1].sum()) for d in (0, 1)]
            m["nsd"][t] = _ratio(le[0] + le[1], n[0] + n[1])
            pr, rc = _ratio(le[0], n[0]), _ratio(le[1], n[1])
            m["boundary_precision"][t], m["boundary_recall"][t] = pr, rc
            m["boundary_f1"][t] = float("nan") if np.isnan(pr) or np.isnan(rc) else \
                (2 * pr * rc / (pr + rc) if pr + rc > 0 else 0.0)
        if n[0] + n[1] == 0:
            m["hd"] = float("nan")
        elif none[0] or none[1]:
            m["hd"] = float("inf")
        else:
            m["hd"] = float(np.sqrt(float(max(int(surf[c, 0, cap2 + 3]), int(surf[c, 1, cap2 + 3])))))
        hd95, exceeds = float("nan"), False
        per_dir = []
        for d in (0, 1):
            if n[d] == 0:
                continue
            rank = _percentile_rank(n[d], 0.95)
            cum = np.cumsum(hist[d])
            if rank <= cum[-1]:
                per_dir.append(float(np.sqrt(float(d2[np.searchsorted(cum, rank)]))))
            elif rank <= cum[-1] + over[d]:
                exceeds = True
            else:
                per_dir.append(float("inf"))
        if per_dir and (not exceeds or max(per_dir) == float("inf")):
            hd95 = max(per_dir)
            exceeds = False
        m["hd95"], m["hd95_exceeds_cap"] = hd95, exceeds
        finite = n[0] + n[1] - none[0] - none[1]
        m["assd"] = _ratio((int(surf[c, 0, cap2 + 4]) + int(surf[c, 1, cap2 + 4])) / DIST_SCALE, finite)
        for j, r in enumerate(radii):
            a, b, both = (int(v) for v in band[c, j])
            m["boundary_iou"][r] = _ratio(both, a + b - both)
        result[name] = m
    lists = ([], [])
    for img in range(refrows.shape[0]):
        for c in range(k):
            if refrows[img, c, 0, 1] == 0:  # no pixel of the class in this ground truth: its dilation is empty too
                continue
            for row in (0, 1):
                a, b, both = (int(v) for v in refrows[img, c, row])
                if b > 0:
                    lists[row].append(both / (a + b - both))
    result["boundary_ious_ref"], result["interior_ious_ref"] = lists
    result["boundary_iou_ref"] = float(np.mean(lists[0])) if lists[0] else float("nan")
    result["interior_iou_ref"] = float(np.mean(lists[1])) if lists[1] else float("nan")
    return result


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


# ---- label-map instance metrics (the contingency table of ops.label_pairs) ---------------------------------
PANOPTIC_IOU_PERCENT = tuple(range(50, 100, 5))
INSTANCE_STAT_NAMES = ("n_pred", "n_gt", "tp50", "tp", "iou_sum", "aji_c", "aji_u", "objdice_g", "objdice_gw",
                       "objdice_p", "objdice_pw", "seg_sum")


def _iou_percent(iou_percent) -> Tuple[int, ...]:
    import operator
    try:
        ts = tuple(operator.index(t) for t in iou_percent)
    except TypeError:
        raise ValueError(f"iou_percent must be a sequence of integers, got {iou_percent!r}") from None
    if not ts or any(not 50 <= t <= 99 for t in ts):
        raise ValueError(f"iou_percent must hold integers in 50..99 (above one half a match is unique), got "
                         f"{iou_percent!r}")
    return ts


def _pair_rows(pairs) -> np.ndarray:
    rows = np.asarray(pairs, dtype=np.int64).reshape(-1, 4)
    if len(rows) and (rows.min() < 0 or (rows[:, 3] < 1).any()):
        raise ValueError("pairs: rows are (plane, a, b, n) with ids >= 0 and n >= 1")
    return rows


def empty_instance_stats(num_planes: int, num_thresholds: int = len(PANOPTIC_IOU_PERCENT)) -> Dict[str, np.ndarray]:
    """The statistics of nothing: what instance_stats_from_pairs results are added to."""
    z = {k: np.zeros(num_planes, np.int64) for k in INSTANCE_STAT_NAMES}
    z["tp"] = np.zeros((num_planes, num_thresholds), np.int64)
    for k in ("iou_sum", "objdice_g", "objdice_p", "seg_sum"):
        z[k] = np.zeros(num_planes, np.float64)
    return z


def instance_stats_from_pairs(pairs, num_planes: int, iou_percent: Sequence[int] = PANOPTIC_IOU_PERCENT
                              ) -> Dict[str, np.ndarray]:
    """pairs: the rows (plane, a, b, n) of ops.label_pairs(prediction ids, ground-truth ids), each plane one class ->
    a dict of arrays indexed by plane that add over images with a plain + per entry.

    With n(i, j) the table, area_a[i] = sum_b n(i, b) and area_b[j] = sum_a n(a, j) over the pixels that are not
    ignored (column and row 0 included), and for i, j >= 1 U(i, j) = area_a[i] + area_b[j] - n(i, j):
      n_pred, n_gt       objects (ids >= 1) on either side
      tp [., T]          pairs with IoU > t / 100, decided as 100 n > t U, for t in iou_percent (50..99: unique)
      tp50, iou_sum      the t = 50 matches and the float64 sum of their IoUs n / U in sorted (a, b) order
      aji_c, aji_u       Kumar et al.: for each ground truth j in ascending order the prediction i* of largest IoU
                         among those with n(i, j) > 0 (ranked by cross-multiplication, ties to the smallest i):
                         C += n(i*, j), U += U(i*, j), i* used -- it may serve several ground truths; without an
                         overlapping prediction U += area_b[j]; at the end U += area_a[i] of every unused prediction
      objdice_g, _gw     GlaS: sum over the ground truths j, in id order, of area_b[j] * Dice(j, the prediction of
                         largest n(i, j), ties to the smallest i; 0 without one) and the sum of area_b[j]; the term
                         is the float64 nearest to the integer quotient 2 n area_b[j] / (area_a[i] + area_b[j])
      objdice_p, _pw     the same from the predictions' side
      seg_sum            sum over the ground truths of the IoU of the prediction with 2 n > area_b[j], if any
    All products stay below 2^53 for planes of up to 8192 x 8192 pixels."""
    ts = _iou_percent(iou_percent)
    rows = _pair_rows(pairs)
    if len(rows) and rows[:, 0].max() >= num_planes:
        raise ValueError(f"pairs: plane {int(rows[:, 0].max())} of {num_planes}")
    rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
    st = empty_instance_stats(num_planes, len(ts))
    for q in range(num_planes):
        r = rows[rows[:, 0] == q]
        area_a: Dict[int, int] = {}
        area_b: Dict[int, int] = {}
        for _, i, j, n in r.tolist():
            area_a[i] = area_a.get(i, 0) + n
            area_b[j] = area_b.get(j, 0) + n
        area_a.pop(0, None)
        area_b.pop(0, None)
        inner = [(i, j, n) for _, i, j, n in r.tolist() if i >= 1 and j >= 1]  # sorted by (a, b)
        st["n_pred"][q], st["n_gt"][q] = len(area_a), len(area_b)
        iou_sum, tp50, tp = 0.0, 0, [0] * len(ts)
        best_g: Dict[int, Tuple[int, int, int]] = {}   # j -> (n, U, i) of the largest IoU
        over_g: Dict[int, Tuple[int, int]] = {}        # j -> (n, i) of the largest overlap
        over_p: Dict[int, Tuple[int, int]] = {}        # i -> (n, j)
        seg_of: Dict[int, float] = {}
        for i, j, n in inner:
            u = area_a[i] + area_b[j] - n
            if 100 * n > 50 * u:  # no threshold is below 50: nothing else can match
                tp50 += 1
                iou_sum += n / u
                for k, t in enumerate(ts):
                    if 100 * n > t * u:
                        tp[k] += 1
            b = best_g.get(j)
            if b is None or n * b[1] > b[0] * u:  # i ascends within a j: strict keeps the smallest i of a tie
                best_g[j] = (n, u, i)
            if j not in over_g or n > over_g[j][0]:
                over_g[j] = (n, i)
            if i not in over_p or n > over_p[i][0]:  # j ascends within an i
                over_p[i] = (n, j)
            if 2 * n > area_b[j]:
                seg_of[j] = n / u
        st["iou_sum"][q], st["tp50"][q], st["tp"][q] = iou_sum, tp50, tp
        c = u_sum = 0
        used = set()
        seg = dice_g = 0.0
        for j in sorted(area_b):
            b = best_g.get(j)
            if b is None:
                u_sum += area_b[j]
            else:
                c += b[0]
                u_sum += b[1]
                used.add(b[2])
            seg += seg_of.get(j, 0.0)
            if j in over_g:
                n, i = over_g[j]
                dice_g += 2 * n * area_b[j] / (area_a[i] + area_b[j])
        dice_p = 0.0
        for i in sorted(area_a):
            if i not in used:
                u_sum += area_a[i]
            if i in over_p:
                n, j = over_p[i]
                dice_p += 2 * n * area_a[i] / (area_a[i] + area_b[j])
        st["aji_c"][q], st["aji_u"][q] = c, u_sum
        st["seg_sum"][q] = seg
        st["objdice_g"][q], st["objdice_gw"][q] = dice_g, sum(area_b.values())
        st["objdice_p"][q], st["objdice_pw"][q] = dice_p, sum(area_a.values())
    return st


def add_instance_stats(a: Optional[Dict[str, np.ndarray]], b: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """a + b entry by entry (a None: b)."""
    return dict(b) if a is None else {k: a[k] + b[k] for k in INSTANCE_STAT_NAMES}


def _panoptic_rows(st: Dict, ts: Sequence[int], suffix: str) -> Dict[str, float]:
    """The scores of one row of statistics (scalars and tp [T])."""
    tp, n_pred, n_gt = int(st["tp50"]), int(st["n_pred"]), int(st["n_gt"])
    fp, fn = n_pred - tp, n_gt - tp
    m = {
        "pq": _ratio(st["iou_sum"], tp + 0.5 * fp + 0.5 * fn),
        "sq": _ratio(st["iou_sum"], tp),
        "dq": _ratio(tp, tp + 0.5 * fp + 0.5 * fn),
        "aji": _ratio(int(st["aji_c"]), int(st["aji_u"])),
        "objdice": 0.5 * (_ratio(st["objdice_g"], int(st["objdice_gw"])) +
                          _ratio(st["objdice_p"], int(st["objdice_pw"]))),
        "seg": _ratio(st["seg_sum"], n_gt),
    }
    scores = []
    for k, t in enumerate(ts):
        tpt = int(st["tp"][k])
        m[f"f1_{t}"] = _ratio(2 * tpt, n_pred + n_gt)
        scores.append(_ratio(tpt, n_pred + n_gt - tpt))  # TP / (TP + FP + FN)
    m["ap_dsb"] = float(np.mean(scores))
    return {f"{k}{suffix}": v for k, v in m.items()}


def panoptic_keys(class_names: Sequence[str] = INSTANCE_CLASSES, iou_percent: Sequence[int] = PANOPTIC_IOU_PERCENT
                  ) -> Tuple[str, ...]:
    base = ["pq", "sq", "dq", "aji", "objdice", "seg"] + [f"f1_{t}" for t in iou_percent] + ["ap_dsb"]
    return tuple(f"{k}_{c}" for c in class_names for k in base) + tuple(base) + ("mpq",)


def panoptic_metrics_from_stats(stats: Dict[str, np.ndarray], class_names: Sequence[str] = INSTANCE_CLASSES,
                                iou_percent: Sequence[int] = PANOPTIC_IOU_PERCENT) -> Dict[str, float]:
    """The scores of (accumulated) instance_stats_from_pairs statistics, taken with the same iou_percent: per class c
    pq_<c> = iou_sum / (TP + FP / 2 + FN / 2) at t = 50, sq_<c> = iou_sum / TP, dq_<c> = TP / (TP + FP / 2 + FN / 2),
    aji_<c> = C / U, objdice_<c> = (objdice_g / objdice_gw + objdice_p / objdice_pw) / 2, seg_<c> = seg_sum / n_gt,
    f1_<t>_<c> = 2 TP_t / (n_pred + n_gt) for every threshold and ap_dsb_<c> = the mean over the thresholds of
    TP_t / (TP_t + FP_t + FN_t); the same pooled over the classes (their statistics added) without a suffix; mpq =
    the mean of the class PQs over the classes with TP + FP + FN > 0.  An empty denominator gives NaN."""
    ts = _iou_percent(iou_percent)
    tp = np.asarray(stats["tp"])
    if tp.ndim != 2 or tp.shape != (len(class_names), len(ts)):
        raise ValueError(f"stats: tp is {tp.shape}, expected {len(class_names)} classes x {len(ts)} thresholds")
    out: Dict[str, float] = {}
    pqs = []
    for q, name in enumerate(class_names):
        row = {k: np.asarray(stats[k])[q] for k in INSTANCE_STAT_NAMES}
        out.update(_panoptic_rows(row, ts, f"_{name}"))
        if int(row["n_pred"]) + int(row["n_gt"]) - int(row["tp50"]) > 0:
            pqs.append(out[f"pq_{name}"])
    out.update(_panoptic_rows({k: np.asarray(stats[k]).sum(axis=0) for k in INSTANCE_STAT_NAMES}, ts, ""))
    out["mpq"] = float(np.mean(pqs)) if pqs else float("nan")
    return out


def calculate_panoptic_metrics(pred_ids, gt_ids, class_names: Sequence[str] = INSTANCE_CLASSES,
                               iou_percent: Sequence[int] = PANOPTIC_IOU_PERCENT) -> Dict[str, float]:
    """pred_ids, gt_ids: device id maps [len(class_names), h, w] (or [h, w] for one class), int32 or int64, 0 the
    background and a negative id an ignored pixel -> panoptic_metrics_from_stats of their contingency table."""
    planes = 1 if pred_ids.dim() == 2 else int(pred_ids.shape[0])
    if planes != len(class_names):
        raise ValueError(f"calculate_panoptic_metrics: {planes} plane(s) for the classes {tuple(class_names)}")
    stats = instance_stats_from_pairs(ops.label_pairs(pred_ids, gt_ids), planes, iou_percent)
    return panoptic_metrics_from_stats(stats, class_names, iou_percent)


SIZE_EDGES = (100, 500, 1000, 5000)  # visualization.py:1757


def size_strata_from_pairs(pairs, edges: Sequence[int] = SIZE_EDGES) -> List[List[float]]:
    """visualization.py:1762-1782 from a contingency table: pairs are the rows (plane, j, c, n) of
    ops.label_pairs(ground-truth component ids, prediction == class as 0 / 1).  Every object j >= 1 has area(j) =
    n(j, 0) + n(j, 1) and coverage n(j, 1) / area(j) (the float64 of the integer quotient: obj_pred.sum() /
    obj_size); the coverages are placed by min <= area < max into the len(edges) + 1 bins [0, e0), [e0, e1), ...,
    [e_last, inf), in (plane, id) order."""
    edges = [int(e) for e in edges]
    if any(b <= a for a, b in zip(edges, edges[1:])) or (edges and edges[0] <= 0):
        raise ValueError(f"edges must be positive and ascending, got {edges!r}")
    rows = _pair_rows(pairs)
    if len(rows) and rows[:, 2].max() > 1:
        raise ValueError("pairs: the second map must be 0 / 1")
    rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
    bins: List[List[float]] = [[] for _ in range(len(edges) + 1)]
    objs: Dict[Tuple[int, int], List[int]] = {}
    for q, j, c, n in rows.tolist():
        if j >= 1:
            objs.setdefault((q, j), [0, 0])[c] += n  # dicts keep insertion order: (plane, id) ascending
    for (q, j), (n0, n1) in objs.items():
        area = n0 + n1
        bins[int(np.searchsorted(edges, area, side="right"))].append(float(np.int64(n1) / np.int64(area)))
    return bins


# ---- per-cell measurements (the integer tables of ops.cell_stats, cellprops.hip) ---------------------------
MEASUREMENT_SUMMARY_KEYS = ("area", "equivalent_diameter", "major_axis", "minor_axis", "eccentricity", "circularity")
AGREEMENT_KEYS = ("n_matched", "area_rel_err_mean", "area_rel_err_median", "area_bias", "centroid_dist_mean",
                  "count_pred", "count_gt", "mean_area_pred", "mean_area_gt")


def _int_ratios(num: Sequence[int], den: Sequence[int]) -> np.ndarray:
    """num / den entry by entry, each the float64 nearest to the quotient of two Python integers of any size; NaN
    where den is 0."""
    return np.asarray([n / d if d else float("nan") for n, d in zip(num, den)], np.float64).reshape(len(num))


def cell_measurements(stats: Dict, plane: int = 0, pixel_size: float = 1.0) -> Dict[str, np.ndarray]:
    """The descriptors of the labels 1..n of one plane of ops.cell_stats' result (or of any dict with "geom" int64
    [p, n + 1, 14], "shape" (h, w) and, optionally, "intensity" int64 [p, n + 1, c, 4]) -> {name: float64 [n]}, entry
    i - 1 for label i.  A label with no pixel has area 0 and NaN everywhere else.  numpy only, float64.
      area, centroid_x, centroid_y, bbox ([n, 4]: x0, y0, x1, y1 inclusive, in pixels whatever pixel_size is),
      extent (area over the box's area), equivalent_diameter sqrt(4 A / pi)
      mu20, mu02, mu11   the second central moments per pixel about the centroid, from pixel centres without the
                         1 / 12 term of a pixel's own extent (regionprops' convention): (A sum x^2 - (sum x)^2) / A^2
                         and so on, the numerator exact in Python integers (A sum x^2 passes 2^63 on a large cell)
      major_axis, minor_axis   4 sqrt(l1), 4 sqrt(l2) of the eigenvalues l1 >= l2 of [[mu20, mu11], [mu11, mu02]]
      eccentricity       sqrt(1 - l2 / l1), 0 where l1 = 0
      orientation        atan2(2 mu11, mu20 - mu02) / 2: the angle of the major axis from the +x axis with y pointing
                         down, in (-pi / 2, pi / 2]; 0 for an isotropic cell
      perimeter_crack    q1 + q2 + q3 + 2 qd, the unit pixel edges between the label and anything else
      perimeter          Gray's bit-quad estimate q2 + (q1 + q3 + 2 qd) / sqrt 2
      circularity        4 pi A / perimeter^2, not clipped
      euler_number       (q1 - q3 - 2 qd) / 4, 8-connected
      holes              1 - euler_number: meaningful only where an id is one 8-connected component, which
                         ops.label_components and the watershed both give
      touches_border     1 where the box reaches the first or last row or column, else 0
      mean_<ch>, std_<ch> (population), min_<ch>, max_<ch>   per channel ch = 0.. of the intensity table, if present
    pixel_size s scales the lengths (centroid, diameter, axes, perimeters) by s and the areas (area, mu) by s^2."""
    geom = np.asarray(stats["geom"])
    if geom.ndim != 3 or geom.shape[2] != 14 or geom.dtype != np.int64:
        raise ValueError(f"cell_measurements: geom must be int64 [p, n + 1, 14], got {geom.dtype} {geom.shape}")
    if not 0 <= plane < geom.shape[0]:
        raise ValueError(f"cell_measurements: plane {plane} of {geom.shape[0]}")
    s = float(pixel_size)
    if not (s > 0.0 and np.isfinite(s)):
        raise ValueError(f"cell_measurements: pixel_size must be positive and finite, got {pixel_size!r}")
    h, w = (int(v) for v in stats["shape"])
    g = geom[plane, 1:]
    n = len(g)
    cols = [[int(v) for v in g[:, k]] for k in range(14)]  # Python integers: the products below are exact
    A, sx, sy, sxx, syy, sxy = cols[:6]
    present = g[:, 0] > 0
    nan = np.where(present, 0.0, np.nan)  # added to what a label with no pixel must not report
    area = g[:, 0].astype(np.float64)
    A2 = [a * a for a in A]
    mu20 = _int_ratios([a * q - m * m for a, q, m in zip(A, sxx, sx)], A2)
    mu02 = _int_ratios([a * q - m * m for a, q, m in zip(A, syy, sy)], A2)
    mu11 = _int_ratios([a * q - mx * my for a, q, mx, my in zip(A, sxy, sx, sy)], A2)
    half, diff = (mu20 + mu02) / 2.0, (mu20 - mu02) / 2.0
    root = np.sqrt(diff * diff + mu11 * mu11)
    l1, l2 = half + root, np.maximum(half - root, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        ecc = np.where(l1 > 0.0, np.sqrt(np.maximum(1.0 - l2 / np.where(l1 > 0.0, l1, 1.0), 0.0)), 0.0) + nan
        bbox = g[:, 6:10].astype(np.float64) + nan[:, None]
        box_area = (bbox[:, 2] - bbox[:, 0] + 1.0) * (bbox[:, 3] - bbox[:, 1] + 1.0)
        q1, q2, q3, qd = (g[:, k].astype(np.float64) for k in range(10, 14))
        perimeter = q2 + (q1 + q3 + 2.0 * qd) / np.sqrt(2.0) + nan
        euler = (q1 - q3 - 2.0 * qd) / 4.0 + nan
        touches = ((g[:, 6] == 0) | (g[:, 7] == 0) | (g[:, 8] == w - 1) | (g[:, 9] == h - 1)).astype(np.float64) + nan
        out = {
            "area": area * s * s, "centroid_x": _int_ratios(sx, A) * s, "centroid_y": _int_ratios(sy, A) * s, "bbox": bbox,
            "extent": area / box_area, "equivalent_diameter": np.sqrt(4.0 * area / np.pi) * s + nan,
            "mu20": mu20 * s * s, "mu02": mu02 * s * s, "mu11": mu11 * s * s,
            "major_axis": 4.0 * np.sqrt(l1) * s, "minor_axis": 4.0 * np.sqrt(l2) * s, "eccentricity": ecc,
            "orientation": 0.5 * np.arctan2(2.0 * mu11, mu20 - mu02),
            "perimeter_crack": (q1 + q2 + q3 + 2.0 * qd) * s + nan, "perimeter": perimeter * s,
            "circularity": 4.0 * np.pi * area / (perimeter * perimeter), "euler_number": euler, "holes": 1.0 - euler,
            "touches_border": touches,
        }
    inten = stats.get("intensity")
    if inten is not None:
        inten = np.asarray(inten)
        if inten.ndim != 4 or inten.shape[:2] != geom.shape[:2] or inten.shape[3] != 4:
            raise ValueError(f"cell_measurements: intensity must be [p, n + 1, c, 4], got {inten.shape}")
        for ch in range(inten.shape[2]):
            t = inten[plane, 1:, ch]
            sv, sq = [int(v) for v in t[:, 0]], [int(v) for v in t[:, 1]]
            out[f"mean_{ch}"] = _int_ratios(sv, A)
            out[f"std_{ch}"] = np.sqrt(_int_ratios([max(a * q - v * v, 0) for a, q, v in zip(A, sq, sv)], A2))
            out[f"min_{ch}"] = t[:, 2].astype(np.float64) + nan
            out[f"max_{ch}"] = t[:, 3].astype(np.float64) + nan
    assert all(len(v) == n for v in out.values())
    return out


HULL_KEYS = ("convex_area", "solidity", "convex_perimeter", "convexity", "feret_max", "feret_max_angle", "feret_min",
             "feret_min_angle", "feret_ratio", "hull_vertices")


def _fold_angle(dy: np.ndarray, dx: np.ndarray) -> np.ndarray:
    """The direction of (dx, dy) as the angle of a line: atan2 folded into (-pi / 2, pi / 2]."""
    a = np.arctan2(dy, dx)
    return np.where(a > np.pi / 2, a - np.pi, np.where(a <= -np.pi / 2, a + np.pi, a))


def hull_measurements(hulls: Dict, stats: Dict, plane: int = 0, pixel_size: float = 1.0) -> Dict[str, np.ndarray]:
    """The convex-hull descriptors of the labels 1..n of one plane: hulls is ops.cell_hulls' result (or any dict with
    "hull" int64 [p, n + 1, 11]), stats the ops.cell_stats result it was formed from ("geom" int64 [p, n + 1, 14]) ->
    {name: float64 [n]}, entry i - 1 for label i, NaN everywhere for a label with no pixel.  The hull is that of the
    pixel squares (include/eunet.h, "per-cell convex hulls").  numpy only, float64.
      convex_area        the hull's area, column 1 / 2
      solidity           area / convex area = 2 A / column 1, the quotient of two Python integers; in (0, 1]
      convex_perimeter   column 2 / 2^16
      convexity          convex_perimeter / perimeter_crack (cell_measurements'), in (0, 1]
      feret_max          the largest distance between two hull vertices, sqrt(column 3)
      feret_max_angle    the direction of that pair from the +x axis with y pointing down, in (-pi / 2, pi / 2]
      feret_min          the smallest width between two parallel lines that hold the hull, one of them along a hull
                         edge: column 8 / sqrt(column 9^2 + column 10^2)
      feret_min_angle    the direction the width is measured in, across that edge, in (-pi / 2, pi / 2]
      feret_ratio        feret_min / feret_max, in (0, 1]
      hull_vertices      column 0
    pixel_size s scales the lengths (perimeter, Feret diameters) by s and convex_area by s^2."""
    hull, geom = np.asarray(hulls["hull"]), np.asarray(stats["geom"])
    if hull.ndim != 3 or hull.shape[2] != 11 or hull.dtype != np.int64:
        raise ValueError(f"hull_measurements: hull must be int64 [p, n + 1, 11], got {hull.dtype} {hull.shape}")
    if geom.ndim != 3 or geom.shape[2] != 14 or geom.dtype != np.int64 or geom.shape[:2] != hull.shape[:2]:
        raise ValueError(f"hull_measurements: geom must be int64 {hull.shape[:2] + (14,)}, got {geom.dtype} {geom.shape}")
    if not 0 <= plane < hull.shape[0]:
        raise ValueError(f"hull_measurements: plane {plane} of {hull.shape[0]}")
    s = float(pixel_size)
    if not (s > 0.0 and np.isfinite(s)):
        raise ValueError(f"hull_measurements: pixel_size must be positive and finite, got {pixel_size!r}")
    t, g = hull[plane, 1:], geom[plane, 1:]
    if ((t[:, 0] > 0) != (g[:, 0] > 0)).any():
        raise ValueError("hull_measurements: the hulls and the stats disagree on which labels have a pixel")
    nan = np.where(t[:, 0] > 0, 0.0, np.nan)  # added to what a label with no pixel must not report
    f = t.astype(np.float64)  # every column is below 2^53
    crack = (g[:, 10] + g[:, 11] + g[:, 12] + 2 * g[:, 13]).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        per = f[:, 2] / 65536.0 + nan
        fmax = np.sqrt(f[:, 3]) + nan
        fmin = f[:, 8] / np.sqrt(f[:, 9] * f[:, 9] + f[:, 10] * f[:, 10])
        out = {
            "convex_area": f[:, 1] / 2.0 * s * s + nan,
            "solidity": _int_ratios([2 * int(a) for a in g[:, 0]], [int(v) for v in t[:, 1]]),
            "convex_perimeter": per * s, "convexity": per / crack,
            "feret_max": fmax * s, "feret_max_angle": _fold_angle(f[:, 7] - f[:, 5], f[:, 6] - f[:, 4]) + nan,
            "feret_min": fmin * s, "feret_min_angle": _fold_angle(f[:, 9], -f[:, 10]) + nan,
            "feret_ratio": fmin / fmax, "hull_vertices": f[:, 0] + nan,
        }
    assert tuple(out) == HULL_KEYS and all(len(v) == len(t) for v in out.values())
    return out


def population_summary(measurements: Dict[str, np.ndarray], keys: Sequence[str] = MEASUREMENT_SUMMARY_KEYS
                       ) -> Dict[str, float]:
    """cell_measurements' dict -> {"count": the labels with area > 0, "<key>_mean", "<key>_median", "<key>_std"
    (population) of every key in keys over those labels}; NaN where there is none."""
    present = np.asarray(measurements["area"]) > 0
    out = {"count": float(present.sum())}
    for k in keys:
        v = np.asarray(measurements[k], np.float64)
        if v.ndim != 1:
            raise ValueError(f"population_summary: {k} is not one number per label")
        v = v[present]
        for name, f in (("mean", np.mean), ("median", np.median), ("std", np.std)):
            out[f"{k}_{name}"] = float(f(v)) if len(v) else float("nan")
    return out


# ---- cells in relation to each other (the tables of ops.label_contacts and ops.cell_stats, neighbors.hip) --------
NEIGHBOR_KEYS = ("area", "n_neighbors", "shared_border", "touching_fraction", "territory_area",
                 "first_closest_distance", "second_closest_distance", "first_closest_id", "second_closest_id",
                 "angle_between_neighbors")


def _contact_rows(contacts, plane: int, n: int, what: str) -> np.ndarray:
    """The rows (a, b, count) of one plane of ops.label_contacts' table, checked: 1 <= a < b <= n, count >= 1."""
    rows = np.asarray(contacts)
    if rows.ndim != 2 or rows.shape[1] != 4 or rows.dtype != np.int64:
        raise ValueError(f"{what}: contacts must be int64 [m, 4] rows (plane, a, b, n), got {rows.dtype} {rows.shape}")
    rows = rows[rows[:, 0] == plane][:, 1:]
    if len(rows) and not ((rows[:, 0] >= 1) & (rows[:, 0] < rows[:, 1]) & (rows[:, 1] <= n) & (rows[:, 2] >= 1)).all():
        raise ValueError(f"{what}: a contact row of plane {plane} is not 1 <= a < b <= {n} with a count >= 1")
    if len(np.unique(rows[:, :2], axis=0)) != len(rows):
        raise ValueError(f"{what}: a pair of labels has two rows in plane {plane}")
    return rows


def neighbor_graph(contacts, plane: int, n: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The contact graph of the labels 1..n of one plane of ops.label_contacts' table -> the CSR arrays (indptr int64
    [n + 1], indices int64, weights int64): the neighbours of label i are the labels indices[indptr[i - 1]:
    indptr[i]] (ids, ascending), weights the contact counts of those pairs.  Symmetric: every row (a, b, c) of the
    table gives b among a's neighbours and a among b's, both with weight c."""
    n = int(n)
    if n < 0:
        raise ValueError(f"neighbor_graph: n must be >= 0, got {n}")
    rows = _contact_rows(contacts, plane, n, "neighbor_graph")
    src = np.concatenate([rows[:, 0], rows[:, 1]])
    dst = np.concatenate([rows[:, 1], rows[:, 0]])
    wts = np.concatenate([rows[:, 2], rows[:, 2]])
    order = np.lexsort((dst, src))
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(src - 1, minlength=n)[:n], out=indptr[1:])
    return indptr, dst[order].astype(np.int64), wts[order].astype(np.int64)


def neighbor_measurements(contacts, stats: Dict, stats_expanded: Dict, plane: int = 0, pixel_size: float = 1.0
                          ) -> Dict[str, np.ndarray]:
    """What the labels 1..n of one plane are to each other (CellProfiler's MeasureObjectNeighbors): contacts is
    ops.label_contacts' table of the EXPANDED map (ops.expand_label_map), stats ops.cell_stats' result of the original
    map and stats_expanded that of the expanded one, both for the same n -> {name: float64 [n]}, entry i - 1 for label
    i.  numpy only, float64 from the integer tables.
      area                     of the original label (what population_summary counts the present labels by)
      n_neighbors              the labels it shares a contact row with
      shared_border            the sum of its contact counts; at connectivity 4 the pixel sides it shares with others
      touching_fraction        that sum over the crack perimeter q1 + q2 + q3 + 2 qd of the expanded label: at
                               connectivity 4 both count pixel sides, so it lies in [0, 1]; 0 for a label with no pixel
      territory_area           the area of the expanded label
      first_closest_distance, second_closest_distance   between its centroid and the nearest and second nearest
                               centroid of the other labels of the plane that have a pixel (the original map's
                               centroids; the smaller id among equally near ones first); NaN where there are fewer
                               than 2 or 3 such labels, and for a label with no pixel
      first_closest_id, second_closest_id   the ids of those two labels (NaN likewise)
      angle_between_neighbors  the angle at the label's centroid between those two, in degrees, 0..180
    pixel_size s scales the lengths (shared_border, the distances) by s and the areas by s^2."""
    what = "neighbor_measurements"
    geom, geom_e = np.asarray(stats["geom"]), np.asarray(stats_expanded["geom"])
    if geom.ndim != 3 or geom.shape[2] != 14 or geom.dtype != np.int64:
        raise ValueError(f"{what}: geom must be int64 [p, n + 1, 14], got {geom.dtype} {geom.shape}")
    if geom_e.shape != geom.shape or geom_e.dtype != np.int64:
        raise ValueError(f"{what}: the expanded map's geom must be int64 {geom.shape}, got {geom_e.dtype} "
                         f"{geom_e.shape}")
    if not 0 <= plane < geom.shape[0]:
        raise ValueError(f"{what}: plane {plane} of {geom.shape[0]}")
    s = float(pixel_size)
    if not (s > 0.0 and np.isfinite(s)):
        raise ValueError(f"{what}: pixel_size must be positive and finite, got {pixel_size!r}")
    g, e = geom[plane, 1:], geom_e[plane, 1:]
    n = len(g)
    indptr, indices, weights = neighbor_graph(contacts, plane, n)
    degree = np.diff(indptr).astype(np.float64)
    shared = np.zeros(n, np.float64)
    np.add.at(shared, np.repeat(np.arange(n), np.diff(indptr)), weights.astype(np.float64))
    crack = (e[:, 10] + e[:, 11] + e[:, 12] + 2 * e[:, 13]).astype(np.float64)
    present = g[:, 0] > 0
    cx = _int_ratios([int(v) for v in g[:, 1]], [int(v) for v in g[:, 0]])
    cy = _int_ratios([int(v) for v in g[:, 2]], [int(v) for v in g[:, 0]])
    ids = np.flatnonzero(present)  # label - 1 of the labels with a pixel, ascending
    near = np.full((n, 2), np.nan)
    near_id = np.full((n, 2), np.nan)
    angle = np.full(n, np.nan)
    for lo in range(0, len(ids), 1024):  # a block of rows of the centroid distance matrix at a time
        rows = ids[lo:lo + 1024]
        dx, dy = cx[ids][None, :] - cx[rows][:, None], cy[ids][None, :] - cy[rows][:, None]
        d2 = dx * dx + dy * dy
        d2[np.arange(len(rows)), lo + np.arange(len(rows))] = np.inf  # not its own neighbour
        order = np.argsort(d2, axis=1, kind="stable")[:, :2]  # stable: the smaller id among equally near ones
        for k in range(min(2, len(ids) - 1)):
            j = order[:, k]
            near[rows, k] = np.sqrt(d2[np.arange(len(rows)), j])
            near_id[rows, k] = ids[j] + 1.0
        if len(ids) >= 3:
            r = np.arange(len(rows))
            ax, ay, bx, by = dx[r, order[:, 0]], dy[r, order[:, 0]], dx[r, order[:, 1]], dy[r, order[:, 1]]
            with np.errstate(invalid="ignore", divide="ignore"):
                cos = (ax * bx + ay * by) / np.sqrt((ax * ax + ay * ay) * (bx * bx + by * by))
            angle[rows] = np.degrees(np.arccos(np.clip(cos, -1.0, 1.0)))
    with np.errstate(invalid="ignore", divide="ignore"):
        touching = np.where(crack > 0.0, shared / np.where(crack > 0.0, crack, 1.0), 0.0)
    out = {
        "area": g[:, 0].astype(np.float64) * s * s, "n_neighbors": degree, "shared_border": shared * s,
        "touching_fraction": touching, "territory_area": e[:, 0].astype(np.float64) * s * s,
        "first_closest_distance": near[:, 0] * s, "second_closest_distance": near[:, 1] * s,
        "first_closest_id": near_id[:, 0], "second_closest_id": near_id[:, 1], "angle_between_neighbors": angle,
    }
    assert tuple(out) == NEIGHBOR_KEYS and all(len(v) == n for v in out.values())
    return out


def measurement_agreement(pairs, geom_pred, geom_gt, plane: int) -> Dict:
    """How the measurements of one class plane's predicted cells agree with the ground truth's: pairs are the rows
    (plane, a, b, n) of ops.label_pairs(prediction ids, ground-truth ids), geom_pred / geom_gt the "geom" tables of
    ops.cell_stats of the two maps.  A predicted cell i and a ground-truth cell j are matched when 100 n > 50 U, U =
    area_a[i] + area_b[j] - n with the areas of the pair table (instance_stats_from_pairs' integer predicate: IoU above
    one half, hence unique) -> {"matches": int64 [m, 2] of (i, j) sorted, "area_rel": float64 [m] of (A_p - A_g) / A_g
    with the areas of the geom tables, "centroid_dist": float64 [m] in pixels, "count_pred", "count_gt": the labels
    with a pixel, "area_pred", "area_gt": their summed areas}.  agreement_summary pools a list of these."""
    rows = _pair_rows(pairs)
    gp, gg = np.asarray(geom_pred)[plane], np.asarray(geom_gt)[plane]
    r = rows[rows[:, 0] == plane]
    r = r[np.lexsort((r[:, 2], r[:, 1]))]
    area_a: Dict[int, int] = {}
    area_b: Dict[int, int] = {}
    for _, i, j, n in r.tolist():
        area_a[i] = area_a.get(i, 0) + n
        area_b[j] = area_b.get(j, 0) + n
    matches, rel, dist = [], [], []
    for _, i, j, n in r.tolist():
        if i < 1 or j < 1 or not 100 * n > 50 * (area_a[i] + area_b[j] - n):
            continue
        if i >= len(gp) or j >= len(gg):
            raise ValueError(f"measurement_agreement: the pair ({i}, {j}) lies outside the tables")
        ap, ag = int(gp[i, 0]), int(gg[j, 0])
        matches.append((i, j))
        rel.append((ap - ag) / ag)
        dx = int(gp[i, 1]) / ap - int(gg[j, 1]) / ag
        dy = int(gp[i, 2]) / ap - int(gg[j, 2]) / ag
        dist.append(float(np.hypot(dx, dy)))
    return {"matches": np.asarray(matches, np.int64).reshape(-1, 2), "area_rel": np.asarray(rel, np.float64),
            "centroid_dist": np.asarray(dist, np.float64),
            "count_pred": int((gp[1:, 0] > 0).sum()), "count_gt": int((gg[1:, 0] > 0).sum()),
            "area_pred": int(gp[1:, 0].sum()), "area_gt": int(gg[1:, 0].sum())}


def agreement_summary(parts: Sequence[Dict]) -> Dict[str, float]:
    """measurement_agreement results of one class over several images, pooled -> AGREEMENT_KEYS: n_matched,
    area_rel_err_mean / _median of |A_p - A_g| / A_g and area_bias, the mean of (A_p - A_g) / A_g, over the matched
    pairs, centroid_dist_mean in pixels (NaN without a match), count_pred, count_gt, mean_area_pred, mean_area_gt (NaN
    without a cell)."""
    rel = np.concatenate([np.asarray(p["area_rel"], np.float64) for p in parts]) if parts else np.zeros(0)
    dist = np.concatenate([np.asarray(p["centroid_dist"], np.float64) for p in parts]) if parts else np.zeros(0)
    cp, cg = sum(p["count_pred"] for p in parts), sum(p["count_gt"] for p in parts)
    nan = float("nan")
    return {"n_matched": float(len(rel)),
            "area_rel_err_mean": float(np.mean(np.abs(rel))) if len(rel) else nan,
            "area_rel_err_median": float(np.median(np.abs(rel))) if len(rel) else nan,
            "area_bias": float(np.mean(rel)) if len(rel) else nan,
            "centroid_dist_mean": float(np.mean(dist)) if len(dist) else nan,
            "count_pred": float(cp), "count_gt": float(cg),
            "mean_area_pred": sum(p["area_pred"] for p in parts) / cp if cp else nan,
            "mean_area_gt": sum(p["area_gt"] for p in parts) / cg if cg else nan}
