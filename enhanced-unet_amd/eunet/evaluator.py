"""Drop-in inference and evaluation path of reference train_eval.Evaluator.

    Evaluator(model, device, model_name)                       # train_eval.py:356-363
    ._run_model_single(image [C,h,w]) -> probs [K,h,w]          # train_eval.py:397-417
    ._run_tta_inference(image) -> probs (5-view TTA mean)       # train_eval.py:419-453
    .predict_probs(image) -> probs [K,h,w] on the device (what predict_semantic_mask converts)
    ._convert_probs_to_mask(probs) -> int64 mask [h,w] (numpy)  # train_eval.py:455-568
    .predict_semantic_mask(image) -> int64 mask [h,w] (numpy)   # train_eval.py:570-606
    .semantic_to_instances(mask, min_area=3)                    # train_eval.py:654-850
        -> (instance_masks, instance_labels, instance_scores)
    .evaluate(dataloader, coco_map=False) -> mean semantic / instance / viability rows   # train_eval.py:852-1021
        (coco_map=True adds bbox_mAP / segm_mAP, train_eval.py:951-992, 1007-1011)
    .evaluate_semantic(dataloader) -> mean semantic metrics     # train_eval.py:852-904 (semantic rows)
    .evaluate_curves(dataloader) -> per-class ROC / PR / calibration statistics over all pixels
        (what visualization.py:1096-1199, 1819-1900 plot)
    .evaluate_with_curves(dataloader, coco_map=False) -> evaluate()'s rows plus auc_ / ap_ / ece_<class>
    .evaluate_boundary(dataloader) -> per-class contour metrics (HD, HD95, ASSD, surface Dice, boundary F1,
        Boundary IoU) and the two lists of visualization.py:1687-1751 (plot_boundary_accuracy)
    .semantic_to_instance_maps(mask, min_area=3) -> (ids int32 [2,h,w], counts, scores): semantic_to_instances'
        instances as one id map per class
    .evaluate_panoptic(dataloader) -> PQ / SQ / DQ, AJI, object Dice, SEG, F1 and AP over IoU 0.5 .. 0.95 per class
        and pooled, from label maps (no reference counterpart)
    .evaluate_by_size(dataloader) -> per-object coverage binned by object area (visualization.py:1753-1817)

Every per-pixel step runs in HIP (evalpath.hip): the flips and 0.75/1.25
rescales (PyTorch bilinear index math), softmax + crop, the TTA mean, the
thresholded mask conversion (two passes; the pixel-ratio refinement reads the
pass-1 counts on the device).  The network is the fused forward_lowres (the
2H->H bilinear resize of train_eval.py:413 is the exact 2x2 mean it computes).

_prepare_image_tensor (train_eval.py:365-395) runs in HIP too (imgproc.hip):
CHW float -> uint8 (x255 when max <= 1), RGB -> Lab, CLAHE(2.0, 8x8) on L,
Lab -> RGB, filter2D sharpening x0.15, /255.  cv2 is absent, so those kernels
follow OpenCV's documented algorithms (parity unpinned, oracle/imgproc_ref.py).
preprocess=None skips the step, a callable replaces it.

The instance split runs in HIP as well (instances.hip): the 2x2 opening, the
erosion ladder, 8-connected labelling (skimage.measure.label's numbering) and
Suzuki-Abe outer-border following for the compactness score; the host keeps
only the reference's control flow over per-region pixel counts.  As with the
image preprocessing, cv2 is absent: which contour cv2.findContours lists first
for an instance of several components (taken as the one discovered last) and
cv2.arcLength's float32 segment rounding (the perimeter here is the exact
n_axis + n_diag * sqrt(2) in float64) are unpinned; both live in
ops.outer_perimeter / _perimeter alone.

COCO mAP (bbox_mAP / segm_mAP, COCOeval stats[0]) is built natively, without
pycocotools: evaluate(coco_map=True) packs each image's masks with their
bounding boxes, forms the pairwise overlap and runs COCOeval's greedy matching
on the device (eunet_pack_masks_bbox, eunet_pairwise_overlap,
eunet_coco_match); only the match tables come back, and
metrics.coco_map_from_matches accumulates them once at the end.  The default
evaluate() returns the 23 EVALUATE_KEYS rows as before.

Pixel-level ROC, PR and calibration statistics stay on the device as well: the reference copies every
image's softmax to the host, extends Python lists pixel by pixel and sorts them with sklearn, for 20 images
at most (train_eval.py:1291-1319).  Here each image's probabilities are binned once into an exact integer
histogram (ops.score_hist, curves.hip) that accumulates over the whole loader; one copy comes back and
metrics.curve_metrics_from_hist forms the curves, the AUC with a hard bound on its binning error, the
average precision, the reliability curve and its ECE.  Two deliberate departures from the reference's
plots: the last calibration bin holds p == 1, and ignored pixels (255) are left out of the calibration
too, as they are out of its ROC and PR curves.

Contour quality (evaluate_boundary): the reference's plot_boundary_accuracy copies every mask to the host and
runs scipy.ndimage morphology per image and class.  Here the predicted mask never leaves the device: an exact
Euclidean distance transform of both maps' class edges (ops.distance_transform_sq's kernels) feeds one integer
statistics pass (ops.boundary_stats, boundary.hip) that accumulates over the loader; one copy comes back and
metrics.boundary_metrics_from_stats forms the Hausdorff distance, HD95, the average symmetric surface distance,
surface Dice, boundary F1 and Boundary IoU, and the reference's boundary / interior IoU lists.

Label-map instance metrics (evaluate_panoptic, evaluate_by_size): the predicted instances and the ground truth are
two integer id maps per class, and every score is a function of their sparse contingency table, which one pass
builds on the device (ops.label_pairs, pairs.hip) and metrics.instance_stats_from_pairs reads in integers.  No
mask plane per instance is expanded and no pair of masks is compared.

Per-cell measurements (measure_cells, evaluate_measurements; no reference counterpart): the id maps of
semantic_to_instance_maps go through one ops.cell_stats call (cellprops.hip), whose integer tables
metrics.cell_measurements turns into area, centroid, axes, orientation, perimeter, circularity, holes and per-channel
intensity of every cell; evaluate_measurements compares the areas and centroids of the predicted cells with those of
the ground-truth cells they match at IoU > 1/2.

Cells in relation to each other (measure_neighbors; no reference counterpart): the two class planes are pooled into
one id map, grown by ops.expand_label_map (neighbors.hip) by a distance or to the Voronoi partition, and
ops.label_contacts' table of the grown map gives metrics.neighbor_measurements the neighbour counts, shared borders,
territories and closest-cell distances of every cell, and the contact graph.

Overlap-tile inference (no reference counterpart: the reference resizes every image down to max_size):
Evaluator(..., tile=T) sends an image whose padded size exceeds T in either axis through the network tile by
tile (eunet.tiling.plan; ops.tile_gather, forward_lowres on tile_batch tiles at a time, one ops.tile_blend
with the activation and the flips) and everything above _run_model_single runs unchanged on the full-size
probabilities.  With the default blend "crop" and margin (tiling.RECEPTIVE_MARGIN) the probabilities are the
whole-image forward's, bit for bit (tests/test_gpu_tiling.py).
"""
from __future__ import annotations

import math
import warnings
from typing import Callable, Dict, Optional, Union

import numpy as np
import torch
import torch.nn.functional as F

from . import ops, tiling
from .metrics import (CLASS_NAMES, INSTANCE_CLASSES, PANOPTIC_IOU_PERCENT, SIZE_EDGES, _dev_long, _stack_masks,
                      add_instance_stats, boundary_metrics_from_stats, calculate_boundary_stats, calculate_dice,
                      calculate_instance_metrics, calculate_iou, calculate_semantic_metrics,
                      calculate_viability_metrics, coco_image_matches, coco_map_from_matches, curve_edges,
                      curve_metrics_from_hist, instance_stats_from_pairs, panoptic_keys, panoptic_metrics_from_stats,
                      size_strata_from_pairs, AGREEMENT_KEYS, agreement_summary, cell_measurements,
                      hull_measurements, measurement_agreement, neighbor_graph, neighbor_measurements)

TTA_SCALES = (0.75, 1.25)

# semantic_to_instances (train_eval.py:686, 793-798, 842)
LARGE_REGION = 200
MAX_AREA = 1500
MIN_AREA_CLASS = {1: 3, 2: 5}
MAX_INSTANCES = 500

# the rows evaluate() averages (train_eval.py:854-880) without bbox_mAP / segm_mAP
EVALUATE_KEYS = ("sem_mean_iou", "sem_mean_dice", "sem_background_iou", "sem_background_dice", "sem_live_iou",
                 "sem_live_dice", "sem_dead_iou", "sem_dead_dice", "live_iou", "live_precision", "live_recall",
                 "live_ap", "dead_iou", "dead_precision", "dead_recall", "dead_ap", "viability_accuracy",
                 "pred_viability", "gt_viability", "pred_live_count", "pred_dead_count", "gt_live_count",
                 "gt_dead_count")
# the two rows evaluate(coco_map=True) adds (train_eval.py:871-872, 1007-1011)
COCO_KEYS = ("bbox_mAP", "segm_mAP")
CURVE_STATS = ("auc", "ap", "ece")


def curve_keys(class_names) -> tuple:
    return tuple(f"{s}_{name}" for name in class_names for s in CURVE_STATS)


# the rows evaluate_panoptic() returns for the default thresholds
PANOPTIC_KEYS = panoptic_keys() + ("aji_image_mean", "gt_overlap_pixels")
# the rows evaluate_with_curves() adds for a three-class model (visualization.py:1131, 1184; the ECE of :1847-1864)
CURVE_KEYS = curve_keys(CLASS_NAMES)


def _perimeter(n_axis: int, n_diag: int) -> float:
    """cv2.arcLength(contours[0], True) of the followed border: axis steps + diagonal steps * sqrt(2)."""
    return n_axis + n_diag * math.sqrt(2.0)


def _count(c: torch.Tensor) -> int:
    return int(c.item())


def reference_preprocess(image: torch.Tensor) -> torch.Tensor:
    """train_eval.py:365-395 on the device: [3,h,w] float -> CLAHE(2.0) + sharpen(0.15) -> [3,h,w] / 255."""
    if image.dim() != 3 or image.shape[0] != 3:
        raise ValueError("the reference preprocessing converts RGB -> Lab: image must be [3, h, w]")
    u8 = ops.chw_to_u8(image)
    return ops.to_tensor(ops.sharpen_u8(ops.clahe_rgb_u8(u8, 2.0), 0.15))


class Evaluator:
    def __init__(self, model, device, model_name, preprocess: Union[str, Callable, None] = "reference", *,
                 activation: str = "softmax", threshold: float = 0.5, tile: Optional[int] = None,
                 tile_blend: str = "crop", tile_margin: Optional[int] = None, tile_overlap: float = 0.25,
                 tile_batch: int = 4, split: str = "erosion", split_depth: float = 1.0):
        """tile: None (one forward per view, as the reference) or the largest tile side, a multiple of 32: a
        view whose padded height or width exceeds it is predicted tile by tile (eunet.tiling.plan with blend
        tile_blend, margin tile_margin for "crop" -- None: tiling.RECEPTIVE_MARGIN, for which the result is
        exact -- and tile_overlap for "constant" / "gaussian"), tile_batch tiles per forward.  Not for a
        dual-branch model: its fusion head widens the receptive field, which has not been measured.

        activation "softmax" is the reference's path.  "sigmoid" is the prediction path of a model trained
        with losses.bce_dice_loss: a sigmoid per logit (ops.sigmoid_crop), the same TTA mean of probabilities,
        then ops.probs_threshold ([p >= threshold] for one logit, the argmax for more); the reference's
        hand-tuned probs_to_mask rules are softmax-specific and are not applied.

        split: how semantic_to_instances separates touching cells.  "erosion" is the reference's ladder of fixed
        erosions (train_eval.py:697-785).  "watershed" splits each class along the ridges of its exact distance
        transform (ops.watershed_from_distance): basins whose peak stands less than split_depth pixels above the
        saddle to a higher neighbour are merged; no area threshold decides what is split."""
        if split not in ("erosion", "watershed"):
            raise ValueError(f"split must be 'erosion' or 'watershed', not {split!r}")
        self.split = split
        self.split_depth = ops._watershed_depth("split_depth", split_depth)
        if activation not in ("softmax", "sigmoid"):
            raise ValueError(f"activation must be 'softmax' or 'sigmoid', not {activation!r}")
        self.activation = activation
        self.threshold = float(threshold)
        self.model = model
        self.device = device
        self.model_name = model_name
        self.enable_tta = model_name == "enhanced_unet"
        self.preprocess = preprocess
        self.tile = None if tile is None else int(tile)
        self.tile_blend, self.tile_margin, self.tile_overlap = tile_blend, tile_margin, float(tile_overlap)
        self.tile_batch = int(tile_batch)
        if self.tile is not None:
            if getattr(model, "dual_branch", False):
                raise ValueError("tile: tiled inference is not built for the dual-branch model (the receptive "
                                 "margin of its fusion head has not been measured)")
            if self.tile_batch < 1:
                raise ValueError(f"tile_batch must be at least 1, not {tile_batch}")
            if not hasattr(model, "forward_lowres"):
                raise ValueError("tile: tiled inference needs a model with forward_lowres")
            self._tile_plan(self.tile, self.tile)  # the plan's refusals (tile, blend, margin, overlap) at construction

    def _tile_plan(self, h: int, w: int) -> tiling.TilePlan:
        return tiling.plan(h, w, self.tile, blend=self.tile_blend, margin=self.tile_margin,
                           overlap=self.tile_overlap)

    # ---- train_eval.py:365-395 -------------------------------------------------
    def _prepare_image_tensor(self, image: torch.Tensor) -> torch.Tensor:
        image = image.to(self.device).float()
        if self.preprocess is None:
            return image
        if callable(self.preprocess):
            return self.preprocess(image)
        if self.preprocess != "reference":
            raise ValueError(f"preprocess must be 'reference', None or a callable, not {self.preprocess!r}")
        return reference_preprocess(image)

    def _logits(self, image_padded: torch.Tensor) -> torch.Tensor:
        m = self.model
        if hasattr(m, "forward_lowres"):
            return m.forward_lowres(image_padded)
        out = m(image_padded)
        return F.interpolate(out, size=image_padded.shape[-2:], mode="bilinear", align_corners=False)

    # ---- train_eval.py:397-417 -------------------------------------------------
    def _run_model_single(self, image: torch.Tensor, flip_h: bool = False, flip_w: bool = False) -> torch.Tensor:
        """image [C,h,w] on the device -> softmax probs [K,h,w]; flip_* mirror the
        probabilities back (the TTA flips of train_eval.py:427-437)."""
        h, w = image.shape[1:]
        h_pad, w_pad = (32 - h % 32) % 32, (32 - w % 32) % 32
        if self.tile is not None and (h + h_pad > self.tile or w + w_pad > self.tile):
            return self._run_model_tiled(image, flip_h, flip_w)
        x = image.unsqueeze(0)
        if h_pad or w_pad:
            x = F.pad(x, (0, w_pad, 0, h_pad), mode="reflect")
        logits = self._logits(x)[0]
        if self.activation == "sigmoid":
            return ops.sigmoid_crop(logits, h, w, flip_h=flip_h, flip_w=flip_w)
        return ops.softmax_crop(logits, h, w, flip_h=flip_h, flip_w=flip_w)

    def _run_model_tiled(self, image: torch.Tensor, flip_h: bool, flip_w: bool) -> torch.Tensor:
        """_run_model_single for a view larger than self.tile: gather tile_batch tiles at a time, forward_lowres
        on the batch into one [N,K,th,tw] buffer, one blend with the activation and the flips."""
        image = image.contiguous().float()
        p = self._tile_plan(*image.shape[1:])
        logits = None
        for first in range(0, p.n, self.tile_batch):
            count = min(self.tile_batch, p.n - first)
            out = self.model.forward_lowres(ops.tile_gather(image, p, first, count))
            if logits is None:
                logits = torch.empty(p.n, out.shape[1], p.th, p.tw, dtype=torch.float32, device=image.device)
            logits[first:first + count].copy_(out)
        return ops.tile_blend(logits, p, self.activation, flip_h=flip_h, flip_w=flip_w)

    # ---- train_eval.py:419-453 -------------------------------------------------
    def _run_tta_inference(self, image: torch.Tensor) -> torch.Tensor:
        image = image.contiguous().float()
        acc = self._run_model_single(image)
        if not self.enable_tta:
            return acc
        h, w = image.shape[1:]
        views = 1 + 2 + len(TTA_SCALES)
        done = 1
        for fh, fw in ((False, True), (True, False)):  # horizontal (dims=[2]) then vertical (dims=[1])
            flipped = ops.resize_bilinear(image, h, w, 1.0, 1.0, flip_h=fh, flip_w=fw)
            p = self._run_model_single(flipped, flip_h=fh, flip_w=fw)
            done += 1
            ops.accumulate(acc, p, 2 if done == views else 1, views)
        for s in TTA_SCALES:
            hs, ws = int(math.floor(h * s)), int(math.floor(w * s))
            scaled = ops.resize_bilinear(image, hs, ws, 1.0 / s, 1.0 / s)
            ps = self._run_model_single(scaled)
            p = ops.resize_bilinear(ps, h, w)
            done += 1
            ops.accumulate(acc, p, 2 if done == views else 1, views)
        return acc

    # ---- train_eval.py:455-568 -------------------------------------------------
    def _convert_probs_to_mask(self, probs: torch.Tensor, h_pad: int = 0, w_pad: int = 0,
                               h_orig: int = None, w_orig: int = None) -> np.ndarray:
        probs = probs.to(self.device)
        if self.activation == "sigmoid":
            mask = ops.probs_threshold(probs, self.threshold)
        else:
            mask = ops.probs_to_mask(probs)
        if h_pad > 0 or w_pad > 0:
            mask = mask[:h_orig, :w_orig]
        return mask.cpu().numpy()

    def predict_probs(self, image: torch.Tensor) -> torch.Tensor:
        """image [C,h,w] -> the probabilities [K,h,w] on the device that predict_semantic_mask converts (the TTA
        mean for 'enhanced_unet', one view otherwise; tiled where the evaluator's tile says so)."""
        self.model.eval()
        with torch.no_grad():
            x = self._prepare_image_tensor(image)
            if self.model_name == "enhanced_unet":
                return self._run_tta_inference(x)
            return self._run_model_single(x)

    def predict_semantic_mask(self, image: torch.Tensor) -> np.ndarray:
        return self._convert_probs_to_mask(self.predict_probs(image))

    def evaluate_semantic(self, dataloader) -> Dict[str, float]:
        """Mean of calculate_semantic_metrics over the images (the semantic rows of evaluate())."""
        acc: Dict[str, list] = {}
        for batch in dataloader:
            for i, item in enumerate(batch["batch_items"]):
                pred = self.predict_semantic_mask(batch["images"][i])
                for k, v in calculate_semantic_metrics(pred, item["semantic_mask"]).items():
                    acc.setdefault(k, []).append(v)
        return {k: float(np.mean(v)) for k, v in acc.items()}

    def evaluate_binary(self, dataloader) -> Dict[str, float]:
        """For a one-logit sigmoid model: the means over the images of metrics.calculate_iou /
        calculate_dice(pred == 1, semantic_mask > 0) as {"bin_iou", "bin_dice"}."""
        if self.activation != "sigmoid":
            raise ValueError("evaluate_binary is the evaluation of a sigmoid model: Evaluator(activation='sigmoid')")
        k = getattr(self.model, "num_classes", None)
        if k != 1:
            raise ValueError(f"evaluate_binary needs a model of one logit (num_classes = 1), this one has {k}")
        ious, dices = [], []
        for batch in dataloader:
            for i, item in enumerate(batch["batch_items"]):
                pred = self.predict_semantic_mask(batch["images"][i])
                gt = item["semantic_mask"]
                gt = gt.cpu().numpy() if isinstance(gt, torch.Tensor) else np.asarray(gt)
                ious.append(calculate_iou(pred == 1, gt > 0))
                dices.append(calculate_dice(pred == 1, gt > 0))
        return {"bin_iou": float(np.mean(ious)) if ious else 0.0, "bin_dice": float(np.mean(dices)) if dices else 0.0}

    # ---- visualization.py:1096-1199, 1819-1900 without the host round trip ---------
    def _bin_scores(self, probs: torch.Tensor, semantic_mask, edges, acc):
        """One image's probabilities [K,h,w] and ground truth into the running (hist, invalid) pair."""
        gt = _dev_long(semantic_mask, probs.device).contiguous()
        return ops.score_hist(probs.contiguous(), gt, edges, out=acc)

    def _curve_result(self, acc, edges, n_cal: int, n_conf: int) -> Dict:
        hist, invalid = acc
        flat = torch.cat([hist.reshape(-1), invalid]).cpu().numpy()  # the one copy to the host
        hist_h = flat[:-1].reshape(tuple(hist.shape))
        result = curve_metrics_from_hist(hist_h, edges, n_cal=n_cal, n_conf=n_conf)
        result.update(invalid=int(flat[-1]), hist=hist_h, edges=edges)
        return result

    def evaluate_curves(self, dataloader, edges=None, tta: bool = True, n_cal: int = 10, n_conf: int = 50) -> Dict:
        """Per-class ROC, PR and calibration statistics over every pixel of the loader:
        metrics.curve_metrics_from_hist's dict ({class name: {fpr, tpr, thresholds, auc, precision, recall,
        ap, auc_resolution, cal_acc, cal_conf, cal_count, ece, conf_hist, ...}}) plus "invalid" (pixels whose
        probability was NaN, infinite or negative), "hist" (the int64 [K, B, 3] histogram) and "edges".

        tta=True bins predict_probs, the probabilities predict_semantic_mask converts; tta=False one
        _run_model_single view, the reference's own definition (train_eval.py:1301-1303), tiled where tile=
        says so.  edges: None for metrics.curve_edges() or a table of its form.  Works for
        activation="sigmoid" as well (one logit: the class "foreground", positive where the mask is >= 1)."""
        edges = curve_edges() if edges is None else np.asarray(edges, dtype=np.float32)
        acc = None
        self.model.eval()
        for batch in dataloader:
            for i, item in enumerate(batch["batch_items"]):
                if tta:
                    probs = self.predict_probs(batch["images"][i])
                else:
                    with torch.no_grad():
                        x = self._prepare_image_tensor(batch["images"][i])
                        probs = self._run_model_single(x.contiguous().float())
                acc = self._bin_scores(probs, item["semantic_mask"], edges, acc)
        if acc is None:
            raise ValueError("evaluate_curves: the loader holds no image")
        return self._curve_result(acc, edges, n_cal, n_conf)

    # ---- visualization.py:1687-1751 and the contour metrics, without the host round trip ---------
    def _predict_mask_device(self, image: torch.Tensor) -> torch.Tensor:
        """predict_semantic_mask's int64 mask [h, w], left on the device."""
        probs = self.predict_probs(image).to(self.device)
        if self.activation == "sigmoid":
            return ops.probs_threshold(probs, self.threshold)
        return ops.probs_to_mask(probs)

    def evaluate_boundary(self, dataloader, tolerances=(1, 2, 3), band_radii=(2,), cap: int = 64,
                          ignore_index: int = 255) -> Dict:
        """Contour metrics over the loader: metrics.boundary_metrics_from_stats' dict ({class name: {nsd,
        boundary_precision, boundary_recall, boundary_f1, hd, hd95, hd95_exceeds_cap, assd, boundary_iou, ...}},
        pooled over the edge pixels of all images, plus the reference's per-image boundary_ious_ref /
        interior_ious_ref lists and their means) and the raw integer buffers "surf", "band" and "refrows" (numpy)
        with "cap" and "band_radii".

        Each image's mask is predicted as predict_semantic_mask predicts it and stays on the device; the
        statistics accumulate there and come back in one copy.  A one-logit sigmoid model is scored on the
        classes background / foreground against the ground truth binarised as evaluate_binary does (gt >= 1,
        ignore_index kept)."""
        one_logit = self.activation == "sigmoid" and getattr(self.model, "num_classes", None) == 1
        names = ("background", "foreground") if one_logit else CLASS_NAMES
        acc = None
        for batch in dataloader:
            for i, item in enumerate(batch["batch_items"]):
                pred = self._predict_mask_device(batch["images"][i])
                gt = _dev_long(item["semantic_mask"], pred.device)
                if one_logit:
                    gt = torch.where(gt == ignore_index, gt, (gt >= 1).long())
                acc = calculate_boundary_stats(pred, gt, num_classes=len(names), ignore_index=ignore_index, cap=cap,
                                               band_radii=band_radii, out=acc)
        if acc is None:
            raise ValueError("evaluate_boundary: the loader holds no image")
        parts = [acc["surf"].reshape(-1), acc["band"].reshape(-1), acc["refrows"].reshape(-1)]
        flat = torch.cat(parts).cpu().numpy()  # the one copy to the host
        cuts = np.cumsum([p.numel() for p in parts])
        host = dict(acc, surf=flat[:cuts[0]].reshape(tuple(acc["surf"].shape)),
                    band=flat[cuts[0]:cuts[1]].reshape(tuple(acc["band"].shape)),
                    refrows=flat[cuts[1]:].reshape(tuple(acc["refrows"].shape)))
        result = boundary_metrics_from_stats(host, tolerances=tolerances, class_names=names)
        result.update(host)
        return result

    # ---- train_eval.py:654-850 -------------------------------------------------
    def _split_large_region(self, region, area: int, final, next_label: int, min_area: int) -> int:
        """The erosion ladder of one region of >= 200 px (train_eval.py:697-785): writes the pieces into
        final (later writes overwrite earlier ones, in stream order) and returns the next free label."""
        def emit(mask, count):
            nonlocal next_label
            if count >= min_area:
                ops.write_label(mask, next_label, final)
                next_label += 1

        def pieces(eroded_labels, n, ksize, iterations, within):
            for sub in range(1, n + 1):
                sub_region, _ = ops.mask_eq(eroded_labels, sub)
                dil, cnt = ops.mask_and(ops.morph_u8(sub_region, ksize, True, iterations), within)
                yield dil, _count(cnt)

        it = max(2, min(area // 1000, 8))
        sub_markers, sub_num, _ = ops.label_components(ops.morph_u8(region, 3, False, it))
        if sub_num > 1:
            for dilated, cnt in pieces(sub_markers, sub_num, 3, it, region):
                if cnt > LARGE_REGION:
                    m2, n2, _ = ops.label_components(ops.morph_u8(dilated, 3, False, 2))
                    if n2 > 1:
                        for d2, c2 in pieces(m2, n2, 3, 2, dilated):
                            emit(d2, c2)
                    else:
                        emit(dilated, cnt)
                else:
                    emit(dilated, cnt)
            return next_label
        eroded = region
        for _ in range(3):
            eroded = ops.morph_u8(eroded, 3, False, 1)
            m, n, _ = ops.label_components(eroded)
            if n > 1:
                for d, c in pieces(m, n, 3, 3, region):
                    emit(d, c)
                return next_label
        m2, n2, _ = ops.label_components(ops.morph_u8(region, 5, False, 3))
        if n2 > 1:
            for d2, c2 in pieces(m2, n2, 5, 3, region):
                emit(d2, c2)
        else:
            emit(region, area)
        return next_label

    def _erosion_ids(self, class_mask, min_area: int) -> tuple:
        """The reference's split of one opened class mask (train_eval.py:686-790): components under 200 px as they
        are, larger ones through the erosion ladder -> (int32 id map, number of ids)."""
        dev = class_mask.device
        markers, num_labels, areas = ops.label_components(class_mask)
        final = torch.zeros_like(markers)
        next_label = 1
        if num_labels:
            areas = areas.cpu().numpy()
            table = np.zeros(num_labels, np.int32)
            for label_id in range(1, num_labels + 1):
                area = int(areas[label_id - 1])
                if area < LARGE_REGION:
                    table[label_id - 1] = next_label
                    next_label += 1
                else:
                    region, _ = ops.mask_eq(markers, label_id)
                    next_label = self._split_large_region(region, area, final, next_label, min_area)
            if table.any():  # every small region in one pass; regions are disjoint components
                ops.relabel_table(markers, ops.upload(table, dev), final)
        return final, next_label - 1

    def _watershed_ids(self, class_mask) -> tuple:
        """The distance-transform watershed of one opened class mask -> (int32 id map, number of ids): every region
        is 8-connected, so outer_perimeter applies to it as it does to the erosion pieces."""
        dist = ops.distance_transform_sq(class_mask.long(), [1], "ne")[0]
        ids, counts, _ = ops.watershed_from_distance(dist, self.split_depth)
        return ids, _count(counts)

    def _select_instances(self, semantic_mask, min_area: int) -> tuple:
        """The selection both semantic_to_instances and semantic_to_instance_maps rest on: per class the 2x2 open, the
        split, the area limits and the score, and the MAX_INSTANCES cut -> (finals {class_id: (the split's int32 id
        map, the number of ids in it)}, entries [(class_id, id in that map, score)] in the order semantic_to_instances returns them, device,
        (h, w))."""
        sem = semantic_mask if isinstance(semantic_mask, torch.Tensor) else \
            torch.from_numpy(np.ascontiguousarray(semantic_mask))
        if sem.dtype not in (torch.int32, torch.int64):
            sem = sem.long()
        dev = sem.device if sem.is_cuda else (self.device if str(self.device) != "cpu" else "cuda")
        sem = sem.to(dev).contiguous()
        finals, entries = {}, []
        for class_id in (1, 2):
            class_mask, cnt = ops.mask_eq(sem, class_id)
            if _count(cnt) == 0:
                continue
            class_mask = ops.morph_u8(ops.morph_u8(class_mask, 2, False), 2, True)  # MORPH_OPEN, 2x2
            if self.split == "watershed":
                final, num_final = self._watershed_ids(class_mask)
            else:
                final, num_final = self._erosion_ids(class_mask, min_area)
            if num_final:
                finals[class_id] = (final, num_final)
                stats = ops.outer_perimeter(final, num_final).cpu().numpy()
                lo, hi = max(MIN_AREA_CLASS[class_id], min_area), MAX_AREA
                for k in range(num_final):
                    n_axis, n_diag, area = (int(v) for v in stats[k, :3])
                    if area < lo or area > hi:
                        continue
                    perimeter = _perimeter(n_axis, n_diag)
                    compactness = 4 * np.pi * area / (perimeter ** 2) if perimeter > 0 else 0.5
                    entries.append((class_id, k + 1, 0.7 * min(area / 150.0, 1.0) + 0.3 * compactness))
            if len(entries) > MAX_INSTANCES:  # inside the class loop, on the combined list (:842-848)
                keep = sorted(range(len(entries)), key=lambda i: entries[i][2], reverse=True)[:MAX_INSTANCES]
                entries = [entries[i] for i in keep]
        return finals, entries, dev, tuple(sem.shape)

    def semantic_to_instances(self, semantic_mask, min_area: int = 3) -> tuple:
        """Semantic mask [h, w] (numpy or tensor; 1 live, 2 dead) -> (instance_masks, instance_labels,
        instance_scores) as the reference returns them; the masks are [h, w] uint8 device tensors (the
        form CellDataset hands out ground truth in), labels 0 live / 1 dead, scores float64."""
        finals, entries, dev, _ = self._select_instances(semantic_mask, min_area)
        plane_of = {}
        for class_id, (final, num_final) in finals.items():
            kept = sorted(k for c, k, _ in entries if c == class_id)
            if not kept:
                continue
            slots = np.full(num_final, -1, np.int32)
            slots[np.asarray(kept) - 1] = np.arange(len(kept), dtype=np.int32)
            planes = ops.expand_labels(final, ops.upload(slots, dev), len(kept))
            plane_of.update({(class_id, k): planes[i] for i, k in enumerate(kept)})
        return ([plane_of[(c, k)] for c, k, _ in entries], [c - 1 for c, _, _ in entries],
                [s for _, _, s in entries])

    def semantic_to_instance_maps(self, semantic_mask, min_area: int = 3) -> tuple:
        """The instances of semantic_to_instances as one id map per class, without a mask plane per instance: (ids
        int32 [2, h, w] on the device, plane 0 live / 1 dead, background 0; counts [n_live, n_dead]; scores [[float64
        per live id], [per dead id]], scores[c][id - 1]).  Within a class the instances are numbered 1.. in ascending
        order of their id in the split's map (ops.relabel_table on that map)."""
        finals, entries, dev, (h, w) = self._select_instances(semantic_mask, min_area)
        ids = torch.zeros(2, h, w, dtype=torch.int32, device=dev)
        counts, scores = [0, 0], [[], []]
        for class_id, (final, num_final) in finals.items():
            kept = sorted((k, s) for c, k, s in entries if c == class_id)
            if not kept:
                continue
            table = np.zeros(num_final, np.int32)  # an entry for every id of the map, as relabel_table requires
            table[np.asarray([k for k, _ in kept]) - 1] = np.arange(1, len(kept) + 1, dtype=np.int32)
            ops.relabel_table(final, ops.upload(table, dev), ids[class_id - 1])
            counts[class_id - 1] = len(kept)
            scores[class_id - 1] = [sc for _, sc in kept]
        return ids, counts, scores

    # ---- label-map instance metrics (no reference counterpart; the size strata are visualization.py:1753-1817) ----
    def _label_map_models_only(self, what: str):
        if self.activation == "sigmoid":
            raise ValueError(f"{what} is not built for sigmoid models (DESIGN.md §7)")
        if getattr(self.model, "dual_branch", False):
            raise ValueError(f"{what} is not built for the dual-branch model (DESIGN.md §7)")

    def _gt_instance_maps(self, item, shape, dev) -> tuple:
        """A dataset item's instance_masks / instance_labels -> (int32 [2, h, w] id maps, -1 where semantic_mask is
        255; the pixels more than one instance of a class claims).  Instance j of the item has id j + 1."""
        masks, labels = item["instance_masks"], [int(l) for l in item["instance_labels"]]
        sem = _dev_long(item["semantic_mask"], dev).contiguous()
        if tuple(sem.shape) != tuple(shape):
            raise ValueError(f"semantic_mask is {tuple(sem.shape)}, the prediction {tuple(shape)}")
        ignore, _ = ops.mask_eq(sem, 255)
        stack = _stack_masks(masks, dev) if len(labels) else torch.zeros((0,) + tuple(shape), dtype=torch.uint8,
                                                                         device=dev)
        planes, overlap = [], 0
        for cid in range(len(INSTANCE_CLASSES)):
            ids = [j + 1 if l == cid else 0 for j, l in enumerate(labels)]
            plane, over = ops.labels_from_stack(stack, ids, ignore)
            planes.append(plane)
            overlap += over
        return torch.stack(planes), overlap

    def evaluate_panoptic(self, dataloader, iou_percent=PANOPTIC_IOU_PERCENT, min_area: int = 3) -> Dict[str, float]:
        """Panoptic Quality, AJI, object Dice, SEG and the F1 / average-precision sweep of the predicted instances
        (predict_semantic_mask on the device, then semantic_to_instance_maps) against the items' instance_masks /
        instance_labels, pixels whose semantic_mask is 255 ignored: metrics.panoptic_metrics_from_stats of the
        statistics pooled over the loader (PANOPTIC_KEYS for the default thresholds), plus aji_image_mean (the mean
        of the per-image AJI, both classes pooled, over the images that have a ground truth or a prediction: the
        MoNuSeg convention) and gt_overlap_pixels (ground-truth pixels that more than one instance of a class
        claims, where the id map keeps the later instance only).  Per image: one contingency table of the two class
        planes (ops.label_pairs); no mask plane is expanded on the prediction side."""
        self._label_map_models_only("evaluate_panoptic")
        stats, image_aji, overlap = None, [], 0
        for batch in dataloader:
            for i, item in enumerate(batch["batch_items"]):
                pred_ids, _, _ = self.semantic_to_instance_maps(self._predict_mask_device(batch["images"][i]), min_area)
                gt_ids, over = self._gt_instance_maps(item, pred_ids.shape[1:], pred_ids.device)
                overlap += over
                st = instance_stats_from_pairs(ops.label_pairs(pred_ids, gt_ids), len(INSTANCE_CLASSES), iou_percent)
                if int(st["n_pred"].sum()) + int(st["n_gt"].sum()) > 0:
                    image_aji.append(int(st["aji_c"].sum()) / int(st["aji_u"].sum()))
                stats = add_instance_stats(stats, st)
        if stats is None:
            raise ValueError("evaluate_panoptic: the loader holds no image")
        result = panoptic_metrics_from_stats(stats, INSTANCE_CLASSES, iou_percent)
        result["aji_image_mean"] = float(np.mean(image_aji)) if image_aji else float("nan")
        result["gt_overlap_pixels"] = overlap
        return result

    # ---- per-cell measurements (no reference counterpart) ------------------------------------------------
    def measure_cells(self, image: torch.Tensor, intensity=None, min_area: int = 3, pixel_size: float = 1.0,
                      hull: bool = False) -> Dict:
        """The measurements of every predicted cell of one image: the mask is predicted on the device
        (predict_semantic_mask's), split into semantic_to_instance_maps' id maps, and one ops.cell_stats call on the
        [2, h, w] ids gives the integer tables -> {"live": m, "dead": m, "n_live", "n_dead", "viability": n_live /
        (n_live + n_dead), 0.0 without a cell}, m = metrics.cell_measurements' dict of the class plus "score", the
        instance scores.  intensity: None (geometry only) or the caller's uint8 [h, w] / [h, w, c] image (c <= 3,
        numpy or tensor) at the mask's size, whose per-cell mean_<ch>, std_<ch>, min_<ch>, max_<ch> are added.
        hull=True adds metrics.hull_measurements' keys (convex area, solidity, the Feret diameters, ...) from one
        ops.cell_hulls call on the same ids."""
        self._label_map_models_only("measure_cells")
        ids, counts, scores = self.semantic_to_instance_maps(self._predict_mask_device(image), min_area)
        if intensity is not None:
            if not isinstance(intensity, torch.Tensor):
                intensity = ops.upload(np.ascontiguousarray(intensity), ids.device)
            elif not intensity.is_cuda:
                intensity = intensity.to(ids.device)
        stats = ops.cell_stats(ids, max(counts), intensity)
        hulls = ops.cell_hulls(ids, stats) if hull else None
        out: Dict = {}
        for plane, name in enumerate(INSTANCE_CLASSES):
            m = cell_measurements(stats, plane, pixel_size)
            if hulls is not None:
                m.update(hull_measurements(hulls, stats, plane, pixel_size))
            m = {k: v[:counts[plane]] for k, v in m.items()}  # the table has max(counts) rows for both classes
            m["score"] = np.asarray(scores[plane], np.float64)
            out[name] = m
        n_live, n_dead = int(counts[0]), int(counts[1])
        out.update(n_live=n_live, n_dead=n_dead, viability=n_live / (n_live + n_dead) if n_live + n_dead else 0.0)
        return out

    def measure_neighbors(self, image: torch.Tensor, distance=None, min_area: int = 3, pixel_size: float = 1.0,
                          connectivity: int = 4) -> Dict:
        """What the predicted cells of one image are to each other: semantic_to_instance_maps' [2, h, w] ids are pooled
        into one plane (live ids 1..n_live, dead ids n_live + 1..n_live + n_dead: the class planes are disjoint by
        construction), the plane is grown by `distance` pixels, or to the Voronoi partition of the image when distance
        is None (ops.expand_label_map), and the grown map's contact table (ops.label_contacts) and the ops.cell_stats
        tables of both maps go through metrics.neighbor_measurements -> {"live": m, "dead": m, "n_live", "n_dead",
        "graph": metrics.neighbor_graph's CSR arrays over the pooled ids}, m = the measurement dict restricted to the
        class plus "n_neighbors_same_class".  first_closest_id / second_closest_id are pooled ids."""
        self._label_map_models_only("measure_neighbors")
        if connectivity not in (4, 8):
            raise ValueError(f"measure_neighbors: connectivity must be 4 or 8, got {connectivity!r}")
        ids, counts, _ = self.semantic_to_instance_maps(self._predict_mask_device(image), min_area)
        n_live, n_dead = int(counts[0]), int(counts[1])
        n = n_live + n_dead
        pooled = (ids[0] + torch.where(ids[1] > 0, ids[1] + n_live, torch.zeros_like(ids[1]))).contiguous()
        grown = ops.expand_label_map(pooled, distance)
        contacts = ops.label_contacts(grown, connectivity)
        m = neighbor_measurements(contacts, ops.cell_stats(pooled, n), ops.cell_stats(grown, n), 0, pixel_size)
        indptr, indices, weights = neighbor_graph(contacts, 0, n)
        owner = np.repeat(np.arange(n), np.diff(indptr))
        same = np.bincount(owner[(owner < n_live) == (indices - 1 < n_live)], minlength=n)[:n].astype(np.float64)
        m["n_neighbors_same_class"] = same
        return {"live": {k: v[:n_live] for k, v in m.items()}, "dead": {k: v[n_live:] for k, v in m.items()},
                "n_live": n_live, "n_dead": n_dead, "graph": (indptr, indices, weights)}

    def evaluate_measurements(self, dataloader, min_area: int = 3) -> Dict[str, float]:
        """How the measurements of the predicted cells agree with the ground truth's over the loader: per item the
        predicted id maps (as evaluate_panoptic forms them) and _gt_instance_maps' go through ops.cell_stats each and
        ops.label_pairs together; a predicted and a ground-truth cell are matched at IoU > 1 / 2
        (metrics.measurement_agreement) -> metrics.AGREEMENT_KEYS per class, "<key>_live" and "<key>_dead":
        n_matched, area_rel_err_mean, area_rel_err_median, area_bias, centroid_dist_mean (pixels), count_pred,
        count_gt, mean_area_pred, mean_area_gt."""
        self._label_map_models_only("evaluate_measurements")
        parts = [[] for _ in INSTANCE_CLASSES]
        seen = False
        for batch in dataloader:
            for i, item in enumerate(batch["batch_items"]):
                seen = True
                pred_ids, counts, _ = self.semantic_to_instance_maps(self._predict_mask_device(batch["images"][i]),
                                                                     min_area)
                gt_ids, _ = self._gt_instance_maps(item, pred_ids.shape[1:], pred_ids.device)
                geom_pred = ops.cell_stats(pred_ids, max(counts))["geom"]
                geom_gt = ops.cell_stats(gt_ids, len(item["instance_labels"]))["geom"]
                pairs = ops.label_pairs(pred_ids, gt_ids)
                for plane in range(len(INSTANCE_CLASSES)):
                    parts[plane].append(measurement_agreement(pairs, geom_pred, geom_gt, plane))
        if not seen:
            raise ValueError("evaluate_measurements: the loader holds no image")
        result = {}
        for plane, name in enumerate(INSTANCE_CLASSES):
            result.update({f"{k}_{name}": v for k, v in agreement_summary(parts[plane]).items()})
        assert set(result) == {f"{k}_{c}" for k in AGREEMENT_KEYS for c in INSTANCE_CLASSES}
        return result

    def evaluate_by_size(self, dataloader, edges=SIZE_EDGES, class_names=CLASS_NAMES) -> Dict:
        """visualization.py:1753-1817 (plot_size_based_performance) without the host round trip: for every class,
        background included, the 4-connected components of the ground truth (ops.label_components(gt == c,
        connectivity=4): scipy.ndimage.label's default) and, per object, the fraction of its pixels the prediction
        gives the same class, binned by object area -> {"edges", "coverage": a list per bin [0, e0), [e0, e1), ...,
        [e_last, inf) in the reference's order (image, class, object), "count", "mean" (NaN for an empty bin)}.
        A 255 pixel belongs to no ground-truth object.  The component ids go through ops.label_pairs, whose ids end at
        2^24 - 1: a class mask with more components than that (a noise mask beyond 4096 x 4096) raises ValueError."""
        self._label_map_models_only("evaluate_by_size")
        edges = tuple(int(e) for e in edges)
        bins = [[] for _ in range(len(edges) + 1)]
        for batch in dataloader:
            for i, item in enumerate(batch["batch_items"]):
                pred = self._predict_mask_device(batch["images"][i]).contiguous()
                gt = _dev_long(item["semantic_mask"], pred.device).contiguous()
                comps, same = [], []
                for c in range(len(class_names)):
                    labels, n, _ = ops.label_components(ops.mask_eq(gt, c)[0], connectivity=4)
                    if n > ops.PAIRS_MAX_ID:
                        raise ValueError(f"evaluate_by_size: the ground truth's class {c} has {n} components, the "
                                         f"pair table's ids end at {ops.PAIRS_MAX_ID}")
                    comps.append(labels)
                    same.append(ops.mask_eq(pred, c)[0])
                pairs = ops.label_pairs(torch.stack(comps), torch.stack(same).to(torch.int32))
                for b, cov in zip(bins, size_strata_from_pairs(pairs, edges)):
                    b.extend(cov)
        return {"edges": edges, "coverage": bins, "count": [len(b) for b in bins],
                "mean": [float(np.mean(b)) if b else float("nan") for b in bins]}

    # ---- train_eval.py:852-1021 ------------------------------------------------
    def evaluate(self, dataloader, coco_map: bool = False) -> Dict[str, float]:
        """Mean over the images of the semantic, instance and viability rows, with the reference's keys
        (a key that collected nothing gives 0.0).  coco_map=True adds COCO_KEYS (bbox_mAP, segm_mAP:
        COCOeval stats[0] over all images, metrics.calculate_coco_metrics' value): per image the matching
        runs on the device and only scores, match tables and ground-truth counts are kept, accumulated once
        at the end.  Without the flag those keys are left out of the dict."""
        return self._evaluate(dataloader, coco_map, False)

    def evaluate_with_curves(self, dataloader, coco_map: bool = False) -> Dict[str, float]:
        """evaluate()'s dict plus auc_<class>, ap_<class> and ece_<class> (CURVE_KEYS for three classes;
        evaluate_curves' values with tta=True) from the same forward: the probabilities are predicted once,
        binned and converted.  A method of its own because evaluate's signature is the reference's plus
        coco_map and is pinned as such."""
        return self._evaluate(dataloader, coco_map, True)

    def _evaluate(self, dataloader, coco_map: bool, curves: bool) -> Dict[str, float]:
        acc: Dict[str, list] = {k: [] for k in EVALUATE_KEYS}
        coco_bbox, coco_segm = [], []
        n_pred = n_gt = 0  # over all images; ground-truth ids are the running positions (metrics.py:240-242)
        orphan = False  # predictions on an image without ground truth: COCO.loadRes refuses them
        edges = curve_edges() if curves else None
        hist = None

        def collect(metrics):
            for k, v in metrics.items():
                if k in acc:
                    acc[k].append(v)

        for batch in dataloader:
            for i, item in enumerate(batch["batch_items"]):
                gt_masks, gt_labels = item["instance_masks"], item["instance_labels"]
                if curves:  # predict_semantic_mask's two steps, with the probabilities binned in between
                    probs = self.predict_probs(batch["images"][i])
                    hist = self._bin_scores(probs, item["semantic_mask"], edges, hist)
                    pred = self._convert_probs_to_mask(probs)
                else:
                    pred = self.predict_semantic_mask(batch["images"][i])
                collect(calculate_semantic_metrics(pred, item["semantic_mask"]))
                masks, labels, scores = self.semantic_to_instances(pred)
                collect(calculate_instance_metrics(masks, labels, scores, gt_masks, gt_labels))
                collect(calculate_viability_metrics(sum(1 for l in labels if l == 0), sum(1 for l in labels if l == 1),
                                                    sum(1 for l in gt_labels if l == 0),
                                                    sum(1 for l in gt_labels if l == 1)))
                if coco_map:  # the image id is the running counter of train_eval.py:898: one entry per image
                    if len(gt_labels) == 0:
                        orphan = orphan or len(labels) > 0
                    else:
                        eb, es = coco_image_matches(masks, labels, scores, gt_masks, gt_labels,
                                                    range(n_gt, n_gt + len(gt_labels)))
                        coco_bbox.append(eb)
                        coco_segm.append(es)
                    n_pred += len(labels)
                    n_gt += len(gt_labels)
        result = {k: (np.mean(v) if v else 0.0) for k, v in acc.items()}
        if coco_map:
            result.update({k: 0.0 for k in COCO_KEYS})
            if orphan and n_gt:
                warnings.warn("evaluate: predictions on an image without ground truth; the reference's "
                              "COCO.loadRes refuses such results, so bbox_mAP and segm_mAP are 0.0")
            elif n_pred and n_gt:
                result["bbox_mAP"] = coco_map_from_matches(coco_bbox)
                result["segm_mAP"] = coco_map_from_matches(coco_segm)
        if curves and hist is not None:
            for name, m in curve_metrics_from_hist(hist[0], edges).items():
                result.update({f"{s}_{name}": m[s] for s in CURVE_STATS})
        return result
