"""A plain-loop numpy restatement of pycocotools' COCOeval for stats[0] (AP@[.50:.95], all areas, 100
detections), written from the published cocoeval.py / coco.py / maskApi.c, independently of the product
code: nothing is imported from eunet.  It is slow on purpose (Python triple loops) and is the yardstick of
tests/test_coco_host.py and tests/test_gpu_coco.py.

Annotations are the reference's dicts (image_id, category_id, score) with 'segmentation' a [h, w] numpy
mask; the box is cv2.boundingRect of the mask, ground-truth ids are list positions (metrics.py:240-242).
"""
import numpy as np

CAT_IDS = [0, 1]
MAX_DET = 100
IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)


def bounding_rect(mask):
    """cv2.boundingRect of a mask: (x, y, w, h) of the non-zero pixels."""
    ys, xs = np.nonzero(np.asarray(mask))
    if len(ys) == 0:
        raise ValueError("empty mask")
    return int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)


def bbox_iou(d, g):
    """maskApi.c bbIou of two (x, y, w, h) boxes, iscrowd = 0."""
    w = min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0])
    h = min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1])
    if w <= 0 or h <= 0:
        return 0.0
    i = float(w) * float(h)
    u = float(d[2]) * float(d[3]) + float(g[2]) * float(g[3]) - i
    return i / u


def segm_iou_counts(inter, area_d, area_g):
    """maskApi.c rleIou from pixel counts: intersection over union, 0 without intersection."""
    inter, area_d, area_g = int(inter), int(area_d), int(area_g)
    if inter == 0:
        return 0.0
    return float(inter) / float(area_d + area_g - inter)


def segm_iou(md, mg):
    md, mg = np.asarray(md) != 0, np.asarray(mg) != 0
    return segm_iou_counts(np.logical_and(md, mg).sum(), md.sum(), mg.sum())


def evaluate_img(ious, thrs=IOU_THRS):
    """COCOeval.evaluateImg's matching for one image and one category, no crowd, no ignore.  ious [D][G]
    with the detections already in visiting order.  Returns dtm [T][D]: the index of the ground truth each
    detection takes, or -1."""
    D = len(ious)
    G = len(ious[0]) if D else 0
    T = len(thrs)
    dtm = [[-1] * D for _ in range(T)]
    for tind in range(T):
        t = thrs[tind]
        gtm = [False] * G
        for dind in range(D):
            iou = min([t, 1 - 1e-10])
            m = -1
            for gind in range(G):
                if gtm[gind]:
                    continue
                if ious[dind][gind] < iou:
                    continue
                iou = ious[dind][gind]
                m = gind
            if m == -1:
                continue
            dtm[tind][dind] = m
            gtm[m] = True
    return dtm


def visit_order(scores):
    """Stable sort by descending score, cut at MAX_DET."""
    return [int(i) for i in np.argsort([-s for s in scores], kind="mergesort")][:MAX_DET]


def match_image(dts, gts, iou_type):
    """One image: per category (scores in visiting order, dtm [T][d] of GLOBAL ground-truth ids or -1,
    number of ground truths), or None where the category has neither.  dts: (score, category, mask);
    gts: (global id, category, mask)."""
    out = []
    for cat in CAT_IDS:
        gt = [g for g in gts if g[1] == cat]
        dt = [d for d in dts if d[1] == cat]
        if len(gt) == 0 and len(dt) == 0:
            out.append(None)
            continue
        dt = [dt[i] for i in visit_order([d[0] for d in dt])]
        if iou_type == "bbox":
            gb = [bounding_rect(g[2]) for g in gt]
            db = [bounding_rect(d[2]) for d in dt]
            ious = [[bbox_iou(a, b) for b in gb] for a in db]
        else:
            ious = [[segm_iou(d[2], g[2]) for g in gt] for d in dt]
        if len(gt) == 0:
            ious = [[] for _ in dt]
        dtm = evaluate_img(ious)
        ids = [[(gt[m][0] if m >= 0 else -1) for m in row] for row in dtm]
        out.append(([d[0] for d in dt], ids, len(gt)))
    return out


def accumulate_summarize(per_image):
    """COCOeval.accumulate + summarize(ap=1, iouThr=None, areaRng='all', maxDets=100).  per_image: the
    match_image results in image order.  A match id is tested for truth, as pycocotools tests dtm."""
    T, R, K = len(IOU_THRS), len(REC_THRS), len(CAT_IDS)
    precision = -np.ones((T, R, K))
    for k in range(K):
        E = [img[k] for img in per_image if img[k] is not None]
        if len(E) == 0:
            continue
        scores = np.array([s for e in E for s in e[0][:MAX_DET]], dtype=np.float64)
        inds = np.argsort(-scores, kind="mergesort")
        npig = sum(e[2] for e in E)
        if npig == 0:
            continue
        for t in range(T):
            ids = [m for e in E for m in e[1][t][:MAX_DET]]
            ids = [ids[i] for i in inds]
            tp_run, fp_run = 0, 0
            tp, fp = [], []
            for m in ids:
                if m > 0:        # -1: unmatched; 0: the ground truth of id 0, falsy in pycocotools
                    tp_run += 1
                else:
                    fp_run += 1
                tp.append(float(tp_run))
                fp.append(float(fp_run))
            nd = len(tp)
            rc = [x / npig for x in tp]
            pr = [a / (b + a + np.spacing(1)) for a, b in zip(tp, fp)]
            q = [0.0] * R
            for i in range(nd - 1, 0, -1):
                if pr[i] > pr[i - 1]:
                    pr[i - 1] = pr[i]
            at = np.searchsorted(np.array(rc, dtype=np.float64), REC_THRS, side="left")
            try:
                for ri, pi in enumerate(at):
                    q[ri] = pr[pi]
            except IndexError:
                pass
            precision[t, :, k] = np.array(q)
    s = precision[precision > -1]
    return -1.0 if len(s) == 0 else float(np.mean(s))


def per_image_matches(pred_annotations, gt_annotations, iou_type):
    """The match_image results of every image (sorted unique ground-truth image_ids), or None when a
    prediction sits on an image without ground truth (COCO.loadRes asserts)."""
    img_ids = sorted(set(a["image_id"] for a in gt_annotations))
    for a in pred_annotations:
        if a["image_id"] not in img_ids:
            return None
    out = []
    for iid in img_ids:
        gts = [(i, int(a["category_id"]), np.asarray(a["segmentation"]))
               for i, a in enumerate(gt_annotations) if a["image_id"] == iid]
        dts = [(float(a["score"]), int(a["category_id"]), np.asarray(a["segmentation"]))
               for a in pred_annotations if a["image_id"] == iid]
        out.append(match_image(dts, gts, iou_type))
    return out


def coco_metrics(pred_annotations, gt_annotations):
    """metrics.py:197-301 with masks in place of RLEs."""
    res = {"bbox_mAP": 0.0, "segm_mAP": 0.0}
    if not pred_annotations or not gt_annotations:
        return res
    for key, ty in (("bbox_mAP", "bbox"), ("segm_mAP", "segm")):
        per = per_image_matches(pred_annotations, gt_annotations, ty)
        if per is None:
            return {"bbox_mAP": 0.0, "segm_mAP": 0.0}
        res[key] = accumulate_summarize(per)
    return res
