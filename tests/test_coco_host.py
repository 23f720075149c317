"""Host side of the COCO mAP (no GPU): eunet.metrics.coco_map_from_matches (COCOeval.accumulate + summarize
for stats[0]) against the plain-loop restatement of tests/_coco_ref.py and against answers worked out by
hand, and the new entry points' declaration, binding and public surface.

Tolerance 1e-12: the values lie in [0, 1], the mean has 2020 terms (10 thresholds x 101 recall points x 2
classes) and float64 eps is 1.1e-16, so rounding stays below 2.3e-13."""
import inspect
import os
import re

import numpy as np
import pytest

import _coco_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12
NEW_SYMBOLS = ("eunet_pack_masks_bbox", "eunet_coco_match")


def _as_entries(per_image):
    """The restatement's per-image matches -> coco_map_from_matches' input (a class with neither detections
    nor ground truth is an empty entry)."""
    out = []
    for img in per_image:
        out.append(tuple((np.zeros(0), np.full((len(R.IOU_THRS), 0), -1, np.int64), 0) if e is None else
                         (np.asarray(e[0], np.float64), np.asarray(e[1], np.int64).reshape(len(R.IOU_THRS), -1), e[2])
                         for e in img))
    return out


def _host_map(preds, gts, iou_type):
    from eunet.metrics import coco_map_from_matches
    return coco_map_from_matches(_as_entries(R.per_image_matches(preds, gts, iou_type)))


def test_coco_map_from_matches_against_the_restatement():
    """The restatement produces the matches of the seeded three-image recipe (tests/test_gpu_coco.py); the
    product's accumulate must give the restatement's value on them, for both IoU types."""
    from test_gpu_coco import make_case
    preds, gts = make_case()
    ref = R.coco_metrics(preds, gts)
    assert 0.05 < ref["bbox_mAP"] < 0.95 and 0.05 < ref["segm_mAP"] < 0.95 and ref["bbox_mAP"] != ref["segm_mAP"]
    for key, ty in (("bbox_mAP", "bbox"), ("segm_mAP", "segm")):
        got = _host_map(preds, gts, ty)
        assert abs(got - ref[key]) <= TOL, (key, got, ref[key])
    # a subset that leaves class 1 without ground truth on some images and changes every cut
    sub_p, sub_g = preds[::3], gts[1::2]
    for key, ty in (("bbox_mAP", "bbox"), ("segm_mAP", "segm")):
        assert abs(_host_map(sub_p, sub_g, ty) - R.coco_metrics(sub_p, sub_g)[key]) <= TOL


# ---- known answers: one image; A = (0, 0, 10, 10), B = (20, 0, 10, 10), C = (50, 50, 4, 4) as x, y, w, h
def _rect(x, y, w, h):
    m = np.zeros((64, 64), np.uint8)
    m[y:y + h, x:x + w] = 1
    return m


A, B, C = _rect(0, 0, 10, 10), _rect(20, 0, 10, 10), _rect(50, 50, 4, 4)


def _gt(mask, cat, image_id=0):
    return {"image_id": image_id, "category_id": cat, "segmentation": mask}


def _dt(mask, cat, score, image_id=0):
    return {"image_id": image_id, "category_id": cat, "score": score, "segmentation": mask}


def _both(preds, gts):
    """The restatement's value and the product's accumulate on the restatement's matches, per IoU type
    (full rectangles: bbox and segm IoU coincide)."""
    ref = R.coco_metrics(preds, gts)
    return [(ref[key], _host_map(preds, gts, ty)) for key, ty in (("bbox_mAP", "bbox"), ("segm_mAP", "segm"))]


def test_known_answer_k1_ground_truth_id_0_is_a_false_positive():
    # Ground truth [A (id 0), B (id 1)], class 0; detections B@.9, A@.8, both IoU 1 with their own box, so both
    # match at all ten thresholds.  Visiting order B, A: dtm = [1, 0].  Id 0 is falsy: tp = [1, 0], fp = [0, 1];
    # cumulative tp = [1, 1], fp = [0, 1]; npig = 2: rc = [.5, .5], pr = [1, .5] (the envelope changes nothing).
    # searchsorted(rc, r, 'left') = 0 for r <= .5 -> precision 1 at the 51 recall points 0, .01, ..., .50, and
    # 2 (past the end) for the other 50 -> 0.  Class 1 has neither ground truth nor detections: excluded.
    # Every threshold gives 51 / 101, and so does the mean.
    for ref, got in _both([_dt(B, 0, .9), _dt(A, 0, .8)], [_gt(A, 0), _gt(B, 0)]):
        assert abs(ref - 51 / 101) <= TOL and abs(got - 51 / 101) <= TOL


def test_known_answer_k2_class_with_ground_truth_and_no_detection():
    # Ground truth [C class 1 (id 0), A class 0 (id 1), B class 0 (id 2)], detections B@.9, A@.8 of class 0.
    # Class 0: dtm = [2, 1], both truthy: tp cum = [1, 2], fp = [0, 0], rc = [.5, 1], pr = [1, 1]: precision 1
    # at all 101 recall points -> AP 1.  Class 1: npig = 1 and no detection: every recall point is past the
    # end and keeps 0 -> AP 0.  Mean over 2 x 10 x 101 entries = 0.5.
    for ref, got in _both([_dt(B, 0, .9), _dt(A, 0, .8)], [_gt(C, 1), _gt(A, 0), _gt(B, 0)]):
        assert abs(ref - 0.5) <= TOL and abs(got - 0.5) <= TOL


def test_known_answer_k3_partial_overlap_and_id_0():
    # Ground truth as K2; detections B@.9 (class 0), (0, 0, 10, 6)@.8 (class 0), C@.5 (class 1).
    # Class 0: B matches id 2 at all ten thresholds.  (0,0,10,6) against A: 60 / 100 = 0.6, which reaches the
    # thresholds .5, .55 and .6 (three of ten).  There: tp cum = [1, 2], rc = [.5, 1], pr = [1, 1] -> 101 ones.
    # At the other seven: tp cum = [1, 1], fp cum = [0, 1], rc = [.5, .5], pr = [1, .5] -> 51 ones (as K1).
    # Class 1: C matches id 0 -> a false positive: tp = [0], rc = [0], pr = [0]: searchsorted gives 0 for
    # r = 0 (precision 0) and 1, past the end, for the rest -> all 0.
    # Sum = 3 * 101 + 7 * 51 = 660 over 2020 entries = 33 / 101.
    assert sum(1 for t in R.IOU_THRS if 60 / 100 >= min(t, 1 - 1e-10)) == 3
    preds = [_dt(B, 0, .9), _dt(_rect(0, 0, 10, 6), 0, .8), _dt(C, 1, .5)]
    for ref, got in _both(preds, [_gt(C, 1), _gt(A, 0), _gt(B, 0)]):
        assert abs(ref - 33 / 101) <= TOL and abs(got - 33 / 101) <= TOL


def test_known_answer_k4_prediction_on_an_image_without_ground_truth():
    # COCO.loadRes asserts that every result's image is one of the ground truth's images; the reference's
    # except then returns the zeros it started from.
    ref = R.coco_metrics([_dt(A, 0, .9, image_id=5)], [_gt(A, 0, image_id=0)])
    assert ref == {"bbox_mAP": 0.0, "segm_mAP": 0.0}
    assert R.per_image_matches([_dt(A, 0, .9, image_id=5)], [_gt(A, 0, image_id=0)], "bbox") is None


def test_coco_map_from_matches_rules():
    from eunet.metrics import COCO_IOU_THRS, COCO_REC_THRS, coco_map_from_matches
    assert np.array_equal(COCO_IOU_THRS, R.IOU_THRS) and np.array_equal(COCO_REC_THRS, R.REC_THRS)
    T = len(COCO_IOU_THRS)
    none = (np.zeros(0), np.full((T, 0), -1, np.int64), 0)
    assert coco_map_from_matches([]) == -1.0 and coco_map_from_matches([(none, none)]) == -1.0
    # detections only (npig == 0): the class stays -1 and is excluded
    only_dt = ([0.5], np.full((T, 1), -1, np.int64), 0)
    assert coco_map_from_matches([(only_dt, none)]) == -1.0
    # K1 from hand-written tables; scores tie across images: the stable sort keeps the image order
    k1 = ([0.9, 0.8], np.tile(np.array([[1, 0]]), (T, 1)), 2)
    assert abs(coco_map_from_matches([(k1, none)]) - 51 / 101) <= TOL
    a = ([0.5], np.full((T, 1), -1, np.int64), 1)          # image 0: a miss, visited first on the tie
    b = ([0.5], np.full((T, 1), 1, np.int64), 0)           # image 1: a hit
    # tp cum = [0, 1], fp cum = [1, 1]: rc = [0, 1], pr = [0, .5] -> envelope [.5, .5]: AP .5
    assert abs(coco_map_from_matches([(a, none), (b, none)]) - 0.5) <= TOL
    assert abs(coco_map_from_matches([(b, none), (a, none)]) - 1.0) <= TOL


def test_coco_symbols_declared_bound_and_exported():
    from eunet import _lib
    src = open(os.path.join(ROOT, "include", "eunet.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int\s+" + name + r"\s*\(", src, flags=re.M), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert name in _lib.exported_symbols()
    for cite in ("train_eval.py:959, 978", "train_eval.py:951-992", "metrics.py:283-294"):
        assert cite in src, cite


def test_coco_public_surface():
    from eunet import metrics, ops
    from eunet.evaluator import COCO_KEYS, EVALUATE_KEYS, Evaluator
    sig = inspect.signature(Evaluator.evaluate)
    assert list(sig.parameters) == ["self", "dataloader", "coco_map"] and sig.parameters["coco_map"].default is False
    assert COCO_KEYS == ("bbox_mAP", "segm_mAP") and not set(EVALUATE_KEYS) & set(COCO_KEYS)
    assert len(EVALUATE_KEYS) == 23
    assert list(inspect.signature(metrics.calculate_coco_metrics).parameters) == ["pred_annotations", "gt_annotations"]
    assert hasattr(ops, "pack_masks_bbox") and hasattr(ops, "coco_match")
    # the empty sides need no device
    zeros = {"bbox_mAP": 0.0, "segm_mAP": 0.0}
    assert metrics.calculate_coco_metrics([], [_gt(A, 0)]) == zeros
    assert metrics.calculate_coco_metrics([_dt(A, 0, .9)], []) == zeros
    with pytest.warns(UserWarning):     # K4 through the public function: no launch is needed to refuse it
        assert metrics.calculate_coco_metrics([_dt(A, 0, .9, image_id=5)], [_gt(A, 0, image_id=0)]) == zeros
