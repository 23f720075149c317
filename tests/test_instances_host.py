"""Host side of the instance-level evaluation (no GPU): the greedy matching from integer count matrices
and the viability function reproduce the reference's recorded dicts bit for bit
(tests/golden/instances.npz, written by tests/golden/gen_golden_instances.py), and the new C-ABI entry
points are declared, bound and exported."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("eunet_pack_masks", "eunet_pairwise_overlap", "eunet_morph_u8", "eunet_label_workspace_bytes",
               "eunet_label_components", "eunet_outer_perimeter", "eunet_mask_eq", "eunet_mask_and",
               "eunet_write_label", "eunet_relabel_table", "eunet_expand_labels")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "instances.npz"))


def _numpy_counts(pred, gt):
    """(inter [P, G], area_p, area_g) of uint8 mask stacks, the way the reference counts (metrics.py:14)."""
    inter = np.array([[np.logical_and(p, g).sum() for g in gt] for p in pred], np.int64).reshape(len(pred), len(gt))
    return inter, pred.sum(axis=(1, 2)).astype(np.int64), gt.sum(axis=(1, 2)).astype(np.int64)


def test_match_from_counts_reproduces_recorded_dicts(golden):
    from eunet.metrics import instance_metrics_from_counts, match_from_counts
    assert int(golden["m_n"]) >= 9
    saw_extra = False
    for i in range(int(golden["m_n"])):
        pred, gt = golden[f"m{i}_pred"], golden[f"m{i}_gt"]
        pl, gl, sc = golden[f"m{i}_pred_labels"], golden[f"m{i}_gt_labels"], golden[f"m{i}_scores"]
        thr = float(golden[f"m{i}_thr"])
        per_class = []
        for cid in (0, 1):
            if not (gl == cid).any():
                per_class.append(None)
                continue
            inter, ap, ag = _numpy_counts(pred[pl == cid], gt[gl == cid])
            per_class.append((inter, ap, ag, [float(s) for s in sc[pl == cid]]))
        got = instance_metrics_from_counts(per_class, thr)
        assert sorted(got) == list(golden[f"m{i}_keys"]), i
        for k, v in zip(golden[f"m{i}_keys"], golden[f"m{i}_vals"]):
            assert float(got[str(k)]) == v, (i, k, got[str(k)], v)
        saw_extra |= "live_avg_iou_below_threshold" in got
        for cid, name in enumerate(("live", "dead")):  # the per-class function carries the same numbers
            if per_class[cid] is not None:
                one = match_from_counts(*per_class[cid], thr=thr)
                assert all(float(got[f"{name}_{k}"]) == float(v) for k, v in one.items())
    assert saw_extra


def test_match_from_counts_rules():
    from eunet.metrics import match_from_counts
    # equal IoU: the first ground truth wins; union 0 counts as IoU 1.0; a class without ground truth is an error
    m = match_from_counts(np.array([[8, 8]]), [16], [16, 16], [0.5])
    assert m["iou"] == 8 / 24 and m["precision"] == 1.0 and m["recall"] == 0.5 and m["ap"] == 0.5
    assert match_from_counts(np.zeros((1, 1), np.int64), [0], [0], [0.1])["iou"] == 1.0
    assert match_from_counts(np.zeros((0, 2), np.int64), [], [3, 4], []) == \
        {"iou": 0.0, "precision": 0.0, "recall": 0.0, "ap": 0.0}
    with pytest.raises(ValueError):
        match_from_counts(np.zeros((1, 0), np.int64), [1], [], [0.5])


def test_viability_metrics_bit_exact(golden):
    from eunet.metrics import calculate_viability_metrics
    keys = [str(k) for k in golden["v_keys"]]
    assert len(golden["v_in"]) >= 4
    for args, vals in zip(golden["v_in"], golden["v_vals"]):
        got = calculate_viability_metrics(*(int(a) for a in args))
        assert sorted(got) == keys
        assert [float(got[k]) for k in keys] == list(vals), args


def test_instance_symbols_declared_bound_and_exported():
    from eunet import _lib
    src = open(os.path.join(ROOT, "include", "eunet.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int\s+" + name + r"\s*\(", src, flags=re.M), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    for cite in ("metrics.py:61-194", "train_eval.py:819-821", "train_eval.py:654-850"):
        assert cite in src, cite


def test_evaluator_surface():
    import inspect
    from eunet.evaluator import EVALUATE_KEYS, Evaluator
    sig = inspect.signature(Evaluator.semantic_to_instances)
    assert list(sig.parameters) == ["self", "semantic_mask", "min_area"] and sig.parameters["min_area"].default == 3
    assert "bbox_mAP" not in EVALUATE_KEYS and "segm_mAP" not in EVALUATE_KEYS and len(EVALUATE_KEYS) == 23
    assert hasattr(Evaluator, "evaluate")
