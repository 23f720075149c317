"""The host half of the label-map instance metrics (eunet.metrics: instance_stats_from_pairs,
panoptic_metrics_from_stats, size_strata_from_pairs) against the plain-loop restatement of tests/_panoptic_ref.py and
against answers worked out by hand.  The pair tables come from the restatement's np.unique (the device's table is
held to the same function in tests/test_gpu_pairs.py).

Integer outputs are compared with array_equal.  iou_sum, seg_sum and the Dice sums are compared at 1e-12 absolute:
both sides add, in the same id order, at most a few hundred float64 terms each of which is the correctly rounded
quotient of the same two integers, so they agree far inside that bound."""
import math

import numpy as np
import pytest

import _panoptic_ref as R
from eunet import metrics as M

INT_KEYS = ("n_pred", "n_gt", "tp50", "tp", "aji_c", "aji_u", "objdice_gw", "objdice_pw")
FLOAT_KEYS = ("iou_sum", "seg_sum", "objdice_g", "objdice_p")


def _compare(pred, gt, iou_percent=R.IOU_PERCENT):
    pred, gt = np.asarray(pred), np.asarray(gt)
    if pred.ndim == 2:
        pred, gt = pred[None], gt[None]
    got = M.instance_stats_from_pairs(R.pair_table(pred, gt), len(pred), iou_percent)
    ref = R.stats(pred, gt, iou_percent)
    assert set(got) == set(INT_KEYS + FLOAT_KEYS) == set(M.INSTANCE_STAT_NAMES)
    for k in INT_KEYS:
        assert got[k].dtype == np.int64 and np.array_equal(got[k], ref[k]), (k, got[k], ref[k])
    for k in FLOAT_KEYS:
        assert got[k].dtype == np.float64 and np.abs(got[k] - ref[k]).max() <= 1e-12, (k, got[k], ref[k])
    return got, ref


def _same(a, b):
    return a == b or (a != a and b != b)


def _blobs(rng, h, w, n, ignore=False):
    m = np.zeros((h, w), np.int64)
    for k in range(1, n + 1):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        m[max(0, y - int(rng.integers(2, 7))):y + int(rng.integers(2, 7)),
          max(0, x - int(rng.integers(2, 7))):x + int(rng.integers(2, 7))] = k
    if ignore:
        m[rng.random((h, w)) < 0.05] = -1
    return m


@pytest.mark.parametrize("seed", range(6))
def test_random_small_maps_against_the_restatement(seed):
    rng = np.random.default_rng(seed)
    h, w = 24 + seed, 31 - seed
    gt = np.stack([_blobs(rng, h, w, 6, ignore=seed % 2 == 1), _blobs(rng, h, w, 3)])
    pred = gt.copy()
    pred[pred < 0] = 0
    pred = np.roll(pred, (seed % 2, 1), axis=(1, 2))  # shifted copies: matches at several IoU levels
    pred[0][rng.random((h, w)) < 0.05] = 0
    pred[1][:, : w // 2][pred[1][:, : w // 2] > 0] += 7  # other ids, one object cut in two
    got, ref = _compare(pred, gt)
    assert got["n_gt"].sum() > 0 and got["tp50"].sum() > 0
    ts = (50, 60, 75, 99)
    _compare(pred, gt, ts)
    names = ("live", "dead")
    scores = M.panoptic_metrics_from_stats(got, names)
    assert tuple(scores) == M.panoptic_keys(names)
    pooled = {k: (ref[k].sum(axis=0) if k != "tp" else ref[k].sum(axis=0).tolist()) for k in ref}
    for q, name in enumerate(names):
        for k, v in R.scores({kk: (ref[kk][q].tolist() if kk == "tp" else ref[kk][q].item()) for kk in ref}).items():
            assert _same(scores[f"{k}_{name}"], v), (k, name)
    for k, v in R.scores({kk: (vv if kk == "tp" else vv.item()) for kk, vv in pooled.items()}).items():
        assert _same(scores[k], v), k


def test_statistics_add_over_images():
    rng = np.random.default_rng(11)
    maps = [(np.stack([_blobs(rng, 20, 20, 4)]), np.stack([_blobs(rng, 20, 20, 4)])) for _ in range(3)]
    acc = None
    for pred, gt in maps:
        acc = M.add_instance_stats(acc, M.instance_stats_from_pairs(R.pair_table(pred, gt), 1))
    refs = [R.stats(pred, gt) for pred, gt in maps]
    for k in INT_KEYS:
        assert np.array_equal(acc[k], sum(r[k] for r in refs)), k
    zero = M.empty_instance_stats(1)
    assert all(np.array_equal(M.add_instance_stats(zero, acc)[k], acc[k]) for k in M.INSTANCE_STAT_NAMES)


@pytest.mark.parametrize("k", [1, 8, 50])
def test_one_object_predicted_as_two_halves(k):
    """A ground truth of 2k pixels predicted as two halves of k: both IoUs are exactly 1/2, so at t = 50 (strict) TP = 0,
    FP = 2, FN = 1 and PQ = 0; AJI takes id 1 by the tie rule, C = k, U = 2k + k: 1/3; neither half covers more than
    half: SEG = 0."""
    gt = np.zeros((3, 2 * k + 2), np.int64)
    gt[1, 1:2 * k + 1] = 1
    pred = np.zeros_like(gt)
    pred[1, 1:k + 1] = 1
    pred[1, k + 1:2 * k + 1] = 2
    got, _ = _compare(pred, gt)
    assert got["tp50"].tolist() == [0] and got["n_pred"].tolist() == [2] and got["n_gt"].tolist() == [1]
    assert got["aji_c"].tolist() == [k] and got["aji_u"].tolist() == [3 * k] and got["seg_sum"].tolist() == [0.0]
    s = M.panoptic_metrics_from_stats(got, ("live",))
    assert s["pq_live"] == 0.0 and s["pq"] == 0.0 and s["mpq"] == 0.0 and s["dq_live"] == 0.0 and math.isnan(s["sq_live"])
    assert s["aji_live"] == 1 / 3 and s["seg_live"] == 0.0 and s["f1_50_live"] == 0.0 and s["ap_dsb_live"] == 0.0
    # each half against the ground truth, and the ground truth against half 1: 2k / 3k
    assert s["objdice_live"] == pytest.approx(2 / 3, abs=1e-12)


def test_identical_maps_score_one_everywhere():
    rng = np.random.default_rng(3)
    ids = np.stack([_blobs(rng, 30, 30, 7), _blobs(rng, 30, 30, 2)])
    got, _ = _compare(ids, ids)
    assert np.array_equal(got["tp"], np.repeat(got["n_gt"][:, None], 10, axis=1)) and got["n_gt"].min() >= 1
    s = M.panoptic_metrics_from_stats(got)
    assert set(s) == set(M.panoptic_keys()) and all(v == 1.0 for v in s.values()), s


@pytest.mark.parametrize("case", ["no prediction", "no ground truth", "neither"])
def test_empty_sides_give_ratio_conventions_not_errors(case):
    obj = np.zeros((1, 8, 8), np.int64)
    obj[0, 2:5, 2:6] = 4
    none = np.zeros_like(obj)
    pred, gt = {"no prediction": (none, obj), "no ground truth": (obj, none), "neither": (none, none)}[case]
    got, _ = _compare(pred, gt)
    s = M.panoptic_metrics_from_stats(got, ("live",))
    if case == "neither":
        assert all(math.isnan(v) for v in s.values())
        return
    for k in ("pq", "dq", "aji", "f1_50", "ap_dsb", "pq_live", "mpq"):
        assert s[k] == 0.0, k
    assert math.isnan(s["sq"]) and math.isnan(s["objdice"])  # one side of the Dice has no area
    assert (s["seg"] == 0.0) if case == "no prediction" else math.isnan(s["seg"])
    assert got["aji_u"].tolist() == [12] and got["aji_c"].tolist() == [0]
    two = M.panoptic_metrics_from_stats(M.instance_stats_from_pairs(R.pair_table(np.concatenate([pred, none]),
                                                                                 np.concatenate([gt, none])), 2))
    assert two["mpq"] == 0.0 and math.isnan(two["pq_dead"]) and two["pq"] == 0.0  # an empty class is left out of mpq


def test_a_tie_in_the_aji_argmax_goes_to_the_smallest_id():
    """Ground truth 1 (8 px) overlaps prediction 3 and prediction 5 with 2 px each, both of area 4: equal IoU 2 / 10.
    Id 3 is taken, id 5 stays unused and its area joins the union."""
    gt = np.zeros((4, 10), np.int64)
    gt[1, 1:9] = 1
    pred = np.zeros_like(gt)
    pred[1, 1:3], pred[2, 1:3] = 5, 5
    pred[1, 7:9], pred[2, 7:9] = 3, 3
    got, _ = _compare(pred, gt)
    assert got["aji_c"].tolist() == [2] and got["aji_u"].tolist() == [10 + 4]
    pred[pred == 3] = 9  # now 5 is the smaller id: the same numbers, by the other object
    got, _ = _compare(pred, gt)
    assert got["aji_c"].tolist() == [2] and got["aji_u"].tolist() == [10 + 4]
    pred[2, 3] = 9  # 9 grows: its IoU drops to 2 / 11 and 5 wins on IoU, whatever the ids
    got, _ = _compare(pred, gt)
    assert got["aji_u"].tolist() == [10 + 5]


@pytest.mark.parametrize("t,n,u", [(50, 1, 2), (60, 3, 5), (75, 3, 4), (80, 4, 5), (90, 9, 10), (95, 19, 20)])
def test_the_threshold_is_strict_at_an_iou_of_exactly_t_percent(t, n, u):
    """A pair with n common pixels and a union of u, n / u = t / 100 exactly: no match at t; one more common pixel and it
    is one."""
    gt = np.zeros((2, 2 * u), np.int64)
    pred = np.zeros_like(gt)
    gt[0, :n] = 1
    pred[0, :n] = 1
    pred[0, n:u] = 1  # prediction of area u containing the ground truth of area n: IoU n / u
    for ts in ((t,), (50, t) if t != 50 else (50,)):
        got, _ = _compare(pred, gt, ts)
        assert got["tp"][0, -1] == 0
    gt[0, n] = 1
    got, _ = _compare(pred, gt, (t,))
    assert got["tp"][0, 0] == 1
    with pytest.raises(ValueError):
        M.instance_stats_from_pairs(R.pair_table(pred, gt), 1, (49,))
    with pytest.raises(ValueError):
        M.instance_stats_from_pairs(R.pair_table(pred, gt), 1, (100,))


def test_size_strata_against_the_reference_loops():
    rng = np.random.default_rng(5)
    gts = [rng.choice([0, 1, 2, 255], size=(40, 47), p=[0.5, 0.3, 0.15, 0.05]) for _ in range(2)]
    for g in gts:
        g[5:30, 5:30] = 1   # 625 px and more: the middle bins
        g[32:38, 2:45] = 2
    preds = [np.where(rng.random(g.shape) < 0.7, np.minimum(g, 2), rng.integers(0, 3, g.shape)) for g in gts]
    edges = (3, 100, 500)
    ref = R.size_strata(gts, preds, 3, edges)
    got = [[] for _ in range(len(edges) + 1)]
    for g, p in zip(gts, preds):  # one table per image, one plane per class
        comps = np.stack([R.label4(g == c)[0] for c in range(3)])
        same = np.stack([(p == c).astype(np.int64) for c in range(3)])
        for b, cov in zip(got, M.size_strata_from_pairs(R.pair_table(comps, same), edges)):
            b.extend(cov)
    assert [len(b) for b in ref] == [len(b) for b in got] and min(len(b) for b in ref[:3]) >= 1
    assert all(x == y for a, b in zip(ref, got) for x, y in zip(a, b))
    assert len(M.size_strata_from_pairs(np.zeros((0, 4), np.int64))) == len(M.SIZE_EDGES) + 1
    with pytest.raises(ValueError):
        M.size_strata_from_pairs(np.zeros((0, 4), np.int64), (500, 100))


def test_flood_fill_labelling_by_hand():
    m = np.array([[1, 0, 1, 1], [0, 1, 0, 1], [1, 1, 0, 0]])
    lab, n = R.label4(m)
    assert n == 3 and lab.tolist() == [[1, 0, 2, 2], [0, 3, 0, 2], [3, 3, 0, 0]]
