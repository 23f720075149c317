"""Host side of the pixel-level curve statistics: metrics.curve_edges and metrics.curve_metrics_from_hist against
the sorting restatement of tests/_curves_ref.py (and, where sklearn is installed, the restatement against
sklearn).  No GPU: the histograms here come from the restatement's own binning."""
import numpy as np
import pytest

import _curves_ref as R

from eunet import metrics as M

TOL = 1e-12  # ratios of exact integers, summed over at most 3072 terms in float64
ARRAYS = ("fpr", "tpr", "thresholds", "precision", "recall", "cal_acc", "cal_conf", "cal_count", "conf_hist")
SCALARS = ("auc", "ap", "auc_resolution", "ece")


def _scores(kind, n=6000, seed=0):
    """(p float32 [n], label bool [n]): a sigmoid of a noisy logit, saturated (steepness 8: most scores within
    1e-3 of 0 or 1) or not (steepness 1)."""
    rng = np.random.default_rng(seed)
    y = rng.random(n) < 0.3
    z = rng.normal(0.0, 1.0, n) + np.where(y, 1.5, -1.5)
    steep = {"saturated": 8.0, "unsaturated": 1.0}[kind]
    return (1.0 / (1.0 + np.exp(-steep * z))).astype(np.float32), y


def _hist_of(p, y, edges):
    """[1, B, 3] histogram of one class from per-pixel scores and labels, by the restatement's binning."""
    b = R.pixel_bins(p, edges)
    h = np.zeros((1, len(edges) - 1, 3), np.int64)
    np.add.at(h[0, :, 0], b[~y], 1)
    np.add.at(h[0, :, 1], b[y], 1)
    np.add.at(h[0, :, 2], b, R.pixel_conf(p))
    return h


def _compare(got, ref):
    for key in ARRAYS:
        a, b = np.asarray(got[key], dtype=np.float64), np.asarray(ref[key], dtype=np.float64)
        assert a.shape == b.shape, key
        both_inf = np.isinf(a) & np.isinf(b)
        assert np.all(both_inf | (np.abs(np.where(both_inf, 0, a) - np.where(both_inf, 0, b)) <= TOL)), key
    for key in SCALARS:
        assert abs(got[key] - ref[key]) <= TOL, (key, got[key], ref[key])
    assert got["n_pos"] == ref["n_pos"] and got["n_neg"] == ref["n_neg"]


def test_curve_edges_properties():
    e = M.curve_edges()
    assert e.dtype == np.float32 and e.ndim == 1
    assert len(e) - 1 == 1208
    assert e[0] == 0.0 and e[-1] == 1.0
    assert np.all(np.diff(e) > 0)
    for n in (10, 50):  # the calibration and confidence tables, as float64 comparisons see a float32 score
        assert np.isin(M.ceil32(np.linspace(0, 1, n + 1)), e).all(), n
    # log-spaced tails: at least per_octave edges inside every octave below 1 / uniform, on both sides
    assert (e[(e > 0) & (e < 1e-3)]).size >= 8 * 13 and (e[e > 1 - 1e-3]).size >= 8 * 10


def test_ceil32_is_the_float64_predicate():
    """p >= ceil32(x) in fp32 is p >= x in float64, for the fp32 neighbours of x."""
    x = np.concatenate([np.linspace(0, 1, 1001), 2.0 ** (-np.arange(1, 193) / 8.0)])
    c = M.ceil32(x)
    assert c.dtype == np.float32 and np.all(c.astype(np.float64) >= x)
    below = np.nextafter(c, np.float32(-1))
    assert np.all(below.astype(np.float64) < x)


@pytest.mark.parametrize("kind", ["saturated", "unsaturated"])
def test_curve_metrics_match_the_sorting_restatement(kind):
    e = M.curve_edges()
    p, y = _scores(kind)
    got = M.curve_metrics_from_hist(_hist_of(p, y, e), e)["foreground"]
    _compare(got, R.curve_stats_ref(p, y, e))


@pytest.mark.parametrize("bins", [1, 2, 50, 3000])
def test_curve_metrics_on_other_tables(bins):
    """Uniform tables: one that holds the 10- and 50-bin edges runs with the defaults; a smaller one is refused
    with them and runs with coarse bins it does hold."""
    e = M.ceil32(np.linspace(0, 1, bins + 1))
    p, y = _scores("unsaturated", 2000, 1)
    if bins in (1, 2):
        with pytest.raises(ValueError):
            M.curve_metrics_from_hist(_hist_of(p, y, e), e)
        got = M.curve_metrics_from_hist(_hist_of(p, y, e), e, n_cal=1, n_conf=bins)["foreground"]
        _compare(got, R.curve_stats_ref(p, y, e, n_cal=1, n_conf=bins))
        return
    got = M.curve_metrics_from_hist(_hist_of(p, y, e), e)["foreground"]
    _compare(got, R.curve_stats_ref(p, y, e))


@pytest.mark.parametrize("kind", ["saturated", "unsaturated"])
def test_auc_is_within_its_resolution_of_the_exact_auc(kind):
    e = M.curve_edges()
    for seed in range(3):
        p, y = _scores(kind, 6000, seed)
        got = M.curve_metrics_from_hist(_hist_of(p, y, e), e)["foreground"]
        exact = R.exact_auc(p, y)
        print(f"{kind} seed {seed}: auc {got['auc']:.6f} exact {exact:.6f} resolution {got['auc_resolution']:.3e}")
        assert abs(got["auc"] - exact) <= got["auc_resolution"] + TOL
        # the plain uniform grid is what the tails are for: its own bound still holds
        u = M.curve_edges(1000, 8, 0)
        gu = M.curve_metrics_from_hist(_hist_of(p, y, u), u)["foreground"]
        assert abs(gu["auc"] - exact) <= gu["auc_resolution"] + TOL
        assert got["auc_resolution"] <= gu["auc_resolution"]


def test_degenerate_classes_give_nan():
    e = M.curve_edges()
    p, y = _scores("unsaturated", 500, 2)
    for lab in (np.zeros_like(y), np.ones_like(y)):
        got = M.curve_metrics_from_hist(_hist_of(p, lab, e), e)["foreground"]
        assert np.isnan(got["auc"]) and np.isnan(got["ap"]) and np.isnan(got["auc_resolution"])
        ref = R.curve_stats_ref(p, lab, e)
        for key in ("cal_acc", "cal_conf", "cal_count", "conf_hist"):  # calibration needs no second class
            assert np.all(np.abs(np.asarray(got[key], np.float64) - ref[key]) <= TOL), key
        assert abs(got["ece"] - ref["ece"]) <= TOL
    empty = M.curve_metrics_from_hist(np.zeros((3, len(e) - 1, 3), np.int64), e)
    assert sorted(empty) == ["background", "dead", "live"]
    for v in empty.values():
        assert all(np.isnan(v[s]) for s in SCALARS)
        assert v["fpr"].shape == (1,) and v["cal_count"].sum() == 0


def test_empty_calibration_bins_follow_the_reference():
    """Scores in [0.2, 0.3) and at 1.0 only: the other bins have accuracy 0 and the bin centre as confidence
    (visualization.py:1861-1864); p == 1 sits in the last bin (the reference drops it)."""
    e = M.curve_edges()
    p = np.array([0.25, 0.25, 0.29, 1.0, 1.0], np.float32)
    y = np.array([True, False, False, True, True])
    got = M.curve_metrics_from_hist(_hist_of(p, y, e), e)["foreground"]
    assert list(got["cal_count"]) == [0, 0, 3, 0, 0, 0, 0, 0, 0, 2]
    centres = (np.arange(10) + 0.5) / 10
    for i in range(10):
        if i not in (2, 9):
            assert got["cal_acc"][i] == 0.0 and abs(got["cal_conf"][i] - centres[i]) <= TOL
    assert abs(got["cal_acc"][2] - 1 / 3) <= TOL and got["cal_acc"][9] == 1.0 and got["cal_conf"][9] == 1.0
    assert abs(got["cal_conf"][2] - float(R.pixel_conf(p[:3]).sum()) / 2 ** 24 / 3) <= TOL
    assert abs(got["ece"] - (3 / 5 * abs(1 / 3 - got["cal_conf"][2]) + 0.0)) <= TOL
    assert got["conf_hist"].sum() == 5 and got["conf_hist"][49] == 2 and got["conf_hist"][12] == 2
    _compare(got, R.curve_stats_ref(p, y, e))


def test_refusals():
    e = M.curve_edges()
    h = np.zeros((3, len(e) - 1, 3), np.int64)
    with pytest.raises(ValueError):
        M.curve_metrics_from_hist(h[:, :-1], e)
    with pytest.raises(ValueError):
        M.curve_metrics_from_hist(h, e, class_names=("a", "b"))
    with pytest.raises(ValueError):
        M.curve_metrics_from_hist(h, e, n_cal=7)  # 1/7 is not an edge of the table
    with pytest.raises(ValueError):
        M.curve_metrics_from_hist(h, e, n_conf=30)
    assert sorted(M.curve_metrics_from_hist(h[:2], e)) == ["background", "live"]
    assert sorted(M.curve_metrics_from_hist(h, e, class_names=("x", "y", "z"))) == ["x", "y", "z"]


def test_the_histogram_restatement_follows_the_stated_rules():
    """tests/_curves_ref.score_hist_ref on a hand-made image: the closed last bin, -0.0, the invalid scores, the
    ignored pixels (not examined), labels outside [0, K) and the one-logit rule."""
    e = np.array([0, 0.25, 0.5, 1.0], np.float32)
    p = np.array([[0.0, -0.0, 0.25, 0.4999, 0.5, 1.0, np.nextafter(np.float32(1), np.float32(2)), 1.5, np.nan, np.inf,
                   -np.inf, -1e-30, np.nan, 0.75]], np.float32).reshape(1, 1, 14)
    m = np.array([[0, 1, 2, 0, 1, 1, 7, -1, 1, 0, 0, 1, 255, 255]], np.int64)
    h, inv = R.score_hist_ref(p, m, e)
    assert inv == 4  # the NaN under an ignored pixel is not examined
    assert h[0, :, :2].tolist() == [[1, 1], [1, 1], [1, 3]]  # K = 1: positive where the mask is >= 1
    q = 2 ** 24
    assert h[0, :, 2].tolist() == [0, int(np.rint(np.float32(0.25) * q)) + int(np.rint(np.float32(0.4999) * np.float32(q))),
                                   q // 2 + 3 * q]
    p3 = np.repeat(p, 3, axis=0)
    h3, inv3 = R.score_hist_ref(p3, m, e)
    assert inv3 == 12
    assert h3[2, :, :2].tolist() == [[2, 0], [1, 1], [4, 0]]  # labels 7 and -1 are negatives of every class


def test_restatement_agrees_with_sklearn():
    sk = pytest.importorskip("sklearn.metrics")
    e = M.curve_edges()
    for kind in ("saturated", "unsaturated"):
        p, y = _scores(kind, 4000, 5)
        b = R.pixel_bins(p, e)
        ref = R.curve_stats_ref(p, y, e)
        assert abs(ref["auc"] - sk.roc_auc_score(y, b)) <= 1e-12
        assert abs(ref["ap"] - sk.average_precision_score(y, b)) <= 1e-12
        fpr, tpr, thr = sk.roc_curve(y, b, drop_intermediate=False)
        assert np.allclose(ref["fpr"], fpr, rtol=0, atol=1e-12) and np.allclose(ref["tpr"], tpr, rtol=0, atol=1e-12)
        assert np.array_equal(ref["thresholds"][1:], e[thr[1:].astype(np.int64)].astype(np.float64))
        prec, rec, _ = sk.precision_recall_curve(y, b)
        assert np.allclose(ref["precision"], prec, rtol=0, atol=1e-12)
        assert np.allclose(ref["recall"], rec, rtol=0, atol=1e-12)
        assert abs(R.exact_auc(p, y) - sk.roc_auc_score(y, p.astype(np.float64))) <= 1e-12
