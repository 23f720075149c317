"""Host side of the boundary evaluation.  The restatement of tests/_boundary_ref.py is held to an all-pairs brute
force and to scipy.ndimage; metrics.boundary_metrics_from_stats is held to numpy computed from explicit distance
lists and to hand-derived cases.  No GPU: the statistics here come from the restatement."""
import math
import os
import re

import numpy as np
import pytest

import _boundary_ref as R

from eunet import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUES = np.array([0, 1, 2, 255, 7, -1], np.int64)


def _random_map(rng, h, w, p=(0.4, 0.2, 0.2, 0.1, 0.05, 0.05)):
    return rng.choice(VALUES, size=(h, w), p=p)


def _blobs(rng, h, w, n=6):
    """Discs of class 1 and 2 on background: regions with interiors, as masks have."""
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), np.int64)
    for _ in range(n):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(2, max(3, min(h, w) / 3))
        m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = rng.integers(1, 3)
    return m


def _brute_edges(r):
    h, w = r.shape
    e = np.zeros_like(r)
    for y in range(h):
        for x in range(w):
            if not r[y, x]:
                continue
            for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                yy, xx = y + dy, x + dx
                if yy < 0 or yy >= h or xx < 0 or xx >= w or not r[yy, xx]:
                    e[y, x] = True
    return e


def _brute_edt(s):
    ys, xs = np.nonzero(s)
    h, w = s.shape
    if ys.size == 0:
        return np.full((h, w), R.NONE, np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy[..., None] - ys) ** 2 + (xx[..., None] - xs) ** 2).min(axis=-1).astype(np.int64)


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (2, 3), (7, 5), (24, 31)])
def test_restatement_against_all_pairs(shape):
    rng = np.random.default_rng(sum(shape))
    for m in (_random_map(rng, *shape), _blobs(rng, *shape), np.ones(shape, np.int64), np.zeros(shape, np.int64)):
        for v in (0, 1, 2, 5):
            r = R.region(m, v)
            assert np.array_equal(R.edges(r), _brute_edges(r))
            for mode in ("eq", "ne", "edge"):
                s = R.sites(m, v, mode)
                assert np.array_equal(R.edt_sq(s), _brute_edt(s)), (v, mode)


def test_values_are_compared_in_64_bits():
    m = np.array([[1, 1 + 2 ** 32, 1], [-1, 2 ** 32 - 1, 1]], np.int64)
    assert R.region(m, 1).tolist() == [[True, False, True], [False, False, True]]
    assert R.region(m, -1).sum() == 1 and R.region(m, 1 + 2 ** 32).sum() == 1


@pytest.mark.parametrize("shape", [(40, 57), (96, 130)])
def test_restatement_against_scipy(shape):
    nd = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(5)
    for m in (_random_map(rng, *shape), _blobs(rng, *shape, n=10)):
        for v in (0, 1, 2):
            r = R.region(m, v)
            e = R.edges(r)
            assert np.array_equal(e, r & ~nd.binary_erosion(r))
            for s in (r, ~r, e):
                if s.any():  # scipy measures the distance to the nearest zero
                    ref = np.rint(nd.distance_transform_edt(~s) ** 2).astype(np.int64)
                    assert np.array_equal(R.edt_sq(s), ref)
            b, i = R.ref_sets(r)
            assert np.array_equal(b, nd.binary_dilation(r) & ~nd.binary_erosion(r))
            assert np.array_equal(i, nd.binary_erosion(r, iterations=2))


def test_reference_lists_against_scipy():
    """boundary_ious_ref / interior_ious_ref are what visualization.py:1687-1751 appends, image by image."""
    nd = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(9)
    pairs = [(_blobs(rng, 40, 50), _blobs(rng, 40, 50)), (np.zeros((20, 20), np.int64), _blobs(rng, 20, 20, n=2)),
             (_blobs(rng, 31, 17), np.zeros((31, 17), np.int64))]
    want = ([], [])
    rows = []
    for pred, gt in pairs:
        rows.append(R.boundary_stats(pred, gt, radii=())[2])
        for c in range(3):
            t, p = gt == c, pred == c
            if t.sum() == 0:
                continue
            tb, pb = (nd.binary_dilation(m) & ~nd.binary_erosion(m) for m in (t, p))
            ti, pi = (nd.binary_erosion(m, iterations=2) for m in (t, p))
            if tb.sum() > 0:
                want[0].append((tb & pb).sum() / (tb | pb).sum())
            if ti.sum() > 0:
                want[1].append((ti & pi).sum() / (ti | pi).sum())
    stats = {"surf": np.zeros((3, 2, 69), np.int64), "band": np.zeros((3, 0, 3), np.int64),
             "refrows": np.concatenate(rows), "cap": 8, "band_radii": ()}
    got = M.boundary_metrics_from_stats(stats)
    assert got["boundary_ious_ref"] == want[0] and got["interior_ious_ref"] == want[1] and len(want[1]) >= 4
    assert got["boundary_iou_ref"] == np.mean(want[0]) and got["interior_iou_ref"] == np.mean(want[1])


def test_the_fixed_point_root_is_the_integer_square_root():
    for d2 in list(range(0, 4200)) + [2 * 8191 ** 2, 8191 ** 2, 2 ** 27 - 1, 12345678]:
        s = R.isqrt_q16(d2)
        assert s == math.isqrt(d2 << 32) and s * s <= d2 << 32 < (s + 1) ** 2
        # the device route: a double root and a fix-up by one
        t = int(math.sqrt(float(d2 << 32)))
        assert abs(t - s) <= 1
        assert abs(s / 65536.0 - math.sqrt(d2)) < 2.0 ** -16


def _metrics(pred, gt, k=3, cap=64, radii=(2,), tolerances=(1, 2, 3), **kw):
    surf, band, refrows = R.boundary_stats(pred, gt, k=k, cap=cap, radii=radii, **kw)
    stats = {"surf": surf, "band": band, "refrows": refrows, "cap": cap, "band_radii": tuple(radii)}
    return M.boundary_metrics_from_stats(stats, tolerances=tolerances), stats


def test_percentile_rank_is_numpys_inverted_cdf():
    rng = np.random.default_rng(0)
    for n in list(range(1, 130)) + [200, 1000, 4001]:
        x = np.sort(rng.integers(0, 50, n)).astype(np.float64)
        assert x[M._percentile_rank(n, 0.95) - 1] == np.percentile(x, 95, method="inverted_cdf"), n


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_metrics_against_explicit_distance_lists(seed):
    """Two images accumulated: every pooled metric equals numpy on the concatenated per-pixel distance lists."""
    rng = np.random.default_rng(seed)
    pairs = []
    for h, w in ((48, 61), (37, 40)):
        gt = _blobs(rng, h, w, n=7)
        pred = np.roll(gt, (int(rng.integers(-3, 4)), int(rng.integers(-3, 4))), axis=(0, 1))
        pred[rng.random((h, w)) < 0.01] = rng.integers(0, 3)
        gt[2:6, 3:20] = 255
        pairs.append((pred, gt))
    cap = 64
    parts = [R.boundary_stats(p, g, cap=cap, radii=(0, 2)) for p, g in pairs]
    stats = {"surf": R.combine(parts[0][0], parts[1][0], cap), "band": parts[0][1] + parts[1][1],
             "refrows": np.concatenate([parts[0][2], parts[1][2]]), "cap": cap, "band_radii": (0, 2)}
    got = M.boundary_metrics_from_stats(stats)
    for c, name in enumerate(M.CLASS_NAMES):
        lists = [R.edge_distances(p, g, c) for p, g in pairs]
        d0 = np.concatenate([l[0] for l in lists])
        d1 = np.concatenate([l[1] for l in lists])
        m = got[name]
        assert m["n_pred_edge"] == d0.size and m["n_gt_edge"] == d1.size and d0.size and d1.size
        for t in (1, 2, 3):
            assert m["nsd"][t] == ((d0 <= t).sum() + (d1 <= t).sum()) / (d0.size + d1.size)
            assert m["boundary_precision"][t] == (d0 <= t).mean() and m["boundary_recall"][t] == (d1 <= t).mean()
            p, r = (d0 <= t).mean(), (d1 <= t).mean()
            assert abs(m["boundary_f1"][t] - 2 * p * r / (p + r)) <= 1e-15
        assert m["hd"] == max(d0.max(), d1.max())
        assert m["hd95"] == max(np.percentile(d0, 95, method="inverted_cdf"),
                                np.percentile(d1, 95, method="inverted_cdf"))
        assert not m["hd95_exceeds_cap"]
        both = np.concatenate([d0, d1])
        assert np.isfinite(both).all()
        assert 0 <= both.mean() - m["assd"] < 2.0 ** -16
    present = sum(int((g == c).any()) for _, g in pairs for c in range(3))
    assert len(got["boundary_ious_ref"]) == present >= 4 and 0 < got["boundary_iou_ref"] < 1


def test_a_square_against_its_copy_shifted_by_three_columns():
    """gt: the 10 x 10 square rows 5..14, columns 5..14 of a 20 x 30 map; pred: the same square at columns 8..17.

    Edges: the 36 pixels of each square's outline.  pred -> gt, pixel by pixel:
      rows 5 and 14, columns 8..14 (14 pixels) lie on gt's outline: d = 0;
      rows 5 and 14, columns 15, 16, 17 (6 pixels): d = 1, 2, 3 from gt's corner (., 14);
      column 8, rows 6..13 (8 pixels) lie inside gt, 3 from its left side and 1, 2, 3, 4, 4, 3, 2, 1 rows from its
        top or bottom side: d = 1, 2, 3, 3, 3, 3, 2, 1;
      column 17, rows 6..13 (8 pixels): the nearest gt pixel is in column 14 of the same row: d = 3.
    So pred -> gt has d = 0: 14, d = 1: 4, d = 2: 4, d = 3: 14 pixels, and by symmetry gt -> pred the same.
    NSD: t = 1: 36 / 72 = 0.5; t = 2: 44 / 72; t = 3: 1.  HD = 3, HD95 = 3 (rank ceil(0.95 * 36) = 35 > 22),
    ASSD = (4 * 1 + 4 * 2 + 14 * 3) / 36 = 1.5.
    Band r = 0 (the outlines): 36 and 36 pixels; shared are rows 5 and 14, columns 8..14 (14 pixels) and nothing
    else (pred's column 8 is interior to gt except in those rows; gt's column 14 likewise): IoU = 14 / 58.
    Reference rows: interior = the square eroded twice, 6 x 6 at rows 7..12; gt columns 7..12, pred 10..15:
    overlap 6 x 3 = 18, IoU 18 / 54 = 1 / 3."""
    gt = np.zeros((20, 30), np.int64)
    pred = np.zeros((20, 30), np.int64)
    gt[5:15, 5:15] = 1
    pred[5:15, 8:18] = 1
    got, stats = _metrics(pred, gt, radii=(0,))
    m = got["live"]
    assert m["n_pred_edge"] == 36 and m["n_gt_edge"] == 36
    for d in (0, 1):
        assert stats["surf"][1, d, [0, 1, 4, 9]].tolist() == [14, 4, 4, 14]
        assert stats["surf"][1, d, 64 * 64 + 3] == 9
        assert stats["surf"][1, d, 64 * 64 + 4] == 4 * 65536 + 4 * 2 * 65536 + 14 * 3 * 65536
    assert m["nsd"] == {1: 0.5, 2: 44 / 72, 3: 1.0}
    assert m["boundary_precision"][1] == 0.5 and m["boundary_recall"][1] == 0.5 and m["boundary_f1"][1] == 0.5
    assert m["hd"] == 3.0 and m["hd95"] == 3.0 and m["assd"] == 1.5
    assert m["boundary_iou"][0] == 14 / 58
    assert stats["refrows"][0, 1, 1].tolist() == [36, 36, 18]
    assert got["interior_ious_ref"][1] == 18 / 54  # image 0: background first, then live
    assert len(got["boundary_ious_ref"]) == 2 and len(got["interior_ious_ref"]) == 2  # dead is absent from gt
    assert np.isnan(got["dead"]["hd"]) and np.isnan(got["dead"]["nsd"][1]) and got["dead"]["n_gt_edge"] == 0


def test_a_class_missing_on_one_side_or_on_both():
    """live only in gt (a 3 x 3 block: 8 edge pixels... all 9 but the centre), dead nowhere.  live: recall 0,
    precision without a denominator, HD = inf, HD95 = inf (every gt edge pixel lacks a counterpart), ASSD nan;
    dead: everything nan.  background: pred has the image border only as its edge, gt also the ring around the
    block."""
    gt = np.zeros((9, 9), np.int64)
    gt[3:6, 3:6] = 1
    pred = np.zeros((9, 9), np.int64)
    got, stats = _metrics(pred, gt)
    live, dead = got["live"], got["dead"]
    assert live["n_pred_edge"] == 0 and live["n_gt_edge"] == 8
    assert stats["surf"][1, 1, 64 * 64 + 2] == 8 and stats["surf"][1, 0].sum() == 0
    assert live["hd"] == float("inf") and live["hd95"] == float("inf") and not live["hd95_exceeds_cap"]
    assert np.isnan(live["assd"]) and live["boundary_recall"][1] == 0.0 and np.isnan(live["boundary_precision"][1])
    assert np.isnan(live["boundary_f1"][1]) and live["nsd"][3] == 0.0 and live["boundary_iou"][2] == 0.0
    for key in ("hd", "hd95", "assd"):
        assert np.isnan(dead[key]), key
    assert not dead["hd95_exceeds_cap"] and np.isnan(dead["nsd"][1]) and np.isnan(dead["boundary_iou"][2])
    # the reversed pair: HD is inf from the other direction
    rev, _ = _metrics(gt, pred)
    assert rev["live"]["hd"] == float("inf") and rev["live"]["boundary_precision"][1] == 0.0
    assert len(rev["boundary_ious_ref"]) == 1  # only background is in this ground truth


def test_a_percentile_beyond_cap_is_flagged():
    """Two single pixels of live 10 columns apart with cap = 3: every distance (10) is in the overflow bin.  HD is
    exact (10, from the maximum), HD95 is nan and flagged, ASSD exact (10), NSD 0."""
    gt = np.zeros((5, 20), np.int64)
    pred = np.zeros((5, 20), np.int64)
    gt[2, 3] = 1
    pred[2, 13] = 1
    got, stats = _metrics(pred, gt, cap=3)
    m = got["live"]
    assert stats["surf"].shape == (3, 2, 14) and stats["surf"][1, :, 10].tolist() == [1, 1]
    assert m["hd"] == 10.0 and np.isnan(m["hd95"]) and m["hd95_exceeds_cap"] and m["assd"] == 10.0
    assert m["nsd"][3] == 0.0
    with pytest.raises(ValueError):
        M.boundary_metrics_from_stats(stats, tolerances=(4,))
    with pytest.raises(ValueError):
        M.boundary_metrics_from_stats(stats, class_names=("a",))
    assert sorted(k for k in M.boundary_metrics_from_stats(stats, class_names=("x", "y", "z")) if len(k) == 1) == \
        ["x", "y", "z"]


def test_the_ignore_rule_applies_to_the_statistics_and_not_to_the_reference_rows():
    """A predicted live block under ignored ground truth: with the rule, pred has no live pixel left (it reads 255
    there), so surf and band of live see no pred edge; the reference rows still count the block."""
    gt = np.zeros((12, 12), np.int64)
    gt[2:9, 2:9] = 255
    pred = np.zeros((12, 12), np.int64)
    pred[3:8, 3:8] = 1
    surf, band, refrows = R.boundary_stats(pred, gt, radii=(0, 2))
    assert surf[1].sum() == 0 and band[1].sum() == 0
    assert refrows[0, 1, 0].tolist() == [16 + 20, 0, 0] and refrows[0, 1, 1].tolist() == [1, 0, 0]
    # background: both maps have the same edge along the ignored block, at distance 0
    assert surf[0, 0, 0] == surf[0, 1, 0] == surf[0, 0, :64 * 64 + 3].sum() > 0


def test_header_library_and_binding_agree_on_the_new_symbols():
    from eunet import _lib
    src = open(os.path.join(ROOT, "include", "eunet.h")).read()
    lib = _lib.load()
    for name in ("eunet_edt_sq", "eunet_boundary_workspace_bytes", "eunet_boundary_stats"):
        assert re.search(rf"^int {name}\(", src, flags=re.M), name
        assert name in _lib.SIGNATURES and name in _lib.exported_symbols() and hasattr(lib, name), name
    for macro, value in (("EUNET_EDT_EQ", _lib.EDT_EQ), ("EUNET_EDT_NE", _lib.EDT_NE), ("EUNET_EDT_EDGE", _lib.EDT_EDGE),
                         ("EUNET_EDT_NONE", _lib.EDT_NONE), ("EUNET_EDT_MAX_VALUES", _lib.EDT_MAX_VALUES),
                         ("EUNET_EDT_MAX_SIDE", _lib.EDT_MAX_SIDE), ("EUNET_BOUNDARY_MAX_CAP", _lib.BOUNDARY_MAX_CAP),
                         ("EUNET_BOUNDARY_MAX_RADII", _lib.BOUNDARY_MAX_RADII)):
        assert re.search(rf"^#define {macro} \(?{value}\)?$", src, flags=re.M), macro
    # the host-only refusals of the launchers: nothing is dereferenced, nothing is launched
    import ctypes
    size = ctypes.c_size_t()
    assert lib.eunet_boundary_workspace_bytes(2, 3, 10, 20, ctypes.byref(size)) == 0 and size.value == 2 * 2 * 3 * 200 * 4
    assert lib.eunet_boundary_workspace_bytes(1, 4, 10, 20, ctypes.byref(size)) != 0
    vals = (ctypes.c_int64 * 1)(1)
    for n, h, w, nv, mode in ((1, 0, 8, 1, 0), (1, 8, 8193, 1, 0), (0, 8, 8, 1, 0), (1, 8, 8, 0, 0), (1, 8, 8, 9, 0),
                              (1, 8, 8, 1, 3)):
        assert lib.eunet_edt_sq(0x1000, n, h, w, vals, nv, mode, 0x2000, None) != 0, (n, h, w, nv, mode)
