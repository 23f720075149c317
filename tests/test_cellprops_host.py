"""The per-cell measurements on the host: the restatement of tests/_cellprops_ref.py held to hand-derived answers and
to scipy.ndimage, metrics.cell_measurements on the restatement's integer tables against the restatement's own
descriptors, the population and agreement summaries on hand-made tables, and what ops.cell_stats refuses before any
device call.  No GPU."""
import math
import os
import re

import numpy as np
import pytest

import _cellprops_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_planes():
    """Blobs and noise with sides 1..23 (seeded), as (plane, n)."""
    rng = np.random.default_rng(7)
    out = []
    for k in range(60):
        h, w = int(rng.integers(1, 24)), int(rng.integers(1, 24))
        n = int(rng.integers(1, 6))
        out.append((R.blobs(h, w, n, k) if k % 2 else R.noise(h, w, n, k), n))
    return out


def _stats(plane, n, image=None):
    geom, inten, _ = R.cell_stats(plane, n, image)
    return {"geom": geom, "intensity": inten, "shape": np.asarray(plane).shape[-2:]}


def test_a_single_pixel():
    plane = np.zeros((3, 4), np.int64)
    plane[1, 2] = 1
    geom, _, _ = R.cell_stats(plane, 1)
    assert geom[0, 1].tolist() == [1, 2, 1, 4, 1, 2, 2, 1, 2, 1, 4, 0, 0, 0] and not geom[0, 0].any()
    d = R.descriptors(plane, 1)
    assert d["perimeter_crack"] == 4 and d["perimeter"] == 4 / math.sqrt(2) and d["euler_number"] == 1
    assert d["mu20"] == d["mu02"] == d["mu11"] == 0 and d["major_axis"] == d["minor_axis"] == 0
    assert d["eccentricity"] == 0
    from eunet import metrics as M
    m = M.cell_measurements(_stats(plane, 1))
    assert m["area"][0] == 1 and m["perimeter"][0] == 4 / math.sqrt(2) and m["euler_number"][0] == 1
    assert m["mu20"][0] == m["mu02"][0] == m["mu11"][0] == m["major_axis"][0] == m["eccentricity"][0] == 0
    assert m["orientation"][0] == 0 and m["bbox"][0].tolist() == [2, 1, 2, 1] and m["touches_border"][0] == 0


@pytest.mark.parametrize("a,b", [(3, 7), (7, 3), (1, 5), (4, 4)])
def test_a_rectangle(a, b):
    """a rows by b columns: mu20 = (b^2 - 1) / 12, mu02 = (a^2 - 1) / 12, crack 2 (a + b), q1 = 4, q2 = 2 (a - 1) +
    2 (b - 1)."""
    from eunet import metrics as M
    plane = np.zeros((a + 3, b + 2), np.int64)
    plane[2:2 + a, 1:1 + b] = 1
    geom, _, _ = R.cell_stats(plane, 1)
    assert geom[0, 1, 10:].tolist() == [4, 2 * (a - 1) + 2 * (b - 1), 0, 0] and geom[0, 1, 0] == a * b
    m = M.cell_measurements(_stats(plane, 1))
    for d in (R.descriptors(plane, 1), {k: v[0] for k, v in m.items()}):
        assert abs(d["mu20"] - (b * b - 1) / 12) < 1e-12 and abs(d["mu02"] - (a * a - 1) / 12) < 1e-12
        assert abs(d["mu11"]) < 1e-12 and d["perimeter_crack"] == 2 * (a + b) and d["extent"] == 1
        lo, hi = sorted((a * a - 1, b * b - 1))
        assert abs(d["eccentricity"] - (math.sqrt(1 - lo / hi) if hi else 0.0)) < 1e-12
        if a != b:
            assert abs(d["orientation"] - (0.0 if b > a else math.pi / 2)) < 1e-12
        assert d["euler_number"] == 1 and d["holes"] == 0
    if (a, b) == (3, 7):
        assert abs(m["eccentricity"][0] - math.sqrt(1 - 8 / 48)) < 1e-12


def test_diagonal_lines_have_the_orientation_of_their_axis():
    from eunet import metrics as M
    diag = np.eye(5, dtype=np.int64)  # y = x, y pointing down
    for plane, angle in ((diag, math.pi / 4), (diag[:, ::-1], -math.pi / 4)):
        assert abs(R.descriptors(plane, 1)["orientation"] - angle) < 1e-12
        assert abs(M.cell_measurements(_stats(plane, 1))["orientation"][0] - angle) < 1e-12


def test_a_ring_has_one_hole_and_two_diagonal_pixels_are_one_8_connected_cell():
    from eunet import metrics as M
    ring = np.ones((5, 5), np.int64)
    ring[2, 2] = 0
    d = R.descriptors(ring, 1)
    assert d["euler_number"] == 0 and d["holes"] == 1 and d["touches_border"] == 1
    m = M.cell_measurements(_stats(ring, 1))
    assert m["euler_number"][0] == 0 and m["holes"][0] == 1 and m["touches_border"][0] == 1
    two = np.zeros((4, 4), np.int64)
    two[1, 1] = two[2, 2] = 1
    assert R.quads(two, 1) == (6, 0, 0, 1, 0)
    d = R.descriptors(two, 1)
    assert d["euler_number"] == 1 and d["euler_number_4"] == 2 and d["perimeter_crack"] == 8


def test_a_window_of_several_labels_counts_for_each():
    plane = np.array([[1, 2], [3, 1]], np.int64)
    geom, _, _ = R.cell_stats(plane, 3)
    assert geom[0, 1, 10:].tolist() == [6, 0, 0, 1] and geom[0, 2, 10:].tolist() == [4, 0, 0, 0]
    assert geom[0, 3, 10:].tolist() == [4, 0, 0, 0]


def test_the_quad_identities_on_random_planes():
    """Crack perimeter = the differing 4-neighbour edges of the padded plane; area = (q1 + 2 q2 + 2 qd + 3 q3 + 4 q4)
    / 4."""
    for plane, n in _random_planes():
        for label in range(1, n + 1):
            q1, q2, q3, qd, q4 = R.quads(plane, label)
            m = np.pad(plane == label, 1)
            edges = int((m[1:] != m[:-1]).sum() + (m[:, 1:] != m[:, :-1]).sum())
            assert q1 + q2 + q3 + 2 * qd == edges
            assert q1 + 2 * q2 + 2 * qd + 3 * q3 + 4 * q4 == 4 * int(m.sum())
            assert (q1 - q3 - 2 * qd) % 4 == 0 and (q1 - q3 + 2 * qd) % 4 == 0


def test_the_restatement_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    eight, four = np.ones((3, 3), int), None
    for plane, n in _random_planes():
        geom, _, _ = R.cell_stats(plane, n)
        h, w = plane.shape
        yy, xx = np.mgrid[:h, :w]
        index = list(range(1, n + 1))
        assert np.array_equal(geom[0, 1:, 0], ndi.sum(np.ones_like(plane), plane, index).astype(np.int64))
        for col, v in ((1, xx), (2, yy), (3, xx * xx), (4, yy * yy), (5, xx * yy)):
            assert np.array_equal(geom[0, 1:, col], ndi.sum(v, plane, index).astype(np.int64)), col
        objs = ndi.find_objects(plane.astype(np.int32), max_label=n)
        for label in index:
            row = geom[0, label]
            if row[0] == 0:
                assert objs[label - 1] is None and row[6:10].tolist() == [w, h, -1, -1]
                continue
            sy, sx = objs[label - 1]
            assert row[6:10].tolist() == [sx.start, sy.start, sx.stop - 1, sy.stop - 1]
            cy, cx = ndi.center_of_mass(plane == label)
            assert abs(row[1] / row[0] - cx) < 1e-9 and abs(row[2] / row[0] - cy) < 1e-9
            mask = plane == label
            comps = ndi.label(mask, eight)[1]
            holes = ndi.label(~np.pad(mask, 1), four)[1] - 1  # the 4-connected background regions but the outside
            assert (row[10] - row[12] - 2 * row[13]) // 4 == comps - holes


def test_cell_measurements_is_the_restatements_descriptors():
    """The moments agree within 1e-10 (mu20 + mu02 + 1): float64 sums of at most 129 x 257 terms carry about 4e-12
    relative error, and the library's side is exact up to one rounding.  Eccentricity and orientation are compared
    only where l1 - l2 > 1e-3 l1: on an isotropic cell they are ill-conditioned."""
    from eunet import metrics as M
    planes = _random_planes() + [(R.blobs(129, 257, 9, 5), 9), (R.noise(37, 131, 50, 6), 50)]
    checked = 0
    for plane, n in planes:
        img = R.image(plane.shape[0], plane.shape[1], 2, 3)
        m = M.cell_measurements(_stats(plane, n + 1, img))  # the last label has no pixel
        assert m["area"][n] == 0 and all(np.isnan(np.asarray(v[n])).all() for k, v in m.items() if k != "area")
        for label in range(1, n + 1):
            d, i = R.descriptors(plane, label), label - 1
            if d is None:
                assert m["area"][i] == 0 and np.isnan(m["centroid_x"][i]) and np.isnan(m["bbox"][i]).all()
                continue
            tol = 1e-10 * (d["mu20"] + d["mu02"] + 1)
            for k in ("mu20", "mu02", "mu11"):
                assert abs(m[k][i] - d[k]) <= tol, (k, m[k][i], d[k])
            for k in ("area", "extent", "perimeter_crack", "euler_number", "holes", "touches_border"):
                assert m[k][i] == d[k], k
            for k in ("centroid_x", "centroid_y", "equivalent_diameter", "perimeter", "circularity"):
                assert abs(m[k][i] - d[k]) <= 1e-12 * max(1.0, abs(d[k])), k
            assert m["bbox"][i].tolist() == list(d["bbox"])
            for k in ("major_axis", "minor_axis"):  # d sqrt(l) = d l / (2 sqrt l): compare the squares
                assert abs(m[k][i] ** 2 - d[k] ** 2) <= 16 * 4 * tol, k
            if d["l1"] - d["l2"] > 1e-3 * d["l1"]:
                # d ecc = d(l2 / l1) / (2 ecc) and d theta = d mu / (l1 - l2): both within 1e3 tol / l1 here
                assert abs(m["eccentricity"][i] ** 2 - d["eccentricity"] ** 2) <= 4 * tol / d["l1"]
                delta = abs(m["orientation"][i] - d["orientation"])
                assert min(delta, math.pi - delta) <= 4 * tol / (d["l1"] - d["l2"])
                checked += 1
            v = img[plane == label].astype(np.float64)
            for ch in range(2):
                assert abs(m[f"mean_{ch}"][i] - v[:, ch].mean()) <= 1e-10
                assert abs(m[f"std_{ch}"][i] - v[:, ch].std()) <= 1e-9
                assert m[f"min_{ch}"][i] == v[:, ch].min() and m[f"max_{ch}"][i] == v[:, ch].max()
    assert checked > 50


def test_pixel_size_scales_lengths_and_areas():
    from eunet import metrics as M
    plane = R.blobs(23, 19, 4, 2)
    one, half = M.cell_measurements(_stats(plane, 4)), M.cell_measurements(_stats(plane, 4), pixel_size=0.5)
    for k in ("centroid_x", "equivalent_diameter", "major_axis", "minor_axis", "perimeter", "perimeter_crack"):
        assert np.array_equal(half[k], one[k] * 0.5, equal_nan=True), k
    for k in ("area", "mu20", "mu11"):
        assert np.array_equal(half[k], one[k] * 0.25, equal_nan=True), k
    for k in ("bbox", "extent", "circularity", "eccentricity", "orientation", "euler_number"):
        assert np.array_equal(half[k], one[k], equal_nan=True), k
    with pytest.raises(ValueError):
        M.cell_measurements(_stats(plane, 4), pixel_size=0.0)
    with pytest.raises(ValueError):
        M.cell_measurements(_stats(plane, 4), plane=1)


def test_the_moment_numerator_is_formed_in_exact_integers():
    """One cell of area 2^26 as a table: the 8192 x 8192 plane filled.  A sum x^2 passes 2^63, so an int64 product
    wraps; the exact numerator gives mu20 = (8192^2 - 1) / 12."""
    from eunet import metrics as M
    s = 8192
    A = s * s
    sx = s * (s * (s - 1) // 2)
    sxx = s * ((s - 1) * s * (2 * s - 1) // 6)
    sxy = (s * (s - 1) // 2) ** 2
    geom = np.zeros((1, 2, 14), np.int64)
    geom[0, 1] = [A, sx, sx, sxx, sxx, sxy, 0, 0, s - 1, s - 1, 4, 4 * (s - 1), 0, 0]
    assert sxx > 1.5e15 and A * sxx > 2 ** 63  # the largest sum x^2 an 8192 x 8192 plane holds: 1.5e15
    with np.errstate(over="ignore"):
        wrapped = np.int64(A) * np.int64(sxx) - np.int64(sx) * np.int64(sx)
    assert int(wrapped) != A * sxx - sx * sx  # what an int64 numerator would have been
    m = M.cell_measurements({"geom": geom, "shape": (s, s)})
    exact = (s * s - 1) / 12
    assert abs(m["mu20"][0] - exact) <= 1e-15 * exact and abs(m["mu02"][0] - exact) <= 1e-15 * exact
    assert m["mu11"][0] == 0 and m["eccentricity"][0] == 0 and m["orientation"][0] == 0
    assert m["centroid_x"][0] == (s - 1) / 2 and m["extent"][0] == 1 and m["perimeter_crack"][0] == 4 * s


def test_population_summary_on_a_hand_made_table():
    from eunet import metrics as M
    meas = {"area": np.array([4.0, 0.0, 10.0, 1.0]), "circularity": np.array([0.5, np.nan, 1.5, 1.0]),
            "bbox": np.zeros((4, 4))}
    s = M.population_summary(meas, keys=("area", "circularity"))
    assert s == {"count": 3.0, "area_mean": 5.0, "area_median": 4.0, "area_std": float(np.std([4.0, 10.0, 1.0])),
                 "circularity_mean": 1.0, "circularity_median": 1.0,
                 "circularity_std": float(np.std([0.5, 1.5, 1.0]))}
    empty = M.population_summary({"area": np.zeros(2), "circularity": np.full(2, np.nan)}, keys=("circularity",))
    assert empty["count"] == 0 and math.isnan(empty["circularity_mean"])
    with pytest.raises(ValueError):
        M.population_summary(meas, keys=("bbox",))
    plane = R.blobs(23, 19, 4, 2)
    full = M.population_summary(M.cell_measurements(_stats(plane, 4)))
    assert set(full) == {"count"} | {f"{k}_{t}" for k in M.MEASUREMENT_SUMMARY_KEYS for t in ("mean", "median", "std")}


def test_measurement_agreement_on_hand_made_tables():
    """Plane 1 of two maps: prediction 1 (area 10) overlaps ground truth 2 (area 12) in 8 pixels, IoU 8 / 14 > 1 / 2:
    matched; prediction 2 (area 6) overlaps ground truth 1 (area 6) in 4, IoU exactly 1 / 2: not matched; prediction 3
    has no partner.  The pair table's areas decide the match, the geom tables' areas are compared."""
    from eunet import metrics as M
    pairs = [(1, 1, 2, 8), (1, 1, 0, 2), (1, 0, 2, 4), (1, 2, 1, 4), (1, 2, 0, 2), (1, 0, 1, 2), (1, 3, 0, 5),
             (0, 1, 1, 9)]
    gp, gg = np.zeros((2, 4, 14), np.int64), np.zeros((2, 3, 14), np.int64)
    gp[1, 1, :3], gp[1, 2, :3], gp[1, 3, :3] = (10, 30, 50), (6, 6, 6), (5, 5, 5)
    gg[1, 1, :3], gg[1, 2, :3] = (6, 12, 6), (12, 72, 48)
    gp[0, 1, :3], gg[0, 1, :3] = (9, 9, 9), (9, 9, 9)
    a = M.measurement_agreement(pairs, gp, gg, 1)
    assert a["matches"].tolist() == [[1, 2]] and a["area_rel"].tolist() == [(10 - 12) / 12]
    assert a["centroid_dist"].tolist() == [math.hypot(3.0 - 6.0, 5.0 - 4.0)]
    assert (a["count_pred"], a["count_gt"], a["area_pred"], a["area_gt"]) == (3, 2, 21, 18)
    b = M.measurement_agreement(pairs, gp, gg, 0)
    assert b["matches"].tolist() == [[1, 1]] and b["area_rel"].tolist() == [0.0] and b["centroid_dist"].tolist() == [0.0]
    s = M.agreement_summary([a, b])
    assert tuple(s) == M.AGREEMENT_KEYS
    assert s == {"n_matched": 2.0, "area_rel_err_mean": (2 / 12) / 2, "area_rel_err_median": (2 / 12) / 2,
                 "area_bias": (-2 / 12) / 2, "centroid_dist_mean": math.hypot(3.0, 1.0) / 2, "count_pred": 4.0,
                 "count_gt": 3.0, "mean_area_pred": 30 / 4, "mean_area_gt": 27 / 3}
    none = M.agreement_summary([M.measurement_agreement([], gp[:, :1], gg[:, :1], 0)])
    assert none["n_matched"] == 0 and math.isnan(none["area_bias"]) and math.isnan(none["mean_area_gt"])


def test_header_library_and_binding_agree_on_the_new_symbol():
    import ctypes
    from eunet import _lib, ops
    src = open(os.path.join(ROOT, "include", "eunet.h")).read()
    lib = _lib.load()
    name = "eunet_cell_stats"
    assert re.search(rf"^int {name}\(", src, flags=re.M)
    assert name in _lib.SIGNATURES and name in _lib.exported_symbols() and hasattr(lib, name)
    decl = re.search(rf"^int {name}\((.*?)\);", src, flags=re.M | re.S).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES[name]) == 12
    assert re.search(rf"^#define EUNET_CELL_GEOM_COLS {_lib.CELL_GEOM_COLS}$", src, flags=re.M)
    assert _lib.CELL_GEOM_COLS == ops.CELL_GEOM_COLS == R.GEOM_COLS == 14
    hip = open(os.path.join(ROOT, "enhanced-unet_amd", "csrc", "cellprops.hip")).read()
    assert "EUNET_DEBUG_UNIT(cellprops)" in hip and hip.count("EUNET_DASSERT") >= 8
    assert "debug_read_cellprops" in open(os.path.join(ROOT, "enhanced-unet_amd", "csrc", "capi.hip")).read()
    # the host-only refusals of the launcher: nothing is dereferenced, nothing is launched
    ok = dict(ids=0x1000, eb=4, p=1, h=8, w=8, n=3, image=None, c=0, geom=0x2000, inten=None, skipped=0x3000)
    bad = [dict(eb=2), dict(p=0), dict(p=65536), dict(h=0), dict(w=8193), dict(n=-1), dict(n=_lib.PAIRS_MAX_ID + 1),
           dict(c=1), dict(image=0x4000, c=0, inten=0x5000), dict(image=0x4000, c=4, inten=0x5000),
           dict(image=0x4000, c=3), dict(geom=0x2004), dict(skipped=0x3004), dict(ids=0x1002), dict(ids=None),
           dict(geom=None), dict(ids=0x1004, eb=8)]
    for change in bad:
        a = dict(ok, **change)
        assert lib.eunet_cell_stats(a["ids"], a["eb"], a["p"], a["h"], a["w"], a["n"], a["image"], a["c"], a["geom"],
                                    a["inten"], a["skipped"], None) != 0, change


def test_cell_stats_refuses_bad_arguments_before_any_device_call():
    """Everything a host tensor can show is refused with ValueError; the device checks come first in the list only
    because a CPU tensor is all this test has, so each case below fails at its own check or at the device check,
    never later."""
    import torch
    from eunet import ops
    ids = torch.zeros(4, 5, dtype=torch.int32)
    cases = [(np.zeros((4, 5)), 1, None), (ids, 1, None), (ids.float(), 1, None), (ids.short(), 1, None),
             (torch.zeros(5, dtype=torch.int32), 1, None), (torch.zeros(1, 1, 4, 5, dtype=torch.int64), 1, None)]
    for a, n, img in cases:
        with pytest.raises(ValueError):
            ops.cell_stats(a, n, img)


def test_cell_stats_argument_checks_in_order(monkeypatch):
    """The remaining refusals, reached with a stand-in for the device check (no device call is made: the C-ABI call is
    replaced by one that fails the test)."""
    import torch
    from eunet import _lib, ops

    def no_call(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(ops, "call", no_call)
    monkeypatch.setattr(ops, "_id_maps", lambda name, what, t: t)
    ids = torch.zeros(4, 5, dtype=torch.int32)
    img = torch.zeros(4, 5, 3, dtype=torch.uint8)
    bad = [(ids, -1, None), (ids, _lib.PAIRS_MAX_ID + 1, None), (ids, 1.5, None), (ids, "3", None),
           (torch.zeros(1, 8193, dtype=torch.int32), 1, None), (torch.zeros(8193, 1, dtype=torch.int64), 1, None),
           (ids, 1, img.float()), (ids, 1, np.zeros((4, 5), np.uint8)), (ids, 1, img[:, :4]), (ids, 1, img[:3]),
           (ids, 1, torch.zeros(4, 5, 4, dtype=torch.uint8)), (ids, 1, torch.zeros(4, 5, 0, dtype=torch.uint8)),
           (ids, 1, torch.zeros(1, 4, 5, 1, dtype=torch.uint8)), (ids, 1, torch.zeros(5, 4, 3, dtype=torch.uint8)),
           (ids, 1, torch.zeros(4, 5, 6, dtype=torch.uint8)[:, :, ::2]),
           (ids, 1, torch.zeros(4, 5, 3, dtype=torch.uint8, device="meta"))]
    for a, n, image in bad:
        with pytest.raises(ValueError):
            ops.cell_stats(a, n, image)
