"""The per-cell convex hulls on the host: the restatement of tests/_hull_ref.py held to hand-derived answers and to
scipy.spatial.ConvexHull, metrics.hull_measurements on a hand-made table, the agreement of header, binding and
library on the new entry, and what the launcher and ops.cell_hulls refuse before any device call.  No GPU."""
import inspect
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import _hull_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _one(plane):
    ext, verts, hull, row_off, lists = H.cell_hulls(plane, 1)
    return hull[0, 1].tolist(), lists[0][0], ext.tolist()


def test_a_single_pixel():
    plane = np.zeros((1, 1), np.int64) + 1
    row, v, ext = _one(plane)
    assert v == [(0, 0), (1, 0), (1, 1), (0, 1)] and ext == [[0, 0]]
    assert row == [4, 2, 4 * 65536, 2, 0, 0, 1, 1, 1, 1, 0]


def test_a_rectangle_resolves_the_diagonal_tie_to_vertices_0_and_2():
    plane = np.ones((2, 3), np.int64)  # 3 across, 2 down
    row, v, _ = _one(plane)
    assert v == [(0, 0), (3, 0), (3, 2), (0, 2)]
    assert row[:4] == [4, 12, 10 * 65536, 13] and row[4:8] == [0, 0, 3, 2]  # not (3, 0) - (0, 2)
    # the widths c / |e|: 6 / 3 across the top edge, 6 / 2 across the right one; the top edge is also the first
    assert row[8:] == [6, 3, 0]


def test_an_l_and_a_u_have_the_exact_solidity():
    from eunet import metrics as M
    ell = np.zeros((4, 4), np.int64)
    ell[:, 0], ell[3, :] = 1, 1  # area 7; hull (0,0) (1,0) (4,3) (4,4) (0,4): 16 - 9 / 2
    row, v, _ = _one(ell)
    assert v == [(0, 0), (1, 0), (4, 3), (4, 4), (0, 4)] and row[1] == 23
    u = np.ones((3, 5), np.int64)
    u[:2, 1:4] = 0  # area 9; the hull is the 5 x 3 box
    row_u, v_u, ext_u = _one(u)
    assert v_u == [(0, 0), (5, 0), (5, 3), (0, 3)] and row_u[1] == 30 and ext_u == [[0, 4]] * 3
    for plane, area, area2 in ((ell, 7, 23), (u, 9, 30)):
        import _cellprops_ref as R
        hull = H.cell_hulls(plane, 1)[2]
        m = M.hull_measurements({"hull": hull}, {"geom": R.cell_stats(plane, 1)[0]})
        assert m["solidity"][0] == float(Fraction(2 * area, area2)) < 1 and m["convex_area"][0] == area2 / 2


def test_a_staircase_of_slope_one_half_drops_its_collinear_corners():
    row, v, _ = _one(H.staircase(6))
    assert v == [(1, 1), (3, 1), (13, 6), (13, 7), (11, 7), (1, 2)] and row[0] == 6
    # the long edges (10, 5) and (-10, -5) are parallel; from (3, 1) the corner (1, 2) lies at (-2, 1):
    # c = 10 * 1 - 5 * (-2) = 20
    assert row[8:] == [20, 10, 5] and row[3] == 12 * 12 + 6 * 6


def test_a_label_in_two_pieces_has_empty_rows_between():
    plane = np.zeros((7, 6), np.int64)
    plane[0, 1:3], plane[5, 4] = 1, 1
    ext, verts, hull, row_off, lists = H.cell_hulls(plane, 1)
    assert ext.tolist() == [[1, 2], [6, -1], [6, -1], [6, -1], [6, -1], [4, 4]] and row_off.tolist() == [0, 0, 6]
    assert lists[0][0] == [(1, 0), (3, 0), (5, 5), (5, 6), (4, 6), (1, 1)]
    assert verts[2:8].tolist() == [list(q) for q in lists[0][0]] and not verts[8:].any() and not verts[:2].any()


def test_the_restatement_against_scipy():
    sp = pytest.importorskip("scipy.spatial")
    rng = np.random.default_rng(11)
    for k in range(50):
        h, w = int(rng.integers(2, 18)), int(rng.integers(2, 18))
        plane = H.blob(rng, h, w)
        assert plane.sum() >= 2
        pts = sorted(H.corners(plane, 1))
        row, v, _ = _one(plane)
        q = sp.ConvexHull(np.asarray(pts, np.float64))
        assert {pts[i] for i in q.vertices.tolist()} == set(v), k
        # the area.  Qhull sums at most 40 float64 terms below 18^2 = 324: its own error stays below 40 * 324 * 2^-52
        # = 3e-12, so its volume is held to 1e-10; the exact form of the same statement is the integer shoelace sum
        # over Qhull's own vertices (2-d vertices come in counterclockwise order for x right, y up: negative here)
        assert abs(q.volume - row[1] / 2) <= 1e-10
        ring = [pts[i] for i in q.vertices.tolist()]
        assert abs(sum(a[0] * b[1] - b[0] * a[1] for a, b in zip(ring, ring[1:] + ring[:1]))) == row[1]
        assert 2 * int(plane.sum()) <= row[1] and 4 <= row[0] <= 2 * (int(np.ptp(np.nonzero(plane)[0])) + 2)


def test_hull_measurements_on_a_hand_made_table():
    from eunet import metrics as M
    hull, geom = np.zeros((1, 4, 11), np.int64), np.zeros((1, 4, 14), np.int64)
    hull[0, 1] = [4, 12, 10 * 65536, 13, 0, 0, 3, 2, 6, 3, 0]   # the 3 x 2 rectangle
    geom[0, 1, 0], geom[0, 1, 10:] = 6, (4, 6, 0, 0)
    hull[0, 3] = [5, 23, 12 * 65536 + 65536, 32, 0, 0, 4, 4, 12, -4, 0]  # the L, its perimeter rounded to a number
    geom[0, 3, 0], geom[0, 3, 10:] = 7, (5, 10, 1, 0)
    geom[0, 2, 6:10] = (9, 9, -1, -1)  # label 2 has no pixel
    one = M.hull_measurements({"hull": hull}, {"geom": geom})
    assert tuple(one) == M.HULL_KEYS and all(v.shape == (3,) and v.dtype == np.float64 for v in one.values())
    assert all(np.isnan(v[1]) for v in one.values()) and not any(np.isnan(v[[0, 2]]).any() for v in one.values())
    assert one["convex_area"].tolist()[0] == 6 and one["solidity"][0] == 1 and one["solidity"][2] == 14 / 23
    assert one["convex_perimeter"][0] == 10 and one["convexity"][0] == 1 and one["convexity"][2] == 13 / 16
    assert one["feret_max"][0] == math.sqrt(13) and one["feret_max_angle"][0] == math.atan2(2, 3)
    assert one["feret_min"][0] == 2 and one["feret_min_angle"][0] == math.pi / 2  # across the horizontal top edge
    assert one["feret_min"][2] == 3 and one["feret_min_angle"][2] == math.pi / 2 and one["hull_vertices"][2] == 5
    assert one["feret_ratio"][0] == 2 / math.sqrt(13) and (one["feret_min"][[0, 2]] <= one["feret_max"][[0, 2]]).all()
    half = M.hull_measurements({"hull": hull}, {"geom": geom}, pixel_size=0.5)
    for k in ("convex_perimeter", "feret_max", "feret_min"):
        assert np.array_equal(half[k], one[k] * 0.5, equal_nan=True), k
    assert np.array_equal(half["convex_area"], one["convex_area"] * 0.25, equal_nan=True)
    for k in ("solidity", "convexity", "feret_max_angle", "feret_min_angle", "feret_ratio", "hull_vertices"):
        assert np.array_equal(half[k], one[k], equal_nan=True), k
    for bad in (dict(pixel_size=0.0), dict(plane=1)):
        with pytest.raises(ValueError):
            M.hull_measurements({"hull": hull}, {"geom": geom}, **bad)
    with pytest.raises(ValueError):
        M.hull_measurements({"hull": hull}, {"geom": geom[:, :3]})
    assert set(M.HULL_KEYS).isdisjoint(M.cell_measurements({"geom": geom, "shape": (9, 9)}))  # its key set is untouched


def test_the_angles_are_folded_into_the_half_open_half_turn():
    from eunet import metrics as M
    a = M._fold_angle(np.array([0.0, 1.0, -1.0, 1.0, -1.0, 0.0]), np.array([1.0, 0.0, 0.0, -1.0, -1.0, -1.0]))
    assert np.allclose(a, [0.0, math.pi / 2, math.pi / 2, -math.pi / 4, math.pi / 4, 0.0], atol=1e-15)
    assert (a > -math.pi / 2).all() and (a <= math.pi / 2).all()


def test_header_library_and_binding_agree_on_the_new_symbol():
    from eunet import _lib, ops
    src = open(os.path.join(ROOT, "include", "eunet.h")).read()
    lib = _lib.load()
    name = "eunet_cell_hulls"
    assert re.search(rf"^int {name}\(", src, flags=re.M)
    assert name in _lib.SIGNATURES and name in _lib.exported_symbols() and hasattr(lib, name)
    decl = re.search(rf"^int {name}\((.*?)\);", src, flags=re.M | re.S).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES[name]) == 13
    assert re.search(rf"^#define EUNET_CELL_HULL_COLS {_lib.CELL_HULL_COLS}$", src, flags=re.M)
    assert _lib.CELL_HULL_COLS == ops.CELL_HULL_COLS == H.HULL_COLS == 11
    assert re.search(rf"^#define EUNET_CELL_HULL_MAX_ROWS {_lib.CELL_HULL_MAX_ROWS} ", src, flags=re.M)
    hip = open(os.path.join(ROOT, "enhanced-unet_amd", "csrc", "hull.hip")).read()
    assert "EUNET_DEBUG_UNIT(hull)" in hip and hip.count("EUNET_DASSERT") >= 8 and "asm" not in hip
    capi = open(os.path.join(ROOT, "enhanced-unet_amd", "csrc", "capi.hip")).read()
    units = re.findall(r"^int debug_read_(\w+)\(", capi, flags=re.M)
    assert "hull" in units and "cellprops" in units
    assert all(f"eunet::debug_read_{u}" in capi.split("readers[")[1] for u in units + ["capi"])  # every unit reported


def test_the_launcher_refuses_bad_arguments_on_the_host():
    """Nothing is dereferenced, nothing is launched."""
    from eunet import _lib
    lib = _lib.load()
    ok = dict(ids=0x1000, eb=4, p=1, h=8, w=8, n=3, off=0x2000, y0=0x3000, ext=0x4000, verts=0x5000, hull=0x6000,
              outside=0x7000)
    bad = [dict(eb=2), dict(eb=0), dict(p=0), dict(p=65536), dict(h=0), dict(h=8193), dict(w=0), dict(w=8193),
           dict(n=-1), dict(n=_lib.PAIRS_MAX_ID + 1), dict(ids=None), dict(off=None), dict(y0=None), dict(ext=None),
           dict(verts=None), dict(hull=None), dict(outside=None), dict(ids=0x1002), dict(ids=0x1004, eb=8),
           dict(off=0x2004), dict(y0=0x3002), dict(ext=0x4004), dict(verts=0x5004), dict(hull=0x6004),
           dict(outside=0x7004)]
    for change in bad:
        a = dict(ok, **change)
        assert lib.eunet_cell_hulls(a["ids"], a["eb"], a["p"], a["h"], a["w"], a["n"], a["off"], a["y0"], a["ext"],
                                    a["verts"], a["hull"], a["outside"], None) != 0, change
        assert b"cell_hulls" in lib.eunet_last_error()


def test_cell_hulls_refuses_bad_arguments_before_any_device_call(monkeypatch):
    import torch
    from eunet import ops
    ids = torch.zeros(4, 5, dtype=torch.int32)
    geom = np.zeros((1, 3, 14), np.int64)
    geom[0, 1:, 6:10] = (5, 4, -1, -1)
    good = {"geom": geom, "shape": (4, 5)}
    for a in (np.zeros((4, 5)), ids, ids.float()):  # not a tensor, not on the device, not integer
        with pytest.raises(ValueError):
            ops.cell_hulls(a, good)

    def no_call(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(ops, "call", no_call)
    monkeypatch.setattr(ops, "upload", no_call)
    monkeypatch.setattr(ops, "_id_maps", lambda name, what, t: t)
    box = geom.copy()
    box[0, 1, 6:10] = (0, 2, 4, 4)  # rows 2..4 of a map of 4 rows
    neg = geom.copy()
    neg[0, 2, 6:10] = (0, -1, 4, 1)
    huge = np.zeros((1, 2 ** 15 + 2, 14), np.int64)
    huge[0, 1:, 7], huge[0, 1:, 9] = 0, 8191  # 2^15 + 1 labels of 8192 rows: above 2^28
    bad = [(ids, None), (ids, {"geom": geom}), (ids, {"shape": (4, 5)}), (ids, {"geom": geom, "shape": (5, 4)}),
           (ids, {"geom": geom.astype(np.int32), "shape": (4, 5)}), (ids, {"geom": geom[0], "shape": (4, 5)}),
           (ids, {"geom": geom[:, :, :13], "shape": (4, 5)}), (ids, {"geom": geom[:, :0], "shape": (4, 5)}),
           (ids, {"geom": np.concatenate([geom, geom]), "shape": (4, 5)}), (ids, {"geom": box, "shape": (4, 5)}),
           (ids, {"geom": neg, "shape": (4, 5)}),
           (torch.zeros(1, 8193, dtype=torch.int32), {"geom": geom, "shape": (1, 8193)}),
           (torch.zeros(8192, 1, dtype=torch.int32), {"geom": huge, "shape": (8192, 1)})]
    for a, stats in bad:
        with pytest.raises(ValueError):
            ops.cell_hulls(a, stats)


def test_measure_cells_takes_hull_last_and_off_by_default():
    from eunet.evaluator import Evaluator
    params = list(inspect.signature(Evaluator.measure_cells).parameters.values())
    assert [q.name for q in params] == ["self", "image", "intensity", "min_area", "pixel_size", "hull"]
    assert params[-1].default is False
