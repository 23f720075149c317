"""The nearest-cell transform, label expansion and contact table on the host: the restatement of
tests/_neighbors_ref.py held to scipy.ndimage and to itself (all pairs against the separable passes the kernels
follow), metrics.neighbor_graph / neighbor_measurements against hand-derived answers, the agreement of header,
binding and library on the new entries, and what the launchers and the ops refuse before any device call.  No GPU."""
import inspect
import math
import os
import re

import numpy as np
import pytest

import _cellprops_ref as C
import _neighbors_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("eunet_nearest_site", "eunet_expand_label_map", "eunet_label_contacts")


def _random_map(rng):
    h, w = rng.randint(1, 10), rng.randint(1, 10)
    return (rng.rand(h, w) < rng.choice([0.05, 0.2, 0.6])).astype(np.int64) * rng.randint(1, 4, (h, w))


# ---- the restatement ---------------------------------------------------------------------------------------
def test_the_all_pairs_distances_are_scipys():
    from scipy.ndimage import distance_transform_edt
    rng = np.random.RandomState(0)
    seen = 0
    for _ in range(100):
        plane = _random_map(rng)
        if not (plane >= 1).any():
            continue
        seen += 1
        dist, site = R.nearest_site(plane)
        ref = np.rint(distance_transform_edt(plane < 1) ** 2).astype(np.int64)  # distances only: scipy's ties differ
        assert np.array_equal(dist, ref)
        sy, sx = np.divmod(site.astype(np.int64), plane.shape[1])
        yy, xx = np.mgrid[0:plane.shape[0], 0:plane.shape[1]]
        assert np.array_equal((yy - sy) ** 2 + (xx - sx) ** 2, ref) and (plane[sy, sx] >= 1).all()
    assert seen > 80


def test_the_separable_passes_with_the_strict_stop_are_the_all_pairs_minimum():
    rng = np.random.RandomState(1)
    wrong = 0
    for i in range(300):
        plane = _random_map(rng)
        dist, site = R.nearest_site(plane)
        d2, s2 = R.nearest_site_separable(plane)
        assert np.array_equal(dist, d2) and np.array_equal(site, s2), plane
        d3, s3 = R.nearest_site_separable(plane, strict=False)
        assert np.array_equal(dist, d3)  # the distance-only stop is right for distances ...
        wrong += not np.array_equal(site, s3)
    assert wrong > 0  # ... and wrong for sites


def test_the_smallest_counter_example_of_the_distance_only_stop():
    plane = np.array([[1, 0], [0, 1]])
    dist, site = R.nearest_site(plane)
    assert dist.tolist() == [[0, 1], [1, 0]] and site.tolist() == [[0, 0], [0, 3]]
    assert R.nearest_site_separable(plane)[1].tolist() == [[0, 0], [0, 3]]
    assert R.nearest_site_separable(plane, strict=False)[1].tolist() == [[0, 3], [0, 3]]


def test_named_ties_ignored_ids_and_an_empty_plane():
    assert R.nearest_site(np.array([[1, 0, 1]]))[1].tolist() == [[0, 0, 2]]
    above_left = np.array([[0, 0, 5, 0], [0, 0, 0, 0], [7, 0, 0, 0]])  # (2, 2): 2 below (0, 2), 2 right of (2, 0)
    assert R.nearest_site(above_left)[1][2, 2] == 2 and R.nearest_site(above_left)[0][2, 2] == 4
    diag = np.array([[1, 0, 0], [0, 0, 0], [0, 0, 1]])
    assert R.nearest_site(diag)[1][1, 1] == 0 and R.nearest_site(diag)[1][0, 2] == 0
    dist, site = R.nearest_site(np.array([[[0, -1], [-3, 0]], [[0, 2], [0, 0]]]))
    assert (dist[0] == R.NONE).all() and (site[0] == -1).all() and site[1].tolist() == [[1, 1], [1, 1]]


def test_the_expansion_rule():
    ids = np.array([[3, 0, 0, 0, 0, -1, 0, 4]])
    assert R.expand(ids, 0).tolist() == ids.tolist()
    assert R.expand(ids, 1).tolist() == [[3, 3, 0, 0, 0, -1, 4, 4]]
    assert R.expand(ids, 4).tolist() == [[3, 3, 3, 0, 0, -1, 4, 4]]
    assert R.expand(ids).tolist() == [[3, 3, 3, 3, 4, -1, 4, 4]]
    assert R.expand(np.array([[5, 0, 2]])).tolist() == [[5, 5, 2]]  # 1 from both: the site of smaller index
    assert R.expand(np.zeros((2, 3), np.int64)).tolist() == [[0] * 3] * 2


def test_the_contact_count():
    ids = np.array([[1, 1, 2], [1, 3, 2], [0, 3, -5]])
    assert R.contacts(ids, 4).tolist() == [[0, 1, 2, 1], [0, 1, 3, 2], [0, 2, 3, 1]]
    # diagonals: (0,0)-(1,1) 1|3, (0,1)-(1,2) 1|2, (0,2)-(1,1) 2|3, (1,0)-(2,1) 1|3, (1,2)-(2,1) 2|3
    assert R.contacts(ids, 8).tolist() == [[0, 1, 2, 2], [0, 1, 3, 4], [0, 2, 3, 3]]


# ---- the host measurements ---------------------------------------------------------------------------------
def _stats(plane, n):
    return {"geom": C.cell_stats(plane, n)[0], "shape": plane.shape}


def test_two_squares_that_share_a_side():
    from eunet import metrics as M
    plane = np.zeros((4, 6), np.int64)
    plane[1:3, 1:3], plane[1:3, 3:5] = 1, 2
    table = R.contacts(plane, 4)
    assert table.tolist() == [[0, 1, 2, 2]]
    st = _stats(plane, 2)
    m = M.neighbor_measurements(table, st, st, 0)
    assert tuple(m) == M.NEIGHBOR_KEYS
    assert m["shared_border"].tolist() == [2.0, 2.0] and m["touching_fraction"].tolist() == [2 / 8, 2 / 8]
    assert m["n_neighbors"].tolist() == [1.0, 1.0] and m["territory_area"].tolist() == [4.0, 4.0]
    assert m["first_closest_distance"].tolist() == [2.0, 2.0] and m["first_closest_id"].tolist() == [2.0, 1.0]
    assert np.isnan(m["second_closest_distance"]).all() and np.isnan(m["angle_between_neighbors"]).all()
    half = M.neighbor_measurements(table, st, st, 0, pixel_size=0.5)
    assert half["shared_border"].tolist() == [1.0, 1.0] and half["first_closest_distance"].tolist() == [1.0, 1.0]
    assert half["territory_area"].tolist() == [1.0, 1.0] and half["touching_fraction"].tolist() == [0.25, 0.25]
    indptr, indices, weights = M.neighbor_graph(table, 0, 2)
    assert indptr.tolist() == [0, 1, 2] and indices.tolist() == [2, 1] and weights.tolist() == [2, 2]
    # the expanded map's tables are what the fraction and the territory are taken from
    grown = R.expand(plane)
    mg = M.neighbor_measurements(R.contacts(grown, 4), st, _stats(grown, 2), 0)
    assert mg["territory_area"].tolist() == [12.0, 12.0] and mg["shared_border"].tolist() == [4.0, 4.0]
    assert mg["touching_fraction"].tolist() == [4 / 14, 4 / 14] and mg["area"].tolist() == [4.0, 4.0]


def test_three_collinear_cells_a_single_cell_and_an_absent_label():
    from eunet import metrics as M
    plane = np.zeros((3, 12), np.int64)
    plane[1, 1], plane[1, 4], plane[1, 9] = 1, 2, 4  # label 3 has no pixel
    st = _stats(plane, 4)
    m = M.neighbor_measurements(np.zeros((0, 4), np.int64), st, st, 0)
    assert m["angle_between_neighbors"][1] == 180.0  # label 2 sits between 1 and 4
    assert m["angle_between_neighbors"][0] == 0.0 and m["angle_between_neighbors"][3] == 0.0
    assert m["first_closest_id"].tolist()[:2] == [2.0, 1.0] and m["second_closest_id"].tolist()[:2] == [4.0, 4.0]
    assert m["first_closest_distance"].tolist()[:2] == [3.0, 3.0] and m["second_closest_distance"][1] == 5.0
    assert m["first_closest_id"][3] == 2.0 and m["second_closest_distance"][3] == 8.0
    for k in ("first_closest_distance", "second_closest_id", "angle_between_neighbors"):
        assert math.isnan(m[k][2])
    assert m["touching_fraction"][2] == 0.0 and m["n_neighbors"].tolist() == [0.0] * 4 and m["area"][2] == 0.0
    summary = M.population_summary(m, M.NEIGHBOR_KEYS)
    assert summary["count"] == 3.0 and summary["first_closest_distance_mean"] == (3 + 3 + 5) / 3
    one = np.zeros((3, 3), np.int64)
    one[1, 1] = 1
    m1 = M.neighbor_measurements(np.zeros((0, 4), np.int64), _stats(one, 1), _stats(one, 1), 0)
    assert m1["n_neighbors"].tolist() == [0.0] and math.isnan(m1["first_closest_distance"][0])
    assert math.isnan(m1["second_closest_distance"][0]) and math.isnan(m1["first_closest_id"][0])
    m0 = M.neighbor_measurements(np.zeros((0, 4), np.int64), _stats(one, 0), _stats(one, 0), 0)
    assert all(len(v) == 0 for v in m0.values())
    assert M.neighbor_graph(np.zeros((0, 4), np.int64), 0, 0)[0].tolist() == [0]


def test_the_graph_is_symmetric_and_the_tables_are_checked():
    from eunet import metrics as M
    plane = R.blobs(24, 31, 9, 5)
    table = R.contacts(np.stack([plane, plane[::-1]]), 8)
    for q in (0, 1):
        indptr, indices, weights = M.neighbor_graph(table, q, 9)
        dense = np.zeros((10, 10), np.int64)
        for i in range(1, 10):
            dense[i, indices[indptr[i - 1]:indptr[i]]] = weights[indptr[i - 1]:indptr[i]]
            assert (np.diff(indices[indptr[i - 1]:indptr[i]]) > 0).all()
        assert np.array_equal(dense, dense.T) and dense.sum() == 2 * table[table[:, 0] == q][:, 3].sum() > 0
    st = _stats(plane, 9)
    for bad in (table[:, :3], table.astype(np.int32), np.array([[0, 2, 2, 1]]), np.array([[0, 1, 10, 1]]),
                np.array([[0, 0, 1, 1]]), np.array([[0, 1, 2, 0]]), np.array([[0, 1, 2, 1], [0, 1, 2, 1]])):
        with pytest.raises(ValueError):
            M.neighbor_graph(bad, 0, 9)
    with pytest.raises(ValueError):
        M.neighbor_measurements(table, st, _stats(plane, 8), 0)
    with pytest.raises(ValueError):
        M.neighbor_measurements(table, st, st, 1)
    with pytest.raises(ValueError):
        M.neighbor_measurements(table, st, st, 0, pixel_size=0.0)


# ---- header, binding, library ------------------------------------------------------------------------------
def test_header_library_and_binding_agree_on_the_new_symbols():
    from eunet import _lib
    src = open(os.path.join(ROOT, "include", "eunet.h")).read()
    lib = _lib.load()
    for name, nargs in zip(NAMES, (8, 9, 12)):
        assert name in _lib.SIGNATURES and name in _lib.exported_symbols() and hasattr(lib, name)
        decl = re.search(rf"^int {name}\((.*?)\);", src, flags=re.M | re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name]) == nargs
    for rule in ("smallest linear index", "lexicographic minimum", "never overwritten", "floor(distance^2)",
                 "r^2 > best, strictly"):
        assert rule in src, rule
    hip = open(os.path.join(ROOT, "enhanced-unet_amd", "csrc", "neighbors.hip")).read()
    assert "EUNET_DEBUG_UNIT(neighbors)" in hip and hip.count("EUNET_DASSERT") >= 8 and "asm" not in hip
    assert hip.index('#include "common.h"') < hip.index('#include "labelmap.h"') < hip.index("EUNET_DEBUG_UNIT")
    capi = open(os.path.join(ROOT, "enhanced-unet_amd", "csrc", "capi.hip")).read()
    units = re.findall(r"^int debug_read_(\w+)\(", capi, flags=re.M)
    readers = re.findall(r"eunet::debug_read_(\w+)", capi.split("readers[")[1].split("}")[0])
    assert units[-1] == "neighbors" and readers[0] == "capi" and readers[1:] == units and len(readers) == 20


def test_the_signatures_of_the_ops_and_of_the_evaluator_methods():
    from eunet import ops
    from eunet.evaluator import Evaluator

    def params(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]

    e = inspect.Parameter.empty
    assert params(ops.nearest_site) == [("ids", e)]
    assert params(ops.expand_label_map) == [("ids", e), ("distance", None), ("out", None)]
    assert params(ops.label_contacts) == [("ids", e), ("connectivity", 4), ("_table_capacity", None)]
    assert params(Evaluator.measure_neighbors) == [("self", e), ("image", e), ("distance", None), ("min_area", 3),
                                                   ("pixel_size", 1.0), ("connectivity", 4)]
    assert params(Evaluator.measure_cells) == [("self", e), ("image", e), ("intensity", None), ("min_area", 3),
                                                ("pixel_size", 1.0), ("hull", False)]
    assert params(ops.expand_labels) == [("labels", e), ("table", e), ("m", e)]  # the instance unit's op keeps its name


def test_the_launchers_refuse_bad_arguments_on_the_host():
    """Nothing is dereferenced, nothing is launched."""
    from eunet import _lib
    lib = _lib.load()
    ok = dict(ids=0x1000, eb=4, p=1, h=8, w=8, a=0x2000, b=0x3000)
    shapes = [dict(eb=2), dict(eb=0), dict(p=0), dict(p=65536), dict(h=0), dict(h=8193), dict(w=0), dict(w=8193),
              dict(ids=None), dict(ids=0x1002), dict(ids=0x1004, eb=8), dict(a=None), dict(b=None), dict(a=0x2002)]
    for change in shapes + [dict(b=0x3002)]:
        a = dict(ok, **change)
        assert lib.eunet_nearest_site(a["ids"], a["eb"], a["p"], a["h"], a["w"], a["a"], a["b"], None) != 0, change
        assert b"nearest_site" in lib.eunet_last_error()
    for change in shapes + [dict(b=0x3002), dict(b=0x1000), dict(b=0x1080), dict(ids=0x3010)]:  # out over ids
        a = dict(ok, **change)
        rc = lib.eunet_expand_label_map(a["ids"], a["eb"], a["p"], a["h"], a["w"], -1, a["a"], a["b"], None)
        assert rc != 0, change
        assert b"expand_label_map" in lib.eunet_last_error()
    table = dict(conn=4, keys=0x2000, vals=0x3000, cap=8, over=0x4000, inv=0x5000)
    for change in shapes[:11] + [dict(conn=6), dict(conn=0), dict(keys=None), dict(vals=None), dict(over=None),
                                 dict(inv=None), dict(keys=0x2004), dict(inv=0x5004), dict(cap=0), dict(cap=1),
                                 dict(cap=12), dict(cap=2 ** 31)]:
        a = dict(ok, **table)
        a.update(change)
        assert lib.eunet_label_contacts(a["ids"], a["eb"], a["p"], a["h"], a["w"], a["conn"], a["keys"], a["vals"],
                                        a["cap"], a["over"], a["inv"], None) != 0, change
        assert b"label_contacts" in lib.eunet_last_error()


def test_the_ops_refuse_bad_arguments_before_any_device_call(monkeypatch):
    import torch
    from eunet import ops
    ids = torch.zeros(4, 5, dtype=torch.int32)
    for f in (ops.nearest_site, ops.expand_label_map, ops.label_contacts):
        for a in (np.zeros((4, 5)), ids, ids.float()):  # not a tensor, not on the device (checked before the dtype)
            with pytest.raises(ValueError):
                f(a)

    def no_call(*a, **k):
        raise AssertionError("a device call was made")

    class Fake:
        """What _id_maps looks at, of a map that would live on a GPU."""
        is_cuda, device = True, "cuda:0"

        def __init__(self, shape, dtype=torch.int32, contiguous=True):
            self.shape, self.dtype, self._c = shape, dtype, contiguous

        def dim(self):
            return len(self.shape)

        def is_contiguous(self):
            return self._c

        def element_size(self):
            return 4

    monkeypatch.setattr(ops, "call", no_call)
    monkeypatch.setattr(torch, "empty", no_call)
    monkeypatch.setattr(torch, "empty_like", no_call)
    monkeypatch.setattr(torch, "Tensor", Fake)  # isinstance(t, torch.Tensor) inside ops
    maps = [Fake((4, 5), torch.float32), Fake((4, 5), torch.uint8), Fake((4, 5), contiguous=False), Fake((5,)),
            Fake((1, 1, 4, 5)), Fake((1, 8193)), Fake((8193, 1)), Fake((65536, 1, 1)), Fake((0, 5))]
    for f in (ops.nearest_site, ops.expand_label_map, ops.label_contacts):
        for m in maps:
            with pytest.raises(ValueError):
                f(m)
    good = Fake((4, 5))
    for d in (-1, -0.5, float("nan"), "far", [1]):
        with pytest.raises(ValueError):
            ops.expand_label_map(good, d)
    for out in (ids, 3, Fake((4, 6)), Fake((4, 5), torch.int64)):
        with pytest.raises(ValueError):
            ops.expand_label_map(good, 1.0, out=out)
    for c in (0, 6, "4", None, 4.5):
        with pytest.raises(ValueError):
            ops.label_contacts(good, c)
    for cap in (1, 3, 0, 2 ** 31):
        with pytest.raises(ValueError):
            ops.label_contacts(good, 4, _table_capacity=cap)
