"""The watershed definition (tests/_watershed_ref.py) against answers worked out by hand and against the figures
the default depth rests on, and the host half of the product (eunet.ops.merge_basins) against the restatement."""
import math
import os

import numpy as np
import pytest

import _watershed_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_a_row_with_two_peaks_on_both_sides_of_the_depth_boundary():
    """D = 1 4 9 4 9 16 9 4 1.  Pixel 3 (D 4) sees 9 on both sides and takes the smaller index, so the basins are
    {0..3} (root 2, peak 9) and {4..8} (root 5, peak 16); the only pair across is (3, 4): saddle min(4, 9) = 4.  The
    lower basin joins when sqrt(9) - sqrt(4) = 1 < depth."""
    D = np.array([[1, 4, 9, 4, 9, 16, 9, 4, 1]], np.int64)
    b = R.Basins(D)
    assert b.root.tolist() == [2, 2, 2, 2, 5, 5, 5, 5, 5] and b.sad == {(2, 5): 4}
    for depth in (0.0, 0.5, 1.0):
        ids, m, areas = b.split(depth)
        assert ids.tolist() == [[1, 1, 1, 1, 2, 2, 2, 2, 2]] and m == 2 and areas.tolist() == [4, 5]
    for depth in (1.0 + 1e-9, 1.25, math.inf):
        ids, m, areas = b.split(depth)
        assert ids.tolist() == [[1] * 9] and m == 1 and areas.tolist() == [9]


def test_a_flat_plateau_is_one_region_by_the_index_tie_break_alone():
    for value in (5, R.NONE):
        D = np.full((4, 6), value, np.int64)
        b = R.Basins(D)
        assert set(b.root.tolist()) == {0} and b.sad == {}
        ids, m, areas = b.split(0.0)
        assert (ids == 1).all() and m == 1 and areas.tolist() == [24]
    D = np.full((4, 6), 5, np.int64)
    D[:, 3] = 0  # two plateaus: two regions, numbered in raster order
    ids, m, areas = R.split(D, math.inf)
    assert m == 2 and (ids[:, :3] == 1).all() and (ids[:, 4:] == 2).all() and areas.tolist() == [12, 8]


def test_exact_distance_of_the_restatement():
    m = np.zeros((5, 7), bool)
    m[1:4, 1:6] = True
    D = R.edt_sq(m)
    assert D[2].tolist() == [0, 1, 4, 4, 4, 1, 0] and D[1].tolist() == [0, 1, 1, 1, 1, 1, 0]
    assert (R.edt_sq(np.ones((3, 4), bool)) == R.NONE).all() and (R.edt_sq(np.zeros((3, 4), bool)) == 0).all()


def test_two_overlapping_discs():
    """Radius 8, centres 12 apart: two regions up to depth 2, one at 3.  10 apart: two up to depth 1."""
    D = R.edt_sq(R.discs(40, 60, [(20, 20, 8), (20, 32, 8)]))
    b = R.Basins(D)
    assert [b.split(d)[1] for d in (0, 0.5, 1.0, 1.5, 2.0, 3.0)] == [2, 2, 2, 2, 2, 1]
    ids, _, areas = b.split(1.0)
    assert ids[20, 14] == 1 and ids[20, 38] == 2 and int(areas.sum()) == int((D > 0).sum())
    b = R.Basins(R.edt_sq(R.discs(40, 60, [(20, 20, 8), (20, 30, 8)])))
    assert [b.split(d)[1] for d in (0.5, 1.0)] == [2, 2] and b.split(math.inf)[1] == 1


def test_single_ellipses_stay_whole_at_the_default_depth():
    """60 random ellipses, semi-axes 4..18 x 4..12 at any angle and fractional centre: one region each at depth
    1.0, 1.5 and 2.0 (the default is 1.0); at 0.5 two of them are over-split."""
    rng = np.random.default_rng(0)
    bad = {0.5: 0, 1.0: 0, 1.5: 0, 2.0: 0}
    for _ in range(60):
        h = w = 48
        yy, xx = np.mgrid[0:h, 0:w]
        cy, cx = rng.uniform(20, 28, 2)
        a, b = rng.uniform(4, 18), rng.uniform(4, 12)
        th = rng.uniform(0, np.pi)
        u = (yy - cy) * np.cos(th) + (xx - cx) * np.sin(th)
        v = -(yy - cy) * np.sin(th) + (xx - cx) * np.cos(th)
        basins = R.Basins(R.edt_sq((u / a) ** 2 + (v / b) ** 2 <= 1))
        for d in bad:
            bad[d] += basins.split(d)[1] != 1
    assert bad == {0.5: 2, 1.0: 0, 1.5: 0, 2.0: 0}


@pytest.mark.parametrize("density", [0.5, 0.7, 0.9])
def test_infinite_depth_is_connected_component_labelling(density):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(int(density * 10))
    m = rng.random((37, 131)) < density
    D = R.edt_sq(m)
    assert np.array_equal(D, np.rint(ndimage.distance_transform_edt(m) ** 2).astype(np.int64))
    b = R.Basins(D)
    ids, n, areas = b.split(math.inf)
    ref, n_ref = ndimage.label(m, structure=np.ones((3, 3), int))
    assert n == n_ref and np.array_equal(ids, ref)
    assert areas.tolist() == np.bincount(ref.ravel())[1:].tolist()
    # a region never spans two components, whatever the depth
    for depth in (0.0, 1.0):
        part, k, _ = b.split(depth)
        assert k >= n and len(set(zip(part[m].tolist(), ref[m].tolist()))) == k


# ---- the host half of the product ---------------------------------------------------------------------------
def _device_view(b):
    """What the device hands merge_basins for one plane: the basins as slots in raster order of their first pixel,
    with root and peak, and the saddle edges between slots."""
    first = {}
    for p in np.flatnonzero(b.root >= 0).tolist():
        first.setdefault(int(b.root[p]), p)
    order = sorted(first, key=first.get)
    slot = {r: i for i, r in enumerate(order)}
    root = np.array(order, np.int64)
    peak = b.D.ravel()[root] if len(order) else np.zeros(0, np.int64)
    edges = [(min(slot[a], slot[c]), max(slot[a], slot[c]), s) for (a, c), s in b.sad.items()]
    return slot, root, peak, np.array(edges, np.int64).reshape(-1, 3)


@pytest.mark.parametrize("depth", [0.0, 0.5, 1.0, 2.0, math.inf])
def test_merge_basins_equals_the_restatement_on_two_planes(depth):
    from eunet import ops
    rng = np.random.default_rng(5)
    planes = [R.Basins(R.edt_sq(rng.random((23, 41)) < 0.8)),
              R.Basins(R.edt_sq(R.discs(23, 41, [(11, 12, 8), (11, 24, 8), (3, 36, 4)])))]
    views = [_device_view(b) for b in planes]
    offs = np.concatenate([[0], np.cumsum([len(v[1]) for v in views])])
    rng.shuffle(views[0][3])  # the hash table hands the edges over in no order
    a = np.concatenate([v[3][:, 0] + offs[i] for i, v in enumerate(views)])
    c = np.concatenate([v[3][:, 1] + offs[i] for i, v in enumerate(views)])
    s = np.concatenate([v[3][:, 2] for v in views])
    table, m = ops.merge_basins(np.concatenate([v[2] for v in views]), np.concatenate([v[1] for v in views]), offs,
                                a, c, s, depth)
    assert table.dtype == np.int32 and m.dtype == np.int64
    for i, (b, v) in enumerate(zip(planes, views)):
        ids, n, _ = b.split(depth)
        assert int(m[i]) == n
        got = np.zeros(b.root.shape, np.int32)
        fg = b.root >= 0
        got[fg] = [table[offs[i] + v[0][int(r)]] for r in b.root[fg]]
        assert np.array_equal(got.reshape(ids.shape), ids)


def test_merge_basins_without_basins_or_edges():
    from eunet import ops
    table, m = ops.merge_basins([], [], [0, 0], [], [], [], 1.0)
    assert len(table) == 0 and m.tolist() == [0]
    table, m = ops.merge_basins([9, 4], [7, 2], [0, 1, 2], [], [], [], math.inf)
    assert table.tolist() == [1, 1] and m.tolist() == [1, 1]


def test_the_header_declares_the_watershed_and_the_debug_unit():
    from eunet import _lib
    src = open(os.path.join(ROOT, "include", "eunet.h")).read()
    for name in ("eunet_watershed_workspace_bytes", "eunet_watershed_basins", "eunet_watershed_peaks",
                 "eunet_watershed_saddles", "eunet_watershed_relabel"):
        assert name in src and name in _lib.SIGNATURES and name in _lib.exported_symbols()
        assert hasattr(_lib.load(), name), name
    assert "13 watershed" in src  # the debug build's unit list
    hip = open(os.path.join(ROOT, "enhanced-unet_amd", "csrc", "watershed.hip")).read()
    assert "EUNET_DEBUG_UNIT(watershed)" in hip and hip.count("EUNET_DASSERT") >= 10


def test_evaluator_split_argument():
    import inspect
    from eunet.evaluator import Evaluator
    sig = inspect.signature(Evaluator.__init__)
    for name, default in (("split", "erosion"), ("split_depth", 1.0)):
        assert sig.parameters[name].default == default and sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
    ev = Evaluator(None, "cpu", "unet")
    assert ev.split == "erosion" and ev.split_depth == 1.0
    assert Evaluator(None, "cpu", "unet", split="watershed", split_depth=2).split_depth == 2.0
    for kw in (dict(split="flood"), dict(split=None), dict(split_depth=-1.0), dict(split_depth=float("nan")),
               dict(split_depth="deep")):
        with pytest.raises(ValueError):
            Evaluator(None, "cpu", "unet", **kw)
