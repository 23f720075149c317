"""ops.nearest_site, ops.expand_label_map, ops.label_contacts (csrc/neighbors.hip) and Evaluator.measure_neighbors
against the plain-loop restatement of tests/_neighbors_ref.py.  Everything is an integer: every comparison is
torch.equal / np.array_equal, no tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _cellprops_ref as C
import _neighbors_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the column pass's 64-column blocks and 16-row chunks and the row pass's 256 threads, each with one below and above
SHAPES = [(1, 1), (1, 70), (70, 1), (15, 63), (16, 64), (17, 65), (33, 130), (3, 255), (2, 256), (3, 257)]
_REF = {}


def _dev(a, dtype=torch.int64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def _sparse(h, w, seed, density=0.08):
    rng = np.random.RandomState(seed)
    ids = (rng.rand(h, w) < density) * rng.randint(1, 6, (h, w))
    ids[rng.rand(h, w) < 0.05] = -2  # ignored pixels are no sites
    return ids.astype(np.int64)


def _ref_sites(key, ids):
    """The restatement's (dist, site) of a map, computed once per key."""
    if key not in _REF:
        _REF[key] = R.nearest_site(ids)
    return _REF[key]


def _check_sites(ids, dtype=torch.int64, key=None):
    from eunet import ops
    ids = np.asarray(ids)
    dist, site = ops.nearest_site(_dev(ids, dtype))
    rd, rs = R.nearest_site(ids) if key is None else _ref_sites(key, ids)
    assert dist.dtype == torch.int32 and site.dtype == torch.int32 and dist.shape == ids.shape == site.shape
    assert np.array_equal(site.cpu().numpy(), rs), np.argwhere(site.cpu().numpy() != rs)[:5]
    assert np.array_equal(dist.cpu().numpy(), rd)
    return dist, site


# ---- nearest_site ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("shape", SHAPES)
def test_sites_equal_the_all_pairs_minimum_at_the_block_and_chunk_edges(shape, dtype):
    h, w = shape
    ids = _sparse(h, w, 100 * h + w)
    ids[h // 2, w // 2] = 3  # at least one site
    _check_sites(ids, dtype, key=shape)
    far = np.zeros((h, w), np.int64)  # one site in the last corner: every pixel scans to the end of its row
    far[h - 1, w - 1] = 7
    _check_sites(far, dtype, key=shape + ("far",))


def test_the_named_ties():
    d, s = _check_sites(np.array([[1, 0], [0, 1]]))
    assert s.tolist() == [[0, 0], [0, 3]] and d.tolist() == [[0, 1], [1, 0]]  # (0, 1): site 0, not site 3
    assert _check_sites(np.array([[1, 0, 1]]))[1].tolist() == [[0, 0, 2]]
    above_left = np.array([[0, 0, 5, 0], [0, 0, 0, 0], [7, 0, 0, 0]])  # (2, 2): 2 below (0, 2), 2 right of (2, 0)
    d, s = _check_sites(above_left)
    assert s[2, 2].item() == 2 and d[2, 2].item() == 4
    diag = np.array([[1, 0, 0], [0, 0, 0], [0, 0, 1]])
    d, s = _check_sites(diag)
    assert s[1, 1].item() == 0 and s[0, 2].item() == 0 and s[2, 0].item() == 0 and d[1, 1].item() == 2
    both = np.array([[0, 4, 0], [0, 0, 0], [0, 4, 0]])  # above and below at the same distance: the row above
    assert _check_sites(both)[1][1].tolist() == [1, 1, 1]


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_a_stack_whose_middle_plane_has_no_site_and_a_plane_that_is_all_sites(dtype):
    h, w = 19, 67
    stack = np.stack([_sparse(h, w, 1), np.where(_sparse(h, w, 2) < 0, -2, 0), np.full((h, w), 9, np.int64)])
    d, s = _check_sites(stack, dtype)
    assert (d[1] == R.NONE).all() and (s[1] == -1).all()
    assert torch.equal(s[2].cpu(), torch.arange(h * w, dtype=torch.int32).reshape(h, w)) and (d[2] == 0).all()
    alone, _ = _check_sites(stack[0], dtype)
    assert torch.equal(alone, d[0])  # untouched by its neighbour


@pytest.mark.parametrize("case", [(96, 130, 12, 3), (75, 97, 5, 4), (40, 128, 30, 5)])
def test_random_blob_maps(case):
    h, w, n, seed = case
    _check_sites(R.blobs(h, w, n, seed, ignore=True), torch.int32)


def test_two_runs_give_identical_bits():
    from eunet import ops
    ids = _dev(R.blobs(64, 130, 9, 8), torch.int32)
    a, b = ops.nearest_site(ids), ops.nearest_site(ids)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(ops.expand_label_map(ids), ops.expand_label_map(ids))


# ---- expand_label_map --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_the_floor_of_the_squared_distance_decides(dtype):
    from eunet import ops
    ids = np.zeros((7, 9), np.int64)
    ids[3, 4] = 6
    dev = _dev(ids, dtype)
    assert torch.equal(ops.expand_label_map(dev, 0), dev)
    for distance, limit2, area in ((1, 1, 5), (1.5, 2, 9), (2, 4, 13), (0.99, 0, 1), (2.9, 8, 25)):
        got = ops.expand_label_map(dev, distance)
        assert got.dtype == dtype and np.array_equal(got.cpu().numpy(), R.expand(ids, limit2)), distance
        assert int((got == 6).sum()) == area
    assert (ops.expand_label_map(dev) == 6).all() and (ops.expand_label_map(dev, 1e9) == 6).all()


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("distance", [None, 0, 1.5, 3, 7.2])
def test_expansion_keeps_every_id_and_negative_ones_and_leaves_an_empty_plane_alone(distance, dtype):
    from eunet import ops
    h, w = 33, 130
    empty = np.where(_sparse(h, w, 11) < 0, -2, 0)
    stack = np.stack([R.blobs(h, w, 4, 10, ignore=True), empty, _sparse(h, w, 12, 0.01)])
    limit2 = None if distance is None else int(np.floor(distance * distance))
    key = ("expand", distance)
    if key not in _REF:
        _REF[key] = R.expand(stack, limit2)
    dev = _dev(stack, dtype)
    got = ops.expand_label_map(dev, distance)
    assert np.array_equal(got.cpu().numpy(), _REF[key])
    assert torch.equal(got[dev != 0], dev[dev != 0]) and torch.equal(got[1], dev[1]) and (dev[1] < 0).any()
    if distance is None:
        assert (got[0] != 0).all() and (got[2] != 0).all()  # the Voronoi partition leaves no background
    out = torch.full_like(dev, 77)
    assert ops.expand_label_map(dev, distance, out=out) is out and torch.equal(out, got)  # written in place
    with pytest.raises(ValueError):
        ops.expand_label_map(dev, distance, out=dev)
    with pytest.raises(ValueError):
        ops.expand_label_map(dev, distance, out=out[:, :, :-1])


# ---- label_contacts ----------------------------------------------------------------------------------------
def _check_contacts(ids, connectivity, dtype=torch.int64, **kw):
    from eunet import ops
    got = ops.label_contacts(_dev(ids, dtype), connectivity, **kw)
    ref = R.contacts(ids, connectivity)
    assert got.dtype == np.int64 and got.shape == ref.shape and np.array_equal(got, ref)
    return got


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (33, 65), (3, 255), (3, 256), (2, 257), (5, 513), (9, 1)])
def test_contacts_of_noise_and_blobs(shape, dtype, connectivity):
    h, w = shape
    rng = np.random.RandomState(h * 1000 + w)
    noise = rng.randint(-1, 6, (h, w)).astype(np.int64)  # every pixel on a border, the last row and column too
    _check_contacts(noise, connectivity, dtype)
    _check_contacts(np.stack([R.blobs(h, w, 6, h + w, ignore=True), noise, np.zeros((h, w), np.int64)]), connectivity,
                    dtype)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_a_straight_contact_longer_than_a_waves_run_and_contacts_across_waves_and_blocks(dtype):
    ids = np.zeros((6, 1100), np.int64)  # 5 waves a row, more than a block's 4
    ids[0], ids[1], ids[2], ids[3] = 1, 2, 2, 3
    ids[4, :256], ids[4, 256:1024], ids[4, 1024:] = 4, 5, 6  # borders on the first pixel of a wave and of a block
    ids[5, :255], ids[5, 255:] = 7, 8  # ... and on the last of one
    got4 = _check_contacts(ids, 4, dtype)
    assert [0, 1, 2, 1100] in got4.tolist() and [0, 2, 3, 1100] in got4.tolist() and [0, 4, 5, 1] in got4.tolist()
    got8 = _check_contacts(ids, 8, dtype)
    assert [0, 1, 2, 1100 + 2 * 1099] in got8.tolist()
    _check_contacts(ids[:, 1:], 4, dtype)  # rows that start off the 16-byte boundary


def test_ids_that_take_no_part_an_id_too_large_and_the_regrown_table():
    from eunet import ops
    ids = np.array([[0, 1, -3, 2], [2, 0, 0, 2], [0, 1, 0, -1]])  # 1 and 2 meet on two diagonals only
    assert _check_contacts(ids, 4).tolist() == []
    assert _check_contacts(ids, 8).tolist() == [[0, 1, 2, 2]]
    top = np.array([[1, 2 ** 24 - 1], [5, 1]])
    assert _check_contacts(top, 4).tolist() == [[0, 1, 5, 2], [0, 1, 2 ** 24 - 1, 2]]
    for dtype in (torch.int32, torch.int64):
        with pytest.raises(ValueError):
            ops.label_contacts(_dev(np.array([[1, 2 ** 24], [5, 1]]), dtype))
    noise = np.random.RandomState(5).randint(0, 40, (33, 65)).astype(np.int64)
    for connectivity in (4, 8):
        roomy = _check_contacts(noise, connectivity)
        small = _check_contacts(noise, connectivity, _table_capacity=2)  # regrown eight times and more
        assert np.array_equal(roomy, small) and len(roomy) > 256
        assert np.array_equal(roomy, ops.label_contacts(_dev(noise), connectivity))  # two runs, identical arrays


# ---- the evaluator -----------------------------------------------------------------------------------------
_STATE = {}


def _model():
    if "model" not in _STATE:
        from eunet.models import EnhancedUNet
        torch.manual_seed(3)
        _STATE["model"] = EnhancedUNet(num_classes=3, in_channels=3, base_ch=16).to(DEV).eval()
    return _STATE["model"]


def _mask_evaluator(masks, **kw):
    """An Evaluator whose predicted masks are given, one per call (tests/test_gpu_cellprops.py's): a randomly
    initialised small model predicts no usable cells, and what is under test here is everything after the mask."""
    from eunet.evaluator import Evaluator
    ev = Evaluator(_model(), DEV, "enhanced_unet", preprocess=None, **kw)
    queue = [torch.from_numpy(np.ascontiguousarray(m).astype(np.int64)).to(DEV) for m in masks]
    ev._predict_mask_device = lambda image: queue.pop(0)
    return ev


@pytest.mark.parametrize("distance,connectivity", [(None, 4), (3, 4), (None, 8)])
def test_measure_neighbors_is_neighbor_measurements_on_the_ops_outputs(distance, connectivity):
    from eunet import metrics as M
    from eunet import ops, synth
    x, sem = synth.tile(96, 128, 40, num_classes=3, in_channels=3)
    sem = np.ascontiguousarray(sem).astype(np.int64)
    image = torch.from_numpy(np.asarray(x))
    ev = _mask_evaluator([sem, sem], split="watershed")
    got = ev.measure_neighbors(image, distance=distance, pixel_size=0.5, connectivity=connectivity)
    ids, counts, _ = ev.semantic_to_instance_maps(torch.from_numpy(sem).to(DEV))
    n_live, n_dead = counts
    assert min(counts) >= 1 and (got["n_live"], got["n_dead"]) == (n_live, n_dead)
    assert set(got) == {"live", "dead", "n_live", "n_dead", "graph"}
    pooled = ids[0].cpu().numpy().astype(np.int64)
    dead = ids[1].cpu().numpy().astype(np.int64)
    assert not ((pooled > 0) & (dead > 0)).any()  # disjoint by construction
    pooled = pooled + np.where(dead > 0, dead + n_live, 0)
    n = n_live + n_dead
    grown = ops.expand_label_map(_dev(pooled, torch.int32), distance)
    assert np.array_equal(grown.cpu().numpy(), R.expand(pooled, None if distance is None else distance * distance))
    table = ops.label_contacts(grown, connectivity)
    assert np.array_equal(table, R.contacts(grown.cpu().numpy(), connectivity))
    assert distance is not None or len(table) > 0
    stats = {"geom": C.cell_stats(pooled, n)[0], "shape": pooled.shape}
    stats_e = {"geom": C.cell_stats(grown.cpu().numpy().astype(np.int64), n)[0], "shape": pooled.shape}
    ref = M.neighbor_measurements(table, stats, stats_e, 0, 0.5)
    indptr, indices, weights = got["graph"]
    for a, b in zip(got["graph"], M.neighbor_graph(table, 0, n)):
        assert np.array_equal(a, b)
    dense = np.zeros((n + 1, n + 1), np.int64)
    for i in range(1, n + 1):
        dense[i, indices[indptr[i - 1]:indptr[i]]] = weights[indptr[i - 1]:indptr[i]]
    assert np.array_equal(dense, dense.T) and dense.sum() == 2 * table[:, 3].sum()
    same = np.concatenate([(dense[1:n_live + 1, 1:n_live + 1] > 0).sum(1),
                           (dense[n_live + 1:, n_live + 1:] > 0).sum(1)])
    assert set(got["live"]) == set(got["dead"]) == set(M.NEIGHBOR_KEYS) | {"n_neighbors_same_class"}
    for name, sl in (("live", slice(0, n_live)), ("dead", slice(n_live, n))):
        m = got[name]
        for k, v in ref.items():
            assert np.array_equal(m[k], v[sl], equal_nan=True), (name, k)
        assert np.array_equal(m["n_neighbors_same_class"], same[sl].astype(np.float64))
        assert (m["n_neighbors_same_class"] <= m["n_neighbors"]).all() and (m["area"] > 0).all()
        if connectivity == 4:
            assert (m["touching_fraction"] >= 0).all() and (m["touching_fraction"] <= 1).all()
        assert (m["territory_area"] >= m["area"]).all()
    if distance is None:
        total = got["live"]["territory_area"].sum() + got["dead"]["territory_area"].sum()
        assert total == 96 * 128 * 0.25  # the territories tile the image


def test_measure_neighbors_without_a_cell_and_on_models_it_is_not_built_for():
    from eunet import synth
    from eunet.evaluator import Evaluator
    x, _ = synth.tile(96, 128, 40, num_classes=3, in_channels=3)
    image = torch.from_numpy(np.asarray(x))
    empty = _mask_evaluator([np.zeros((96, 128), np.int64)]).measure_neighbors(image)
    assert (empty["n_live"], empty["n_dead"]) == (0, 0) and len(empty["live"]["area"]) == 0
    assert empty["graph"][0].tolist() == [0] and len(empty["graph"][1]) == 0
    ran = Evaluator(_model(), DEV, "enhanced_unet", preprocess=None).measure_neighbors(image, distance=2)
    assert len(ran["live"]["n_neighbors"]) == ran["n_live"] and len(ran["dead"]["n_neighbors"]) == ran["n_dead"]
    sig = Evaluator(_model(), DEV, "enhanced_unet", preprocess=None, activation="sigmoid")
    with pytest.raises(ValueError):
        sig.measure_neighbors(image)
    with pytest.raises(ValueError):
        _mask_evaluator([np.zeros((96, 128), np.int64)]).measure_neighbors(image, connectivity=6)


# ---- the bounds-checked build ------------------------------------------------------------------------------
DEBUG_CHILD = r'''
import sys, numpy as np, torch
sys.path[:0] = [ROOT, ROOT + "/enhanced-unet_amd", ROOT + "/tests"]
from eunet import _lib, ops
import _neighbors_ref as R
assert _lib.load().eunet_debug_enabled() == 1, "not the debug build"
assert _lib.debug_status(reset=True) == (0, 0)
h, w = 37, 261
maps = (("blobs", R.blobs(h, w, 7, 2, ignore=True)), ("empty", np.zeros((h, w), np.int64)),
        ("noise", np.random.RandomState(3).randint(-1, 9, (h, w)).astype(np.int64)))
for name, ids in maps:
    for dtype in (torch.int32, torch.int64):
        dev = torch.from_numpy(ids).to("cuda").to(dtype)
        dist, site = ops.nearest_site(dev)
        rd, rs = R.nearest_site(ids)
        assert np.array_equal(dist.cpu().numpy(), rd) and np.array_equal(site.cpu().numpy(), rs)
        for distance, limit2 in ((None, None), (2.5, 6)):
            assert np.array_equal(ops.expand_label_map(dev, distance).cpu().numpy(), R.expand(ids, limit2))
        for conn in (4, 8):
            assert np.array_equal(ops.label_contacts(dev, conn, _table_capacity=16), R.contacts(ids, conn))
        st = _lib.debug_status()
        print(name, dtype, "debug status", st)
        assert st == (0, 0), (name, st)
print("DEBUG_OK")
'''


def test_debug_build_bounds_checks_pass():
    """The kernels' EUNET_DASSERT checks of every row, LDS index, site index and table slot stay silent."""
    lib = os.path.join(ROOT, "enhanced-unet_amd", "eunet", "libeunet_hip_debug.so")
    assert os.path.exists(lib), "build it: make -C enhanced-unet_amd debug"
    child = DEBUG_CHILD.replace("ROOT", repr(ROOT))
    r = subprocess.run([sys.executable, "-c", child], env=dict(os.environ, EUNET_LIB=lib), capture_output=True,
                       text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0 and "DEBUG_OK" in r.stdout
