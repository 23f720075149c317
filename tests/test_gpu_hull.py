"""ops.cell_hulls (csrc/hull.hip) and Evaluator.measure_cells(hull=True) against the plain-loop restatement of
tests/_hull_ref.py.  Every table is an integer table: every comparison is np.array_equal."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _cellprops_ref as R
import _hull_ref as H

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a, dtype=torch.int64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def _check(ids, n, dtypes=(torch.int32, torch.int64)):
    """ops.cell_hulls on the device against the restatement, for both id types; returns the last device result."""
    from eunet import ops
    ids = np.asarray(ids)
    ext, verts, hull, row_off, lists = H.cell_hulls(ids, n)
    for dtype in dtypes:
        d = _dev(ids, dtype)
        got = ops.cell_hulls(d, ops.cell_stats(d, n))
        assert got["hull"].dtype == np.int64 and got["hull"].shape == hull.shape
        assert np.array_equal(got["row_off"], row_off) and got["shape"] == ids.shape[-2:]
        assert got["ext"].dtype == np.int32 and np.array_equal(got["ext"], ext)
        assert np.array_equal(got["hull"], hull)
        for q in range(hull.shape[0]):
            assert len(got["verts"][q]) == n
            for i in range(n):
                v = got["verts"][q][i]
                assert v.dtype == np.int32 and v.shape == (len(lists[q][i]), 2)
                assert v.tolist() == [list(t) for t in lists[q][i]], (q, i)
        present = hull[:, :, 0] > 0
        geom = R.cell_stats(ids, n)[0]
        assert (2 * geom[:, :, 0][present] <= hull[:, :, 1][present]).all() and (hull[:, :, 0][present] >= 4).all()
    return got


def _raw_verts(ids, n, dtype=torch.int32):
    """The whole verts table through the C ABI: the slots past a label's vertices must be zero."""
    from eunet import _lib, ops
    ids = np.asarray(ids)
    ext, verts, hull, row_off, _ = H.cell_hulls(ids, n)
    p = 1 if ids.ndim == 2 else ids.shape[0]
    h, w = ids.shape[-2:]
    L, Rr = p * (n + 1), int(row_off[-1])
    geom = R.cell_stats(ids, n)[0].reshape(L, 14)
    y0 = np.where(np.diff(row_off) > 0, geom[:, 7], 0).astype(np.int32)
    d = _dev(ids, dtype)
    off_d, y0_d = _dev(row_off), _dev(y0, torch.int32)
    out = [torch.full((max(k, 1),), 77, dtype=t, device=DEV)  # dirty: the call writes every entry
           for k, t in ((2 * Rr, torch.int32), (4 * (Rr + L), torch.int32), (11 * L, torch.int64), (p, torch.int64))]
    _lib.call("eunet_cell_hulls", ops._ptr(d), d.element_size(), p, h, w, n, ops._ptr(off_d), ops._ptr(y0_d),
              *[ops._ptr(t) for t in out], ops._stream())
    assert np.array_equal(out[0].cpu().numpy()[:2 * Rr].reshape(-1, 2), ext)
    assert np.array_equal(out[1].cpu().numpy().reshape(-1, 2), verts)
    assert np.array_equal(out[2].cpu().numpy().reshape(hull.shape), hull) and not out[3].cpu().numpy().any()


def _shapes():
    ring = np.ones((7, 9), np.int64)
    ring[2:5, 2:7] = 0
    ell = np.zeros((9, 8), np.int64)
    ell[:, 1], ell[7, 1:7] = 1, 1
    u = np.ones((6, 9), np.int64)
    u[:4, 2:7] = 0
    plus = np.zeros((9, 9), np.int64)
    plus[3:6, :], plus[:, 3:6] = 1, 1
    diag = np.zeros((42, 44), np.int64)
    diag[np.arange(40) + 1, np.arange(40) + 2] = 1
    two = np.zeros((20, 30), np.int64)
    two[1:4, 20:27], two[12:17, 2:6] = 1, 1
    border = np.zeros((37, 131), np.int64)
    border[0, :], border[-1, :], border[:, 0], border[:, -1] = 2, 2, 2, 2
    border[10:20, 10:30] = 1
    straddle = np.zeros((3, 600), np.int64)
    straddle[0, 255:300], straddle[1, 252:258], straddle[2, 253:513] = 1, 2, 3
    straddle[2, 0:3], straddle[2, 599] = 4, 4
    out = {"pixel": (np.ones((1, 1), np.int64), 1), "row": (np.ones((1, 300), np.int64), 1),
           "column": (np.ones((300, 1), np.int64), 1), "ring": (ring, 1), "L": (ell, 1), "U": (u, 1),
           "plus": (plus, 1), "diagonal": (diag, 1), "disc": (H.disc(45, 47, 22, 23, 20), 1),
           "ellipse": (H.ellipse(50, 70, 24, 35, 30, 9, 0.6), 1), "staircase": (H.staircase(20), 1),
           "two blobs": (two, 1), "borders": (border, 3), "straddle": (straddle, 4)}
    for w in (1, 255, 256, 257, 513):
        out[f"full {w}"] = (np.full((3, w), 2, np.int64), 2)
    return out


SHAPES = _shapes()


@pytest.mark.parametrize("name", list(SHAPES))
def test_tables_equal_the_restatement(name):
    ids, n = SHAPES[name]
    _check(ids, n)


def test_the_slots_past_the_vertices_are_zero_and_a_dirty_buffer_is_overwritten():
    for name in ("disc", "staircase", "two blobs", "full 257"):
        _raw_verts(*SHAPES[name])


def test_planes_with_labels_absent_from_one_plane():
    ids = np.stack([R.blobs(37, 131, 6, 10), R.blobs(37, 131, 6, 11)])
    ids[ids == 6] = 0
    ids[1, 30:33, 100:120] = 6
    ids[0][ids[0] == 2] = 0
    got = _check(ids, 6)
    assert not got["hull"][0, 6].any() and not got["hull"][0, 2].any() and got["hull"][1, 6, :2].tolist() == [4, 120]
    assert got["verts"][0][5].shape == (0, 2)
    _raw_verts(ids, 6, torch.int64)


def test_ids_out_of_range_and_n_of_zero():
    ids = R.noise(23, 40, 9, 5)  # ids 6..9 lie above n = 5; every seventh pixel is negative
    ids.reshape(-1)[::7] = -1 - (np.arange(ids.size)[::7] % 3)
    _check(ids, 5)
    got = _check(ids, 0)
    assert got["hull"].shape == (1, 1, 11) and not got["hull"].any() and got["ext"].shape == (0, 2)
    assert got["verts"] == [[]]


def test_noise_where_every_label_spans_nearly_every_row():
    ids = np.random.default_rng(3).integers(0, 8, (61, 67)).astype(np.int64)
    _check(ids, 7)


def test_a_synthetic_tile_through_label_components_and_two_runs_agree():
    from eunet import ops, synth
    _, sem, _ = synth.tile(256, 256, 5, num_classes=3, instances=True)
    labels, n, _ = ops.label_components(torch.from_numpy((np.asarray(sem) > 0).astype(np.uint8)).to(DEV))
    assert n >= 3
    ids = labels.cpu().numpy()
    a = _check(ids, n, dtypes=(torch.int32,))
    b = ops.cell_hulls(labels, ops.cell_stats(labels, n))
    for k in ("hull", "ext", "row_off"):
        assert np.array_equal(a[k], b[k]), k
    assert all(np.array_equal(x, y) for x, y in zip(a["verts"][0], b["verts"][0]))


def test_stats_of_a_shifted_copy_are_refused():
    from eunet import ops
    ids = np.zeros((40, 50), np.int64)
    ids[5:15, 5:20], ids[20:30, 10:40] = 1, 2
    moved = np.roll(ids, 4, axis=0)  # the same boxes four rows down: shapes and label count agree
    d = _dev(ids, torch.int32)
    with pytest.raises(ValueError, match="outside"):
        ops.cell_hulls(d, ops.cell_stats(_dev(moved, torch.int32), 2))
    _check(ids, 2)  # and the call after the refusal is sound


# ---- the evaluator ------------------------------------------------------------------------------------------
def test_measure_cells_with_hulls_is_the_restatement_and_without_is_todays_dict():
    from eunet import metrics as M
    from eunet import synth
    from eunet.evaluator import Evaluator
    from eunet.models import EnhancedUNet
    torch.manual_seed(3)
    model = EnhancedUNet(num_classes=3, in_channels=3, base_ch=16).to(DEV).eval()
    x, sem, _ = synth.tile(96, 128, 40, num_classes=3, in_channels=3, instances=True)
    sem = np.ascontiguousarray(sem).astype(np.int64)
    ev = Evaluator(model, DEV, "enhanced_unet", preprocess=None, split="watershed")
    ev._predict_mask_device = lambda image: torch.from_numpy(sem).to(DEV)
    ids, counts, scores = ev.semantic_to_instance_maps(torch.from_numpy(sem).to(DEV))
    assert min(counts) >= 1
    image = torch.from_numpy(np.asarray(x))
    plain, with_hull = ev.measure_cells(image, pixel_size=0.5), ev.measure_cells(image, pixel_size=0.5, hull=True)
    ids_np, n = ids.cpu().numpy(), max(counts)
    stats = {"geom": R.cell_stats(ids_np, n)[0], "intensity": None, "shape": (96, 128)}
    hulls = {"hull": H.cell_hulls(ids_np, n)[2]}
    for plane, name in enumerate(M.INSTANCE_CLASSES):
        base = M.cell_measurements(stats, plane, 0.5)
        assert set(plain[name]) == set(base) | {"score"}  # the default: key for key what it was
        ref = M.hull_measurements(hulls, stats, plane, 0.5)
        assert set(with_hull[name]) == set(plain[name]) | set(M.HULL_KEYS)
        for k, v in plain[name].items():
            assert np.array_equal(with_hull[name][k], v), (name, k)
        for k in M.HULL_KEYS:
            assert np.array_equal(with_hull[name][k], ref[k][:counts[plane]]), (name, k)
        assert (with_hull[name]["solidity"] > 0).all() and (with_hull[name]["solidity"] <= 1).all()
        assert (with_hull[name]["feret_min"] <= with_hull[name]["feret_max"]).all()
    assert (with_hull["n_live"], with_hull["n_dead"], with_hull["viability"]) == \
        (plain["n_live"], plain["n_dead"], plain["viability"])


DEBUG_CHILD = r'''
import sys, numpy as np, torch
sys.path[:0] = [ROOT, ROOT + "/enhanced-unet_amd", ROOT + "/tests"]
from eunet import _lib, ops
import _hull_ref as H
import test_gpu_hull as T
assert _lib.load().eunet_debug_enabled() == 1, "not the debug build"
assert _lib.debug_status(reset=True) == (0, 0)
for name, (ids, n) in T.SHAPES.items():
    T._check(ids, n)
    st = _lib.debug_status()
    print(name, "debug status", st)
    assert st == (0, 0), (name, st)
ids = np.random.default_rng(3).integers(0, 8, (61, 67)).astype(np.int64)
T._check(ids, 7)
moved = np.roll(ids, 3, axis=0)
moved[:3] = 0
d = torch.from_numpy(ids).to("cuda")
try:
    ops.cell_hulls(d, ops.cell_stats(torch.from_numpy(moved).to("cuda"), 7))
except ValueError as e:
    print("refused:", e)
assert _lib.debug_status() == (0, 0)
print("DEBUG_OK")
'''


def test_debug_build_bounds_checks_pass():
    """The kernels' EUNET_DASSERT checks of every table index and pixel address stay silent over the suite's shapes,
    and over stats that are not the map's."""
    lib = os.path.join(ROOT, "enhanced-unet_amd", "eunet", "libeunet_hip_debug.so")
    assert os.path.exists(lib), "build it: make -C enhanced-unet_amd debug"
    child = DEBUG_CHILD.replace("ROOT", repr(ROOT))
    r = subprocess.run([sys.executable, "-c", child], env=dict(os.environ, EUNET_LIB=lib), capture_output=True,
                       text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0 and "DEBUG_OK" in r.stdout
