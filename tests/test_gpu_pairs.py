"""ops.label_pairs and ops.labels_from_stack (csrc/pairs.hip) and ops.label_components(connectivity=4)
(csrc/instances.hip) against numpy and the plain-loop restatement of tests/_panoptic_ref.py.  Everything is integer:
compared with np.array_equal / torch.equal, no tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _panoptic_ref as R
import _watershed_ref as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 300), (2, 65), (37, 131), (129, 257)]
PATTERNS = ("background", "one id", "rectangles", "noise", "negative")
DTYPES = [(torch.int32, torch.int32), (torch.int32, torch.int64), (torch.int64, torch.int32), (torch.int64, torch.int64)]
ID_MAX = 2 ** 24 - 1


def _maps(shape, pattern, seed=0):
    h, w = shape
    rng = np.random.default_rng(h * 7919 + w + 31 * PATTERNS.index(pattern) + seed)
    if pattern == "background":
        return np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    if pattern == "one id":  # whole-wave runs
        return np.full((h, w), 3, np.int64), np.full((h, w), 5, np.int64)
    if pattern == "noise":  # one insert per lane, ~50 x 50 keys: many collisions
        return rng.integers(0, 50, (h, w)), rng.integers(0, 50, (h, w))
    a, b = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    for m in (a, b):  # rectangles: long runs, runs that continue from the end of one row into the next
        for k in range(1, 9):
            y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
            m[y:y + int(rng.integers(1, max(2, h // 2))), x:x + int(rng.integers(1, max(2, w)))] = k * 1000 + 7
        m[h // 2] = 77  # a full row: its run goes on into the next row where that starts with 77 too
        m[min(h - 1, h // 2 + 1), :max(1, w // 3)] = 77
    if pattern == "negative":
        a[rng.random((h, w)) < 0.1] = -1
        b[rng.random((h, w)) < 0.1] = -int(rng.integers(1, 9))
        b[0, 0] = -2 ** 31 if h * w > 1 else b[0, 0]
    return a, b


def _pairs(a, b, ta=torch.int64, tb=torch.int64, **kw):
    from eunet import ops
    got = ops.label_pairs(torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(ta),
                          torch.from_numpy(np.ascontiguousarray(b)).to(DEV).to(tb), **kw)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.ndim == 2 and got.shape[1] == 4
    return got


def _check(a, b, ta=torch.int64, tb=torch.int64, **kw):
    got = _pairs(a, b, ta, tb, **kw)
    ref = R.pair_table(a, b)
    assert np.array_equal(got, ref), (got[:5], ref[:5])
    a, b = np.asarray(a), np.asarray(b)
    counted = (a >= 0) & (b >= 0) & ~((a == 0) & (b == 0))
    assert int(got[:, 3].sum()) == int(counted.sum())
    return got


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_and_patterns(shape, pattern):
    a, b = _maps(shape, pattern)
    got = _check(a, b)
    if pattern == "background":
        assert got.shape == (0, 4)
    if pattern == "one id":
        assert got.tolist() == [[0, 3, 5, shape[0] * shape[1]]]


@pytest.mark.parametrize("ta,tb", DTYPES)
def test_the_four_dtype_combinations(ta, tb):
    for shape in ((2, 65), (37, 131)):
        for pattern in ("rectangles", "noise", "negative"):
            _check(*_maps(shape, pattern), ta, tb)


def test_ids_at_the_limit():
    a, b = _maps((37, 131), "rectangles")
    a[3, 5:40], b[3, 20:60] = ID_MAX, ID_MAX
    got = _check(a, b, torch.int32, torch.int64)
    assert (got[:, 1] == ID_MAX).any() and (got[:, 2] == ID_MAX).any()
    for side in (0, 1):
        bad = [a.copy(), b.copy()]
        bad[side][7, 9] = ID_MAX + 1
        with pytest.raises(ValueError):
            _pairs(*bad)
    b[7, 9], a[7, 9] = -1, ID_MAX + 1  # an ignored pixel is counted nowhere, whatever the other side holds
    _check(a, b)
    big = np.full((4, 4), 2 ** 40, np.int64)
    with pytest.raises(ValueError):
        _pairs(big, big)


def test_three_planes_with_different_contents():
    """A plane offset that leaks shows as a count in the wrong plane; (1, 300)-like planes end inside a wave."""
    for shape in ((1, 300), (37, 131), (1, 1), (1, 3)):
        planes = [_maps(shape, p, seed=s) for s, p in enumerate(("noise", "rectangles", "one id"))]
        a, b = np.stack([p[0] for p in planes]), np.stack([p[1] for p in planes])
        got = _check(a, b, torch.int32, torch.int64)
        for q in range(3):
            one = _check(a[q], b[q])
            assert np.array_equal(got[got[:, 0] == q][:, 1:], one[:, 1:]), (shape, q)
    a = np.ones((40000, 1, 2), np.int64)  # a plane above 32767 sets the key's top bit
    a[:, 0, 1] = np.arange(40000) % 7
    got = _check(a, a, torch.int32, torch.int32)
    assert got[-1, 0] == 39999


def test_a_small_table_grows_to_the_identical_result():
    a, b = _maps((129, 257), "noise")
    full = _check(a, b)
    assert len(full) > 2000  # far more keys than 2 slots: the pass is rerun with 4, 8, ... slots
    assert np.array_equal(_check(a, b, _table_capacity=2), full)
    assert np.array_equal(_check(a, b, _table_capacity=4096), full)
    assert np.array_equal(_pairs(a, b), _pairs(a, b))  # two runs give equal bits


@pytest.mark.parametrize("ta,tb", [(torch.int32, torch.int32), (torch.int64, torch.int32)])
def test_a_map_larger_than_one_round_of_the_grid(ta, tb):
    """2048 blocks of four waves hold 2^21 pixels a round: 1500 x 1500 sends 597 waves round a second time, with their
    shuffles, their inserts and their count of ids past the limit.  The reference is np.unique over a << 24 | b."""
    h = w = 1500
    assert h * w > 2048 * 4 * 256
    yy, xx = np.mgrid[0:h, 0:w]
    a = ((yy // 37) * 50 + xx // 41 + 1) * ((yy % 37 < 30) & (xx % 41 < 33))  # blocks of ids on background
    b = np.roll(a, (5, 7), axis=(0, 1))
    b[1450:1470, 200:900] = -1  # ignored pixels in the second round's part
    counted = (a >= 0) & (b >= 0) & ~((a == 0) & (b == 0))
    keys, n = np.unique((a[counted] << 24) | b[counted], return_counts=True)
    ref = np.stack([np.zeros_like(keys), keys >> 24, keys & ID_MAX, n], axis=1)
    got = _pairs(a, b, ta, tb)
    assert np.array_equal(got, ref) and int(got[:, 3].sum()) == int(counted.sum())
    assert (got[:, 1] == a[h - 1, w - 9]).any() and a[h - 1, w - 9] > 0  # an id that only the second round sees
    a[h - 2, w - 2] = ID_MAX + 1  # and an id past the limit there
    with pytest.raises(ValueError):
        _pairs(a, b, ta, tb)


def test_unaligned_views_take_the_scalar_loads():
    a, b = _maps((37, 131), "rectangles")
    from eunet import ops
    ta = torch.zeros(37 * 131 + 1, dtype=torch.int32, device=DEV)
    ta[1:] = torch.from_numpy(a.astype(np.int32)).to(DEV).reshape(-1)
    got = ops.label_pairs(ta[1:].view(37, 131), torch.from_numpy(b).to(DEV))  # a's base is 4 bytes off a 16-byte line
    assert np.array_equal(got, R.pair_table(a, b))


def test_cross_check_with_the_packed_mask_kernels():
    """For disjoint instance stacks the interior of the table and its area sums are pairwise_overlap(pack_masks(...))
    and pack_masks' areas."""
    from eunet import ops
    a, b = _maps((129, 257), "rectangles")
    ida, idb = [i for i in np.unique(a) if i > 0], [j for j in np.unique(b) if j > 0]
    sa = torch.from_numpy(np.stack([a == i for i in ida]).astype(np.uint8)).to(DEV)
    sb = torch.from_numpy(np.stack([b == j for j in idb]).astype(np.uint8)).to(DEV)
    (pa, area_a), (pb, area_b) = ops.pack_masks(sa), ops.pack_masks(sb)
    inter = ops.pairwise_overlap(pa, pb).cpu().numpy()
    got = _pairs(a, b)
    dense = np.zeros((len(ida), len(idb)), np.int64)
    sum_a, sum_b = np.zeros(len(ida), np.int64), np.zeros(len(idb), np.int64)
    for _, i, j, n in got.tolist():
        if i > 0:
            sum_a[ida.index(i)] += n
        if j > 0:
            sum_b[idb.index(j)] += n
        if i > 0 and j > 0:
            dense[ida.index(i), idb.index(j)] = n
    assert np.array_equal(dense, inter)
    assert np.array_equal(sum_a, area_a.cpu().numpy()) and np.array_equal(sum_b, area_b.cpu().numpy())


def test_refusals():
    from eunet import ops
    t = torch.ones(2, 8, 9, dtype=torch.int32, device=DEV)
    bad = [
        (t.cpu(), t, {}), (t, t.cpu(), {}), (np.ones((8, 9), np.int32), t, {}), (t.float(), t, {}), (t, t.to(torch.int16), {}),
        (t[0, 0], t[0, 0], {}), (t.unsqueeze(0), t.unsqueeze(0), {}), (t, t[:1], {}), (t[:, :, ::2], t[:, :, ::2], {}),
        (t[:, :0], t[:, :0], {}), (torch.ones(1, 1, 8193, dtype=torch.int32, device=DEV),) * 2 + ({},),
        (t, t, {"_table_capacity": 12}), (t, t, {"_table_capacity": 1}), (t, t, {"_table_capacity": 0}),
    ]
    for a, b, kw in bad:
        with pytest.raises(ValueError):
            ops.label_pairs(a, b, **kw)
    m = torch.ones(2, 8, 9, dtype=torch.uint8, device=DEV)
    bad = [
        (m.cpu(), [1, 2], {}), (m.int(), [1, 2], {}), (m[0], [1], {}), (m, [1], {}), (m, [1, 2, 3], {}), (m, [1.5, 2], {}),
        (m, torch.ones(2, dtype=torch.int64, device=DEV), {}), (m, [1, 2], {"ignore": m}), (m, [1, 2], {"ignore": m[0].cpu()}),
        (m, [1, 2], {"ignore": m[0].int()}),
    ]
    for masks, ids, kw in bad:
        with pytest.raises(ValueError):
            ops.labels_from_stack(masks, ids, **kw)
    with pytest.raises(ValueError):
        ops.label_components(m[0], connectivity=6)


# ---- labels_from_stack ---------------------------------------------------------------------------------------
def _stack_ref(masks, ids, ignore):
    out = np.zeros(masks.shape[1:], np.int32)
    claims = np.zeros(masks.shape[1:], np.int64)
    for j in range(len(masks)):
        if ids[j] > 0:
            out[masks[j] != 0] = ids[j]
            claims += masks[j] != 0
    if ignore is not None:
        out[ignore != 0] = -1
    return out, int((claims > 1).sum())


@pytest.mark.parametrize("n", [1, 2, 7])
@pytest.mark.parametrize("shape", SHAPES + [(16, 48), (32, 64), (64, 80)])  # the last three: 16 pixels per lane
def test_labels_from_stack(shape, n):
    from eunet import ops
    h, w = shape
    rng = np.random.default_rng(h * 131 + w + n)
    masks = (rng.random((n, h, w)) < 0.4) * rng.integers(1, 256, (n, h, w))  # overlapping planes, any non-zero byte
    masks = masks.astype(np.uint8)
    ignore = (rng.random((h, w)) < 0.2).astype(np.uint8) * 255
    t = torch.from_numpy(masks).to(DEV)
    id_sets = [list(range(1, n + 1)), [int(v) for v in rng.integers(0, 3, n) * 1000], [0] * n, [5] * n]
    id_sets.append([-4] + [ID_MAX] * (n - 1))
    for ids in id_sets:
        for ign in (None, ignore):
            got, overlap = ops.labels_from_stack(t, ids, None if ign is None else torch.from_numpy(ign).to(DEV))
            ref, ref_overlap = _stack_ref(masks, ids, ign)
            assert got.dtype == torch.int32 and got.is_cuda and torch.equal(got.cpu(), torch.from_numpy(ref)), ids
            assert isinstance(overlap, int) and overlap == ref_overlap, ids
    got, overlap = ops.labels_from_stack(t.bool(), torch.tensor(id_sets[0], dtype=torch.int32, device=DEV),
                                         torch.from_numpy(ignore).to(DEV).bool())
    assert torch.equal(got.cpu(), torch.from_numpy(_stack_ref(masks, id_sets[0], ignore)[0]))
    if n == 1:  # no plane at all: background, or ignored
        got, overlap = ops.labels_from_stack(t[:0], [], torch.from_numpy(ignore).to(DEV))
        assert overlap == 0 and torch.equal(got.cpu(), torch.from_numpy(-(ignore != 0).astype(np.int32)))


# ---- 4-connected labelling -------------------------------------------------------------------------------------
KINDS = ("random0.5", "random0.7", "discs", "empty", "full", "checkerboard", "diagonal")


def _mask(shape, kind):
    h, w = shape
    rng = np.random.default_rng(h * 7919 + w + KINDS.index(kind))
    yy, xx = np.mgrid[0:h, 0:w]
    if kind.startswith("random"):
        return rng.random((h, w)) < float(kind[6:])
    if kind == "discs":
        r = max(1.0, min(h, w) / 5)
        return W.discs(h, w, [(h / 2, w / 2 - r * 0.8, r), (h / 2, w / 2 + r * 0.8, r), (h / 4, w / 5, r / 2)])
    if kind == "empty":
        return np.zeros((h, w), bool)
    if kind == "full":
        return np.ones((h, w), bool)
    if kind == "checkerboard":
        return (yy + xx) % 2 == 0
    return xx == yy if h > 1 else xx % 3 == 0  # a diagonal line: one pixel per row, corners touching


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_four_connected_components(shape, kind):
    from eunet import ops
    m = _mask(shape, kind)
    img = torch.from_numpy(m.astype(np.uint8)).to(DEV)
    labels, n, areas = ops.label_components(img, connectivity=4)
    ref, ref_n = R.label4(m)
    assert n == ref_n and labels.dtype == torch.int32 and torch.equal(labels.cpu(), torch.from_numpy(ref))
    assert areas.cpu().tolist() == [int((ref == k).sum()) for k in range(1, ref_n + 1)]
    eight = ops.label_components(img, connectivity=8)
    plain = ops.label_components(img)
    assert eight[1] == plain[1] and torch.equal(eight[0], plain[0]) and torch.equal(eight[2], plain[2])
    if kind == "checkerboard":
        assert n == (shape[0] * shape[1] + 1) // 2  # every set pixel alone: the areas buffer is exactly full
        assert plain[1] == (1 if shape[0] > 1 else n)  # joined through the corners, where there is a second row
    if kind == "diagonal" and shape[0] > 1 and shape[1] >= shape[0]:
        assert n == shape[0] and plain[1] == 1  # one pixel per row, joined through the corners only


DEBUG_CHILD = r'''
import sys, numpy as np, torch
sys.path[:0] = [ROOT, ROOT + "/enhanced-unet_amd"]
from eunet import _lib, ops
assert _lib.load().eunet_debug_enabled() == 1, "not the debug build"
assert _lib.debug_status(reset=True) == (0, 0)
for h, w in SHAPES:
    rng = np.random.default_rng(h * 31 + w)
    a = torch.from_numpy(rng.integers(-1, 40, (3, h, w))).to("cuda")
    b = torch.from_numpy(np.repeat(rng.integers(0, 9, (3, h, (w + 6) // 7)), 7, axis=2)[:, :, :w].copy()).to("cuda")
    n = sum(len(ops.label_pairs(x, y, _table_capacity=c)) for x, y, c in ((a, b, 2), (a.int(), b, None), (b, b.int(), 8)))
    ops.labels_from_stack((a > 20).to(torch.uint8), [1, 0, 3], (b[0] == 0).to(torch.uint8))
    ops.label_components((b[0] > 3).to(torch.uint8), connectivity=4)
    st = _lib.debug_status()
    print((h, w), n, "debug status", st)
    assert st == (0, 0), (h, w, st)
print("DEBUG_OK")
'''


def test_debug_build_bounds_checks_pass():
    """The kernels' EUNET_DASSERT index checks (the bounds-checked debug build) stay silent on every shape above."""
    lib = os.path.join(ROOT, "enhanced-unet_amd", "eunet", "libeunet_hip_debug.so")
    assert os.path.exists(lib), "build it: make -C enhanced-unet_amd debug"
    child = DEBUG_CHILD.replace("ROOT", repr(ROOT)).replace("SHAPES", repr(SHAPES + [(16, 48)]))
    r = subprocess.run([sys.executable, "-c", child], env=dict(os.environ, EUNET_LIB=lib), capture_output=True,
                       text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0 and "DEBUG_OK" in r.stdout
