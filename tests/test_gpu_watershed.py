"""ops.watershed_from_distance and ops.watershed_split (csrc/watershed.hip) against the plain-loop restatement of
tests/_watershed_ref.py, and the evaluator's split="watershed" on top of them.  Everything is integer: compared with
torch.equal, no tolerance."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _boundary_ref as B
import _watershed_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 300), (300, 1), (2, 65), (37, 131), (64, 64), (129, 257)]
DEPTHS = (0.0, 0.5, 1.0, 2.0, math.inf)
KINDS = ("random0.5", "random0.7", "random0.9", "discs", "empty", "full", "checkerboard", "cut")


def _mask(shape, kind):
    h, w = shape
    rng = np.random.default_rng(h * 7919 + w + KINDS.index(kind))
    yy, xx = np.mgrid[0:h, 0:w]
    if kind.startswith("random"):
        return rng.random((h, w)) < float(kind[6:])
    if kind == "discs":  # touching and overlapping discs inside the image
        r = max(1.0, min(h, w) / 5)
        return R.discs(h, w, [(h / 2, w / 2 - r * 0.8, r), (h / 2, w / 2 + r * 0.8, r), (h / 4, w / 5, r / 2)])
    if kind == "empty":
        return np.zeros((h, w), bool)
    if kind == "full":  # EDT_NONE everywhere: one plateau, the longest chains
        return np.ones((h, w), bool)
    if kind == "checkerboard":  # D = 1 on every set pixel: an all-ones plateau, 8-connected through the diagonals
        return (yy + xx) % 2 == 0
    r = max(2.0, min(h, w) / 3)  # regions cut by the image edge, at every side and corner
    return R.discs(h, w, [(0, 0, r), (0, w - 1, r), (h - 1, w / 2, r), (h / 2, w - 1, r * 0.7), (h / 2, 0, r * 0.7)])


_CASES = {}


def _case(shape, kind):
    """(mask, D as the device's transform gives it, the restatement's basins), computed once per case and shared."""
    key = (shape, kind)
    if key not in _CASES:
        from eunet import ops
        m = _mask(shape, kind)
        d = ops.distance_transform_sq(torch.from_numpy(m.astype(np.int64)).to(DEV), [1], "ne")[0]
        D = d.cpu().numpy().astype(np.int64)
        assert np.array_equal(D, R.edt_sq(m)), key
        _CASES[key] = (m, D, R.Basins(D))
    return _CASES[key]


def _run(D, depth, **kw):
    from eunet import ops
    t = torch.from_numpy(np.ascontiguousarray(D, dtype=np.int32)).to(DEV)
    ids, counts, areas = ops.watershed_from_distance(t, depth, **kw)
    assert ids.is_cuda and ids.dtype == torch.int32 and tuple(ids.shape) == tuple(t.shape)
    assert counts.is_cuda and counts.dtype == torch.int64 and areas.is_cuda and areas.dtype == torch.int32
    return ids.cpu(), counts.cpu(), areas.cpu()


def _check(D, basins, depth, **kw):
    ids, counts, areas = _run(D, depth, **kw)
    ref_ids, n, ref_areas = basins.split(depth)
    assert counts.tolist() == [n], (depth, counts.tolist(), n)
    assert torch.equal(ids, torch.from_numpy(ref_ids)), depth
    assert tuple(areas.shape) == (n,) and torch.equal(areas, torch.from_numpy(ref_areas)), depth
    return ids


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_masks_and_depths(shape, kind):
    m, D, basins = _case(shape, kind)
    for depth in DEPTHS:
        ids = _check(D, basins, depth)
        assert torch.equal(ids > 0, torch.from_numpy(m))


@pytest.mark.parametrize("shape", [(2, 65), (37, 131), (129, 257)])
def test_infinite_depth_is_label_components(shape):
    from eunet import ops
    for kind in ("random0.5", "random0.9", "discs", "full", "checkerboard", "cut"):
        m, D, _ = _case(shape, kind)
        ids, counts, areas = _run(D, math.inf)
        labels, n, lab_areas = ops.label_components(torch.from_numpy(m.astype(np.uint8)).to(DEV))
        assert counts.tolist() == [n] and torch.equal(ids, labels.cpu()) and torch.equal(areas, lab_areas.cpu()), kind


def test_two_planes_of_more_blocks_than_one_scan_pass_holds():
    """257 x 256 pixels are 257 blocks of 256 per plane: the scan of the per-block counts takes its second pass, and
    the second plane's counts start 257 entries in.  Too large for the restatement's loops: depth inf against
    label_components, depth 0 as a refinement of it."""
    from eunet import ops
    shape = (257, 256)
    masks = [_mask(shape, kind) for kind in ("random0.5", "discs")]
    stack = torch.from_numpy(np.stack(masks).astype(np.int64)).to(DEV)
    D = ops.distance_transform_sq(stack, [1], "ne")[:, 0].cpu().numpy()
    assert D.shape == (2,) + shape
    whole, whole_counts, whole_areas = _run(D, math.inf)
    fine, fine_counts, fine_areas = _run(D, 0.0)
    for i, m in enumerate(masks):
        labels, n, lab_areas = ops.label_components(torch.from_numpy(m.astype(np.uint8)).to(DEV))
        assert int(whole_counts[i]) == n and torch.equal(whole[i], labels.cpu()), i
        assert torch.equal(whole_areas[i, :n], lab_areas.cpu()) and int(whole_areas[i, n:].abs().sum()) == 0, i
        f, c = fine[i].numpy(), whole[i].numpy()
        assert np.array_equal(f > 0, m), i
        nf = int(fine_counts[i])
        assert nf >= n and np.array_equal(np.unique(f[f > 0]), np.arange(1, nf + 1)), i
        parent = np.zeros(nf + 1, np.int64)
        parent[f[f > 0]] = c[f > 0]
        assert np.array_equal(parent[f], c), i   # every fine region lies in one component
        assert np.array_equal(fine_areas[i, :nf].numpy(), np.bincount(f.ravel(), minlength=nf + 1)[1:]), i


@pytest.mark.parametrize("depth", DEPTHS)
def test_a_batch_of_three_planes(depth):
    """Planes with many, few and no basins side by side: each keeps its own numbering, the areas are padded with 0."""
    shape = (37, 131)
    cases = [_case(shape, k) for k in ("random0.7", "empty", "discs")]
    ids, counts, areas = _run(np.stack([c[1] for c in cases]), depth)
    refs = [c[2].split(depth) for c in cases]
    assert counts.tolist() == [r[1] for r in refs] and tuple(areas.shape) == (3, max(r[1] for r in refs))
    for i, (ref_ids, n, ref_areas) in enumerate(refs):
        assert torch.equal(ids[i], torch.from_numpy(ref_ids)), i
        assert torch.equal(areas[i, :n], torch.from_numpy(ref_areas)) and int(areas[i, n:].abs().sum()) == 0, i
    one = _run(cases[2][1][None], depth)  # a batch of one
    assert tuple(one[0].shape) == (1,) + shape and torch.equal(one[0][0], ids[2]) and one[1].tolist() == [refs[2][1]]
    assert tuple(one[2].shape) == (1, refs[2][1])


def test_a_small_table_grows_until_every_pair_fits():
    m, D, basins = _case((37, 131), "random0.7")
    assert len(basins.sad) > 64  # far more pairs than the 8 slots: the pass is rerun with 16, 32, ... slots
    for depth in (0.0, 1.0, math.inf):
        small = _check(D, basins, depth, _table_capacity=8)
        assert torch.equal(small, _run(D, depth)[0])
    _check(D, basins, 1.0, _table_capacity=2)


def test_two_runs_give_equal_bits():
    for kind in ("random0.7", "full"):
        _, D, _ = _case((129, 257), kind)
        a, b = _run(D, 1.0), _run(D, 1.0)
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_out_buffer():
    from eunet import ops
    _, D, basins = _case((37, 131), "discs")
    t = torch.from_numpy(D.astype(np.int32)).to(DEV)
    out = torch.full((37, 131), -7, dtype=torch.int32, device=DEV)
    ids, counts, _ = ops.watershed_from_distance(t, 1.0, out=out)
    assert ids is out and torch.equal(out.cpu(), torch.from_numpy(basins.split(1.0)[0]))
    again, _, _ = ops.watershed_from_distance(t, 1.0, out=out)  # a buffer that holds ids already
    assert again is out and torch.equal(out.cpu(), torch.from_numpy(basins.split(1.0)[0]))
    assert torch.equal(t.cpu(), torch.from_numpy(D.astype(np.int32)))  # the input is left alone
    empty = torch.zeros(5, 9, dtype=torch.int32, device=DEV)
    out = torch.full((5, 9), -7, dtype=torch.int32, device=DEV)
    ids, counts, areas = ops.watershed_from_distance(empty, out=out)
    assert ids is out and int(out.abs().sum()) == 0 and counts.tolist() == [0] and tuple(areas.shape) == (0,)


def test_refusals():
    from eunet import ops
    t = torch.ones(2, 8, 9, dtype=torch.int32, device=DEV)
    bad = [
        (t.long(), {}), (t.cpu(), {}), (np.ones((8, 9), np.int32), {}), (t[0, 0], {}), (t.unsqueeze(0), {}),
        (t[:, :, ::2], {}), (t[:, :0], {}), (torch.ones(1, 1, 8193, dtype=torch.int32, device=DEV), {}),
        (t, {"depth": -0.5}), (t, {"depth": float("nan")}), (t, {"depth": "deep"}), (t, {"depth": None}),
        (t, {"_table_capacity": 12}), (t, {"_table_capacity": 1}), (t, {"_table_capacity": 0}),
        (t, {"out": torch.zeros(2, 8, 9, dtype=torch.int64, device=DEV)}),
        (t, {"out": torch.zeros(1, 8, 9, dtype=torch.int32, device=DEV)}),
        (t, {"out": torch.zeros(2, 8, 9, dtype=torch.int32)}),
        (t, {"out": torch.zeros(2, 8, 18, dtype=torch.int32, device=DEV)[..., ::2]}),
        (t, {"out": t}),
    ]
    for d, kw in bad:
        with pytest.raises(ValueError):
            ops.watershed_from_distance(d, **kw)
    maps = torch.zeros(2, 8, 9, dtype=torch.int64, device=DEV)
    bad = [
        (maps.int(), [1], {}), (maps.cpu(), [1], {}), (maps[:, :, ::2], [1], {}), (maps[0, 0], [1], {}),
        (maps, [], {}), (maps, list(range(9)), {}), (maps, [1.5], {}), (maps, 1, {}),
        (maps, [1], {"depth": -1.0}), (maps, [1], {"depth": float("nan")}),
        (maps, [1], {"out": torch.zeros(2, 2, 8, 9, dtype=torch.int32, device=DEV)}),
        (maps, [1], {"out": torch.zeros(2, 1, 8, 9, dtype=torch.int64, device=DEV)}),
        (maps, [1], {"out": torch.zeros(2, 1, 8, 9, dtype=torch.int32)}),
    ]
    for labels, values, kw in bad:
        with pytest.raises(ValueError):
            ops.watershed_split(labels, values, **kw)


@pytest.mark.parametrize("values", [[1], [2, 0, 255], [0, 1, 2, 255, 7, -1, 5, 1]])
def test_split_of_label_maps(values):
    """watershed_split: one plane per (sample, value), the transform included."""
    from eunet import ops
    rng = np.random.default_rng(len(values))
    h, w = 33, 70
    yy, xx = np.mgrid[0:h, 0:w]
    maps = rng.choice(np.array([0, 1, 2, 255, 7, -1], np.int64), size=(2, h, w), p=[0.3, 0.3, 0.2, 0.1, 0.05, 0.05])
    for cy, cx, r, v in ((10, 20, 8, 1), (10, 31, 8, 1), (22, 50, 9, 2), (24, 8, 6, 0)):
        maps[0][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = v
    D = B.edt_sq_maps(maps, values, "ne").astype(np.int64)
    t = torch.from_numpy(maps).to(DEV)
    ids, counts, areas = ops.watershed_split(t, values, depth=1.0)
    assert tuple(ids.shape) == (2, len(values), h, w) and ids.dtype == torch.int32
    assert tuple(counts.shape) == (2, len(values)) and counts.dtype == torch.int64 and areas.shape[:2] == counts.shape
    for i in range(2):
        for j in range(len(values)):
            ref_ids, n, ref_areas = R.split(D[i, j], 1.0)
            assert int(counts[i, j]) == n and torch.equal(ids[i, j].cpu(), torch.from_numpy(ref_ids)), (i, j)
            assert torch.equal(areas[i, j, :n].cpu(), torch.from_numpy(ref_areas)), (i, j)
    out = torch.full((len(values), h, w), -7, dtype=torch.int32, device=DEV)
    single = ops.watershed_split(t[0], tuple(values), out=out)  # a single map, the default depth, a buffer
    assert single[0] is out and torch.equal(out, ids[0]) and torch.equal(single[1], counts[0])
    assert tuple(single[2].shape) == (len(values), int(counts[0].max()))


DEBUG_CHILD = r'''
import sys, numpy as np, torch
sys.path[:0] = [ROOT, ROOT + "/enhanced-unet_amd"]
from eunet import _lib, ops
assert _lib.load().eunet_debug_enabled() == 1, "not the debug build"
assert _lib.debug_status(reset=True) == (0, 0)
for h, w in SHAPES:
    rng = np.random.default_rng(h * 31 + w)
    maps = np.stack([(rng.random((h, w)) < 0.7).astype(np.int64), np.ones((h, w), np.int64)])
    ids, counts, areas = ops.watershed_split(torch.from_numpy(maps).to("cuda"), [1, 0], depth=1.0)
    ops.watershed_from_distance(ops.distance_transform_sq(torch.from_numpy(maps).to("cuda"), [1], "ne")[:, 0], 0.5,
                                _table_capacity=4)
    st = _lib.debug_status()
    print((h, w), counts.tolist(), "debug status", st)
    assert st == (0, 0), (h, w, st)
print("DEBUG_OK")
'''


def test_debug_build_bounds_checks_pass():
    """The kernels' EUNET_DASSERT index checks (the bounds-checked debug build) stay silent on every shape above."""
    lib = os.path.join(ROOT, "enhanced-unet_amd", "eunet", "libeunet_hip_debug.so")
    assert os.path.exists(lib), "build it: make -C enhanced-unet_amd debug"
    child = DEBUG_CHILD.replace("ROOT", repr(ROOT)).replace("SHAPES", repr(SHAPES))
    r = subprocess.run([sys.executable, "-c", child], env=dict(os.environ, EUNET_LIB=lib), capture_output=True,
                       text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0 and "DEBUG_OK" in r.stdout


# ---- evaluator ----------------------------------------------------------------------------------------------
def _evaluator(**kw):
    from eunet.evaluator import Evaluator
    return Evaluator(None, DEV, "enhanced_unet", preprocess=None, **kw)


def _tail_on_reference_ids(sem, depth, min_area=3):
    """semantic_to_instances with split="watershed", its ids taken from the restatement: the 2x2 open and the exact
    transform by the existing ops, R.split on the host, then the tail (outer_perimeter, area limits, score, one plane
    per kept id, the MAX_INSTANCES cut) written out again."""
    from eunet import evaluator as E
    from eunet import ops
    t = torch.from_numpy(sem).to(DEV)
    masks, labels, scores = [], [], []
    for class_id in (1, 2):
        cm, cnt = ops.mask_eq(t, class_id)
        if int(cnt.item()) == 0:
            continue
        cm = ops.morph_u8(ops.morph_u8(cm, 2, False), 2, True)
        D = ops.distance_transform_sq(cm.long(), [1], "ne")[0].cpu().numpy().astype(np.int64)
        ids, n, areas = R.split(D, depth)
        if n == 0:
            continue
        stats = ops.outer_perimeter(torch.from_numpy(ids).to(DEV), n).cpu().numpy()
        assert stats[:, 2].tolist() == areas.tolist()
        for k in range(n):
            area = int(areas[k])
            if area < max(E.MIN_AREA_CLASS[class_id], min_area) or area > E.MAX_AREA:
                continue
            perimeter = int(stats[k, 0]) + int(stats[k, 1]) * math.sqrt(2.0)
            compactness = 4 * np.pi * area / (perimeter ** 2) if perimeter > 0 else 0.5
            masks.append(torch.from_numpy((ids == k + 1).astype(np.uint8)))
            labels.append(class_id - 1)
            scores.append(0.7 * min(area / 150.0, 1.0) + 0.3 * compactness)
        if len(masks) > E.MAX_INSTANCES:
            keep = sorted(range(len(scores)), key=lambda i: scores[i], reverse=True)[:E.MAX_INSTANCES]
            masks, labels, scores = [masks[i] for i in keep], [labels[i] for i in keep], [scores[i] for i in keep]
    return masks, labels, scores


def _synth_mask(h, w, seed):
    from eunet import synth
    _, m = synth.tile(h, w, seed, num_classes=3, in_channels=3)
    return np.ascontiguousarray(m).astype(np.int64)


@pytest.mark.parametrize("depth", [1.0, 0.0])
def test_semantic_to_instances_with_the_watershed_split(depth):
    sem = _synth_mask(96, 128, 40)
    assert (sem == 1).any() and (sem == 2).any()
    ev = _evaluator(split="watershed", split_depth=depth)
    masks, labels, scores = ev.semantic_to_instances(sem)
    ref_masks, ref_labels, ref_scores = _tail_on_reference_ids(sem, depth)
    assert len(ref_masks) >= 2 and labels == ref_labels
    assert [float(s) for s in scores] == [float(s) for s in ref_scores]  # float64 equality
    got = torch.stack(masks)
    assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got.cpu(), torch.stack(ref_masks))


def test_two_touching_cells_come_out_as_two_instances():
    sem = np.zeros((40, 60), np.int64)
    sem[R.discs(40, 60, [(20, 20, 8), (20, 32, 8)])] = 1
    masks, labels, scores = _evaluator(split="watershed").semantic_to_instances(sem)
    assert labels == [0, 0] and len(scores) == 2
    a, b = (m.cpu().numpy().astype(bool) for m in masks)
    assert a[20, 14] and b[20, 38] and not (a & b).any()
    both = a | b  # together: the 2x2-opened class mask
    from eunet import ops
    opened = ops.morph_u8(ops.morph_u8(torch.from_numpy((sem == 1).astype(np.uint8)).to(DEV), 2, False), 2, True)
    assert np.array_equal(both, opened.cpu().numpy().astype(bool))
    masks, labels, _ = _evaluator(split="watershed", split_depth=math.inf).semantic_to_instances(sem)
    assert labels == [0] and np.array_equal(masks[0].cpu().numpy().astype(bool), both)  # merged: one component


def test_the_erosion_split_is_the_default_and_unchanged():
    sem = _synth_mask(96, 128, 41)
    default = _evaluator().semantic_to_instances(sem)
    erosion = _evaluator(split="erosion").semantic_to_instances(sem)
    assert len(default[0]) >= 2 and default[1] == erosion[1] and default[2] == erosion[2]
    assert torch.equal(torch.stack(default[0]), torch.stack(erosion[0]))
    with pytest.raises(ValueError):
        _evaluator(split="flood")


def test_evaluate_runs_on_the_watershed_split_with_its_keys():
    """evaluate, evaluate_with_curves and coco_map=True on top of split="watershed": the keys are the ones the
    erosion split gives; the rows that do not depend on the split are equal."""
    from eunet import evaluator as E
    from eunet import synth
    from eunet.models import EnhancedUNet
    torch.manual_seed(3)
    model = EnhancedUNet(num_classes=3, in_channels=3, base_ch=16).to(DEV).eval()
    x, m = synth.tile(96, 128, 42, num_classes=3, in_channels=3)
    gt = [torch.from_numpy(((m == c) & (np.indices(m.shape)[1] < 64)).astype(np.uint8)) for c in (1, 2)]
    loader = [{"images": [torch.from_numpy(x)],
               "batch_items": [{"semantic_mask": m, "instance_masks": gt, "instance_labels": [0, 1]}]}]
    results = {}
    for split in ("erosion", "watershed"):
        ev = E.Evaluator(model, DEV, "enhanced_unet", preprocess=None, split=split)
        results[split] = (ev.evaluate(loader, coco_map=True), ev.evaluate_with_curves(loader))
    for a, b in zip(results["erosion"], results["watershed"]):
        assert list(a) == list(b)
        for k in a:
            if k.startswith("sem_") or k.startswith(("auc_", "ap_", "ece_")) or k.startswith("gt_"):
                assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), k
    assert set(E.EVALUATE_KEYS) | set(E.COCO_KEYS) <= set(results["watershed"][0])
    assert set(E.CURVE_KEYS) <= set(results["watershed"][1])
