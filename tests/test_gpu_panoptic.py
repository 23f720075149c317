"""The evaluator's label-map path (semantic_to_instance_maps, evaluate_panoptic, evaluate_by_size) against the mask
stacks of semantic_to_instances, against metrics.calculate_panoptic_metrics applied by hand and against the plain-loop
restatement of tests/_panoptic_ref.py.  Integer results are compared exactly; the float sums at 1e-12 absolute (see
tests/test_panoptic_host.py)."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _panoptic_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
_STATE = {}


def _model():
    if "model" not in _STATE:
        from eunet.models import EnhancedUNet
        torch.manual_seed(3)
        _STATE["model"] = EnhancedUNet(num_classes=3, in_channels=3, base_ch=16).to(DEV).eval()
    return _STATE["model"]


def _evaluator(model=None, **kw):
    from eunet.evaluator import Evaluator
    return Evaluator(model, DEV, "enhanced_unet", preprocess=None, **kw)


def _item(h, w, seed, ignore=True):
    """A synthetic tile as a dataset item: one uint8 mask per cell that is still visible, its class as the label."""
    from eunet import synth
    x, m, inst = synth.tile(h, w, seed, num_classes=3, in_channels=3, instances=True)
    m = np.ascontiguousarray(m).astype(np.int64)
    masks, labels = [], []
    for j in np.unique(inst[inst > 0]).tolist():
        sel = inst == j
        masks.append(torch.from_numpy(sel.astype(np.uint8)))
        labels.append(int(m[sel][0]) - 1)
    if ignore:
        m[:6, :9] = 255
    return x, {"semantic_mask": m, "instance_masks": masks, "instance_labels": labels}


def _loader():
    if "loader" not in _STATE:
        items = [_item(96, 128, 40), _item(128, 96, 43)]
        assert all(0 in it["instance_labels"] and 1 in it["instance_labels"] for _, it in items)
        _STATE["loader"] = [{"images": [torch.from_numpy(x)], "batch_items": [it]} for x, it in items]
    return _STATE["loader"]


def _many_regions():
    """A hand-made semantic mask with more than MAX_INSTANCES small regions of both classes."""
    sem = np.zeros((120, 160), np.int64)
    for y in range(0, 116, 4):
        for x in range(0, 156, 4):
            sem[y:y + 3, x:x + 3 - (x // 4) % 2] = 1 + (y // 4 + x // 4) % 3 // 2  # 3 x 3 and 3 x 2 squares, 2/3 live
    return sem


def _check_maps_against_masks(ev, sem):
    from eunet import ops
    masks, labels, scores = ev.semantic_to_instances(sem)
    ids, counts, map_scores = ev.semantic_to_instance_maps(sem)
    assert ids.is_cuda and ids.dtype == torch.int32 and tuple(ids.shape) == (2,) + tuple(sem.shape)
    assert counts == [labels.count(0), labels.count(1)] and [len(s) for s in map_scores] == counts
    for c in (0, 1):
        mine = [m for m, l in zip(masks, labels) if l == c]
        assert sorted(map_scores[c]) == sorted(s for s, l in zip(scores, labels) if l == c)  # the same multiset
        if not mine:
            assert int(ids[c].abs().sum()) == 0
            continue
        stack = torch.stack(mine)
        from_masks, overlap = ops.labels_from_stack(stack, list(range(1, len(mine) + 1)))
        assert overlap == 0
        pairs = ops.label_pairs(ids[c], from_masks)
        # a bijection between the map's ids and the planes, each pair's count both areas: no (id, 0) or (0, plane) row
        assert len(pairs) == counts[c] and (pairs[:, 1:3] > 0).all()
        assert sorted(pairs[:, 1].tolist()) == sorted(pairs[:, 2].tolist()) == list(range(1, counts[c] + 1))
        areas = stack.flatten(1).ne(0).sum(1).cpu().numpy()
        assert np.array_equal(pairs[:, 3], areas[pairs[:, 2] - 1])
        by_id = {int(i): int(j) for _, i, j, _ in pairs}
        mine_scores = [s for s, l in zip(scores, labels) if l == c]
        assert all(map_scores[c][i - 1] == mine_scores[j - 1] for i, j in by_id.items())  # float64 equality
    return counts


@pytest.mark.parametrize("split", ["erosion", "watershed"])
def test_instance_maps_are_the_instances_of_the_mask_stack(split):
    from eunet import synth
    ev = _evaluator(split=split)
    _, m = synth.tile(96, 128, 40, num_classes=3, in_channels=3)
    counts = _check_maps_against_masks(ev, np.ascontiguousarray(m).astype(np.int64))
    assert sum(counts) >= 2
    _, m = synth.tile(160, 96, 44, num_classes=3, in_channels=3)
    _check_maps_against_masks(ev, torch.from_numpy(np.ascontiguousarray(m)).to(DEV))
    only_dead = np.zeros((40, 50), np.int64)
    only_dead[10:20, 10:25] = 2
    assert _check_maps_against_masks(ev, only_dead) == [0, 1]
    assert _check_maps_against_masks(ev, np.zeros((33, 47), np.int64)) == [0, 0]


@pytest.mark.parametrize("split", ["erosion", "watershed"])
def test_the_instance_cut_is_taken_on_the_maps_too(split):
    from eunet import evaluator as E
    sem = _many_regions()
    ev = _evaluator(split=split)
    counts = _check_maps_against_masks(ev, sem)
    assert sum(counts) == E.MAX_INSTANCES and min(counts) >= 1
    _, uncut, _ = ev.semantic_to_instance_maps(np.where(sem == 1, 1, 0))
    assert uncut[0] == E.MAX_INSTANCES > counts[0]  # the second cut, on the combined list, took live instances too


DEBUG_CHILD = r'''
import sys, numpy as np, torch
sys.path[:0] = [ROOT, ROOT + "/enhanced-unet_amd"]
from eunet import _lib
from eunet.evaluator import Evaluator, MAX_INSTANCES
assert _lib.load().eunet_debug_enabled() == 1, "not the debug build"
assert _lib.debug_status(reset=True) == (0, 0)
MANY_REGIONS
masks = {"many regions": (_many_regions(), 3)}
last = np.zeros((80, 90), np.int64)  # the regions that come last in raster order are under the area limits
last[2:8, 2:8], last[74:76, 10:13] = 1, 1    # 36 px kept, 6 px under min_area = 10
last[2:8, 20:26], last[74:76, 40:42] = 2, 2  # 36 px kept, 4 px under the dead class's minimum
masks["last ids filtered"] = (last, 10)
for name, (sem, min_area) in masks.items():
    for split in ("erosion", "watershed"):
        ev = Evaluator(None, "cuda", "enhanced_unet", preprocess=None, split=split)
        ids, counts, scores = ev.semantic_to_instance_maps(sem, min_area)
        m, labels, _ = ev.semantic_to_instances(sem, min_area)
        assert counts == [labels.count(0), labels.count(1)] and int(ids[0].max()) == counts[0]
        st = _lib.debug_status()
        print(name, split, counts, "debug status", st)
        assert st == (0, 0), (name, split, st)
        assert sum(counts) == (MAX_INSTANCES if name == "many regions" else 2), (name, counts)
print("DEBUG_OK")
'''


def test_debug_build_bounds_checks_pass_on_the_instance_maps():
    """semantic_to_instance_maps and semantic_to_instances under the bounds-checked debug build, on masks whose
    highest-numbered regions are dropped by the selection (the MAX_INSTANCES cut, the minimum areas): the
    relabel and expand tables hold an entry for every id of the split's map."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "enhanced-unet_amd", "eunet", "libeunet_hip_debug.so")
    assert os.path.exists(lib), "build it: make -C enhanced-unet_amd debug"
    child = DEBUG_CHILD.replace("MANY_REGIONS", inspect.getsource(_many_regions)).replace("ROOT", repr(root))
    r = subprocess.run([sys.executable, "-c", child], env=dict(os.environ, EUNET_LIB=lib), capture_output=True,
                       text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0 and "DEBUG_OK" in r.stdout


def _by_hand(ev, loader, iou_percent):
    """evaluate_panoptic's steps written out: the maps of every image, then their statistics two ways."""
    from eunet import metrics as M
    from eunet import ops
    maps, acc, ajis = [], None, []
    for batch in loader:
        item = batch["batch_items"][0]
        pred = torch.from_numpy(ev.predict_semantic_mask(batch["images"][0])).to(DEV)
        pred_ids, _, _ = ev.semantic_to_instance_maps(pred)
        stack = torch.stack(item["instance_masks"]).to(DEV)
        ignore = torch.from_numpy((item["semantic_mask"] == 255).astype(np.uint8)).to(DEV)
        gt_ids = torch.stack([ops.labels_from_stack(stack, [j + 1 if l == c else 0 for j, l in
                                                            enumerate(item["instance_labels"])], ignore)[0]
                              for c in (0, 1)])
        maps.append((pred_ids, gt_ids))
        st = M.instance_stats_from_pairs(ops.label_pairs(pred_ids, gt_ids), 2, iou_percent)
        ref = R.stats(pred_ids.cpu().numpy(), gt_ids.cpu().numpy(), iou_percent)
        for k in ("n_pred", "n_gt", "tp50", "tp", "aji_c", "aji_u", "objdice_gw", "objdice_pw"):
            assert np.array_equal(st[k], ref[k]), k
        for k in ("iou_sum", "seg_sum", "objdice_g", "objdice_p"):
            assert np.abs(st[k] - ref[k]).max() <= 1e-12, k
        ajis.append(int(st["aji_c"].sum()) / int(st["aji_u"].sum()))
        acc = M.add_instance_stats(acc, st)
    return maps, acc, ajis


def _same(a, b):
    return a == b or (a != a and b != b)


def test_evaluate_panoptic_is_the_one_call_form_applied_by_hand():
    from eunet import evaluator as E
    from eunet import metrics as M
    ev = _evaluator(_model(), split="watershed")
    loader = _loader()
    result = ev.evaluate_panoptic(loader)
    assert tuple(result) == E.PANOPTIC_KEYS
    maps, acc, ajis = _by_hand(ev, loader, M.PANOPTIC_IOU_PERCENT)
    pooled = M.panoptic_metrics_from_stats(acc)
    assert all(_same(result[k], v) for k, v in pooled.items())
    assert result["aji_image_mean"] == float(np.mean(ajis)) and result["gt_overlap_pixels"] == 0
    one = ev.evaluate_panoptic(loader[:1])  # one image: the one-call form on its maps
    by_hand = M.calculate_panoptic_metrics(*maps[0])
    assert all(_same(one[k], v) for k, v in by_hand.items()) and one["aji_image_mean"] == one["aji"]
    ts = (50, 75, 90)
    few = ev.evaluate_panoptic(loader, iou_percent=ts)
    assert tuple(few) == M.panoptic_keys(iou_percent=ts) + ("aji_image_mean", "gt_overlap_pixels")
    assert all(_same(few[k], result[k]) for k in few if not k.startswith("ap_dsb"))
    with pytest.raises(ValueError):
        ev.evaluate_panoptic([])
    with pytest.raises(ValueError):
        _evaluator(_model(), activation="sigmoid").evaluate_panoptic(loader)


def test_a_prediction_equal_to_the_ground_truth_scores_one():
    """The ground truth's own maps on both sides, and through evaluate_panoptic with the prediction steps replaced:
    the semantic mask predicted is the item's, the instances are the item's."""
    from eunet import metrics as M
    from eunet import ops
    _, item = _item(96, 128, 40)
    stack = torch.stack(item["instance_masks"]).to(DEV)
    ignore = torch.from_numpy((item["semantic_mask"] == 255).astype(np.uint8)).to(DEV)
    gt_ids = torch.stack([ops.labels_from_stack(stack, [j + 1 if l == c else 0 for j, l in
                                                        enumerate(item["instance_labels"])], ignore)[0] for c in (0, 1)])
    scores = M.calculate_panoptic_metrics(gt_ids.clamp(min=0), gt_ids)
    assert set(scores) == set(M.panoptic_keys()) and all(v == 1.0 for v in scores.values()), scores

    class Oracle(type(_evaluator())):
        def _predict_mask_device(self, image):
            return image

        def semantic_to_instance_maps(self, semantic_mask, min_area=3):
            return gt_ids.clamp(min=0), None, None

    ev = Oracle(None, DEV, "enhanced_unet", preprocess=None)
    result = ev.evaluate_panoptic([{"images": [torch.from_numpy(item["semantic_mask"]).to(DEV)], "batch_items": [item]}])
    assert all(v == 1.0 for k, v in result.items() if k != "gt_overlap_pixels"), result
    assert result["gt_overlap_pixels"] == 0


def test_overlapping_ground_truth_planes_are_counted():
    _, item = _item(96, 128, 40)
    live = [j for j, l in enumerate(item["instance_labels"]) if l == 0]
    grown = item["instance_masks"][live[0]].clone()
    grown[item["instance_masks"][live[1]] != 0] = 1  # instance live[0] now also claims all of live[1]
    masks = list(item["instance_masks"])
    masks[live[0]] = grown
    ev = _evaluator(None)
    _, overlap = ev._gt_instance_maps(dict(item, instance_masks=masks), item["semantic_mask"].shape, torch.device(DEV, 0))
    assert overlap == int((item["instance_masks"][live[1]] != 0).sum())
    empty = dict(item, instance_masks=[], instance_labels=[])
    ids, overlap = ev._gt_instance_maps(empty, item["semantic_mask"].shape, torch.device(DEV, 0))
    assert overlap == 0 and torch.equal(ids[0].cpu(), torch.from_numpy(-(item["semantic_mask"] == 255).astype(np.int32)))


def test_evaluate_by_size_is_the_reference_loops():
    ev = _evaluator(_model())
    loader = _loader()
    edges = (20, 100, 500, 1000)
    got = ev.evaluate_by_size(loader, edges=edges)
    gts = [b["batch_items"][0]["semantic_mask"] for b in loader]
    preds = [ev.predict_semantic_mask(b["images"][0]) for b in loader]
    ref = R.size_strata(gts, preds, 3, edges)
    assert got["edges"] == edges and got["count"] == [len(b) for b in ref] and sum(got["count"]) >= 6
    assert all(x == y for a, b in zip(got["coverage"], ref) for x, y in zip(a, b))
    for mean, b in zip(got["mean"], ref):
        assert (mean != mean) if not b else mean == float(np.mean(b))
    assert len(ev.evaluate_by_size(loader[:1])["coverage"]) == 5  # the reference's five ranges by default
