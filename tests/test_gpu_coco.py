"""COCO bbox / segm mAP on the GPU (instances.hip: eunet_pack_masks_bbox, eunet_coco_match) against numpy and
the plain-loop restatement of COCOeval in tests/_coco_ref.py.  The kernels are integer / correctly rounded
fp64, so their checks are exact; the mAP values are compared at 1e-12 (values in [0, 1], a mean of 2020
float64 terms: rounding stays below 2.3e-13)."""
import os
import warnings

import numpy as np
import pytest
import torch

import _coco_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-12


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- pack_masks_bbox -----------------------------------------------------------------------------------
def _bbox_masks(h, w, n, seed):
    """n masks per kind: a single pixel in each corner, full, empty, sparse random, only the last partial
    word set."""
    g = np.random.default_rng(seed)
    hw = h * w
    kinds = []
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        m = np.zeros((h, w), np.uint8)
        m[y, x] = 1
        kinds.append(m)
    kinds.append(np.full((h, w), 7, np.uint8))
    kinds.append(np.zeros((h, w), np.uint8))
    kinds.append(((g.random((h, w)) < 0.08) * g.integers(1, 255, (h, w))).astype(np.uint8))
    m = np.zeros(hw, np.uint8)
    m[(hw - 1) // 64 * 64:] = 1     # the pixels of the last (partial, unless hw % 64 == 0) word
    kinds.append(m.reshape(h, w))
    stacks = []
    for i in range(len(kinds)):     # rotate, so every kind sits at every position of an n-stack
        stacks.append(np.stack([kinds[(i + j) % len(kinds)] for j in range(n)]))
    return stacks


def _bbox_ref(m, h, w):
    ys, xs = np.nonzero(m)
    if len(ys) == 0:
        return (w, h, -1, -1)
    return (xs.min(), ys.min(), xs.max(), ys.max())


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("h,w", [(1, 1), (3, 64), (5, 65), (7, 129), (40, 70), (64, 64)])
def test_pack_masks_bbox_exact(h, w, n):
    from eunet import ops
    for stack in _bbox_masks(h, w, n, 100 * h + w):
        d = dev(stack)
        packed, areas, bbox = ops.pack_masks_bbox(d)
        p0, a0 = ops.pack_masks(d)
        assert torch.equal(packed, p0) and torch.equal(areas, a0)
        flat = stack.reshape(n, -1) != 0
        assert np.array_equal(areas.cpu().numpy(), flat.sum(1))
        bits = np.zeros((n, packed.shape[1] * 64), bool)
        bits[:, :h * w] = flat
        words = (bits.reshape(n, -1, 64) * (np.uint64(1) << np.arange(64, dtype=np.uint64))).sum(2, dtype=np.uint64)
        assert np.array_equal(packed.cpu().numpy().view(np.uint64), words)
        assert bbox.dtype == torch.int32 and bbox.shape == (n, 4)
        ref = np.array([_bbox_ref(m, h, w) for m in stack], np.int32)
        assert np.array_equal(bbox.cpu().numpy(), ref), (h, w, bbox.cpu().numpy(), ref)


# ---- coco_match ----------------------------------------------------------------------------------------
FRACTIONS = ((1, 2), (11, 20), (3, 5), (13, 20), (7, 10), (3, 4), (4, 5), (17, 20), (9, 10), (19, 20))


def _match_inputs(D, G, seed, gt_all_class0):
    """Integer inputs built directly (not from masks).  Planted: pairs whose IoU is exactly each of
    FRACTIONS for both types (segm: inter 2p, both areas p + q -> 2p / 2q; bbox: widths p + q shifted by
    q - p -> (2p) / (2q)); duplicated ground-truth columns (equal IoU: the later must win); pairs with
    intersecting boxes and zero pixel overlap."""
    g = np.random.default_rng(seed)
    cls_d = g.integers(0, 2, D).astype(np.int32)
    cls_g = g.integers(0, 2, G).astype(np.int32)
    if gt_all_class0:
        cls_g[:] = 0                 # class 1 then has detections and no ground truth
        cls_d[D - 1] = 1
    area_d = g.integers(40, 90, D).astype(np.int64)
    area_g = g.integers(40, 90, G).astype(np.int64)
    cap = np.minimum(area_d[:, None], area_g[None, :])
    inter = np.where(g.random((D, G)) < 0.25, g.integers(0, 40, (D, G)), 0).astype(np.int64)
    close = g.random((D, G)) < 0.05
    inter = np.where(close, cap - g.integers(0, 4, (D, G)), inter)   # IoUs near 1 as well
    box_d = np.stack([g.integers(0, 40, D), g.integers(0, 40, D), g.integers(1, 30, D), g.integers(1, 30, D)], 1)
    box_g = np.stack([g.integers(0, 40, G), g.integers(0, 40, G), g.integers(1, 30, G), g.integers(1, 30, G)], 1)
    box_d, box_g = box_d.astype(np.int32), box_g.astype(np.int32)
    for i, (p, q) in enumerate(FRACTIONS):
        d, gi = (3 * i) % D, (7 * i + 1) % G
        if gt_all_class0:
            cls_d[d] = 0
        else:
            cls_g[gi] = cls_d[d]
        area_d[d] = area_g[gi] = p + q
        inter[d, :] = np.minimum(inter[d, :], np.minimum(area_d[d], area_g))
        inter[:, gi] = np.minimum(inter[:, gi], np.minimum(area_d, area_g[gi]))
        inter[d, gi] = 2 * p
        box_d[d] = (5, 6, p + q, 4)
        box_g[gi] = (5 + q - p, 6, p + q, 4)
    if G >= 2:                       # equal IoU on two untaken ground truths: duplicate planted columns
        for src, dst in (((7 * 2 + 1) % G, G - 1), ((7 * 5 + 1) % G, (G // 2))):
            if src != dst:
                inter[:, dst], area_g[dst], box_g[dst], cls_g[dst] = inter[:, src], area_g[src], box_g[src], cls_g[src]
    d, gi = D - 1, 0                 # intersecting boxes, zero pixel overlap
    box_d[d] = box_g[gi]
    inter[d, gi] = 0
    if not gt_all_class0:
        cls_d[d] = cls_g[gi]
    cap = np.minimum(area_d[:, None], area_g[None, :])
    inter = np.minimum(inter, cap)
    return inter, area_d, area_g, box_d, box_g, cls_d, cls_g


def _match_ref(inter, area_d, area_g, box_d, box_g, cls_d, cls_g, thrs):
    D, G = inter.shape
    exp = -np.ones((2, len(thrs), D), np.int32)
    for c in (0, 1):
        ds, gs = np.nonzero(cls_d == c)[0], np.nonzero(cls_g == c)[0]
        for ty in (0, 1):
            if ty == 0:
                ious = [[R.bbox_iou(box_d[d], box_g[k]) for k in gs] for d in ds]
            else:
                ious = [[R.segm_iou_counts(inter[d, k], area_d[d], area_g[k]) for k in gs] for d in ds]
            dtm = R.evaluate_img(ious, thrs)
            for t in range(len(thrs)):
                for j, m in enumerate(dtm[t]):
                    exp[ty, t, ds[j]] = gs[m] if m >= 0 else -1
    return exp


def _run_match(inp, thrs):
    from eunet import ops
    inter, area_d, area_g, box_d, box_g, cls_d, cls_g = inp
    return ops.coco_match(dev(inter), dev(area_d), dev(area_g), dev(box_d), dev(box_g), dev(cls_d), dev(cls_g),
                          thrs).cpu().numpy()


@pytest.mark.parametrize("G", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("D", [1, 63, 64, 65, 200])
def test_coco_match_exact(D, G):
    for gt_all_class0 in (False, True):
        inp = _match_inputs(D, G, 1000 * D + G, gt_all_class0)
        got = _run_match(inp, R.IOU_THRS)
        exp = _match_ref(*inp, R.IOU_THRS)
        assert got.shape == (2, 10, D) and got.dtype == np.int32
        assert np.array_equal(got, exp), (D, G, gt_all_class0, np.argwhere(got != exp)[:5])
        if D >= 63 and G >= 63:
            assert (exp >= 0).any() and (exp == -1).any() and not np.array_equal(exp[0], exp[1])
        if gt_all_class0 and D > 1:
            assert (inp[5] == 1).any() and (exp[:, :, inp[5] == 1] == -1).all()


def test_coco_match_planted_cases():
    """The planted rows by hand: an IoU of exactly p / q matches at every threshold <= p / q as the host
    compares them; of two equal ground truths the later is taken first, the earlier by the next detection."""
    inter = np.array([[6, 6], [6, 6], [0, 0]], np.int64)            # 6 / (8 + 8 - 6) = 3 / 5
    area_d, area_g = np.array([8, 8, 8], np.int64), np.array([8, 8], np.int64)
    box_d = np.array([[0, 0, 8, 4], [0, 0, 8, 4], [1, 1, 3, 3]], np.int32)   # (8 - 2) * 4 / ((8 + 2) * 4) = 3 / 5
    box_g = np.array([[2, 0, 8, 4], [2, 0, 8, 4]], np.int32)
    cls = np.zeros(3, np.int32)
    got = _run_match((inter, area_d, area_g, box_d, box_g, cls, cls[:2]), R.IOU_THRS)
    n_match = sum(1 for t in R.IOU_THRS if 6 / 10 >= min(t, 1 - 1e-10))
    assert n_match in (2, 3)
    for ty in (0, 1):
        for t in range(10):
            assert list(got[ty, t]) == ([1, 0, -1] if t < n_match else [-1, -1, -1]), (ty, t, got[ty, t])


def test_coco_match_limits_raise():
    from eunet import ops
    from eunet._lib import EunetError

    def call(D, G, T, cd=0, cg=0):
        z = lambda *s, dt=torch.int64: torch.zeros(*s, dtype=dt, device="cuda")  # noqa: E731
        return ops.coco_match(z(D, G), z(D) + 1, z(G) + 1, z(D, 4, dt=torch.int32) + 1, z(G, 4, dt=torch.int32) + 1,
                              z(D, dt=torch.int32) + cd, z(G, dt=torch.int32) + cg, [0.5] * T)

    assert call(2, 3, 16).shape == (2, 16, 2)
    for bad in ((4097, 1, 1), (1, 8193, 1), (1, 1, 17)):
        with pytest.raises(EunetError):
            call(*bad)
    for cd, cg in ((2, 0), (0, 2), (-1, 0)):
        with pytest.raises(EunetError):
            call(2, 2, 1, cd, cg)


# ---- calculate_coco_metrics end to end -------------------------------------------------------------------
H, W = 40, 70


def _rect_mask(g, x, y, w, h):
    """A rectangle with at least one corner pixel knocked out (so segm != bbox IoU), clipped to the image."""
    x, y = int(np.clip(x, 0, W - 3)), int(np.clip(y, 0, H - 3))
    w, h = int(np.clip(w, 3, W - x)), int(np.clip(h, 3, H - y))   # >= 3 x 3: never empty without its corners
    m = np.zeros((H, W), np.uint8)
    m[y:y + h, x:x + w] = 1
    corners = [(y, x), (y, x + w - 1), (y + h - 1, x), (y + h - 1, x + w - 1)]
    drop = g.random(4) < 0.5
    drop[g.integers(0, 4)] = True
    for (cy, cx), dr in zip(corners, drop):
        if dr:
            m[cy, cx] = 0
    return m, (x, y, w, h)


def make_case(seed=20260101):
    """(pred_annotations, gt_annotations) with numpy masks at 40 x 70: image 0 has 70 ground truths and 130
    predictions (one class exceeds 100 detections), image 1 has 5 and 3, image 2 has 9 and 0.  Most
    predictions are perturbed ground truths, some with the wrong class, some unrelated; scores are k / 8."""
    g = np.random.default_rng(seed)
    gt_by_image, preds = {}, []
    for iid, (n_gt, n_pred) in enumerate(((70, 130), (5, 3), (9, 0))):
        gts = []
        for _ in range(n_gt):
            w, h = int(g.integers(4, 10)), int(g.integers(4, 10))
            m, box = _rect_mask(g, g.integers(0, W - w + 1), g.integers(0, H - h + 1), w, h)
            gts.append({"image_id": iid, "category_id": int(g.random() < 0.08), "segmentation": m, "_box": box})
        gt_by_image[iid] = gts
        for j in range(n_pred):
            if g.random() < 0.1:    # unrelated
                w, h = int(g.integers(3, 10)), int(g.integers(3, 10))
                m, _ = _rect_mask(g, g.integers(0, W - w + 1), g.integers(0, H - h + 1), w, h)
                cat = int(g.random() < 0.12)
            else:
                src = gts[j % n_gt] if j < n_gt else gts[int(g.integers(0, n_gt))]
                x, y, w, h = src["_box"]
                dx, dy, dw, dh = (int(v) for v in g.integers(-1, 2, 4) * (g.random(4) < 0.4))
                m, _ = _rect_mask(g, x + dx, y + dy, w + dw, h + dh)
                cat = src["category_id"] if g.random() < 0.93 else 1 - src["category_id"]
            preds.append({"image_id": iid, "category_id": cat, "score": int(g.integers(1, 8)) / 8,
                          "segmentation": m})
    gt_list = gt_by_image[1] + gt_by_image[0] + gt_by_image[2]   # ids by list position, images interleaved
    for a in gt_list:
        del a["_box"]
    preds = [preds[i] for i in g.permutation(len(preds))]
    return preds, gt_list


@pytest.fixture(scope="module")
def case():
    preds, gts = make_case()
    n0 = [sum(1 for a in preds if a["image_id"] == 0 and a["category_id"] == c) for c in (0, 1)]
    assert max(n0) > 100 and len(preds) == 133 and len(gts) == 84
    ref = R.coco_metrics(preds, gts)
    # on the restatement alone: the case does not pass by degenerating
    assert 0.05 < ref["bbox_mAP"] < 0.95 and 0.05 < ref["segm_mAP"] < 0.95
    assert ref["bbox_mAP"] != ref["segm_mAP"]
    return preds, gts, ref


@pytest.mark.parametrize("as_tensors", [False, True])
def test_calculate_coco_metrics_matches_the_restatement(case, as_tensors):
    from eunet.metrics import calculate_coco_metrics
    preds, gts, ref = case
    if as_tensors:
        preds = [dict(a, segmentation=dev(a["segmentation"])) for a in preds]
        gts = [dict(a, segmentation=dev(a["segmentation"])) for a in gts]
    got = calculate_coco_metrics(preds, gts)
    print("coco", got, ref)
    assert sorted(got) == ["bbox_mAP", "segm_mAP"]
    for k in got:
        assert abs(got[k] - ref[k]) <= TOL, (k, got[k], ref[k])


def test_calculate_coco_metrics_edges(case):
    from eunet.metrics import calculate_coco_metrics
    preds, gts, _ = case
    zeros = {"bbox_mAP": 0.0, "segm_mAP": 0.0}
    assert calculate_coco_metrics([], gts) == zeros and calculate_coco_metrics(preds, []) == zeros
    with pytest.warns(UserWarning):    # a prediction on an image without ground truth
        assert calculate_coco_metrics(preds + [dict(preds[0], image_id=99)], gts) == zeros
    empty = dict(preds[0], segmentation=np.zeros((H, W), np.uint8))
    with pytest.raises(ValueError):
        calculate_coco_metrics([empty] + preds, gts)
    # a supplied bbox is not read
    junk = [dict(a, bbox=[0.0, 0.0, 1.0, 1.0]) for a in preds[:20]]
    assert calculate_coco_metrics(junk, gts) == calculate_coco_metrics(preds[:20], gts)


# ---- evaluate(coco_map=True) -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "instances.npz"))


def _evaluator(golden):
    from eunet.evaluator import Evaluator
    ev = Evaluator(None, "cuda", "enhanced_unet", preprocess=None)
    ev.predict_semantic_mask = lambda image: golden[f"e{int(image)}_pred"]
    return ev


def _batch(golden, idx, drop_gt=()):
    items = []
    for i in idx:
        keep = i not in drop_gt
        items.append({"instance_masks": list(dev(golden[f"e{i}_gt_masks"])) if keep else [],
                      "instance_labels": [int(v) for v in golden[f"e{i}_gt_labels"]] if keep else [],
                      "semantic_mask": dev(golden[f"e{i}_gt_sem"]), "image_id": f"img{i}"})
    return {"images": [torch.tensor(i) for i in idx], "batch_items": items}


def test_evaluate_with_coco_map(golden):
    from eunet.evaluator import COCO_KEYS, EVALUATE_KEYS
    from eunet.metrics import calculate_coco_metrics
    ev = _evaluator(golden)
    assert int(golden["e_n"]) == 3
    loader = [_batch(golden, [0, 1]), _batch(golden, [2])]
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        res = ev.evaluate(loader, coco_map=True)
        plain = ev.evaluate(loader)
    assert not [w for w in rec if "ground truth" in str(w.message)]
    assert sorted(res) == sorted(EVALUATE_KEYS + COCO_KEYS)
    assert [float(res[str(k)]) for k in golden["e_keys"]] == list(golden["e_vals"])   # the 23 old keys, exactly
    assert "bbox_mAP" not in plain and "segm_mAP" not in plain and sorted(plain) == list(golden["e_keys"])
    preds, gts = [], []
    for i in range(3):
        masks, labels, scores = ev.semantic_to_instances(golden[f"e{i}_pred"])
        preds += [{"image_id": i, "category_id": int(l), "score": float(s), "segmentation": m}
                  for m, l, s in zip(masks, labels, scores)]
        gts += [{"image_id": i, "category_id": int(l), "segmentation": m}
                for m, l in zip(golden[f"e{i}_gt_masks"], golden[f"e{i}_gt_labels"])]
    assert preds and gts
    direct = calculate_coco_metrics(preds, gts)
    ref = R.coco_metrics([dict(a, segmentation=a["segmentation"].cpu().numpy()) for a in preds], gts)
    print("evaluate coco", {k: res[k] for k in COCO_KEYS}, direct, ref)
    for k in COCO_KEYS:
        assert float(res[k]) == direct[k], (k, res[k], direct[k])
        assert abs(float(res[k]) - ref[k]) <= TOL, (k, res[k], ref[k])


def test_evaluate_coco_map_image_without_ground_truth(golden):
    ev = _evaluator(golden)
    with pytest.warns(UserWarning):
        res = ev.evaluate([_batch(golden, [0, 1], drop_gt=(1,))], coco_map=True)
    assert res["bbox_mAP"] == 0.0 and res["segm_mAP"] == 0.0
