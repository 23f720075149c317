"""Instance-level evaluation on the GPU (instances.hip): every check is exact -- integer kernels against
numpy / scipy, and the Python surface against the reference's recorded results
(tests/golden/instances.npz, tests/golden/gen_golden_instances.py).  No tolerance appears anywhere."""
import os

import numpy as np
import pytest
import torch
from scipy import ndimage

pytestmark = pytest.mark.gpu

ONES3 = np.ones((3, 3), np.int32)
ELEMS = {
    2: np.array([[0, 1], [1, 1]], np.uint8),
    3: np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], np.uint8),
    5: np.array([[0, 0, 1, 0, 0], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [0, 0, 1, 0, 0]], np.uint8),
}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "instances.npz"))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- pack + overlap ----------------------------------------------------------------------------------
def _masks(g, n, h, w, p=0.4):
    return (g.random((n, h, w)) < p).astype(np.uint8)


def _check_overlap(a, b):
    from eunet import ops
    pa, area_a = ops.pack_masks(dev(a))
    pb, area_b = ops.pack_masks(dev(b))
    inter = ops.pairwise_overlap(pa, pb).cpu().numpy()
    fa, fb = a.reshape(len(a), -1) != 0, b.reshape(len(b), -1) != 0
    ref = np.array([[np.logical_and(x, y).sum() for y in fb] for x in fa], np.int64)
    assert np.array_equal(inter, ref)
    assert np.array_equal(area_a.cpu().numpy(), fa.sum(1)) and np.array_equal(area_b.cpu().numpy(), fb.sum(1))
    return pa


@pytest.mark.parametrize("h,w,P,G", [(7, 9, 5, 7), (8, 8, 5, 7), (5, 13, 5, 7), (33, 67, 70, 65),
                                     (9, 11, 1, 6), (9, 11, 6, 1), (512, 512, 40, 40)])
def test_pack_and_pairwise_overlap_exact(h, w, P, G):
    g = np.random.default_rng(h * 1000 + w + P)
    a, b = _masks(g, P, h, w), _masks(g, G, h, w, 0.55)
    a[0] = 0                     # an empty mask
    b[-1] = 1                    # a full one
    if P > 2:
        a[2] = a[1]              # masks that overlap one another
        a[1] *= 200              # any non-zero value is set
    pa = _check_overlap(a, b)
    words = (h * w + 63) // 64
    assert pa.shape == (P, words)
    if (h * w) % 64:             # the tail word is zero-filled above the last pixel
        tail = pa[:, -1].cpu().numpy().astype(np.uint64)
        assert not (tail >> np.uint64((h * w) % 64)).any()
    word0 = sum(1 << i for i, v in enumerate(a[1].reshape(-1)[:64]) if v) if P > 1 else None
    if word0 is not None:
        assert int(pa[1, 0].cpu().numpy().astype(np.uint64)) == word0


# ---- labelling ----------------------------------------------------------------------------------------
def _spiral(h, w):
    # a one-pixel-wide rectangular spiral: walk inwards, turning right, two cells between the arms
    m = np.zeros((h, w), np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    m[y, x] = 1
    for _ in range(h * w):
        ny, nx = y + dy, x + dx
        ahead_free = 0 <= ny < h and 0 <= nx < w and not m[ny, nx]
        ny2, nx2 = y + 2 * dy, x + 2 * dx
        if ahead_free and not (0 <= ny2 < h and 0 <= nx2 < w and m[ny2, nx2]):
            y, x = ny, nx
            m[y, x] = 1
            continue
        dy, dx = dx, -dy  # turn right
        ny, nx = y + dy, x + dx
        ny2, nx2 = y + 2 * dy, x + 2 * dx
        if not (0 <= ny < h and 0 <= nx < w) or m[ny, nx] or (0 <= ny2 < h and 0 <= nx2 < w and m[ny2, nx2]):
            break
        y, x = ny, nx
        m[y, x] = 1
    return m


def _label_cases():
    g = np.random.default_rng(3)
    c = {}
    m = np.zeros((6, 7), np.uint8)
    m[0, 0] = m[1, 1] = m[2, 2] = m[1, 3] = 1      # pixels touching only diagonally
    m[4, 6] = m[5, 5] = 1
    c["diagonal"] = m
    c["spiral"] = _spiral(40, 70)
    m = np.zeros((21, 37), np.uint8)
    m[20, :] = 1
    m[:, ::2] = 1                                   # a comb: the teeth meet only in the last row
    m[0:5, 3] = 0
    c["comb"] = m
    yy, xx = np.indices((17, 19))
    c["checkerboard"] = ((yy + xx) % 2 == 0).astype(np.uint8)   # one 8-connected component
    m = np.zeros((9, 40), np.uint8)
    m[2:5, 3:6] = m[2:7, 20:23] = m[6:8, 8:12] = 1  # two components whose first pixels share a row
    c["same_row"] = m
    c["empty"] = np.zeros((13, 17), np.uint8)
    c["full"] = np.ones((33, 35), np.uint8)
    c["row"] = (g.random((1, 300)) < 0.6).astype(np.uint8)
    c["column"] = (g.random((300, 1)) < 0.6).astype(np.uint8)
    c["noise"] = (g.random((70, 130)) < 0.45).astype(np.uint8) * 9
    return c


@pytest.mark.parametrize("name", ["diagonal", "spiral", "comb", "checkerboard", "same_row", "empty", "full", "row",
                                  "column", "noise"])
def test_label_components_matches_scipy_numbering(name):
    from eunet import ops
    img = _label_cases()[name]
    ref, n_ref = ndimage.label(img, structure=ONES3)
    labels, n, areas = ops.label_components(dev(img))
    assert n == n_ref
    assert np.array_equal(labels.cpu().numpy(), ref.astype(np.int32))
    assert np.array_equal(areas.cpu().numpy(), np.bincount(ref.ravel(), minlength=n_ref + 1)[1:])
    if name == "spiral":
        assert n_ref == 1 and img.sum() > 600    # one long equivalence chain across many blocks
    if name == "checkerboard":
        assert n_ref == 1


@pytest.mark.parametrize("connectivity", [8, 4])
def test_label_components_scans_more_blocks_than_one_pass_holds(connectivity):
    """257 x 256 pixels are 257 blocks of 256: the scan of the per-block root counts takes its second pass of 256
    counts and carries the first pass's total into it.  Noise of the `noise` case's density, against scipy."""
    from eunet import ops
    img = (np.random.default_rng(11).random((257, 256)) < 0.45).astype(np.uint8)
    ref, n_ref = ndimage.label(img, structure=ONES3 if connectivity == 8 else None)
    labels, n, areas = ops.label_components(dev(img), connectivity=connectivity)
    assert n == n_ref and np.setdiff1d(ref[256], ref[:256]).size > 0   # the 257th block numbers roots too
    assert np.array_equal(labels.cpu().numpy(), ref.astype(np.int32))
    assert np.array_equal(areas.cpu().numpy(), np.bincount(ref.ravel(), minlength=n_ref + 1)[1:])


# ---- morphology ---------------------------------------------------------------------------------------
def _morph_ref(img, k, dilate, iterations):
    out = img
    for _ in range(iterations):
        out = ndimage.maximum_filter(out, footprint=ELEMS[k], mode="constant", cval=0) if dilate else \
            ndimage.minimum_filter(out, footprint=ELEMS[k], mode="constant", cval=1)
    return out


@pytest.mark.parametrize("k", [2, 3, 5])
@pytest.mark.parametrize("iterations", [1, 2, 3])
def test_morph_matches_scipy_filters(k, iterations):
    from eunet import ops
    g = np.random.default_rng(10 * k + iterations)
    img = np.zeros((37, 53), np.uint8)
    img[0:9, 10:30] = img[28:37, 5:20] = img[10:30, 0:7] = img[5:25, 45:53] = 1   # shapes on all four borders
    img[12:26, 15:40] = 1
    img[g.random(img.shape) < 0.04] ^= 1
    for dilate in (False, True):
        got = ops.morph_u8(dev(img), k, dilate, iterations).cpu().numpy()
        assert np.array_equal(got, _morph_ref(img, k, dilate, iterations)), (k, dilate, iterations)


def test_opening_of_a_2x2_block_is_an_l_of_three():
    from eunet import ops
    img = np.zeros((6, 6), np.uint8)
    img[1:3, 2:4] = 1
    opened = ops.morph_u8(ops.morph_u8(dev(img), 2, False), 2, True).cpu().numpy()
    assert opened.sum() == 3
    assert np.array_equal(opened, _morph_ref(_morph_ref(img, 2, False, 1), 2, True, 1))


# ---- perimeter counts -----------------------------------------------------------------------------------
def test_outer_perimeter_counts():
    from eunet import ops
    lab = np.zeros((40, 48), np.int32)
    expect = {}
    lab[1, 1] = 1
    expect[1] = (0, 0, 1)                                   # a single pixel
    lab[3, 2:11] = 2
    expect[2] = (16, 0, 9)                                  # a 1 x 9 line: traversed twice
    lab[6:11, 3:9] = 3
    expect[3] = (2 * (4 + 5), 0, 30)                        # a 5 x 6 square: between pixel centres
    for i in range(6):
        lab[12 + i, 20 + i] = 4
    expect[4] = (0, 10, 6)                                  # a diagonal line: 5 steps out, 5 back
    lab[20:27, 2] = 5
    lab[26, 2:8] = 5
    expect[5] = (20, 1, 12)                                 # a one-pixel-wide L: out along both arms, back with
                                                            # one diagonal step across the inner corner
    lab[20:27, 12:19] = 6
    lab[22:25, 14:17] = 0
    expect[6] = (24, 0, 40)                                 # a 7 x 7 ring: only the outer border counts
    lab[30:33, 30:33] = 7
    lab[36, 40:44] = 7
    expect[7] = (6, 0, 13)                                  # two components: the one found last is followed
    lab[0:3, 45:48] = 8
    expect[8] = (8, 0, 9)                                   # in the image corner
    # label 9 is absent (an instance that was overwritten completely)
    lab[30:32, 2:4] = 10
    lab[32, 4] = 10
    expect[9] = (0, 0, 0)
    expect[10] = (4, 2, 5)                                  # 2 x 2 block with a diagonal tail
    stats = ops.outer_perimeter(dev(lab), 10).cpu().numpy()
    for k, (na, nd, area) in expect.items():
        assert tuple(stats[k - 1, :3]) == (na, nd, area), (k, stats[k - 1])
    assert tuple(stats[2, 4:8]) == (3, 6, 8, 10)            # bounding box x0, y0, x1, y1
    assert stats[6, 3] == 36 * 48 + 40 and stats[8, 3] == -1


def test_outer_perimeter_matches_a_host_follower_on_random_blobs():
    """The kernel against a host border follower on the labelled components of smoothed noise."""
    from eunet import ops
    g = np.random.default_rng(5)
    img = (ndimage.uniform_filter(g.random((60, 90)), 3) > 0.52).astype(np.uint8)
    ref, n = ndimage.label(img, structure=ONES3)
    assert n > 20
    stats = ops.outer_perimeter(dev(ref.astype(np.int32)), n).cpu().numpy()
    dx, dy = (1, 1, 0, -1, -1, -1, 0, 1), (0, -1, -1, -1, 0, 1, 1, 1)

    def follow(mask, y0, x0):
        h, w = mask.shape
        at = lambda y, x: 0 <= y < h and 0 <= x < w and mask[y, x]  # noqa: E731
        s = 4
        while True:
            s = (s - 1) & 7
            if at(y0 + dy[s], x0 + dx[s]) or s == 4:
                break
        if s == 4:
            return 0, 0
        first, cur, na, nd = (y0 + dy[s], x0 + dx[s]), (y0, x0), 0, 0
        while True:
            for t in range(1, 9):
                ss = (s + t) & 7
                if at(cur[0] + dy[ss], cur[1] + dx[ss]):
                    s = ss
                    break
            nxt = (cur[0] + dy[s], cur[1] + dx[s])
            na, nd = na + (not s & 1), nd + (s & 1)
            if nxt == (y0, x0) and cur == first:
                return na, nd
            cur, s = nxt, (s + 4) & 7

    for k in range(1, n + 1):
        m = ref == k
        i0 = int(np.flatnonzero(m)[0])
        assert tuple(stats[k - 1, :2]) == follow(m, i0 // 90, i0 % 90), k
        assert stats[k - 1, 2] == m.sum() and stats[k - 1, 3] == i0


# ---- helpers ----------------------------------------------------------------------------------------------
def test_split_helpers():
    from eunet import ops
    g = np.random.default_rng(9)
    sem = g.integers(0, 3, (23, 41))
    for src in (sem.astype(np.int64), sem.astype(np.int32)):
        m, c = ops.mask_eq(dev(src), 2)
        assert np.array_equal(m.cpu().numpy(), (sem == 2).astype(np.uint8)) and int(c) == (sem == 2).sum()
    a, b = (g.random((23, 41)) < 0.5).astype(np.uint8) * 3, (g.random((23, 41)) < 0.5).astype(np.uint8)
    m, c = ops.mask_and(dev(a), dev(b))
    assert np.array_equal(m.cpu().numpy(), ((a != 0) & (b != 0)).astype(np.uint8)) and int(c) == ((a != 0) & (b != 0)).sum()
    markers = torch.zeros(23, 41, dtype=torch.int32, device="cuda")
    ops.write_label(dev(b), 7, markers)
    ops.write_label(dev(a), 9, markers)
    ref = np.zeros((23, 41), np.int32)
    ref[b != 0] = 7
    ref[a != 0] = 9
    assert np.array_equal(markers.cpu().numpy(), ref)
    labels = g.integers(0, 6, (23, 41)).astype(np.int32)
    table = np.array([0, 4, 0, 2, 1], np.int32)
    ops.relabel_table(dev(labels), dev(table), markers)
    for l, t in enumerate(table, 1):
        if t > 0:
            ref[labels == l] = t
    assert np.array_equal(markers.cpu().numpy(), ref)
    slots = np.array([1, -1, 0, -1, 2], np.int32)
    planes = ops.expand_labels(dev(labels), dev(slots), 3).cpu().numpy()
    for l, s in enumerate(slots, 1):
        if s >= 0:
            assert np.array_equal(planes[s], (labels == l).astype(np.uint8))


# ---- semantic_to_instances ----------------------------------------------------------------------------
def _evaluator():
    from eunet.evaluator import Evaluator
    return Evaluator(None, "cuda", "enhanced_unet", preprocess=None)


def test_semantic_to_instances_matches_the_reference(golden):
    ev = _evaluator()
    names = [str(n) for n in golden["s_names"]]
    assert len(names) >= 10
    for name in names:
        sem = golden[f"s_{name}_sem"]
        masks, labels, scores = ev.semantic_to_instances(sem if name != "neck3" else dev(sem))
        assert len(masks) == len(golden[f"s_{name}_labels"]), name
        assert labels == list(golden[f"s_{name}_labels"]), name
        assert [float(s) for s in scores] == list(golden[f"s_{name}_scores"]), name   # float64 equality
        index = golden[f"s_{name}_index"]
        if masks:
            got = torch.stack(masks)
            assert got.is_cuda and got.dtype == torch.uint8 and got.shape[1:] == sem.shape
            exp = (index[None] == np.arange(1, len(masks) + 1)[:, None, None]).astype(np.uint8)
            assert np.array_equal(got.cpu().numpy(), exp), name


# ---- metrics and evaluate -------------------------------------------------------------------------------
@pytest.mark.parametrize("as_tensors", [False, True])
def test_calculate_instance_metrics_matches_the_reference(golden, as_tensors):
    from eunet.metrics import calculate_instance_metrics
    for i in range(int(golden["m_n"])):
        pred, gt = list(golden[f"m{i}_pred"]), list(golden[f"m{i}_gt"])
        if as_tensors:
            pred, gt = [dev(m) for m in pred], [dev(m) for m in gt]
        got = calculate_instance_metrics(pred, [int(v) for v in golden[f"m{i}_pred_labels"]],
                                         [float(v) for v in golden[f"m{i}_scores"]], gt,
                                         [int(v) for v in golden[f"m{i}_gt_labels"]],
                                         iou_threshold=float(golden[f"m{i}_thr"]))
        assert sorted(got) == list(golden[f"m{i}_keys"]), i
        assert [float(got[str(k)]) for k in golden[f"m{i}_keys"]] == list(golden[f"m{i}_vals"]), i


def test_evaluate_matches_the_reference(golden):
    ev = _evaluator()
    n = int(golden["e_n"])
    ev.predict_semantic_mask = lambda image: golden[f"e{int(image)}_pred"]

    def batch(idx):
        return {"images": [torch.tensor(i) for i in idx],
                "batch_items": [{"instance_masks": list(dev(golden[f"e{i}_gt_masks"])),
                                 "instance_labels": [int(v) for v in golden[f"e{i}_gt_labels"]],
                                 "semantic_mask": dev(golden[f"e{i}_gt_sem"]), "image_id": f"img{i}"} for i in idx]}

    assert n == 3
    res = ev.evaluate([batch([0, 1]), batch([2])])
    assert "bbox_mAP" not in res and "segm_mAP" not in res
    assert sorted(res) == list(golden["e_keys"])
    assert [float(res[str(k)]) for k in golden["e_keys"]] == list(golden["e_vals"])
