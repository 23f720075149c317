"""ops.distance_transform_sq and ops.boundary_stats (csrc/boundary.hip) against the restatement of
tests/_boundary_ref.py, and the evaluator's boundary evaluation on top of them.  Everything is integer: compared
with torch.equal, no tolerance."""
import numpy as np
import pytest
import torch

import _boundary_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
VALUES = np.array([0, 1, 2, 255, 7, -1], np.int64)
MODES = ("eq", "ne", "edge")
NONE = R.NONE


def _random_maps(rng, n, h, w):
    return rng.choice(VALUES, size=(n, h, w), p=[0.4, 0.2, 0.2, 0.1, 0.05, 0.05])


def _discs(rng, h, w, n=8, classes=(1, 2)):
    """Discs of the given classes on background: regions with interiors and long distances."""
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), np.int64)
    for _ in range(n):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(2, max(3.0, min(h, w) / 4))
        m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = classes[int(rng.integers(0, len(classes)))]
    return m


def _edt(maps, values, mode, **kw):
    from eunet import ops
    out = ops.distance_transform_sq(torch.from_numpy(np.ascontiguousarray(maps)).to(DEV), values, mode, **kw)
    assert out.dtype == torch.int32 and out.is_cuda
    return out.cpu()


def _check_edt(maps, values, modes=MODES):
    for mode in modes:
        got = _edt(maps, values, mode)
        ref = R.edt_sq_maps(maps, values, mode)
        assert tuple(got.shape) == ref.shape
        assert torch.equal(got, torch.from_numpy(ref)), mode


@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (2, 65), (37, 131), (64, 64), (129, 257), (65, 1025)])
def test_transform_shapes(shape):
    rng = np.random.default_rng(shape[0] * 7919 + shape[1])
    _check_edt(_random_maps(rng, 2, *shape), [0, 1, 255])
    if min(shape) > 1:
        _check_edt(np.stack([_discs(rng, *shape), _discs(rng, *shape, n=2)]), [0, 1, 2])


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("values", [[1], [2, 0, 255], [0, 1, 2, 255, 7, -1, 5, 1]])
def test_transform_batches_and_value_counts(n, values):
    rng = np.random.default_rng(n * 10 + len(values))
    _check_edt(_random_maps(rng, n, 37, 131), values)


def test_a_site_in_each_corner_of_a_wide_map():
    """Distances far beyond any tile of the row pass: the outward scan runs hundreds of pixels."""
    h, w = 70, 1100
    for corners in ([(0, 0)], [(0, w - 1)], [(h - 1, 0)], [(h - 1, w - 1)], [(0, 0), (h - 1, w - 1)]):
        m = np.zeros((1, h, w), np.int64)
        for y, x in corners:
            m[0, y, x] = 1
        _check_edt(m, [1], modes=("eq", "edge"))
    got = _edt(m, [1], "eq")
    assert int(got[0, 0, 0, w - 1]) == min((w - 1) ** 2, (h - 1) ** 2)


def test_no_site_every_pixel_a_site_and_a_batch_with_an_empty_sample():
    h, w = 33, 70
    zeros = np.zeros((1, h, w), np.int64)
    assert torch.equal(_edt(zeros, [1], "eq"), torch.full((1, 1, h, w), NONE, dtype=torch.int32))
    assert torch.equal(_edt(zeros, [0], "ne"), torch.full((1, 1, h, w), NONE, dtype=torch.int32))
    assert torch.equal(_edt(zeros, [1], "edge"), torch.full((1, 1, h, w), NONE, dtype=torch.int32))
    assert torch.equal(_edt(zeros, [0], "eq"), torch.zeros((1, 1, h, w), dtype=torch.int32))
    assert torch.equal(_edt(zeros, [1], "ne"), torch.zeros((1, 1, h, w), dtype=torch.int32))
    # the second sample has no site of value 1, the first none of value 2: the sentinel stays in its own plane
    rng = np.random.default_rng(3)
    m = np.stack([_discs(rng, h, w, classes=(1,)), _discs(rng, h, w, classes=(2,))])
    for mode in ("eq", "edge"):
        got = _edt(m, [1, 2], mode)
        assert bool((got[1, 0] == NONE).all()) and bool((got[0, 1] == NONE).all())
        assert int(got[0, 0].max()) < NONE and int(got[1, 1].max()) < NONE
    _check_edt(m, [1, 2])


def test_sparse_sites():
    rng = np.random.default_rng(4)
    m = (rng.random((1, 257, 513)) < 0.001).astype(np.int64)
    assert 50 < m.sum() < 300
    _check_edt(m, [1], modes=("eq", "edge"))


def test_values_equal_in_their_low_32_bits():
    rng = np.random.default_rng(5)
    m = rng.choice(np.array([1, 1 + 2 ** 32, 2 ** 32, 0, -1, 2 ** 32 - 1], np.int64), size=(1, 40, 70))
    _check_edt(m, [1, 1 + 2 ** 32, 2 ** 32, 0, -1, 2 ** 32 - 1])


def test_transform_out_reuse_and_single_maps():
    from eunet import ops
    rng = np.random.default_rng(6)
    m = _random_maps(rng, 2, 20, 45)
    t = torch.from_numpy(m).to(DEV)
    out = torch.full((2, 2, 20, 45), -7, dtype=torch.int32, device=DEV)
    assert ops.distance_transform_sq(t, [1, 2], "edge", out=out) is out
    first = out.clone()
    assert ops.distance_transform_sq(t, [1, 2], "edge", out=out) is out and torch.equal(out, first)
    assert torch.equal(out.cpu(), torch.from_numpy(R.edt_sq_maps(m, [1, 2], "edge")))
    single = ops.distance_transform_sq(t[0], (1, 2), mode="edge")
    assert tuple(single.shape) == (2, 20, 45) and torch.equal(single, out[0])
    assert "distance_transform_sq" in ops.DISPATCHED and "boundary_stats" in ops.DISPATCHED


def test_transform_refusals():
    from eunet import ops
    t = torch.zeros(2, 8, 9, dtype=torch.int64, device=DEV)
    bad = [
        (t.int(), [1], {}), (t.cpu(), [1], {}), (np.zeros((8, 9), np.int64), [1], {}),
        (t[0, 0], [1], {}), (t.unsqueeze(0), [1], {}), (t[:, :, ::2], [1], {}), (t[:, :0], [1], {}),
        (torch.zeros(1, 1, 8193, dtype=torch.int64, device=DEV), [1], {}),
        (t, [], {}), (t, list(range(9)), {}), (t, [1.5], {}), (t, [2 ** 63], {}), (t, 1, {}),
        (t, [1], {"mode": "inside"}),
        (t, [1], {"out": torch.zeros(2, 1, 8, 9, dtype=torch.int64, device=DEV)}),
        (t, [1], {"out": torch.zeros(2, 2, 8, 9, dtype=torch.int32, device=DEV)}),
        (t, [1], {"out": torch.zeros(2, 1, 8, 9, dtype=torch.int32)}),
        (t, [1], {"out": torch.zeros(2, 1, 8, 18, dtype=torch.int32, device=DEV)[..., ::2]}),
    ]
    for labels, values, kw in bad:
        with pytest.raises(ValueError):
            ops.distance_transform_sq(labels, values, **kw)


# ---- statistics -------------------------------------------------------------------------------------------
def _stats(pred, gt, **kw):
    from eunet import ops
    out = ops.boundary_stats(torch.from_numpy(np.ascontiguousarray(pred)).to(DEV),
                             torch.from_numpy(np.ascontiguousarray(gt)).to(DEV), **kw)
    assert all(t.dtype == torch.int64 and t.is_cuda for t in out)
    return tuple(t.cpu() for t in out)


def _check_stats(pred, gt, k=3, cap=64, radii=(2,), ignore_index=255):
    got = _stats(pred, gt, num_classes=k, cap=cap, band_radii=radii, ignore_index=ignore_index)
    ref = R.boundary_stats(pred, gt, k=k, cap=cap, radii=radii, ignore_index=ignore_index)
    for name, a, b in zip(("surf", "band", "refrows"), got, ref):
        assert tuple(a.shape) == b.shape, name
        assert torch.equal(a, torch.from_numpy(b)), name
    return got


def _pair(rng, h, w, ignored=False):
    """A ground truth of discs and a prediction that is its shifted, speckled copy (with stray labels)."""
    gt = _discs(rng, h, w) if min(h, w) > 4 else rng.integers(0, 3, (h, w)).astype(np.int64)
    pred = np.roll(gt, (int(rng.integers(-2, 3)), int(rng.integers(-2, 3))), axis=(0, 1))
    speck = rng.random((h, w)) < 0.03
    pred[speck] = rng.choice(VALUES, size=int(speck.sum()))
    if ignored:
        gt[h // 4:h // 2 + 1, w // 3:2 * w // 3 + 1] = 255
    return pred, gt


@pytest.mark.parametrize("shape", [(1, 1), (3, 3), (5, 64), (61, 67), (130, 259)])
@pytest.mark.parametrize("ignored", [False, True])
def test_statistics_shapes_and_classes(shape, ignored):
    rng = np.random.default_rng(shape[0] * 131 + shape[1] + int(ignored))
    pred, gt = _pair(rng, *shape, ignored=ignored)
    k = {(1, 1): 1, (3, 3): 2}.get(shape, 3)
    got = _check_stats(pred, gt, k=k, cap=64, radii=(0, 1, 2, 5))
    if shape == (130, 259):
        assert int(got[0][:, :, :64 * 64 + 3].sum()) > 1000
        for kk in (1, 2):
            _check_stats(pred, gt, k=kk, cap=64, radii=(2,))


@pytest.mark.parametrize("ignored", [False, True])
def test_a_small_cap_uses_the_overflow_bin_and_the_maximum(ignored):
    rng = np.random.default_rng(11 + int(ignored))
    gt = _discs(rng, 61, 67, n=5)
    pred = _discs(rng, 61, 67, n=5)  # unrelated masks: many distances beyond 3 pixels
    if ignored:
        gt[10:30, 20:50] = 255
    surf, _, _ = _check_stats(pred, gt, cap=3, radii=())
    assert tuple(surf.shape) == (3, 2, 14)
    assert int(surf[:, :, 10].sum()) > 0 and int(surf[:, :, 12].max()) > 9


def test_a_class_absent_from_pred_from_gt_and_from_both():
    rng = np.random.default_rng(12)
    gt = _discs(rng, 40, 70, classes=(1,))
    pred = _discs(rng, 40, 70, classes=(2,))
    surf, band, _ = _check_stats(pred, gt, cap=64, radii=(0, 2))
    c2 = 64 * 64
    assert int(surf[1, 0].sum()) == 0 and int(surf[1, 1, c2 + 2]) == int(surf[1, 1].sum()) > 0  # live: gt only
    assert int(surf[2, 1].sum()) == 0 and int(surf[2, 0, c2 + 2]) == int(surf[2, 0].sum()) > 0  # dead: pred only
    zeros = np.zeros((40, 70), np.int64)
    surf, band, refrows = _check_stats(zeros, zeros)
    assert int(surf[1:].sum()) == 0 and int(band[1:].sum()) == 0 and int(refrows[:, 1:].sum()) == 0


def test_identical_maps_put_every_edge_pixel_in_bin_zero():
    """pred == gt at 130 x 259: whole waves add to one address, in both directions."""
    rng = np.random.default_rng(13)
    gt = _discs(rng, 130, 259, n=12)
    surf, band, refrows = _check_stats(gt, gt, cap=64, radii=(0, 2))
    for c in range(3):
        n_edge = int(R.edges(R.region(gt, c)).sum())
        assert n_edge > 0 and surf[c, :, 0].tolist() == [n_edge, n_edge]
        assert int(surf[c, :, 1:].sum()) == 0
        assert band[c, 0].tolist() == [n_edge] * 3
    # every pixel an edge pixel of its class: a checkerboard
    yy, xx = np.mgrid[0:130, 0:259]
    board = ((yy + xx) % 2).astype(np.int64)
    surf, _, _ = _check_stats(board, board, k=2)
    assert int(surf[:, :, 0].sum()) == 2 * 130 * 259


def test_accumulation_through_out():
    from eunet import ops
    rng = np.random.default_rng(14)
    a = _pair(rng, 61, 67, ignored=True)
    b = (_discs(rng, 61, 67, n=3), _discs(rng, 61, 67, n=3))  # farther apart: a larger maximum
    kw = dict(num_classes=3, cap=5, band_radii=(1, 3))
    sa, sb = _stats(*a, **kw), _stats(*b, **kw)
    for first, second in ((a, b), (b, a)):
        out = ops.boundary_stats(torch.from_numpy(first[0]).to(DEV), torch.from_numpy(first[1]).to(DEV), **kw)
        back = ops.boundary_stats(torch.from_numpy(second[0]).to(DEV), torch.from_numpy(second[1]).to(DEV), out=out, **kw)
        assert all(x is y for x, y in zip(out, back))
        assert torch.equal(out[0].cpu(), torch.from_numpy(R.combine(sa[0].numpy(), sb[0].numpy(), 5)))
        assert torch.equal(out[1].cpu(), sa[1] + sb[1])
        assert torch.equal(out[2].cpu(), sa[2] + sb[2])  # one image slot, added to
    # a batch of two is the two images pooled, with their own reference rows
    both = _stats(np.stack([a[0], b[0]]), np.stack([a[1], b[1]]), **kw)
    assert torch.equal(both[0], torch.from_numpy(R.combine(sa[0].numpy(), sb[0].numpy(), 5)))
    assert torch.equal(both[1], sa[1] + sb[1]) and torch.equal(both[2], torch.cat([sa[2], sb[2]]))


def test_the_ignore_rule_applies_to_the_statistics_and_not_to_the_reference_rows():
    """A predicted live block under 255-pixels of the ground truth: surf and band of live see no pred edge there,
    the reference rows count the block as it is."""
    gt = np.zeros((40, 70), np.int64)
    gt[5:30, 10:50] = 255
    gt[32:38, 55:65] = 1
    pred = np.zeros((40, 70), np.int64)
    pred[8:25, 15:40] = 1
    surf, band, refrows = _check_stats(pred, gt, cap=64, radii=(0, 2))
    assert int(surf[1, 0].sum()) == 0 and int(band[1, :, 0].sum()) == 0  # no pred edge, no pred band
    assert int(surf[1, 1, 64 * 64 + 2]) == 2 * 6 + 2 * 10 - 4  # the gt block's outline has no counterpart
    assert refrows[0, 1, 1, 0] == (17 - 4) * (25 - 4) and refrows[0, 1, 0, 0] > 0
    # without the rule (another ignore value) the block is back
    surf2, _, refrows2 = _check_stats(pred, gt, cap=64, radii=(0, 2), ignore_index=-100)
    assert int(surf2[1, 0, :64 * 64 + 3].sum()) == 2 * 17 + 2 * 25 - 4 and torch.equal(refrows2, refrows)


def test_statistics_refusals():
    from eunet import ops
    t = torch.zeros(8, 9, dtype=torch.int64, device=DEV)
    ok = ops.boundary_stats(t, t, cap=2)
    bad = [
        dict(pred=t.int()), dict(gt=t.cpu()), dict(gt=t[:, :8]), dict(pred=t[::2], gt=t[::2]),
        dict(num_classes=0), dict(num_classes=4), dict(cap=0), dict(cap=65), dict(ignore_index=2 ** 31),
        dict(band_radii=(-1,)), dict(band_radii=tuple(range(9))), dict(band_radii=(1.5,)),
        dict(cap=2, out=(ok[0], ok[1])), dict(cap=3, out=ok), dict(cap=2, band_radii=(1, 2), out=ok),
        dict(cap=2, out=(ok[0], ok[1], ok[2].int())), dict(cap=2, out=(ok[0].cpu(), ok[1], ok[2])),
    ]
    for kw in bad:
        args = dict(pred=t, gt=t)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.boundary_stats(args.pop("pred"), args.pop("gt"), **args)
    assert int(ok[0].sum()) == 2 * 30  # nothing was added by the refused calls: the 30 border pixels, both ways


def test_calculate_boundary_stats_accumulates_and_takes_numpy():
    from eunet import metrics as M
    rng = np.random.default_rng(15)
    a, b = _pair(rng, 33, 47, ignored=True), _pair(rng, 50, 41)
    acc = M.calculate_boundary_stats(a[0], a[1], cap=8, band_radii=(0, 2))
    same = M.calculate_boundary_stats(torch.from_numpy(b[0]).to(DEV), torch.from_numpy(b[1]), cap=8,
                                      band_radii=(0, 2), out=acc)
    assert same is acc and tuple(acc["refrows"].shape) == (2, 3, 2, 3)
    ra, rb = (R.boundary_stats(p, g, cap=8, radii=(0, 2)) for p, g in (a, b))
    assert torch.equal(acc["surf"].cpu(), torch.from_numpy(R.combine(ra[0], rb[0], 8)))
    assert torch.equal(acc["band"].cpu(), torch.from_numpy(ra[1] + rb[1]))
    assert torch.equal(acc["refrows"].cpu(), torch.from_numpy(np.concatenate([ra[2], rb[2]])))
    with pytest.raises(ValueError):
        M.calculate_boundary_stats(a[0], a[1], cap=9, band_radii=(0, 2), out=acc)
    m = M.boundary_metrics_from_stats(acc)
    assert m["live"]["n_gt_edge"] > 0 and 0.0 <= m["live"]["nsd"][2] <= 1.0 and len(m["boundary_ious_ref"]) >= 2


# ---- evaluator ----------------------------------------------------------------------------------------------
_MODELS = {}


def _model(K, **kw):
    """A base-16 enhanced_unet (the narrowest the models accept) in eval mode with random weights and non-trivial BatchNorm statistics; built once."""
    key = (K, tuple(sorted(kw.items())))
    if key not in _MODELS:
        from eunet.models import EnhancedUNet
        torch.manual_seed(3)
        m = EnhancedUNet(num_classes=K, in_channels=3, base_ch=16, **kw)
        g = torch.Generator().manual_seed(4)
        for k, v in m.state_dict().items():
            if k.endswith("running_mean"):
                v.copy_(0.1 * torch.randn(v.shape, generator=g))
            elif k.endswith("running_var"):
                v.copy_(0.5 + torch.rand(v.shape, generator=g))
        _MODELS[key] = m.to(DEV).eval()
    return _MODELS[key]


def _loader():
    """Three eunet.synth images (96 x 128, and two sizes that are no multiples of 32), the last mask with an
    ignored rectangle; batches of two and one."""
    from eunet import synth
    images, items = [], []
    for i, (h, w) in enumerate(((96, 128), (90, 130), (100, 120))):
        x, m = synth.tile(h, w, 40 + i, num_classes=3, in_channels=3)
        if i == 2:
            m[10:30, 20:60] = 255
        images.append(torch.from_numpy(x))
        items.append({"semantic_mask": m, "instance_masks": [], "instance_labels": []})
    return [{"images": images[:2], "batch_items": items[:2]}, {"images": images[2:], "batch_items": items[2:]}]


def _expected(ev, loader, k, gt_of):
    from eunet import metrics as M
    acc = None
    for batch in loader:
        for img, item in zip(batch["images"], batch["batch_items"]):
            acc = M.calculate_boundary_stats(ev.predict_semantic_mask(img), gt_of(item["semantic_mask"]), num_classes=k,
                                             cap=16, band_radii=(0, 2), out=acc)
    return acc


@pytest.mark.parametrize("kind", ["softmax", "sigmoid"])
def test_evaluate_boundary_equals_the_sum_over_predicted_masks(kind):
    from eunet import metrics as M
    from eunet.evaluator import Evaluator
    loader = _loader()
    if kind == "softmax":
        ev = Evaluator(_model(3), DEV, "enhanced_unet", preprocess=None)
        k, names, gt_of = 3, ("background", "live", "dead"), lambda m: m
    else:
        ev = Evaluator(_model(1), DEV, "enhanced_unet", preprocess=None, activation="sigmoid")
        k, names, gt_of = 2, ("background", "foreground"), lambda m: np.where(m == 255, 255, (m >= 1).astype(np.int64))
    res = ev.evaluate_boundary(loader, tolerances=(1, 2), band_radii=(0, 2), cap=16)
    want = _expected(ev, loader, k, gt_of)
    for name in ("surf", "band", "refrows"):
        assert isinstance(res[name], np.ndarray) and res[name].dtype == np.int64
        assert np.array_equal(res[name], want[name].cpu().numpy()), name
    assert res["refrows"].shape == (3, k, 2, 3) and res["cap"] == 16 and res["band_radii"] == (0, 2)
    ref = M.boundary_metrics_from_stats(want, tolerances=(1, 2), class_names=names)
    for name in names:
        assert res[name]["n_gt_edge"] > 0
        np.testing.assert_equal(res[name], ref[name])  # nan equals nan here
    assert res["boundary_ious_ref"] == ref["boundary_ious_ref"] and len(res["interior_ious_ref"]) >= 3
    with pytest.raises(ValueError):
        ev.evaluate_boundary([])


def test_evaluate_boundary_on_the_dual_branch_model_follows_predict_semantic_mask():
    from eunet.evaluator import Evaluator
    ev = Evaluator(_model(3, dual_branch=True), DEV, "enhanced_unet", preprocess=None)
    loader = _loader()[1:]
    try:
        ev.predict_semantic_mask(loader[0]["images"][0])
    except Exception as e:  # whatever predict_semantic_mask raises, evaluate_boundary raises too
        with pytest.raises(type(e)):
            ev.evaluate_boundary(loader)
        return
    res = ev.evaluate_boundary(loader, band_radii=(0, 2), cap=16)
    want = _expected(ev, loader, 3, lambda m: m)
    for name in ("surf", "band", "refrows"):
        assert np.array_equal(res[name], want[name].cpu().numpy()), name
