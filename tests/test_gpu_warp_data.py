"""CellDataset(elastic=...): the geometric stage in front of the photometric augmentations.

The LabelMe fixture is the 96 x 128 one of tests/test_gpu_wmap_data.py (written into tmp_path; the polygons are
not rescaled).  The option draws from a generator of its own, so a plain dataset under the same `random` /
`np.random` seeds takes the same flips and the same photometric decisions: the warped labels are then the
restatement (tests/_warp_ref.py) applied to the plain item's labels, unflipped, through the item's own map."""
import json
import random

import numpy as np
import pytest
import torch

import _warp_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W = 96, 128
SHAPES = [{"label": "live", "points": [[10, 10], [40, 10], [40, 40], [10, 40]]},
          {"label": "dead", "points": [[44, 10], [70, 10], [70, 40], [44, 40]]},
          {"label": "live", "points": [[20, 60], [50, 60], [50, 90], [20, 90]]},
          {"label": "dead", "points": [[50, 60], [80, 60], [80, 90], [50, 90]]},
          {"label": "live", "points": [[100, 5], [120, 5], [120, 20], [100, 20]]}]
REAL = dict(sigma=6.0, grid=3, rotate=20.0, scale=(0.8, 1.2))
WMAP = dict(w0=10.0, sigma=3.0, class_weight=(1.0, 3.0, 2.0))
PLAIN_KEYS = {"image", "instance_masks", "instance_labels", "bboxes", "semantic_mask", "image_id", "original_size"}


def _write(tmp_path, n=10):
    from PIL import Image
    rng = np.random.default_rng(3)
    for i in range(n):
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(tmp_path / f"w{i:02d}.jpg", quality=95)
        (tmp_path / f"w{i:02d}.json").write_text(json.dumps({"shapes": SHAPES}))


def _item(ds, seed, idx=0):
    random.seed(seed)
    np.random.seed(seed)
    item = ds[idx]
    torch.cuda.synchronize()
    return item, random.getstate(), np.random.get_state()


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and torch.equal(a, b)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    return a == b


def _same_np_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _flips(seed):
    r = random.Random(seed)
    return r.random() > 0.5, r.random() > 0.5  # the dataset's first two draws


def _unflip(t, flips):
    """The flips of _augment undone (horizontal was applied first; the two commute) on the last two axes."""
    dims = [d for d, f in ((-1, flips[0]), (-2, flips[1])) if f]
    return t.flip(dims) if dims else t


def _ds(tmp_path, **kw):
    from eunet.data import CellDataset
    return CellDataset(str(tmp_path), split=kw.pop("split", "train"), device=DEV, **kw)


def test_degenerate_option_gives_the_plain_item_and_leaves_the_global_streams(tmp_path):
    """sigma 0, no rotation, scale 1: the map is the identity, so every key of the plain item is bit-equal, and
    `random` / `np.random` end in the plain run's states: the option draws from its own generator only."""
    _write(tmp_path)
    plain = _ds(tmp_path)
    ident = _ds(tmp_path, elastic=dict(sigma=0, rotate=0, scale=(1, 1), seed=1))
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    for seed in range(4):
        a, ra, na = _item(plain, seed, idx=seed)
        b, rb, nb = _item(ident, seed, idx=seed)
        assert set(a) == PLAIN_KEYS and set(b) == PLAIN_KEYS | {"warp_grid"}
        for k in PLAIN_KEYS:
            assert _same(a[k], b[k]), (seed, k)
        assert b["warp_grid"].dtype == torch.float32 and b["warp_grid"].shape == (H, W, 2)
        assert torch.equal(b["warp_grid"].cpu(), torch.stack([x, y], -1).float())
        assert ra == rb and _same_np_state(na, nb)


def test_labels_follow_the_items_own_map_and_the_flips(tmp_path):
    from eunet import ops
    _write(tmp_path)
    plain = _ds(tmp_path, weight_map=dict(WMAP))
    warped = _ds(tmp_path, weight_map=dict(WMAP), elastic=dict(REAL, seed=11))
    seen, moved = set(), 0
    for seed in range(4):
        a, ra, na = _item(plain, seed, idx=seed)
        b, rb, nb = _item(warped, seed, idx=seed)
        assert ra == rb and _same_np_state(na, nb)  # so the flips and the photometric decisions are the plain run's
        flips = _flips(seed)
        seen.add(flips)
        g = b["warp_grid"].cpu().numpy()
        assert g.dtype == np.float32 and g.shape == (H, W, 2)

        def expect(t):  # flip(warp(unflip(plain)))
            src = _unflip(t, flips).cpu().numpy()
            return torch.from_numpy(R.warp_labels_ref(src, g, "reflect", 0, flip_h=flips[0], flip_v=flips[1]))
        assert torch.equal(b["semantic_mask"].cpu(), expect(a["semantic_mask"])), seed
        assert torch.equal(b["instance_label_map"].cpu(), expect(a["instance_label_map"])), seed
        assert len(b["instance_masks"]) == len(a["instance_masks"]) == len(SHAPES)
        for i, (ma, mb) in enumerate(zip(a["instance_masks"], b["instance_masks"])):
            assert mb.dtype == torch.uint8 and torch.equal(mb.cpu(), expect(ma[None])[0]), (seed, i)
        moved += int((b["semantic_mask"] != a["semantic_mask"]).sum())
        # the weight map is computed from the warped ids, never interpolated
        wm = ops.border_weight_map(b["instance_label_map"], b["semantic_mask"], class_weight=WMAP["class_weight"],
                                   w0=WMAP["w0"], sigma=WMAP["sigma"])
        assert torch.equal(b["weight_map"], wm), seed
        assert b["bboxes"] == a["bboxes"] and b["instance_labels"] == a["instance_labels"]
    assert len(seen) >= 2 and moved > 100, (seen, moved)


def _all_off_seed():
    """The first seed under which _augment's ten decisions are all 'off' (both flips, brightness, contrast,
    saturation, CLAHE, noise, gamma, sharpen, HSV jitter), so the item's image is the geometric stage's output."""
    limits = (0.5, 0.5, 0.3, 0.3, 0.5, 0.4, 0.5, 0.5, 0.6, 0.6)
    for seed in range(200000):
        r = random.Random(seed)
        if all(r.random() <= lim for lim in limits):
            return seed
    raise AssertionError("no seed switches every photometric augmentation off")


def test_image_before_the_photometric_stage_is_the_bilinear_restatement(tmp_path):
    _write(tmp_path)
    seed = _all_off_seed()
    a, ra, _ = _item(_ds(tmp_path), seed)
    b, rb, _ = _item(_ds(tmp_path, elastic=dict(REAL, seed=5)), seed)
    assert ra == rb
    r = random.Random(seed)
    for _ in range(10):
        r.random()
    assert r.getstate() == ra  # exactly the ten decisions were drawn: nothing photometric ran

    def u8(t):  # to_tensor is c / 255 in fp32: times 255 and rounded gives the byte back
        return (t * 255.0).round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).cpu().numpy()
    want = R.warp_u8_ref(u8(a["image"]), b["warp_grid"].cpu().numpy(), "reflect", 0)
    assert np.array_equal(u8(b["image"]), want)
    assert (u8(b["image"]) != u8(a["image"])).mean() > 0.5
    # the stage itself, as the dataset exposes it, under the constant border too
    ds = _ds(tmp_path, elastic=dict(REAL, seed=5, border="constant"))
    img = torch.from_numpy(u8(a["image"])).to(DEV)
    wi, wm = ds._warp(img, a["semantic_mask"], b["warp_grid"])
    assert np.array_equal(wi.cpu().numpy(), R.warp_u8_ref(u8(a["image"]), b["warp_grid"].cpu().numpy(), "constant", 0))
    assert np.array_equal(wm.cpu().numpy(), R.warp_labels_ref(a["semantic_mask"].cpu().numpy(), b["warp_grid"].cpu().numpy(),
                                                               "constant", 0))


def test_seeded_map_sequence_repeats_and_items_differ(tmp_path):
    _write(tmp_path)

    def grids(seed):
        ds = _ds(tmp_path, elastic=dict(REAL, seed=seed))
        return [_item(ds, 0, idx=i % len(ds))[0]["warp_grid"].cpu() for i in range(4)]
    g1, g2, g3 = grids(21), grids(21), grids(22)
    assert all(torch.equal(u, v) for u, v in zip(g1, g2))
    assert not any(torch.equal(g1[i], g1[j]) for i in range(4) for j in range(i))
    assert not torch.equal(g1[0], g3[0])
    # the draws are the documented ones, in order: u, angle, scale, control displacements
    from eunet import ops
    from eunet.data import warp_matrix
    rng = np.random.Generator(np.random.PCG64(21))
    for got in g1:
        assert rng.random() < 1.0
        angle, s = rng.uniform(-20.0, 20.0), rng.uniform(0.8, 1.2)
        ctrl = rng.normal(0.0, 6.0, (2, 3, 3))
        assert torch.equal(got, ops.elastic_grid(H, W, ctrl, warp_matrix(H, W, angle, s), device=DEV).cpu())


def test_p_zero_and_other_splits_carry_no_map(tmp_path):
    _write(tmp_path, n=20)
    plain = _ds(tmp_path)
    never = _ds(tmp_path, elastic=dict(REAL, p=0.0, seed=2))
    for seed in range(3):
        a, ra, na = _item(plain, seed, idx=seed)
        b, rb, nb = _item(never, seed, idx=seed)
        assert b["warp_grid"] is None and set(b) == PLAIN_KEYS | {"warp_grid"}
        for k in PLAIN_KEYS:
            assert _same(a[k], b[k]), (seed, k)
        assert ra == rb and _same_np_state(na, nb)
    # p between 0 and 1 skips the items whose first draw is >= p, and only those
    half = _ds(tmp_path, elastic=dict(REAL, p=0.5, seed=9))
    rng = np.random.Generator(np.random.PCG64(9))
    got, want = [], []
    for i in range(6):
        got.append(_item(half, 0, idx=i)[0]["warp_grid"] is not None)
        u = rng.random()
        want.append(bool(u < 0.5))
        if u < 0.5:
            rng.uniform(-20.0, 20.0), rng.uniform(0.8, 1.2), rng.normal(0.0, 6.0, (2, 3, 3))
    assert got == want and True in got and False in got, (got, want)
    for split in ("val", "test"):
        ds = _ds(tmp_path, split=split, elastic=dict(REAL, seed=2))
        ref = _ds(tmp_path, split=split)
        assert len(ds) >= 1
        item, base = _item(ds, 0)[0], _item(ref, 0)[0]
        assert item["warp_grid"] is None
        for k in PLAIN_KEYS:
            assert _same(item[k], base[k]), (split, k)
