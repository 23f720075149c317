"""CellDataset(weight_map=...) and a training loop on the pixel-weighted losses.

The LabelMe fixture (written into tmp_path, as tests/test_gpu_data.py does) is 96x128, so the polygons are not
rescaled: rectangles A (live) and B (dead) are 3 px apart (columns 41..43 are background between them),
C (live) and D (dead) share the edge x = 50 and abut, E (live) lies alone in a corner.

The training cases: enhanced_unet, base 16, 3 channels, 32x32, batch 2, fp32, five eager AdamW steps on one
batch through forward_lowres -- no Trainer, no graph capture.  The first step's logit gradient is held to the
restatement of tests/_wmap_ref.py by the project's loss gates (1e-4 of the largest, 1e-3 per element).
"""
import json
import random

import numpy as np
import pytest
import torch

import _wmap_ref as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W = 96, 128
SHAPES = [{"label": "live", "points": [[10, 10], [40, 10], [40, 40], [10, 40]]},   # A: x 10..40
          {"label": "dead", "points": [[44, 10], [70, 10], [70, 40], [44, 40]]},   # B: x 44..70, 3 px from A
          {"label": "live", "points": [[20, 60], [50, 60], [50, 90], [20, 90]]},   # C
          {"label": "dead", "points": [[50, 60], [80, 60], [80, 90], [50, 90]]},   # D: shares x = 50 with C
          {"label": "live", "points": [[100, 5], [120, 5], [120, 20], [100, 20]]}]  # E
CFG = dict(w0=10.0, sigma=3.0, class_weight=(1.0, 3.0, 2.0))


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
        return torch.equal(a, b)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    return a == b


def test_items_without_the_option_are_unchanged_and_the_option_draws_nothing(tmp_path):
    """weight_map=None: the item's keys are today's; with the option every one of those keys has the same value,
    and random / np.random are left in the same state: the feature draws nothing."""
    from eunet.data import CellDataset
    _write(tmp_path)
    plain = CellDataset(str(tmp_path), split="train", device=DEV)
    withmap = CellDataset(str(tmp_path), split="train", device=DEV, weight_map=dict(CFG))
    keys = {"image", "instance_masks", "instance_labels", "bboxes", "semantic_mask", "image_id", "original_size"}
    for seed in range(4):
        a, ra, na = _item(plain, seed, idx=seed)
        b, rb, nb = _item(withmap, seed, idx=seed)
        assert set(a) == keys and set(b) == keys | {"weight_map", "instance_label_map"}
        for k in keys:
            assert _same(a[k], b[k]), (seed, k)
        assert ra == rb
        assert na[0] == nb[0] and np.array_equal(na[1], nb[1]) and na[2:] == nb[2:]


def test_weight_map_equals_the_restatement_and_follows_the_flips(tmp_path):
    from eunet import ops
    from eunet.data import CellDataset, load_labelme
    _write(tmp_path)
    ds = CellDataset(str(tmp_path), split="train", device=DEV, weight_map=dict(CFG))
    polys, labels, _ = load_labelme(str(tmp_path / "w00.json"), 1.0, 1.0)
    direct = ops.rasterize_polygons(polys, list(range(1, len(polys) + 1)), H, W, DEV)
    assert set(torch.unique(direct).tolist()) == {0, 1, 2, 3, 4, 5}
    seen = set()
    for seed in range(8):
        r = random.Random(seed)
        flips = (r.random() > 0.5, r.random() > 0.5)  # the dataset's first two draws
        seen.add(flips)
        item, _, _ = _item(ds, seed)
        inst, wm = item["instance_label_map"], item["weight_map"]
        assert inst.dtype == torch.int64 and inst.shape == (H, W) and wm.dtype == torch.float32 and wm.shape == (H, W)
        want = direct
        if flips[0]:
            want = want.flip(1)
        if flips[1]:
            want = want.flip(0)
        assert torch.equal(inst, want), (seed, flips)
        # instance ids and the semantic mask describe the same cells
        assert torch.equal(inst > 0, item["semantic_mask"] > 0)
        ref, a = M.border_weight_map(inst.cpu().numpy(), item["semantic_mask"].cpu().numpy(), CFG["class_weight"],
                                     CFG["w0"], CFG["sigma"], "default")
        err = np.abs(wm.double().cpu().numpy() - ref)
        bound = 16 * 2.0 ** -23 * (1 + a) * ref + 2.0 ** -23 * CFG["w0"]
        assert float((err / bound).max()) <= 1.0, (seed, float((err / bound).max()))
        # the background pixels just above and below the shared edge of C and D: d1 = 1, d2 = sqrt(2)
        peak = 1.0 + CFG["w0"] * np.exp(-(1 + np.sqrt(2.0)) ** 2 / (2 * CFG["sigma"] ** 2))
        assert abs(float(wm.max()) - peak) <= 1e-5 * peak
        # the 3 px between A and B, in the unflipped frame: d1 + d2 = 4 on every one of them
        u = wm.flip(1) if flips[0] else wm
        u = (u.flip(0) if flips[1] else u)[10:41, 41:44].double().cpu()
        gap = 1.0 + CFG["w0"] * np.exp(-16.0 / (2 * CFG["sigma"] ** 2))
        assert float((u - gap).abs().max()) <= 1e-5 * gap
    assert len(seen) >= 3 and any(f[0] for f in seen) and any(f[1] for f in seen), seen


def test_separate_opens_the_contact_and_the_map_peaks_there(tmp_path):
    from eunet.data import CellDataset
    _write(tmp_path)
    cfg = dict(CFG, separate=True)
    val = CellDataset(str(tmp_path), split="val", device=DEV, weight_map=cfg)[0]
    plain = CellDataset(str(tmp_path), split="val", device=DEV)[0]
    torch.cuda.synchronize()
    sem, sem0, inst, wm = (t.cpu().numpy() for t in (val["semantic_mask"], plain["semantic_mask"],
                                                     val["instance_label_map"], val["weight_map"]))
    # unseparated: C ends at column 49 and D starts at 50; separated: both lose their contact column
    assert (sem0[62:89, 49] == 1).all() and (sem0[62:89, 50] == 2).all()
    assert (sem[62:89, 49] == 0).all() and (sem[62:89, 50] == 0).all() and (inst[62:89, 49:51] == 0).all()
    assert (sem[62:89, 48] == 1).all() and (sem[62:89, 51] == 2).all()
    # everything else is as before: A, B and E touch nothing
    changed = sem != sem0
    assert changed[:, 49:51].sum() == changed.sum() > 0
    lo, so = M.separate(_instances(tmp_path), sem0)
    assert np.array_equal(inst, lo) and np.array_equal(sem, so)
    # the opened contact (2 px wide: d1 = 1, d2 = 2) is the narrowest gap of the image: the map peaks there
    peak = 1.0 + CFG["w0"] * np.exp(-9.0 / (2 * CFG["sigma"] ** 2))
    assert abs(float(wm.max()) - peak) <= 1e-5 * peak
    ys, xs = np.nonzero(wm == wm.max())
    assert set(xs.tolist()) <= {49, 50} and ys.min() >= 60 and ys.max() <= 90


def _instances(tmp_path):
    from eunet import ops
    from eunet.data import load_labelme
    polys, _, _ = load_labelme(str(tmp_path / "w00.json"), 1.0, 1.0)
    return ops.rasterize_polygons(polys, list(range(1, len(polys) + 1)), H, W, DEV).cpu().numpy()


# ---- a training loop on the weighted losses ------------------------------------------------------------
def _grad_close(name, got, ref):
    scale = float(ref.abs().max())
    assert scale > 0.0 and bool(torch.isfinite(got).all()), name
    err = (got - ref).abs()
    mx = float(err.max()) / scale
    per = float((err / ref.abs().clamp_min(1e-3 * scale)).max())
    print(f"{name}: logit gradient err / max {mx:.2e}, worst element {per:.2e}")
    assert mx <= 1e-4, (name, mx)
    assert per <= 1e-3, (name, per)


def _batch():
    from eunet import ops
    g = torch.Generator().manual_seed(300)
    x = torch.rand(2, 3, 32, 32, generator=g)
    inst = torch.zeros(2, 32, 32, dtype=torch.int64)
    inst[0, 4:14, 3:12], inst[0, 4:14, 14:24], inst[0, 18:28, 8:20] = 1, 2, 3
    inst[1, 2:12, 2:30], inst[1, 14:30, 5:15], inst[1, 14:30, 17:27] = 70000, 5, 6
    sem = torch.where(inst == 0, 0, 1 + inst % 2)
    inst, sem = inst.to(DEV), sem.to(DEV)
    wm = ops.border_weight_map(inst, sem, class_weight=(1.0, 3.0, 2.0), sigma=2.0)
    assert float(wm.max()) > 3.0  # the 2 px gap of sample 0: 1 + 10 exp(-9 / 8) = 4.25
    return x.to(DEV), sem, wm


@pytest.mark.parametrize("kind", ["combined", "bce"])
def test_five_eager_steps_on_a_weighted_loss(kind):
    from eunet.losses import bce_dice_loss, combined_loss
    from eunet.models import EnhancedUNet
    x, sem, wm = _batch()
    torch.manual_seed(3)
    K = 3 if kind == "combined" else 1
    model = EnhancedUNet(num_classes=K, in_channels=3, base_ch=16).to(DEV).train()
    opt = torch.optim.AdamW(model.parameters(), lr=4e-3)
    fn = combined_loss if kind == "combined" else bce_dice_loss
    losses = []
    for step in range(5):
        opt.zero_grad(set_to_none=True)
        logits = model.forward_lowres(x)
        if step == 0:
            logits.retain_grad()
        loss = fn(logits, sem, pixel_weight=wm)
        loss.backward()
        if step == 0:
            ref = (M.combined_w if kind == "combined" else M.bce_dice_w)(logits.detach().float(), sem, wm.cpu())
            tol = 1e-5 * abs(ref[0])
            assert abs(loss.item() - ref[0]) <= tol, (loss.item(), ref[0])
            _grad_close(kind, logits.grad.double().cpu(), ref[2])
            assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None)
        opt.step()
        losses.append(loss.item())
    print(kind, "losses", losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
