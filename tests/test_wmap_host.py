"""Host side of the border weight map and the pixel-weighted losses: the fp64 restatements the GPU tests
compare with (tests/_wmap_ref.py) against tests/_bce_ref.py, the oracle, torch's own losses and scipy, the
truncation bound of include/eunet.h, and the Python layer's refusals.  None of it needs a GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _bce_ref as B
import _wmap_ref as M
from oracle import eunet_ref as R

G = 3.7
IGN = 255


def _inputs(N, K, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(N, K, H, W, generator=g, dtype=torch.float64) * 2).float()
    t = torch.randint(0, 3 if K == 1 else K, (N, H, W), generator=g)
    m = torch.rand(N, H, W, generator=g, dtype=torch.float64) * 12
    m.view(-1)[::5] = 0.0
    return x, t, m


def five_discs():
    """37x45 with five discs: ids 3, 70000, 7, 3 again (a second place of the same instance) and 12."""
    lab = np.zeros((37, 45), np.int64)
    yy, xx = np.mgrid[0:37, 0:45]
    for (cy, cx, r, i) in [(8, 8, 4, 3), (9, 17, 3, 70000), (25, 12, 5, 7), (28, 36, 4, 3), (12, 38, 3, 12)]:
        lab[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = i
    return lab


@pytest.mark.parametrize("K", [1, 2, 3])
def test_weighted_bce_at_weight_one_is_the_unweighted_restatement(K):
    x, t, _ = _inputs(3, K, 9, 11, seed=3 + K)
    t.view(-1)[::7] = IGN
    s = B.spec(pos_weight=(1.5, 3.0, 0.5), class_weight=(2.0, 1.0, 3.0), dice_weight=(1.0, 15.0, 8.0), w_bce=0.7,
               w_dice=1.3, ignore_index=IGN)
    v0, p0, g0 = B.bce_dice(x, t, g=G, **s)
    v1, p1, g1 = M.bce_dice_w(x, t, torch.ones(3, 9, 11), g=G, **s)
    assert abs(v0 - v1) <= 1e-12 * max(1.0, abs(v0))
    assert float((p0 - p1).abs().max()) <= 1e-12
    assert float((g0 - g1).abs().max()) <= 1e-12


@pytest.mark.parametrize("K", [2, 3])
def test_weighted_combined_at_weight_one_is_the_oracle(K):
    x, t, _ = _inputs(3, K, 9, 11, seed=13 + K)
    xd = x.double().clone().requires_grad_(True)
    tot, parts = xd.new_zeros(()), []
    for n in range(3):
        v, p = R.combined_loss(xd[n], t[n], parts=True)
        tot = tot + v / 3
        parts.append([p["focal"].item(), p["dice"].item(), p["tversky"].item()])
    (tot * G).backward()
    v1, p1, g1 = M.combined_w(x, t, torch.ones(3, 9, 11), g=G)
    assert abs(tot.item() - v1) <= 1e-12 * max(1.0, abs(v1))
    assert float((torch.tensor(parts, dtype=torch.float64) - p1).abs().max()) <= 1e-12
    assert float((xd.grad - g1).abs().max()) <= 1e-12


@pytest.mark.parametrize("K", [1, 3])
def test_weighted_bce_equals_torch_bce_with_weight(K):
    """BCE part: F.binary_cross_entropy_with_logits(weight = m cw, pos_weight) summed over the valid pixels over
    K V; Dice part: the unweighted restatement's (w_bce = 0).  Value and gradient, the latter by autograd."""
    x, t, m = _inputs(3, K, 9, 11, seed=23 + K)
    t.view(-1)[::7] = IGN
    m[t == IGN] = 1e30  # an ignored pixel's weight counts nowhere
    s = B.spec(pos_weight=(1.5, 3.0, 0.5), class_weight=(2.0, 1.0, 3.0), dice_weight=(1.0, 15.0, 8.0), w_bce=0.7,
               w_dice=1.3, ignore_index=IGN)
    xd = x.double().clone().requires_grad_(True)
    tt, valid, _ = B.targets(t, K, IGN, None)
    pw = torch.tensor(s["pos_weight"][:K], dtype=torch.float64)
    cw = torch.tensor(s["class_weight"][:K], dtype=torch.float64)
    xs, ts = xd.movedim(1, -1)[valid], tt.movedim(1, -1)[valid]
    wt = m[valid][:, None] * cw[None, :]
    bce = F.binary_cross_entropy_with_logits(xs, ts, weight=wt, pos_weight=pw, reduction="sum") / (K * int(valid.sum()))
    (bce * s["w_bce"] * G).backward()
    dice_spec = dict(s, w_bce=0.0)
    vd, _, gd = B.bce_dice(x, t, g=G, **dice_spec)
    v, parts, grad = M.bce_dice_w(x, t, m, g=G, **s)
    v_ref = s["w_bce"] * bce.item() + vd
    assert abs(v - v_ref) <= 1e-12 * max(1.0, abs(v_ref)), (v, v_ref)
    assert float((grad - (xd.grad + gd)).abs().max()) <= 1e-12
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(parts).all())


@pytest.mark.parametrize("K", [2, 3])
def test_weighted_combined_equals_autograd_focal_from_cross_entropy(K):
    """Focal part: built from F.cross_entropy(reduction="none", weight, ignore_index), multiplied by m and
    divided by N H W; Dice and Tversky: the oracle's batched functions.  Gradient by autograd."""
    x, t, m = _inputs(3, K, 9, 11, seed=33 + K)
    t.view(-1)[::7] = IGN
    m[t == IGN] = 1e30
    sp = M.combined_spec(ignore_index=IGN, gamma=2.0, w_focal=1.7, w_dice=0.9, w_tversky=0.4, class_div=float(K),
                         dice_weight=R.DICE_W[:K] + (0.0,) * (3 - K), tversky_weight=R.TVERSKY_W[:K] + (0.0,) * (3 - K))
    xd = x.double().clone().requires_grad_(True)
    w = torch.tensor(sp["ce_weight"][:K], dtype=torch.float64)
    ce = F.cross_entropy(xd, t, weight=w, ignore_index=IGN, reduction="none")
    al = torch.zeros_like(ce)
    for c in range(K):
        al[t == c] = sp["alpha"][c]
    mz = torch.where(t == IGN, torch.zeros_like(m), m)
    focal = (mz * al * (1 - torch.exp(-ce)) ** sp["gamma"] * ce).sum() / ce.numel()
    tot = sp["w_focal"] * focal
    for n in range(3):
        tot = tot + (sp["w_dice"] * R.dice_loss(xd[n:n + 1], t[n:n + 1], K) +
                     sp["w_tversky"] * R.tversky_loss(xd[n:n + 1], t[n:n + 1], K, sp["tversky_alpha"])) / 3
    (tot * G).backward()
    v, parts, grad = M.combined_w(x, t, m, g=G, **sp)
    assert abs(v - tot.item()) <= 1e-12 * max(1.0, abs(v)), (v, tot.item())
    assert float((grad - xd.grad).abs().max()) <= 1e-12
    assert bool(torch.isfinite(parts).all())


def test_truncation_bound_on_five_discs():
    """Where the truncated (R = 11) and the untruncated map differ, a distance beyond R is involved, so both
    border terms are below w0 exp(-R^2 / (2 sigma^2)) = 2.7e-6 here."""
    lab = five_discs()
    assert set(np.unique(lab)) == {0, 3, 7, 12, 70000}
    w0, sigma, Rr = 10.0, 2.0, 11
    mt, _ = M.border_weight_map(lab, None, w0=w0, sigma=sigma, radius=Rr)
    mu, _ = M.border_weight_map(lab, None, w0=w0, sigma=sigma, radius=None)
    bound = w0 * np.exp(-Rr * Rr / (2 * sigma * sigma))
    diff = float(np.abs(mt - mu).max())
    print(f"truncated against untruncated: max difference {diff:.3g}, bound {bound:.3g}")
    assert diff <= bound
    assert float(mu.max()) > 1.0 + 0.1 * w0  # the discs 3 and 70000 are close: the map does peak
    assert (mt[lab != 0] == 1.0).all() and (mu[lab != 0] == 1.0).all()


def test_instance_distances_equal_scipy_edt():
    ndi = pytest.importorskip("scipy.ndimage")
    lab = five_discs()
    ds = M.instance_distances(lab, None)
    assert set(ds) == {3, 7, 12, 70000}
    for i, d in ds.items():
        edt = ndi.distance_transform_edt(lab != i)
        assert float(np.abs(d - edt).max()) <= 1e-12, i
    # inside a window that holds the nearest pixel, the windowed distance is the same; elsewhere it is inf
    dw = M.instance_distances(lab, 11)
    for i, d in dw.items():
        edt = ndi.distance_transform_edt(lab != i)
        fin = np.isfinite(d)
        assert (d[fin] >= edt[fin] - 1e-12).all()
        assert float(np.abs(d - edt)[edt <= 11].max()) <= 1e-12


def test_separate_restatement():
    lab = np.zeros((5, 6), np.int64)
    lab[1:4, 0:3] = 5
    lab[1:4, 3:6] = 9
    sem = (lab > 0).astype(np.int64)
    lo, so = M.separate(lab, sem)
    assert (lo[:, 2] == 0).all() and (lo[:, 3] == 0).all() and (so[:, 2:4] == 0).all()
    assert (lo[1:4, 0:2] == 5).all() and (lo[1:4, 4:6] == 9).all() and (so[1:4, 0:2] == 1).all()


def test_pixel_weight_refusals():
    from eunet.losses import BCEDiceLoss, bce_dice_loss, combined_loss, make_params
    x = torch.randn(2, 3, 4, 5)
    t = torch.randint(0, 3, (2, 4, 5))
    ok = torch.ones(2, 4, 5)
    bad = {"requires_grad": ok.clone().requires_grad_(True), "shape": torch.ones(2, 5, 4),
           "batch": torch.ones(1, 4, 5), "dtype": ok.double(), "half": ok.half(),
           "strided": torch.ones(2, 4, 10)[:, :, ::2], "not a tensor": 1.0}
    for name, pw in bad.items():
        for fn in (combined_loss, bce_dice_loss, lambda a, b, pixel_weight: BCEDiceLoss()(a, b, pixel_weight)):
            with pytest.raises(ValueError):
                fn(x, t, pixel_weight=pw)
    with pytest.raises(ValueError, match="focal_norm"):
        combined_loss(x, t, params=make_params(focal_norm=1), pixel_weight=ok)


def test_weight_map_config_refusals(tmp_path):
    from eunet.data import CellDataset
    for cfg in ({"sigma": 0}, {"sigma": -1.0}, {"w0": -1.0}, {"radius": 0}, {"radius": 49}, {"sigma": 10.0},
                {"class_weight": (1, 2)}, {"sgima": 5.0}, "on"):
        with pytest.raises(ValueError):
            CellDataset(str(tmp_path), weight_map=cfg)
    ds = CellDataset(str(tmp_path), weight_map={"sigma": 2.0, "separate": True})
    assert ds.weight_map["radius"] == 11 and ds.weight_map["separate"] is True and ds.weight_map["w0"] == 10.0
    assert CellDataset(str(tmp_path)).weight_map is None


def test_ops_argument_refusals():
    """Raised on the host before any launch (the tensors here are CPU tensors and never reach the library)."""
    from eunet import ops
    lab = torch.zeros(4, 5, dtype=torch.int64)
    for kw in ({"radius": 0}, {"radius": 49}, {"sigma": 0.0}, {"sigma": -2.0}, {"w0": -1.0}, {"class_weight": (1, 2)}):
        with pytest.raises(ValueError):
            ops.border_weight_map(lab, **kw)
    with pytest.raises(ValueError):
        ops.border_weight_map(lab.int())
    with pytest.raises(ValueError):
        ops.border_weight_map(lab, torch.zeros(5, 4, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.separate_instances(torch.zeros(4, dtype=torch.int64))
