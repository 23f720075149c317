"""The U-Net border weight map, the separation of touching instances and the two pixel-weighted losses
restated in numpy / fp64 torch on the CPU (include/eunet.h, "U-Net border weight map ...", is the
definition; there is no reference implementation to compare with).

    m, a = border_weight_map(labels, semantic, class_weight, w0, sigma, radius)   # radius None: untruncated
    labels2, semantic2 = separate(labels, semantic)
    value, parts, grad = bce_dice_w(x, target, m, g, **_bce_ref.spec(...))
    value, parts, grad = combined_w(x, target, m, g, **combined_spec(...))

The map is the definition taken literally: per instance id a brute-force minimum of ||x - q|| over the id's
pixels q inside the square window, then a sort over the ids.  a = (d1 + d2)^2 / (2 sigma^2) where the border
term is defined (0 elsewhere) is what the GPU test's error bound scales with.  The losses are computed in
fp64 on the logits as stored; combined_w's gradient is autograd's, bce_dice_w's the closed form of
tests/_bce_ref.py with the weight on its BCE part.  tests/test_wmap_host.py holds all of it against torch's
own losses, the oracle and scipy.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import _bce_ref as B

INF = float("inf")


def default_radius(sigma):
    return int(math.ceil(5.5 * sigma))


def instance_distances(labels, radius=None):
    """{id: d_i [H,W] fp64} for a 2-D int64 label map: d_i(x) = min ||x - q|| over labels(q) = i with
    |qx - xx| <= R and |qy - xy| <= R (R None: no window), inf where no such q exists."""
    lab = np.asarray(labels)
    H, W = lab.shape
    out = {}
    for i in np.unique(lab):
        if i == 0:
            continue
        qy, qx = np.nonzero(lab == i)
        d = np.full((H, W), INF)
        # only pixels within R of the id's bounding box can have one of its pixels in their window
        r = max(H, W) if radius is None else radius
        y0, y1 = max(0, qy.min() - r), min(H, qy.max() + r + 1)
        x0, x1 = max(0, qx.min() - r), min(W, qx.max() + r + 1)
        yy, xx = np.mgrid[y0:y1, x0:x1]
        best = np.full(yy.shape, INF)
        for s in range(0, len(qy), 256):  # chunks of the id's pixels: [region, 256] at a time
            dy = yy[..., None] - qy[s:s + 256]
            dx = xx[..., None] - qx[s:s + 256]
            d2 = (dy * dy + dx * dx).astype(np.float64)
            if radius is not None:
                d2[(np.abs(dy) > radius) | (np.abs(dx) > radius)] = INF
            best = np.minimum(best, d2.min(axis=-1))
        d[y0:y1, x0:x1] = np.sqrt(best)
        out[int(i)] = d
    return out


def border_weight_map(labels, semantic=None, class_weight=(1.0, 1.0, 1.0), w0=10.0, sigma=5.0, radius="default"):
    """(m, a), both fp64 of labels' shape ([H,W] or [N,H,W]); radius "default": ceil(5.5 sigma), None: no
    window (the untruncated map)."""
    lab = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels)
    sem = None if semantic is None else np.asarray(semantic.cpu() if isinstance(semantic, torch.Tensor) else semantic)
    if lab.ndim == 3:
        res = [border_weight_map(lab[n], None if sem is None else sem[n], class_weight, w0, sigma, radius)
               for n in range(lab.shape[0])]
        return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
    if radius == "default":
        radius = default_radius(sigma)
    base = np.ones(lab.shape)
    if sem is not None:
        for c in range(3):
            base[sem == c] = class_weight[c]
    ds = list(instance_distances(lab, radius).values())
    border, a = np.zeros(lab.shape), np.zeros(lab.shape)
    if len(ds) >= 2:
        st = np.sort(np.stack(ds), axis=0)
        d1, d2 = st[0], st[1]
        on = (lab == 0) & np.isfinite(d2)
        s = np.where(on, d1 + d2, 0.0)
        a = np.where(on, s * s / (2.0 * sigma * sigma), 0.0)
        border = np.where(on, w0 * np.exp(-a), 0.0)
    return base + border, a


def separate(labels, semantic=None):
    """Plain loops: labels'(x) = semantic'(x) = 0 where a pixel of x's 3x3 neighbourhood inside the image has a
    label that is neither 0 nor labels(x)."""
    lab = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels)
    sem = None if semantic is None else np.asarray(semantic.cpu() if isinstance(semantic, torch.Tensor) else semantic)
    if lab.ndim == 3:
        res = [separate(lab[n], None if sem is None else sem[n]) for n in range(lab.shape[0])]
        return np.stack([r[0] for r in res]), None if sem is None else np.stack([r[1] for r in res])
    H, W = lab.shape
    lo = lab.copy()
    so = None if sem is None else sem.copy()
    for y in range(H):
        for x in range(W):
            cut = False
            for yy in range(max(0, y - 1), min(H, y + 2)):
                for xx in range(max(0, x - 1), min(W, x + 2)):
                    u = lab[yy, xx]
                    if u != 0 and u != lab[y, x]:
                        cut = True
            if cut:
                lo[y, x] = 0
                if so is not None:
                    so[y, x] = 0
    return lo, so


def bce_dice_w(x, target, m, g=1.0, pos_weight=(1.0, 1.0, 1.0), class_weight=(1.0, 1.0, 1.0),
               dice_weight=(1.0, 1.0, 1.0), w_bce=1.0, w_dice=1.0, smooth=1e-6, ignore_index=None, target_mode=None):
    """tests/_bce_ref.bce_dice with bce(x,t)_c multiplied by m(x) [N,H,W] in BCE and bce_n (and so in the BCE
    part of the gradient); the denominators and the Dice terms are untouched."""
    x = x.detach().double().cpu()
    target = target.cpu()
    mw = torch.as_tensor(m).double().cpu().unsqueeze(1)  # [N,1,H,W]
    N, K = x.shape[:2]
    t, valid, _ = B.targets(target, K, ignore_index, target_mode)
    v = valid.unsqueeze(1).double()
    pw = torch.tensor(pos_weight[:K], dtype=torch.float64).view(1, K, 1, 1)
    cw = torch.tensor(class_weight[:K], dtype=torch.float64).view(1, K, 1, 1)
    dw = torch.tensor(dice_weight[:K], dtype=torch.float64).view(1, K)
    sig, nsig = torch.sigmoid(x), torch.sigmoid(-x)
    # an ignored or out-of-range pixel contributes nothing whatever its weight (0 * inf would be nan)
    mv = torch.where(v > 0, mw, torch.zeros_like(mw))
    bce = cw * (pw * t * B._sp(-x) + (1 - t) * B._sp(x)) * mv
    Vn = valid.flatten(1).sum(1).double()
    V = Vn.sum()
    BCE = bce.sum() / (K * V.clamp_min(1))
    bce_n = bce.flatten(1).sum(1) / (K * Vn.clamp_min(1))
    I = (sig * t * v).flatten(2).sum(2)
    S = (sig * v).flatten(2).sum(2)
    T = (t * v).flatten(2).sum(2)
    U = S + T + smooth
    dice_n = (dw * (1 - (2 * I + smooth) / U)).sum(1) / K
    value = w_bce * BCE + w_dice * dice_n.mean()
    gb = w_bce * cw * (-pw * t * nsig + (1 - t) * sig) / (K * V.clamp_min(1)) * mv
    coef = (w_dice * dw / (N * K)).view(1, K, 1, 1)
    gd = coef * (-2 * t / U.view(N, K, 1, 1) + ((2 * I + smooth) / U ** 2).view(N, K, 1, 1)) * sig * nsig * v
    grad = g * (gb + gd)
    return float(value), torch.stack([bce_n, dice_n], dim=1), grad


def combined_spec(ce_weight=(1.0, 20.0, 10.0), alpha=(1.0, 8.0, 5.0), gamma=5.0, ignore_index=None,
                  dice_weight=(1.0, 15.0, 8.0), tversky_weight=(1.0, 12.0, 6.0), tversky_alpha=0.7, w_focal=2.5,
                  w_dice=2.5, w_tversky=1.0, class_div=3.0):
    """eunet_loss_params without focal_norm (a pixel weight refuses focal_norm = 1); the defaults are the
    reference Trainer's configuration."""
    return dict(ce_weight=ce_weight, alpha=alpha, gamma=gamma, ignore_index=ignore_index, dice_weight=dice_weight,
                tversky_weight=tversky_weight, tversky_alpha=tversky_alpha, w_focal=w_focal, w_dice=w_dice,
                w_tversky=w_tversky, class_div=class_div)


def combined_w(x, target, m, g=1.0, ce_weight=(1.0, 20.0, 10.0), alpha=(1.0, 8.0, 5.0), gamma=5.0, ignore_index=None,
               dice_weight=(1.0, 15.0, 8.0), tversky_weight=(1.0, 12.0, 6.0), tversky_alpha=0.7, w_focal=2.5,
               w_dice=2.5, w_tversky=1.0, class_div=3.0):
    """eunet_loss_fwd's definition with the per-pixel focal summand multiplied by m(x) [N,H,W]: F_den stays
    N*H*W, Dice and Tversky are untouched; a pixel at ignore_index or outside [0, K) gives nothing to the focal
    term (and (target == c) false for every c in Dice and Tversky, its probabilities still in S).
    -> (value, parts [N,3] = focal_n / dice_n / tversky_n, d (g * value) / dx by autograd)."""
    xd = x.detach().double().cpu().clone().requires_grad_(True)
    target = target.cpu()
    mw = torch.as_tensor(m).double().cpu()
    N, K, H, W = xd.shape
    valid = (target >= 0) & (target < K)
    if ignore_index is not None:
        valid = valid & (target != ignore_index)
    tc = torch.where(valid, target, torch.zeros_like(target))
    logp = torch.log_softmax(xd, 1)
    p = logp.exp()
    w = torch.tensor(ce_weight[:K], dtype=torch.float64)
    al = torch.tensor(alpha[:K], dtype=torch.float64)
    ce = -w[tc] * logp.gather(1, tc[:, None])[:, 0]
    pt = torch.exp(-ce)
    fl = al[tc] * (1 - pt) ** gamma * ce
    fl = torch.where(valid, fl * torch.where(valid, mw, torch.zeros_like(mw)), torch.zeros_like(fl))
    focal_n = fl.flatten(1).sum(1) / (H * W)
    dice_n, tv_n = xd.new_zeros(N), xd.new_zeros(N)
    for c in range(K):
        pc = p[:, c]
        t1 = (target == c).double()
        I, S, T = (pc * t1).flatten(1).sum(1), pc.flatten(1).sum(1), t1.flatten(1).sum(1)
        dice_n = dice_n + dice_weight[c] * (1.0 - (2.0 * I + 1e-6) / (S + T + 1e-6))
        fp, fn = S - I, T - I
        tv_n = tv_n + tversky_weight[c] * (1.0 - (I + 1e-6) / (I + tversky_alpha * fp + (1 - tversky_alpha) * fn + 1e-6))
    dice_n, tv_n = dice_n / class_div, tv_n / class_div
    value = w_focal * fl.sum() / (N * H * W) + (w_dice * dice_n + w_tversky * tv_n).mean()
    (value * g).backward()
    parts = torch.stack([focal_n, dice_n, tv_n], dim=1).detach()
    return float(value.detach()), parts, xd.grad
