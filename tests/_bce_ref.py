"""The sigmoid BCE + soft Dice loss restated in fp64 in plain torch on the CPU (include/eunet.h,
eunet_bce_dice_fwd, is the definition; there is no reference implementation to compare with).

    value, parts, grad = bce_dice(x, target, **spec)

x [N,K,H,W] (any float dtype; computed in fp64 on the values as stored), target [N,H,W] int64.  grad is
the closed-form d (g * loss) / dx of the definition, not autograd's; tests/test_bce_dice_host.py holds both
the value and this gradient against F.binary_cross_entropy_with_logits plus an autograd Dice.
"""
import torch


def _sp(z):
    return z.clamp_min(0) + torch.log1p(torch.exp(-z.abs()))


def spec(pos_weight=(1.0, 1.0, 1.0), class_weight=(1.0, 1.0, 1.0), dice_weight=(1.0, 1.0, 1.0), w_bce=1.0,
         w_dice=1.0, smooth=1e-6, ignore_index=None, target_mode=None):
    return dict(pos_weight=pos_weight, class_weight=class_weight, dice_weight=dice_weight, w_bce=w_bce,
                w_dice=w_dice, smooth=smooth, ignore_index=ignore_index, target_mode=target_mode)


def targets(target, K, ignore_index=None, target_mode=None):
    """(t [N,K,H,W] fp64, valid [N,H,W] bool, out-of-range count)."""
    mode = target_mode or ("foreground" if K == 1 else "onehot")
    ign = torch.zeros_like(target, dtype=torch.bool) if ignore_index is None else target == ignore_index
    if mode == "foreground":
        assert K == 1
        ok = target >= 0
        t = (target >= 1).unsqueeze(1)
    else:
        assert K >= 2
        ok = (target >= 0) & (target < K)
        t = torch.stack([target == c for c in range(K)], dim=1)
    valid = ok & ~ign
    return t.double(), valid, int((~ok & ~ign).sum())


def bce_dice(x, target, g=1.0, pos_weight=(1.0, 1.0, 1.0), class_weight=(1.0, 1.0, 1.0),
             dice_weight=(1.0, 1.0, 1.0), w_bce=1.0, w_dice=1.0, smooth=1e-6, ignore_index=None, target_mode=None):
    x = x.detach().double().cpu()
    target = target.cpu()
    N, K = x.shape[:2]
    t, valid, _ = targets(target, K, ignore_index, target_mode)
    m = valid.unsqueeze(1).double()  # [N,1,H,W]
    pw = torch.tensor(pos_weight[:K], dtype=torch.float64).view(1, K, 1, 1)
    cw = torch.tensor(class_weight[:K], dtype=torch.float64).view(1, K, 1, 1)
    dw = torch.tensor(dice_weight[:K], dtype=torch.float64).view(1, K)
    sig, nsig = torch.sigmoid(x), torch.sigmoid(-x)
    bce = cw * (pw * t * _sp(-x) + (1 - t) * _sp(x)) * m
    Vn = valid.flatten(1).sum(1).double()
    V = Vn.sum()
    BCE = bce.sum() / (K * V.clamp_min(1))
    bce_n = bce.flatten(1).sum(1) / (K * Vn.clamp_min(1))
    I = (sig * t * m).flatten(2).sum(2)  # [N,K]
    S = (sig * m).flatten(2).sum(2)
    T = (t * m).flatten(2).sum(2)
    U = S + T + smooth
    dice_n = (dw * (1 - (2 * I + smooth) / U)).sum(1) / K
    value = w_bce * BCE + w_dice * dice_n.mean()
    gb = w_bce * cw * (-pw * t * nsig + (1 - t) * sig) / (K * V.clamp_min(1))
    coef = (w_dice * dw / (N * K)).view(1, K, 1, 1)
    gd = coef * (-2 * t / U.view(N, K, 1, 1) + ((2 * I + smooth) / U ** 2).view(N, K, 1, 1)) * sig * nsig
    grad = g * (gb + gd) * m
    parts = torch.stack([bce_n, dice_n], dim=1)
    return float(value), parts, grad


def sigmoid_bound(x32):
    """(e, 4 e): e the largest error of torch's own fp32 sigmoid (on the CPU) against fp64 on these inputs;
    4 e is what the sigmoid kernels are allowed."""
    x32 = x32.detach().float().cpu()
    own = float((torch.sigmoid(x32).double() - torch.sigmoid(x32.double())).abs().max())
    return own, 4.0 * own
