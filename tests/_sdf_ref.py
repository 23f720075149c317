"""The definitions of include/eunet.h (eunet_signed_distance, eunet_boundary_loss_fwd / _bwd) restated on the CPU in
fp64: the signed distance map from a brute-force nearest-site search over exact integer squared distances, the
boundary loss as plain tensor expressions with its gradient from torch autograd.  tests/test_sdf_host.py holds both
to hand-derived answers, scipy's transform and finite differences; the GPU tests compare with them."""
import numpy as np
import torch


def _min_d2(pix, sites):
    """pix [P, 2], sites [S, 2] int64 -> the exact squared distance of every pixel to its nearest site."""
    out = np.empty(len(pix), dtype=np.int64)
    step = max(1, (1 << 22) // max(1, len(sites)))
    for i in range(0, len(pix), step):
        d = pix[i:i + step, None, :] - sites[None, :, :]
        out[i:i + step] = (d * d).sum(-1).min(1)
    return out


def regions(target, K, ignore_index=None):
    """target int64 [N, H, W] -> (member bool [N, K, H, W], ignored bool [N, H, W]).  K = 1: the class is target >= 1.
    An ignored pixel belongs to no class."""
    t = np.asarray(target, dtype=np.int64)
    ign = np.zeros(t.shape, dtype=bool) if ignore_index is None else t == ignore_index
    if K == 1:
        member = (t >= 1)[:, None]
    else:
        member = np.stack([t == c for c in range(K)], axis=1)
    return member & ~ign[:, None], ign


def signed_distance(target, K, ignore_index=None, clip=None, scale=1.0):
    """target int64 [N, H, W] -> (phi float32 [N, K, H, W], phi64 float64 before the clamp and the scaling, clamped
    bool).  phi is rounded to fp32 once, from scale * clamp(phi64, -clip, clip) in fp64; clip and scale are taken as
    the fp32 values the C ABI carries."""
    member, ign = regions(target, K, ignore_index)
    N, _, H, W = member.shape
    yy, xx = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    coords = np.stack([yy, xx], -1)
    phi = np.zeros((N, K, H, W), dtype=np.float64)
    for n in range(N):
        for c in range(K):
            m = member[n, c]
            if not m.any() or m.all():
                continue  # the class or its complement is empty: no contour, phi = 0
            inside, outside = coords[m], coords[~m]
            p = phi[n, c]
            p[~m] = np.sqrt(_min_d2(outside, inside).astype(np.float64))
            p[m] = 1.0 - np.sqrt(_min_d2(inside, outside).astype(np.float64))
            p[ign[n]] = 0.0
    out = phi
    clamped = np.zeros(phi.shape, dtype=bool)
    if clip is not None:
        cl = float(np.float32(clip))
        clamped = np.abs(phi) > cl
        out = np.clip(phi, -cl, cl)
    out = float(np.float32(scale)) * out
    return out.astype(np.float32), phi, clamped


def probabilities(x, activation):
    """softmax over dim 1 or sigmoid of fp64 logits, written as p_j = 1 / (1 + sum_{c != j} exp(x_c - x_j)) (the
    sigmoid: against a zero logit).  The values are torch.softmax's and torch.sigmoid's; the form matters for
    autograd: torch's own backward forms p (1 - p) and p_j (a_j - sum_c p_c a_c), which cancel to 0 or to rounding
    noise of 1e-16 once a probability rounds to 1 in fp64 (logits 40 apart), where the true derivative is a small
    number the fp32 kernels do resolve.  Here the derivative is p_j^2 exp(x_c - x_j): products only.  The exponent
    is capped at 700 so that exp stays finite (p is then below 1e-304)."""
    if activation == "sigmoid":
        return 1.0 / (1.0 + torch.exp(torch.clamp(-x, max=700.0)))
    assert activation == "softmax" and x.shape[1] >= 2
    K = x.shape[1]
    ps = []
    for j in range(K):
        others = [c for c in range(K) if c != j]
        e = torch.exp(torch.clamp(x[:, others] - x[:, j:j + 1], max=700.0)).sum(dim=1)
        ps.append(1.0 / (1.0 + e))
    return torch.stack(ps, dim=1)


def boundary_loss(x32, dist32, activation="softmax", class_weight=None, g=1.0):
    """logits and dist fp32 [N, K, H, W] as stored -> (loss, parts [N], d (g loss) / d logits, A, parts_A [N]) in
    fp64.  A is the sum of the absolute summands over the loss's denominator: the scale of its rounding error (the sum
    itself cancels by construction)."""
    x = x32.detach().double().clone().requires_grad_(True)
    d = dist32.detach().double()
    N, K, H, W = x.shape
    w = [1.0] * K if class_weight is None else [float(v) for v in class_weight][:K]
    assert len(w) == K
    kw = max(1, sum(1 for v in w if v != 0.0))
    wt = torch.tensor(w, dtype=torch.float64).view(1, K, 1, 1)
    p = probabilities(x, activation)
    summands = wt * p * d
    parts = summands.sum(dim=(1, 2, 3)) / (H * W * kw)
    loss = parts.mean()
    (loss * g).backward()
    parts_a = summands.detach().abs().sum(dim=(1, 2, 3)) / (H * W * kw)
    return float(loss.detach()), parts.detach(), x.grad, float(parts_a.mean()), parts_a


def blobs(N, H, W, values, seed, cell=5):
    """A random label map of cell x cell blocks (so that distances beyond 2 occur) drawn from `values`."""
    rng = np.random.default_rng(seed)
    coarse = rng.choice(np.asarray(values, dtype=np.int64), size=(N, -(-H // cell), -(-W // cell)))
    return np.ascontiguousarray(np.repeat(np.repeat(coarse, cell, axis=1), cell, axis=2)[:, :H, :W])


def discs(H, W, centres, label=1):
    """An int64 [H, W] map, `label` inside the discs (cy, cx, r), 0 elsewhere."""
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    m = np.zeros((H, W), dtype=np.int64)
    for cy, cx, r in centres:
        m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = label
    return m
