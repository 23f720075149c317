"""Overlap-tile gather and blend restated in plain loops, fp64, on the CPU (include/eunet.h, "overlap-tile
inference", is the definition; the reference has no tiling to compare with).

    origins(L, e, S)                          tile origins along one axis
    axis_weights(mode, L, e, o, margin, tab)  fp64 weights of the e tile-local positions of a tile at origin o
    gather(image, p, first, count)            [count, C, th, tw]: slices of the F.pad(reflect) image
    blend(logits, p, activation, flip_h, flip_w) -> (out, mag, den): fp64 [K, h, w] weighted mean, the same mean
                                              of |act| (what a relative rounding bound scales with), weight sums
    act_bound(logits, activation)             (e, 4 e): torch's own CPU fp32 activation error against fp64

Nothing here calls eunet.tiling's arithmetic: the geometry is recomputed from (hp, wp, th, tw, stride, margin)
with loops, so a slip in the plan shows as a disagreement.  The gaussian weights are the plan's fp32 tables --
the tables ARE the definition (formed on the host, uploaded as they are); tests/test_tiling_host.py holds
them to the closed form.
"""
import math

import torch
import torch.nn.functional as F


def origins(L, e, S):
    if L <= e:
        return [0]
    out, i = [], 0
    while True:
        o = i * S
        if o >= L - e:
            out.append(L - e)
            return out
        out.append(o)
        i += 1


def axis_weights(mode, L, e, o, margin, tab):
    if mode == "gaussian":
        return torch.as_tensor(tab).double()
    w = torch.ones(e, dtype=torch.float64)
    if mode == "crop":
        for t in range(e):
            lo = margin if o > 0 else 0
            hi = e - (margin if o + e < L else 0)
            w[t] = 1.0 if lo <= t < hi else 0.0
    return w


def padded(image, p):
    """image [C, h, w] -> [C, hp, wp] by F.pad(mode="reflect") to the bottom / right."""
    return F.pad(image.unsqueeze(0), (0, p.wp - p.w, 0, p.hp - p.h), mode="reflect")[0]


def gather(image, p, first, count):
    x = padded(image, p)
    oys, oxs = origins(p.hp, p.th, p.stride), origins(p.wp, p.tw, p.stride)
    tiles = []
    for n in range(first, first + count):
        oy, ox = oys[n // len(oxs)], oxs[n % len(oxs)]
        tiles.append(x[:, oy:oy + p.th, ox:ox + p.tw])
    return torch.stack(tiles)


def activate(v, activation):
    """v [K, ...] fp64."""
    if activation == "softmax":
        return F.softmax(v, 0)
    if activation == "sigmoid":
        return torch.sigmoid(v)
    return v


def blend(logits, p, activation, flip_h=False, flip_w=False):
    logits = logits.detach().cpu()
    oys, oxs = origins(p.hp, p.th, p.stride), origins(p.wp, p.tw, p.stride)
    assert logits.shape[0] == len(oys) * len(oxs)
    K = logits.shape[1]
    num = torch.zeros(K, p.hp, p.wp, dtype=torch.float64)
    mag = torch.zeros(K, p.hp, p.wp, dtype=torch.float64)
    den = torch.zeros(p.hp, p.wp, dtype=torch.float64)
    n = 0
    for oy in oys:  # increasing tile number
        wy = axis_weights(p.blend, p.hp, p.th, oy, p.margin, p.table(0))
        for ox in oxs:
            wx = axis_weights(p.blend, p.wp, p.tw, ox, p.margin, p.table(1))
            w = wy[:, None] * wx[None, :]
            a = activate(logits[n].double(), activation)
            num[:, oy:oy + p.th, ox:ox + p.tw] += w * a
            mag[:, oy:oy + p.th, ox:ox + p.tw] += w * a.abs()
            den[oy:oy + p.th, ox:ox + p.tw] += w
            n += 1
    assert float(den.min()) > 0.0
    out, mag = (num / den)[:, :p.h, :p.w], (mag / den)[:, :p.h, :p.w]
    if flip_h:
        out, mag = out.flip(1), mag.flip(1)
    if flip_w:
        out, mag = out.flip(2), mag.flip(2)
    return out, mag, den


def act_bound(logits, activation):
    """(e, 4 e): e the largest error of torch's own CPU fp32 softmax / sigmoid against fp64 on these logits
    (per tile, over K); 'none' has no activation error."""
    x = logits.detach().float().cpu()
    if activation == "none":
        return 0.0, 0.0
    if activation == "softmax":
        own = float((F.softmax(x, 1).double() - F.softmax(x.double(), 1)).abs().max())
    else:
        own = float((torch.sigmoid(x).double() - torch.sigmoid(x.double())).abs().max())
    return own, 4.0 * own


def gauss_closed_form(e, sigma_scale):
    return [math.exp(-0.5 * ((t - (e - 1) / 2) / (sigma_scale * e)) ** 2) for t in range(e)]
