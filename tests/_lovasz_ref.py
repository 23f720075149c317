"""The Lovasz losses of include/eunet.h ("Lovasz losses") restated in fp64 numpy / torch on the fp32 inputs as stored.

errors_flags: the errors in fp64 from the fp32 logits, and the flags.  order_of: the stable descending order
(np.lexsort on (index, -error), a NaN ahead of +inf, -0 equal to +0, ignored elements last in index order).
lovasz_grad: g from the closed form in float64, rounded once to float32 -- integer inputs and correctly rounded
operations, so the device must give the same bits.  loss: segment losses, selection and means in fp64.
autograd_loss: the same loss as a torch fp64 graph (the order and g are constants, as in Berman's code), for
gradients.  backward_from_weights: the backward formula of include/eunet.h applied to given weights."""
import numpy as np
import torch


def errors_flags(logits, target, activation, ignore_index=None):
    """logits float32 [N,K,H,W], target int64 [N,H,W] (torch, CPU) -> (errors float64 [N,K,H,W], flags uint8)."""
    x = logits.double().numpy()
    t = target.numpy()
    n, k, h, w = x.shape
    ign = np.zeros_like(t, dtype=bool) if ignore_index is None else t == ignore_index
    if activation == "hinge" and k == 1:
        inrange = t >= 0
        fg = (t >= 1)[:, None]
    else:
        inrange = (t >= 0) & (t < k)
        fg = t[:, None] == np.arange(k)[None, :, None, None]
    skip = ign | ~inrange
    if activation == "softmax":
        z = x - x.max(axis=1, keepdims=True)
        p = np.exp(z)
        p /= p.sum(axis=1, keepdims=True)
        e = np.abs(fg - p)
    else:
        e = 1.0 - x * (2.0 * fg - 1.0)
    skip_k = np.broadcast_to(skip[:, None], e.shape)
    e = np.where(skip_k, 0.0, e)
    flags = np.where(skip_k, 2, np.broadcast_to(fg, e.shape).astype(np.uint8)).astype(np.uint8)
    return e, flags


def segments(a, per_image):
    """[N,K,H,W] -> [S,L]: per_image [N K, H W], otherwise [K, N H W] (sample-major inside a segment)."""
    n, k, h, w = a.shape
    return a.reshape(n * k, h * w) if per_image else np.ascontiguousarray(a.transpose(1, 0, 2, 3)).reshape(k, n * h * w)


def unsegment(a, shape, per_image):
    n, k, h, w = shape
    return a.reshape(n, k, h, w) if per_image else np.ascontiguousarray(a.reshape(k, n, h, w).transpose(1, 0, 2, 3))


def order_of(e, flags):
    """One segment: the indices of the valid elements in sorted order followed by the ignored ones in index order,
    and V."""
    idx = np.arange(e.shape[0])
    valid = flags < 2
    ev = np.asarray(e, dtype=np.float64)[valid]
    nan = np.isnan(ev)
    o = np.lexsort((idx[valid], -np.where(nan, 0.0, ev), ~nan))  # last key first: NaN, then -error, then index
    return np.concatenate([idx[valid][o], idx[~valid]]), int(valid.sum())


def lovasz_grad(fg_sorted):
    """fg_sorted: bool [V] in sorted order -> g float32 [V] (the closed form in float64, rounded once)."""
    v = fg_sorted.shape[0]
    G = int(fg_sorted.sum())
    if G == 0:
        g = np.zeros(v, dtype=np.float32)
        g[:1] = 1.0
        return g
    F = np.cumsum(fg_sorted.astype(np.int64))
    r = np.arange(1, v + 1, dtype=np.int64)
    I = (G - F).astype(np.float64)
    U = G + r - F
    with np.errstate(divide="ignore", invalid="ignore"):
        bg = I / ((U - 1).astype(np.float64) * U.astype(np.float64))
    return np.where(fg_sorted, 1.0 / U.astype(np.float64), bg).astype(np.float32)


def sort_ref(errors, flags):
    """errors [S,L], flags uint8 [S,L] -> (order int32 [S,L], grad float32 [S,L], counts int64 [S,2])."""
    s, l = errors.shape
    order = np.zeros((s, l), dtype=np.int32)
    grad = np.zeros((s, l), dtype=np.float32)
    counts = np.zeros((s, 2), dtype=np.int64)
    for i in range(s):
        o, v = order_of(errors[i], flags[i])
        order[i] = o
        grad[i, o[:v]] = lovasz_grad(flags[i, o[:v]] == 1)
        counts[i] = (int((flags[i] == 1).sum()), v)
    return order, grad, counts


def selection(counts, k, classes, per_image, n, activation):
    """share [S] float64: the weight of every segment loss in the loss (0: not selected)."""
    if classes is None:
        classes = "present" if activation == "softmax" else "all"
    s = counts.shape[0]
    G, V = counts[:, 0], counts[:, 1]
    if classes == "present":
        sel = G > 0
    elif classes == "all":
        sel = V > 0
    else:
        sel = (V > 0) & np.isin(np.arange(s) % k, list(classes))
    share = np.zeros(s)
    groups = n if per_image else 1
    for gi in range(groups):
        sl = slice(gi * (s // groups), (gi + 1) * (s // groups))
        m = int(sel[sl].sum())
        if m:
            share[sl] = np.where(sel[sl], 1.0 / (m * groups), 0.0)
    return sel, share


def loss(logits, target, activation, classes=None, per_image=False, ignore_index=None, errors=None):
    """-> dict(loss, parts [S] (NaN where unselected), weights [N,K,H,W] float64 = g share, g float32 [N,K,H,W],
    share [S], errors [N,K,H,W] float64, flags, counts).  errors: errors to use in place of the fp64 ones (the
    device's, to separate the error of the errors from the rest)."""
    e, flags = errors_flags(logits, target, activation, ignore_index)
    if errors is not None:
        e = np.asarray(errors, dtype=np.float64)
    n, k = logits.shape[:2]
    es, fs = segments(e, per_image), segments(flags, per_image)
    order, grad, counts = sort_ref(es, fs)
    eb = np.maximum(es, 0.0) if activation == "hinge" else es
    eb = np.where(np.isnan(es), es, eb)
    seg = (eb * grad.astype(np.float64)).sum(axis=1)
    sel, share = selection(counts, k, classes, per_image, n, activation)
    return dict(loss=float((seg * share).sum()), parts=np.where(sel, seg, np.nan), share=share, counts=counts,
                g=unsegment(grad, logits.shape, per_image), errors=e, flags=flags,
                weights=unsegment(grad.astype(np.float64) * share[:, None], logits.shape, per_image))


def _torch_errors(x, target, activation):
    n, k, h, w = x.shape
    if activation == "hinge" and k == 1:
        fg = (target >= 1)[:, None].double()
    else:
        fg = (target[:, None] == torch.arange(k)[None, :, None, None]).double()
    if activation == "softmax":
        return (fg - torch.softmax(x, dim=1)).abs()
    return torch.relu(1.0 - x * (2.0 * fg - 1.0))


def autograd_loss(logits, target, activation, classes=None, per_image=False, ignore_index=None, gloss=1.0):
    """The loss as a torch fp64 graph with the restatement's weights as constants -> (loss, d (gloss loss) / d logits)."""
    ref = loss(logits, target, activation, classes, per_image, ignore_index)
    x = logits.double().clone().requires_grad_(True)
    v = (_torch_errors(x, target, activation) * torch.from_numpy(ref["weights"])).sum()
    (v * gloss).backward()
    return float(v), x.grad


def backward_from_weights(logits, target, weights, activation, gloss=1.0):
    """include/eunet.h's backward in fp64: weights [N,K,H,W] (g times the segment's share) -> d (gloss loss) / d logits."""
    x = logits.double().numpy()
    t = target.numpy()
    w = np.asarray(weights, dtype=np.float64)
    n, k, h, wd = x.shape
    if activation == "hinge":
        fg = (t >= 1)[:, None] if k == 1 else t[:, None] == np.arange(k)[None, :, None, None]
        sg = 2.0 * fg - 1.0
        return torch.from_numpy(-gloss * w * sg * ((1.0 - x * sg) > 0))
    fg = t[:, None] == np.arange(k)[None, :, None, None]
    z = x - x.max(axis=1, keepdims=True)
    p = np.exp(z)
    p /= p.sum(axis=1, keepdims=True)
    a = w * np.sign(p - fg)
    return torch.from_numpy(gloss * p * (a - (a * p).sum(axis=1, keepdims=True)))
