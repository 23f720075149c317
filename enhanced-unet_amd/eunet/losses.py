"""Fused combined loss (focal + Dice + Tversky) as one autograd node, and the reference's
loss modules on top of it.

Reference: train_eval.py:28-60 (FocalLoss), :80 (nn.CrossEntropyLoss(weight)), 134-181
(dice/tversky), 183-197 (_compute_combined_loss), 262-337 (per-sample loop, sum, /B).
One kernel pass computes every sample's per-class sums; backward is analytic per pixel.
Each term is differentiable on its own: the kernel takes the term weights
(eunet_loss_params), so FocalLoss / dice_loss / tversky_loss / CrossEntropyLoss are the
same kernel with the other weights at zero.

Targets outside [0, K) (other than ignore_index) make the reference raise inside
F.cross_entropy -- on the GPU as an asynchronous device assert that surfaces at the next
synchronisation.  Here the kernel counts them on the device and check_targets() raises
ValueError at the next host synchronisation of the training loop (Trainer.step's
loss.item(), the end of Trainer.train_epoch), or immediately with combined_loss(...,
validate=True).

bce_dice_loss / BCEDiceLoss are the sigmoid counterpart (csrc/bce_dice.hip): one logit per class, BCE
+ soft Dice, with K = 1 for foreground against background.  The reference has none (BASELINE.json's
north star names it); include/eunet.h holds its definition.  It reports refused targets through the
same counter and check_targets().

boundary_loss / BoundaryLoss (csrc/sdf.hip) are the contour term: the softmax or sigmoid probability integrated
against a signed distance map of the target (ops.signed_distance_map), after Kervadec et al. (MIDL 2019).  It sees
no target, only the map, and is meant to be added to a region loss from the caller's own loop.

lovasz_loss / LovaszLoss (csrc/lovasz.hip) are the IoU surrogate of Berman et al. (CVPR 2018): the errors of a class
sorted on the device (a stable segmented radix sort) and weighted by the gradient of the Jaccard extension.  Like
the boundary loss it is called from the caller's own loop; it reports refused targets through check_targets().
"""
from __future__ import annotations

from typing import Optional, Sequence, Union

import torch
import torch.nn as nn

from . import ops
from . import _lib
from ._lib import BCEDiceParams, LossParams

NO_IGNORE = -(2 ** 31)  # EUNET_NO_IGNORE


_host_copies = {}  # id(tensor) -> (weakref, _version, values): no device sync per training step


def _host_values(t: torch.Tensor):
    """t's values as a Python list.  A device tensor is copied once and re-copied only after an
    in-place change (t._version): the Trainer rebuilds its loss parameters every step from
    self.focal_loss.class_weights, a cuda tensor, and a .cpu() there would drain the launch queue."""
    import weakref
    hit = _host_copies.get(id(t))
    if hit is not None and hit[0]() is t and hit[1] == t._version:
        return hit[2]
    vals = t.detach().cpu().reshape(-1).tolist()
    if len(_host_copies) > 64:
        _host_copies.clear()
    _host_copies[id(t)] = (weakref.ref(t), t._version, vals)
    return vals


def _triple(v, default: float, what: str):
    """A per-class table of 3 floats from None / a scalar / a list / a tensor (missing classes 0)."""
    if v is None:
        return [default] * 3
    if isinstance(v, torch.Tensor):
        v = _host_values(v)
    if isinstance(v, (int, float)):
        return [float(v)] * 3
    v = [float(a) for a in v]
    if len(v) > 3:
        raise ValueError(f"{what}: at most 3 classes are supported, got {len(v)} values")
    return v + [0.0] * (3 - len(v))


def make_params(*, ce_weight=None, alpha=None, gamma: float = 5.0, ignore_index: Optional[int] = None,
                dice_weight=(1.0, 15.0, 8.0), tversky_weight=(1.0, 12.0, 6.0), tversky_alpha: float = 0.7,
                w_focal: float = 2.5, w_dice: float = 2.5, w_tversky: float = 1.0, class_div: float = 3.0,
                focal_norm: int = 0) -> LossParams:
    """eunet_loss_params; the defaults other than ce_weight/alpha are the Trainer's enhanced_unet
    configuration (train_eval.py:74-87, 140, 164, 175).  alpha as FocalLoss treats it: a list
    gives per-class values (classes past its end get 0, train_eval.py:50-53), a scalar applies to
    every class, None means 1."""
    p = LossParams()
    p.ce_weight[:] = _triple(ce_weight, 1.0, "class_weights")
    p.alpha[:] = _triple(alpha, 1.0, "alpha")
    p.gamma = float(gamma)
    p.ignore_index = NO_IGNORE if ignore_index is None else int(ignore_index)
    p.dice_weight[:] = _triple(dice_weight, 1.0, "dice weights")
    p.tversky_weight[:] = _triple(tversky_weight, 1.0, "tversky weights")
    p.tversky_alpha = float(tversky_alpha)
    p.w_focal, p.w_dice, p.w_tversky = float(w_focal), float(w_dice), float(w_tversky)
    p.class_div = float(class_div)
    p.focal_norm = int(focal_norm)
    return p


_REFERENCE = None


def reference_params() -> LossParams:
    """The Trainer's enhanced_unet loss (the library's built-in default)."""
    global _REFERENCE
    if _REFERENCE is None:
        _REFERENCE = ops.loss_reference_params()
    return _REFERENCE


# ---- out-of-range target bookkeeping (see module docstring) --------------------------------
_bad = {}  # device -> fp64 [1] accumulator of out-of-range targets since the last check
_bad_pending = False  # a loss call (or a graph replay holding one) ran since the last check


def bad_target_accumulator(device) -> torch.Tensor:
    """The persistent per-device counter the loss adds its out-of-range count to, in place: a
    captured step graph (train_eval.StepGraph) keeps accumulating into it on every replay."""
    dev = torch.device(device)
    acc = _bad.get(dev)
    if acc is None:
        acc = _bad[dev] = torch.zeros(1, dtype=torch.float64, device=dev)
    return acc


def mark_pending():
    global _bad_pending
    _bad_pending = True


def _record_bad(sums: torch.Tensor):
    bad_target_accumulator(sums.device).add_(sums[-1:])
    mark_pending()


def check_targets():
    """Raise ValueError if any loss call since the last check saw a target outside [0, K)
    (synchronises with the device)."""
    global _bad_pending
    if not _bad_pending:
        return
    _bad_pending = False
    n = 0
    for acc in _bad.values():
        n += int(acc.item())
        acc.zero_()
    if n:
        raise ValueError(f"{n} target value(s) outside [0, num_classes) reached the loss "
                         f"(F.cross_entropy would raise: class index out of bounds)")


def _check_logits_target(what: str, logits, target=None):
    """The shape rules every per-pixel loss shares, as ValueError: [N, K, H, W] logits and a target of [N, H, W]."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 4:
        raise ValueError(f"{what}: expected [N, K, H, W] logits, got "
                         f"{tuple(logits.shape) if isinstance(logits, torch.Tensor) else type(logits).__name__}")
    if target is not None and target.shape != logits.shape[:1] + logits.shape[2:]:
        raise ValueError(f"{what}: target {tuple(target.shape)} does not match logits {tuple(logits.shape)}")


def _check_on_device(what: str, *tensors):
    """The device rule, as EunetError (there is no CPU fallback); it comes after every ValueError rule of a loss."""
    if not all(t.is_cuda for t in tensors):
        raise _lib.EunetError(f"{what} needs device tensors (no CPU fallback)")


def _check_pixel_weight(pixel_weight, logits, target, what: str):
    """The rules of a per-pixel weight: float32, contiguous, on the logits' device, of the target's shape, and
    no gradient (the weight takes none)."""
    if not isinstance(pixel_weight, torch.Tensor):
        raise ValueError(f"{what}: pixel_weight must be a tensor, got {type(pixel_weight).__name__}")
    if pixel_weight.requires_grad:
        raise ValueError(f"{what}: pixel_weight takes no gradient (requires_grad is set)")
    if pixel_weight.dtype != torch.float32:
        raise ValueError(f"{what}: pixel_weight must be float32, got {pixel_weight.dtype}")
    if pixel_weight.shape != target.shape:
        raise ValueError(f"{what}: pixel_weight {tuple(pixel_weight.shape)} does not match target "
                         f"{tuple(target.shape)}")
    if pixel_weight.device != logits.device:
        raise ValueError(f"{what}: pixel_weight is on {pixel_weight.device}, the logits on {logits.device}")
    if not pixel_weight.is_contiguous():
        raise ValueError(f"{what}: pixel_weight must be contiguous")


class _SumsLossFunction(torch.autograd.Function):
    """A loss whose forward saves per-sample sums for an analytic backward (loss, bce_dice): apply(logits, target,
    params, track_targets, pixel_weight=None).  pixel_weight None runs the unweighted entry points, a tensor the
    _w ones.  Subclasses name the loss, the columns of parts and the six ops."""
    what = n_parts = sums_len = workspace_bytes = fwd = bwd = fwd_w = bwd_w = None

    @classmethod
    def check(cls, logits, params):
        pass

    @classmethod
    def forward(cls, ctx, logits, target, params, track_targets, pixel_weight=None):
        logits = logits.contiguous().float()
        target = target.contiguous().long()
        _check_logits_target(cls.what, logits, target)
        cls.check(logits, params)
        _check_on_device(cls.what, logits, target)
        n, k, h, w = logits.shape
        dev = logits.device
        sums = torch.empty(cls.sums_len(n, k), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        parts = torch.empty(n, cls.n_parts, dtype=torch.float32, device=dev)
        ws = torch.empty(cls.workspace_bytes(n, k, h, w), dtype=torch.uint8, device=dev)
        if pixel_weight is None:
            cls.fwd(logits, target, params, sums, loss, parts, ws)
        else:
            cls.fwd_w(logits, target, pixel_weight, params, sums, loss, parts, ws)
        if track_targets:
            _record_bad(sums)
        ctx.save_for_backward(logits, target, sums, *([] if pixel_weight is None else [pixel_weight]))
        ctx.params = params
        ctx.mark_non_differentiable(parts)
        return loss, parts

    @classmethod
    def backward(cls, ctx, gloss, gparts):
        logits, target, sums, *pw = ctx.saved_tensors
        glog = torch.empty_like(logits)
        gloss = gloss.contiguous().float().reshape(1)
        if pw:
            cls.bwd_w(logits, target, pw[0], ctx.params, sums, gloss, glog)
        else:
            cls.bwd(logits, target, ctx.params, sums, gloss, glog)
        return glog, None, None, None, None


class CombinedLossFunction(_SumsLossFunction):
    """Focal + Dice + Tversky (eunet_loss_fwd / _bwd, with a pixel_weight eunet_loss_fwd_w / _bwd_w)."""
    what, n_parts = "combined_loss", 3
    sums_len, workspace_bytes = staticmethod(ops.loss_sums_len), staticmethod(ops.loss_workspace_bytes)
    fwd, bwd = staticmethod(ops.loss_fwd), staticmethod(ops.loss_bwd)
    fwd_w, bwd_w = staticmethod(ops.loss_fwd_w), staticmethod(ops.loss_bwd_w)


class ConsistencyFunction(torch.autograd.Function):
    """sum_b c_b (1/B) sum_i MSE(softmax(branch_b[i]), softmax(fused[i])) (train_eval.py:207-232;
    the fused probabilities are not detached in the reference, so both sides get gradients)."""

    @staticmethod
    def forward(ctx, fused, br0, br1, c0, c1):
        fused, br0, br1 = (t.contiguous().float() for t in (fused, br0, br1))
        n, k, h, w = fused.shape
        part = torch.empty(n * ops.consistency_tiles(h, w) * 2, dtype=torch.float32, device=fused.device)
        loss = torch.empty((), dtype=torch.float32, device=fused.device)
        ops.consistency_fwd(fused, br0, br1, c0, c1, part, loss)
        ctx.save_for_backward(fused, br0, br1)
        ctx.c = (c0, c1)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        fused, br0, br1 = ctx.saved_tensors
        gf, g0, g1 = (torch.zeros_like(t) for t in (fused, br0, br1))
        ops.consistency_bwd(fused, br0, br1, ctx.c[0], ctx.c[1], gloss.contiguous().float().reshape(1), gf, g0, g1)
        return gf, g0, g1, None, None


def consistency_loss(fused, br0, br1, c0: float, c1: float):
    return ConsistencyFunction.apply(fused, br0, br1, float(c0), float(c1))


def combined_loss(logits: torch.Tensor, target: torch.Tensor, return_parts: bool = False,
                  params: Optional[LossParams] = None, validate: bool = False, track_targets: bool = True,
                  pixel_weight: Optional[torch.Tensor] = None):
    """Batched train_eval loss: logits [B,K,H,W] (already at mask size), target [B,H,W]
    -> (1/B) sum_b [w_focal focal_b + w_dice dice_b + w_tversky tversky_b] (params: None =
    the reference Trainer's 2.5 / 2.5 / 1.0 configuration).  pixel_weight (float32 [B,H,W], e.g.
    ops.border_weight_map): multiplies the per-pixel focal summand, the pixel mean keeps its N*H*W
    denominator, Dice and Tversky are untouched; it takes no gradient and cannot be combined with
    focal_norm = 1."""
    if pixel_weight is not None:
        _check_pixel_weight(pixel_weight, logits, target, "combined_loss")
        if params is not None and params.focal_norm != 0:
            raise ValueError("combined_loss: focal_norm = 1 with a pixel_weight is not defined (its denominator "
                             "would need a definition of its own)")
    loss, parts = CombinedLossFunction.apply(logits, target, params, track_targets, pixel_weight)
    if validate:
        check_targets()
    return (loss, parts) if return_parts else loss


# ---- sigmoid BCE + soft Dice (csrc/bce_dice.hip; no reference counterpart: BASELINE.json north star) ----
TARGET_MODES = {None: _lib.BCE_TARGET_AUTO, "onehot": _lib.BCE_TARGET_ONEHOT,
                "foreground": _lib.BCE_TARGET_FOREGROUND}


def make_bce_dice_params(*, pos_weight=None, class_weight=None, dice_weight=None, w_bce: float = 1.0,
                         w_dice: float = 1.0, smooth: float = 1e-6, ignore_index: Optional[int] = None,
                         target_mode: Optional[str] = None) -> BCEDiceParams:
    """eunet_bce_dice_params (include/eunet.h holds the definition of the loss).  The three tables as
    _triple reads them: None means 1 for every class, a scalar applies to every class, a list or tensor
    gives per-class values (at most 3).  target_mode: "onehot" (t_c = [target == c], K >= 2),
    "foreground" (t_0 = [target >= 1], K = 1) or None: by the K of the logits at call time."""
    if target_mode not in TARGET_MODES:
        raise ValueError(f"target_mode must be 'onehot', 'foreground' or None, not {target_mode!r}")
    if not float(smooth) > 0.0:
        raise ValueError(f"smooth must be > 0, got {smooth}")
    p = BCEDiceParams()
    p.pos_weight[:] = _triple(pos_weight, 1.0, "pos_weight")
    p.class_weight[:] = _triple(class_weight, 1.0, "class_weight")
    p.dice_weight[:] = _triple(dice_weight, 1.0, "dice_weight")
    p.w_bce, p.w_dice, p.smooth = float(w_bce), float(w_dice), float(smooth)
    p.ignore_index = NO_IGNORE if ignore_index is None else int(ignore_index)
    p.target_mode = TARGET_MODES[target_mode]
    return p


def check_bce_dice_mode(params: Optional[BCEDiceParams], k: int):
    """The library's rule, raised on the host as ValueError: "foreground" is the mode of K = 1 and its
    only one."""
    mode = _lib.BCE_TARGET_AUTO if params is None else params.target_mode
    if mode == _lib.BCE_TARGET_FOREGROUND and k != 1:
        raise ValueError(f"target_mode 'foreground' needs K = 1, the logits have K = {k}")
    if mode == _lib.BCE_TARGET_ONEHOT and k == 1:
        raise ValueError("K = 1 has the target mode 'foreground' only")


class BCEDiceFunction(_SumsLossFunction):
    """Sigmoid BCE + soft Dice (eunet_bce_dice_fwd / _bwd, with a pixel_weight eunet_bce_dice_fwd_w / _bwd_w)."""
    what, n_parts = "bce_dice_loss", 2
    sums_len, workspace_bytes = staticmethod(ops.bce_dice_sums_len), staticmethod(ops.bce_dice_workspace_bytes)
    fwd, bwd = staticmethod(ops.bce_dice_fwd), staticmethod(ops.bce_dice_bwd)
    fwd_w, bwd_w = staticmethod(ops.bce_dice_fwd_w), staticmethod(ops.bce_dice_bwd_w)

    @classmethod
    def check(cls, logits, params):
        check_bce_dice_mode(params, logits.shape[1])


def bce_dice_loss(logits: torch.Tensor, target: torch.Tensor, return_parts: bool = False,
                  params: Optional[BCEDiceParams] = None, validate: bool = False, track_targets: bool = True,
                  pixel_weight: Optional[torch.Tensor] = None):
    """Sigmoid BCE + soft Dice: logits [N,K,H,W] (K = 1..3, N <= 64), target [N,H,W] ->
    w_bce BCE + w_dice (1/N) sum_n dice_n (params: None = make_bce_dice_params()); parts [N,2] =
    (bce_n, dice_n).  Pixels at ignore_index count nowhere; other invalid targets count nowhere either
    and are reported by check_targets() (at once with validate=True).  pixel_weight (float32 [N,H,W]) multiplies
    bce(x,t)_c in BCE and bce_n; the denominators and the Dice terms are untouched and it takes no gradient."""
    if pixel_weight is not None:
        _check_pixel_weight(pixel_weight, logits, target, "bce_dice_loss")
    loss, parts = BCEDiceFunction.apply(logits, target, params, track_targets, pixel_weight)
    if validate:
        check_targets()
    return (loss, parts) if return_parts else loss


class BCEDiceLoss(nn.Module):
    """bce_dice_loss with its configuration held as attributes (make_bce_dice_params' keywords): set them
    at any time, the next call reads them."""

    def __init__(self, pos_weight=None, class_weight=None, dice_weight=None, w_bce: float = 1.0,
                 w_dice: float = 1.0, smooth: float = 1e-6, ignore_index: Optional[int] = None,
                 target_mode: Optional[str] = None):
        super().__init__()
        self.pos_weight = pos_weight
        self.class_weight = class_weight
        self.dice_weight = dice_weight
        self.w_bce = w_bce
        self.w_dice = w_dice
        self.smooth = smooth
        self.ignore_index = ignore_index
        self.target_mode = target_mode

    def params(self, num_classes: Optional[int] = None) -> BCEDiceParams:
        """The attributes as eunet_bce_dice_params; with num_classes the target mode is checked against it
        and the default mode is resolved for it."""
        p = make_bce_dice_params(pos_weight=self.pos_weight, class_weight=self.class_weight,
                                 dice_weight=self.dice_weight, w_bce=self.w_bce, w_dice=self.w_dice,
                                 smooth=self.smooth, ignore_index=self.ignore_index, target_mode=self.target_mode)
        if num_classes is not None:
            check_bce_dice_mode(p, num_classes)
            if p.target_mode == _lib.BCE_TARGET_AUTO:
                p.target_mode = _lib.BCE_TARGET_FOREGROUND if num_classes == 1 else _lib.BCE_TARGET_ONEHOT
        return p

    def forward(self, logits, target, pixel_weight=None):
        return bce_dice_loss(logits, target, params=self.params(logits.shape[1]), pixel_weight=pixel_weight)


# ---- boundary (surface) loss (csrc/sdf.hip; Kervadec et al., MIDL 2019; include/eunet.h holds the definition) ----
def _check_boundary_args(logits, dist, activation, class_weight, what: str):
    """The rules of boundary_loss that need no device, raised as ValueError; returns the K class weights."""
    if activation not in ops.BOUNDARY_ACTIVATIONS:
        raise ValueError(f"{what}: activation must be 'softmax' or 'sigmoid', not {activation!r}")
    _check_logits_target(what, logits)
    if not logits.is_floating_point():
        raise ValueError(f"{what}: logits must be floating point, got {logits.dtype}")
    k = logits.shape[1]
    if not 1 <= k <= 3:
        raise ValueError(f"{what}: K must be 1..3, the logits have K = {k}")
    if activation == "softmax" and k == 1:
        raise ValueError(f"{what}: a softmax over K = 1 is constant; use activation='sigmoid'")
    if not isinstance(dist, torch.Tensor):
        raise ValueError(f"{what}: dist must be a tensor, got {type(dist).__name__}")
    if dist.requires_grad:
        raise ValueError(f"{what}: dist takes no gradient (requires_grad is set)")
    if dist.dtype != torch.float32:
        raise ValueError(f"{what}: dist must be float32, got {dist.dtype}")
    if dist.shape != logits.shape:
        raise ValueError(f"{what}: dist {tuple(dist.shape)} does not match logits {tuple(logits.shape)}")
    if dist.device != logits.device:
        raise ValueError(f"{what}: dist is on {dist.device}, the logits on {logits.device}")
    if not dist.is_contiguous():
        raise ValueError(f"{what}: dist must be contiguous")
    if class_weight is not None and not isinstance(class_weight, (int, float, torch.Tensor)) and len(class_weight) < k:
        raise ValueError(f"{what}: class_weight has {len(class_weight)} values for K = {k}")
    return _triple(class_weight, 1.0, "class_weight")


class BoundaryLossFunction(torch.autograd.Function):
    """sum w_c p_c dist_c / (N H W Kw) with p the softmax or the sigmoid of the logits (eunet_boundary_loss_fwd);
    the backward pass recomputes p and saves nothing but its inputs."""

    @staticmethod
    def forward(ctx, logits, dist, activation, cw):
        logits = logits.contiguous().float()
        _check_logits_target("boundary_loss", logits)
        _check_on_device("boundary_loss", logits)
        n, k, h, w = logits.shape
        dev = logits.device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        parts = torch.empty(n, dtype=torch.float32, device=dev)
        ws = torch.empty(ops.boundary_loss_workspace_bytes(n, h, w), dtype=torch.uint8, device=dev)
        ops.boundary_loss_fwd(logits, dist, activation, cw[0], cw[1], cw[2], loss, parts, ws)
        ctx.save_for_backward(logits, dist)
        ctx.conf = (activation, cw)
        ctx.mark_non_differentiable(parts)
        return loss, parts

    @staticmethod
    def backward(ctx, gloss, gparts):
        logits, dist = ctx.saved_tensors
        activation, cw = ctx.conf
        glog = torch.empty_like(logits)
        ops.boundary_loss_bwd(logits, dist, activation, cw[0], cw[1], cw[2], gloss.contiguous().float().reshape(1), glog)
        return glog, None, None, None


def boundary_loss(logits: torch.Tensor, dist: torch.Tensor, activation: str = "softmax", class_weight=None,
                  return_parts: bool = False):
    """The boundary loss: logits [N,K,H,W] (K = 2..3 for "softmax", 1..3 for "sigmoid", N <= 64), dist float32
    [N,K,H,W] (ops.signed_distance_map of the target, or any prepared map; it takes no gradient) ->
    sum_{n,c,x} w_c p_c(x) dist_c(x) / (N H W Kw), Kw = max(1, the number of non-zero class weights); parts [N] =
    the same per sample, so the loss is their mean.  class_weight: None (all 1), a scalar, or K values --
    (0, 1, 0) is the paper's idc = [1]."""
    cw = _check_boundary_args(logits, dist, activation, class_weight, "boundary_loss")
    loss, parts = BoundaryLossFunction.apply(logits, dist, ops.BOUNDARY_ACTIVATIONS[activation], tuple(cw))
    return (loss, parts) if return_parts else loss


class BoundaryLoss(nn.Module):
    """weight * boundary_loss(logits, dist) with its configuration held as attributes: set them at any time (the
    paper raises the weight over the epochs), the next call reads them."""

    def __init__(self, activation: str = "softmax", class_weight=None, weight: float = 1.0):
        super().__init__()
        self.activation = activation
        self.class_weight = class_weight
        self.weight = weight

    def forward(self, logits, dist):
        return self.weight * boundary_loss(logits, dist, activation=self.activation, class_weight=self.class_weight)


# ---- Lovasz-Softmax and Lovasz hinge (csrc/lovasz.hip; Berman et al., CVPR 2018; include/eunet.h holds the definition)
def _lovasz_classes(classes, activation: str, k: int, what: str):
    """classes -> (classes_mode, class_mask) of eunet_lovasz_fwd.  None: "present" for softmax and "all" for hinge
    (Berman's two defaults)."""
    if classes is None:
        classes = "present" if activation == "softmax" else "all"
    if isinstance(classes, str):
        if classes not in ("present", "all"):
            raise ValueError(f"{what}: classes must be 'present', 'all' or a sequence of class indices, not {classes!r}")
        return (_lib.LOVASZ_PRESENT if classes == "present" else _lib.LOVASZ_ALL), 0
    try:
        idx = [int(c) for c in classes]
    except TypeError:
        raise ValueError(f"{what}: classes must be 'present', 'all' or a sequence of class indices, not {classes!r}")
    if not idx or any(not 0 <= c < k for c in idx):
        raise ValueError(f"{what}: classes {list(classes)} must name at least one class of 0..{k - 1} and none beyond")
    mask = 0
    for c in idx:
        mask |= 1 << c
    return _lib.LOVASZ_LISTED, mask


class LovaszFunction(torch.autograd.Function):
    """eunet_lovasz_fwd / _bwd: apply(logits, target, activation, per_image, classes_mode, class_mask, ignore_index,
    track_targets) -> (loss, parts).  Saves logits, target, the forward's weights (the Lovasz gradient g at every
    element) and the per-segment factor table; parts takes no gradient."""

    @staticmethod
    def forward(ctx, logits, target, activation, per_image, classes_mode, class_mask, ignore_index, track_targets):
        n, k, h, w = logits.shape
        dev = logits.device
        s, l = ops.lovasz_segments(n, k, h, w, per_image)
        weights = torch.empty_like(logits)
        factor = torch.empty(s, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        parts = torch.empty(s, dtype=torch.float32, device=dev)
        bad = torch.empty(1, dtype=torch.float32, device=dev)
        ws = torch.empty(ops.lovasz_workspace_bytes(s, l), dtype=torch.uint8, device=dev)
        ops.lovasz_fwd(logits, target, activation, per_image, classes_mode, class_mask, ignore_index, weights, factor,
                       loss, parts, None, bad, ws)
        if track_targets:
            _record_bad(bad)
        ctx.save_for_backward(logits, target, weights, factor)
        ctx.conf = (activation, per_image)
        ctx.mark_non_differentiable(parts)
        return loss, parts

    @staticmethod
    def backward(ctx, gloss, gparts):
        logits, target, weights, factor = ctx.saved_tensors
        activation, per_image = ctx.conf
        glog = torch.empty_like(logits)
        ops.lovasz_bwd(logits, target, activation, per_image, weights, factor, gloss.contiguous().float().reshape(1),
                       glog)
        return glog, None, None, None, None, None, None, None


def lovasz_loss(logits: torch.Tensor, target: torch.Tensor, activation: str = "softmax", classes=None,
                per_image: bool = False, ignore_index: Optional[int] = None, return_parts: bool = False,
                validate: bool = False, track_targets: bool = True):
    """The Lovasz-Softmax (activation="softmax", K = 2..3) or Lovasz hinge ("hinge", K = 1..3, one binary problem per
    logit) loss: logits float32 [N,K,H,W] (N <= 64), target int64 [N,H,W], both contiguous on one GPU.  Per segment
    (a class over the batch, or with per_image a class of one sample) the errors are sorted descending and weighted
    by the gradient of the Jaccard extension; the loss is the mean over the selected segments (per_image: the mean
    over samples of each sample's mean).  classes: "present" (segments with foreground), "all" (segments with a
    valid pixel) or a sequence of class indices; None = "present" for softmax, "all" for hinge.  Pixels at
    ignore_index count nowhere; other invalid targets count nowhere either and are reported by check_targets() (at
    once with validate=True).  parts: float32 [S] segment losses, NaN where a segment was not selected."""
    ign = ops._check_lovasz_args(logits, target, activation, ignore_index, "lovasz_loss",
                                 more=lambda: _lovasz_classes(classes, activation, logits.shape[1], "lovasz_loss"))
    mode, mask = _lovasz_classes(classes, activation, logits.shape[1], "lovasz_loss")
    loss, parts = LovaszFunction.apply(logits, target, ops.LOVASZ_ACTIVATIONS[activation], bool(per_image), mode, mask,
                                       ign, track_targets)
    if validate:
        check_targets()
    return (loss, parts) if return_parts else loss


class LovaszLoss(nn.Module):
    """weight * lovasz_loss(logits, target) with its configuration held as attributes: set them at any time, the next
    call reads them."""

    def __init__(self, activation: str = "softmax", classes=None, per_image: bool = False,
                 ignore_index: Optional[int] = None, weight: float = 1.0):
        super().__init__()
        self.activation = activation
        self.classes = classes
        self.per_image = per_image
        self.ignore_index = ignore_index
        self.weight = weight

    def forward(self, logits, target):
        return self.weight * lovasz_loss(logits, target, activation=self.activation, classes=self.classes,
                                         per_image=self.per_image, ignore_index=self.ignore_index)


def _as_pixels(inputs: torch.Tensor, targets: torch.Tensor):
    """[N,K,*] logits / [N,*] targets -> [1,K,1,P] / [1,1,P] (pixel-mean losses only)."""
    if inputs.dim() < 2:
        raise ValueError(f"expected [N, C, ...] logits, got {tuple(inputs.shape)}")
    k = inputs.shape[1]
    if targets.shape != inputs.shape[:1] + inputs.shape[2:]:
        raise ValueError(f"target {tuple(targets.shape)} does not match input {tuple(inputs.shape)}")
    lg = inputs.float().movedim(1, -1).reshape(-1, k).t().reshape(1, k, 1, -1)
    return lg, targets.reshape(1, 1, -1)


class FocalLoss(nn.Module):
    """train_eval.FocalLoss (train_eval.py:28-60): mean over all pixels of
    alpha_t (1-pt)^gamma ce, ce = F.cross_entropy(inputs, targets, weight=class_weights,
    ignore_index, reduction='none'), pt = exp(-ce).  inputs [N,K,...] (K <= 3) on the GPU."""

    def __init__(self, alpha: Union[None, float, Sequence[float], torch.Tensor] = None, gamma: float = 2.0,
                 ignore_index: Optional[int] = None, class_weights: Optional[torch.Tensor] = None):
        super().__init__()
        self.alpha = alpha
        self.gamma = gamma
        self.ignore_index = ignore_index
        self.class_weights = class_weights

    def params(self) -> LossParams:
        return make_params(ce_weight=self.class_weights, alpha=self.alpha, gamma=self.gamma,
                           ignore_index=self.ignore_index, w_focal=1.0, w_dice=0.0, w_tversky=0.0)

    def forward(self, inputs, targets):
        lg, tg = _as_pixels(inputs, targets)
        return combined_loss(lg, tg, params=self.params())


class CrossEntropyLoss(nn.Module):
    """nn.CrossEntropyLoss(weight=...) as the reference Trainer builds it (train_eval.py:80):
    class-weighted mean of -log p_t (sum w_t nll / sum w_t), on the fused loss kernel."""

    def __init__(self, weight: Optional[torch.Tensor] = None, ignore_index: int = -100,
                 reduction: str = "mean"):
        super().__init__()
        if reduction != "mean":
            raise ValueError("only reduction='mean' (the reference's use) is built")
        self.weight = weight
        self.ignore_index = ignore_index

    def forward(self, inputs, targets):
        lg, tg = _as_pixels(inputs, targets)
        p = make_params(ce_weight=self.weight, alpha=None, gamma=0.0, ignore_index=self.ignore_index,
                        w_focal=1.0, w_dice=0.0, w_tversky=0.0, focal_norm=1)
        return combined_loss(lg, tg, params=p)


def dice_loss(pred, target, num_classes: int = 3):
    """Trainer.dice_loss (train_eval.py:134-157): classes range(num_classes), weights [1,15,8],
    mean over samples of each class term, then / num_classes."""
    w = [1.0, 15.0, 8.0]
    w = [w[c] if c < num_classes else 0.0 for c in range(3)]
    p = make_params(dice_weight=w, w_focal=0.0, w_dice=1.0, w_tversky=0.0, class_div=float(num_classes))
    return combined_loss(pred, target, params=p, track_targets=False)


def tversky_loss(pred, target, num_classes: int = 3, alpha: float = 0.7):
    """Trainer.tversky_loss (train_eval.py:159-181): weights [1,12,6], Tversky alpha."""
    w = [1.0, 12.0, 6.0]
    w = [w[c] if c < num_classes else 0.0 for c in range(3)]
    p = make_params(tversky_weight=w, tversky_alpha=alpha, w_focal=0.0, w_dice=0.0, w_tversky=1.0,
                    class_div=float(num_classes))
    return combined_loss(pred, target, params=p, track_targets=False)


__all__ = ["combined_loss", "consistency_loss", "check_targets", "make_params", "reference_params", "FocalLoss",
           "CrossEntropyLoss", "dice_loss", "tversky_loss", "make_bce_dice_params", "BCEDiceFunction", "bce_dice_loss",
           "BCEDiceLoss", "BoundaryLossFunction", "boundary_loss", "BoundaryLoss", "LovaszFunction", "lovasz_loss",
           "LovaszLoss"]
