"""CPU restatement of the reference's unet baseline (TEST INFRASTRUCTURE; imports nothing from the product).

  unet     models.py:175-243, SMP-absent BasicUNet: conv2d(_up2(trunk(...)), dec1) over the trunk of
           oracle/eunet_ref.py, with its pins= / record=

Parity with the reference is pinned by tests/golden/{unet,step_unet}_c3k3.npz
(tests/test_baselines_host.py).  Trainer row: train_eval.py:102-107, 118-119 (the default row).
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import eunet_ref as R
from oracle.weights import formula_state_dict

# train_eval.py:82-119: (dice, focal, tversky) weights and base learning rate
TABLE = {"unet": dict(w=(1.5, 1.5, 0.5), lr=2e-3)}


# ---- parameter schemas ------------------------------------------------------------------------------
def unet_spec(base=64, in_ch=3, num_classes=3):
    """state_spec rows of BasicUNet: the Enhanced-UNet schema without the enhance head."""
    return [r for r in R.state_spec(base, in_ch, num_classes) if not r[0].startswith("enhance.")]


SPECS = {"unet": unet_spec}


def formula_weights(name, base=64, in_ch=3, num_classes=3, dtype=torch.float64) -> Dict[str, torch.Tensor]:
    sd = formula_state_dict(SPECS[name](base, in_ch, num_classes))
    return {k: (torch.tensor(0, dtype=torch.long) if k.endswith("num_batches_tracked")
                else torch.from_numpy(np.asarray(v)).to(dtype)) for k, v in sd.items()}


# ---- forwards ---------------------------------------------------------------------------------------
def unet_forward(S, x, training=True, pins=None, record=None):
    """x [B,C,H,W] -> logits [B,K,2H,2W] (models.py:227-237)."""
    d2, _ = R.trunk(S, x, training, pins, record=record)
    return F.conv2d(R._up2(d2), S["model.dec1.weight"], S["model.dec1.bias"])


FORWARDS = {"unet": unet_forward}


def forward(name, S, x, training=True, pins=None, record=None):
    return FORWARDS[name](S, x, training, pins, record)


# ---- loss and step (train_eval.py:183-197, 236-353 with the rows of :82-119) ------------------------
def combined_loss(name, logits, target):
    _, parts = R.combined_loss(logits, target, parts=True)
    wd, wf, wt = TABLE[name]["w"]
    return wf * parts["focal"] + wd * parts["dice"] + wt * parts["tversky"]


def batch_loss(name, out, target):
    """train_eval.py:262-337: per-sample bilinear resize to the mask size where the sizes differ
    (unet's 2H output), combined loss with the model's weights, / B."""
    B = out.shape[0]
    H, W = target.shape[-2:]
    loss = 0.0
    for i in range(B):
        o = out[i]
        if o.shape[1:] != (H, W):
            o = F.interpolate(o[None], size=(H, W), mode="bilinear", align_corners=False)[0]
        loss = loss + combined_loss(name, o, target[i])
    return loss / B


def lr_trajectory(name, total_epochs):
    return R.lr_trajectory(total_epochs, lr=TABLE[name]["lr"])


def step(name, S, images, masks, total_epochs=50):
    """One Trainer.train_epoch on one batch after warmup_scheduler.step(): (lr, loss, grads before the
    clip-scaled AdamW step, S updated in place)."""
    keys = [k for k in S if S[k].is_floating_point() and "running" not in k]
    for k in keys:
        S[k].requires_grad_(True)
    params = [S[k] for k in keys]
    opt = torch.optim.AdamW(params, lr=TABLE[name]["lr"], weight_decay=1e-4, betas=(0.9, 0.999))
    warm = torch.optim.lr_scheduler.LinearLR(opt, start_factor=0.001, end_factor=1.0,
                                             total_iters=max(1, min(5, total_epochs // 6)))
    warm.step()
    lr = opt.param_groups[0]["lr"]
    images, masks = R.pad32(images, masks)
    loss = batch_loss(name, forward(name, S, images, True), masks)
    loss.backward()
    torch.nn.utils.clip_grad_norm_(params, max_norm=1.0)
    grads = {k: S[k].grad.detach().clone() for k in keys}
    opt.step()
    return lr, float(loss.item()), grads
