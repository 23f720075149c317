"""fp64 restatement of the transpose-upsample trunk and of both models built on it (TEST INFRASTRUCTURE;
imports nothing from the product).

upsample="transpose" has no reference counterpart (BASELINE.json north_star names the option), so there is
no golden fixture: the yardstick is this restatement in fp64 PyTorch on the CPU.  It is composed from
oracle/eunet_ref.py's own pieces (_double_conv, _pool, _bn, _relu, combined_loss, batch_loss, with pins= /
record= passed through); F.conv_transpose2d(kernel 2, stride 2, bias) stands where its trunk calls _up2 for
the three trunk upsamples.  The last upsample (behind dec2, in front of dec1) stays bilinear.
tests/test_upconv_host.py pins it against plain torch.nn modules.
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch
import torch.nn.functional as F

import _baseline_ref as BR
from oracle import eunet_ref as R
from oracle.weights import formula_state_dict

UPS = ("up4", "up3", "up2")  # registration order behind dec1; C = 8b, 4b, 2b


def up_rows(base: int):
    """The six extra state_dict rows in registration order.  fan_in = C: every output element sums C
    products (one tap per output pixel), so the formula weights keep the activation scale."""
    rows = []
    for nm, c in zip(UPS, (8 * base, 4 * base, 2 * base)):
        rows.append((f"model.{nm}.weight", (c, c, 2, 2), c))
        rows.append((f"model.{nm}.bias", (c,), c))
    return rows


def state_spec(name: str, base: int = 64, in_ch: int = 3, num_classes: int = 3):
    """oracle state_spec (enhanced_unet) / its head-less part (unet) with the up* rows behind model.dec1.bias."""
    spec = R.state_spec(base, in_ch, num_classes)
    if name == "unet":
        spec = [r for r in spec if not r[0].startswith("enhance.")]
    elif name != "enhanced_unet":
        raise ValueError(name)
    at = [r[0] for r in spec].index("model.dec1.bias") + 1
    return spec[:at] + up_rows(base) + spec[at:]


def formula_weights(name, base=64, in_ch=3, num_classes=3, dtype=torch.float64) -> Dict[str, torch.Tensor]:
    sd = formula_state_dict(state_spec(name, base, in_ch, num_classes))
    return {k: (torch.tensor(0, dtype=torch.long) if k.endswith("num_batches_tracked")
                else torch.from_numpy(np.asarray(v)).to(dtype)) for k, v in sd.items()}


def _upT(S, nm, h, prefix="model."):
    return F.conv_transpose2d(h, S[f"{prefix}{nm}.weight"], S[f"{prefix}{nm}.bias"], stride=2)


def trunk(S, x, training, pins=None, prefix="model.", record=None):
    """oracle trunk() with the three trunk upsamples learned: d2."""
    pins = pins or {}
    dc = lambda nm, h: R._double_conv(S, nm, h, training, pins, prefix, record)  # noqa: E731
    e1 = dc("enc1", x)
    e2 = dc("enc2", R._pool(e1, pins.get("pool1")))
    e3 = dc("enc3", R._pool(e2, pins.get("pool2")))
    e4 = dc("enc4", R._pool(e3, pins.get("pool3")))
    d4 = dc("dec4", torch.cat([_upT(S, "up4", e4, prefix), e3], 1))
    d3 = dc("dec3", torch.cat([_upT(S, "up3", d4, prefix), e2], 1))
    d2 = dc("dec2", torch.cat([_upT(S, "up2", d3, prefix), e1], 1))
    return d2


def forward(name, S, x, training=True, pins=None, record=None):
    """x [B,C,H,W] -> logits [B,K,2H,2W] of 'enhanced_unet' / 'unet' built with upsample='transpose'.
    pins: the trunk's branch configuration (oracle trunk()) and, optionally, the head ReLU's ('enhance.1');
    record: receives every ReLU input, the head's included."""
    d2 = trunk(S, x, training, pins, record=record)
    u = F.conv2d(R._up2(d2), S["model.dec1.weight"], S["model.dec1.bias"])  # the last upsample stays bilinear
    if name == "unet":
        return u
    h = F.conv2d(u, S["enhance.0.weight"], S["enhance.0.bias"], padding=1)
    h = R._bn(S, "enhance.1", h, training)
    if record is not None:  # the head's ReLU input too: a pinned 'enhance.1' is audited like the trunk's sites
        record["enhance.1"] = h.detach()
    h = R._relu(h, (pins or {}).get("enhance.1"))
    return u + F.conv2d(h, S["enhance.3.weight"], S["enhance.3.bias"])


def batch_loss(name, out, target):
    """The model's Trainer row: oracle batch_loss (enhanced_unet) / the unet row of tests/_baseline_ref.py."""
    return R.batch_loss(out, target) if name == "enhanced_unet" else BR.batch_loss(name, out, target)


def grads(name, base, cin, K, x, msk, dtype, pins=None, record=None):
    """(S with .grad on every parameter, loss) of one training forward + backward."""
    S = formula_weights(name, base, cin, K, dtype=dtype)
    for k in S:
        if S[k].is_floating_point() and "running" not in k:
            S[k].requires_grad_(True)
    loss = batch_loss(name, forward(name, S, x.to(dtype), True, pins=pins, record=record), msk)
    loss.backward()
    return S, loss
