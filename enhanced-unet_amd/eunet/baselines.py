"""Engine of the reference's unet baseline, which is made of the library's ops.

unet (models.py:175-243, SMP-absent BasicUNet) is the trunk UNetEngine already runs, without the
enhance head: out = up2(dec1(d2)) at 2H, with dec1 commuted before the upsample as in the trunk, so
the tail is one K-channel kernel (ops.ktail_fwd: the x2 upsample, or -- for the training loop's
2H -> H resize, train_eval.py:306-310 -- its exact 2x2 mean).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from .engine import GradSink, UNetEngine, _e


class PlainUNetEngine(UNetEngine):
    """UNetEngine's trunk + the K-channel tail of UNet.forward (no enhance head)."""

    def forward(self, x: torch.Tensor, training: bool, want: str = "logits"):
        """x [N,Cin,H,W] -> out2h [N,K,2H,2W] ('out2h', the reference forward) or its 2x2 mean
        [N,K,H,W] ('logits')."""
        S = self.forward_trunk(x, training)
        N, H, W, K = S["N"], S["H"], S["W"], self.K
        if want == "out2h":
            out = _e((N, K, 2 * H, 2 * W), torch.float32, x.device)
            ops.ktail_fwd(ops.KTAIL_UP2, S["z"], out)
        else:
            out = _e((N, K, H, W), torch.float32, x.device)
            ops.ktail_fwd(ops.KTAIL_SMOOTH, S["z"], out)
        S["want"] = want
        return out, S

    def backward(self, S, g_out: torch.Tensor, sink: Optional[GradSink] = None):
        N, H, W, K = S["N"], S["H"], S["W"], self.K
        dev = g_out.device
        sink = sink or GradSink(dev)
        gz = _e((N, H, W, K), torch.float32, dev)
        mode = ops.KTAIL_UP2 if S["want"] == "out2h" else ops.KTAIL_SMOOTH
        ops.ktail_bwd(mode, g_out.contiguous().float(), gz)
        self.backward_trunk(S, gz, sink)
        return sink.finish()
