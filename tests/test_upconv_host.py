"""upsample="transpose" on the host: the parameter schema, the data-parallel gradient order, the argument
checks, the C-ABI surface, and the fp64 restatement (tests/_upconv_ref.py) against plain torch.nn modules."""
import os
import re

import pytest
import torch
import torch.nn as nn

import _upconv_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("eunet_upconv2x2_packed_bytes", "eunet_upconv2x2_pack", "eunet_bnrelu_upconv2x2_fwd",
           "eunet_upconv2x2_dgrad", "eunet_upconv2x2_wgrad_splits", "eunet_upconv2x2_wgrad")
UP_KEYS = [f"model.{u}.{w}" for u in ("up4", "up3", "up2") for w in ("weight", "bias")]


@pytest.mark.parametrize("name,count", [("enhanced_unet", 9167942), ("unet", 9165827)])
def test_transpose_schema_and_parameter_count(name, count):
    """Keys = the extended spec (up4 / up3 / up2 behind model.dec1.bias); counts = the pinned bilinear ones
    (7 790 790 / 7 788 675) + sum(4 C^2 + C) over C = 512, 256, 128 = 1 377 152."""
    from eunet.models import get_model
    m = get_model(name, upsample="transpose")
    spec = U.state_spec(name, 64, 3, 3)
    assert list(m.state_dict().keys()) == [k for k, _, _ in spec]
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(s) for k, s, _ in spec}
    assert sum(p.numel() for p in m.parameters()) == count
    assert count - {"enhanced_unet": 7790790, "unet": 7788675}[name] == sum(4 * c * c + c for c in (512, 256, 128))
    keys = list(m.state_dict().keys())
    at = keys.index("model.dec1.bias")
    assert keys[at + 1:at + 7] == UP_KEYS
    # the default stays the reference's schema
    m0 = get_model(name)
    assert [k for k in keys if k not in UP_KEYS] == list(m0.state_dict().keys())
    assert m0.backward_param_order() is None and m0.upsample == "bilinear"


@pytest.mark.parametrize("name", ["enhanced_unet", "unet"])
def test_backward_param_order_is_the_engines(name):
    from eunet.dp import backward_order
    from eunet.models import get_model
    m = get_model(name, num_classes=2, in_channels=1, base_ch=16, upsample="transpose")
    order = m.backward_param_order()
    names = [n for n, _ in m.named_parameters()]
    assert sorted(order) == sorted(names) and len(set(order)) == len(order)
    assert backward_order(m) == order
    blocks = []
    for n in order:
        b = n.split(".")[0] if n.startswith("enhance.") else n.split(".")[1]
        if not blocks or blocks[-1] != b:
            blocks.append(b)
    want = ["dec1", "dec2", "up2", "dec3", "up3", "dec4", "up4", "enc4", "enc3", "enc2", "enc1"]
    assert blocks == (["enhance"] if name == "enhanced_unet" else []) + want
    pre = "model.dec3."
    assert [n[len(pre)] for n in order if n.startswith(pre)] == ["4", "4", "3", "3", "1", "1", "0", "0"]


def test_bad_values_raise():
    from eunet import EunetError
    from eunet.models import EnhancedUNet, UNet, get_model
    for bad in ("nearest", "Transpose", "", None):
        with pytest.raises(ValueError):
            get_model("enhanced_unet", upsample=bad)
        with pytest.raises(ValueError):
            UNet(upsample=bad)
    with pytest.raises(ValueError, match="not built"):
        EnhancedUNet(dual_branch=True, upsample="transpose")
    for name in ("enhanced_unet", "unet"):
        m = get_model(name, num_classes=2, in_channels=1, base_ch=16, upsample="transpose")
        with pytest.raises(EunetError):
            m(torch.rand(1, 1, 32, 32))


def test_checkpoint_compatibility_with_bilinear_models():
    """A bilinear state_dict loads into a transpose model with strict=False (up* keep their initialisation);
    strict=True fails on exactly the six missing up* keys."""
    from eunet.models import get_model
    src = get_model("enhanced_unet", num_classes=2, in_channels=1, base_ch=16)
    dst = get_model("enhanced_unet", num_classes=2, in_channels=1, base_ch=16, upsample="transpose")
    init = {k: dst.state_dict()[k].clone() for k in UP_KEYS}
    res = dst.load_state_dict(src.state_dict(), strict=False)
    assert sorted(res.missing_keys) == sorted(UP_KEYS) and not res.unexpected_keys
    sd = dst.state_dict()
    assert all(torch.equal(sd[k], v) for k, v in src.state_dict().items())
    assert all(torch.equal(sd[k], init[k]) for k in UP_KEYS)
    with pytest.raises(RuntimeError) as e:
        dst.load_state_dict(src.state_dict(), strict=True)
    assert all(k in str(e.value) for k in UP_KEYS)


def test_c_abi_surface():
    """Declared (in the header's declaration style, with the formula and the north-star citation), exported,
    bound, and registered with the dispatcher."""
    from eunet import _lib, ops
    src = open(os.path.join(ROOT, "include", "eunet.h")).read()
    declared = set(re.findall(r"^\s*int\s+(eunet_\w+)\s*\(", src, flags=re.M))
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES and hasattr(lib, s), s
    at = src.index("eunet_upconv2x2_packed_bytes")
    comment = src[src.rindex("/*", 0, at):at]
    assert "BASELINE.json" in comment and "north_star" in comment and "No reference line" in comment
    assert "W[ci,co,a,b]" in comment and "relu(fmaf(y, scale, shift))" in comment
    assert "7 upconv" in src  # the debug build's unit list
    for op in ("upconv2x2_pack", "bnrelu_upconv2x2", "upconv2x2_dgrad", "upconv2x2_wgrad"):
        assert op in ops.DISPATCHED, op


def test_wgrad_split_count_covers_every_tile():
    """Host-only (descriptors, nothing dereferenced): 1 <= splits <= pixel stages, none empty, partials <= 256 MiB."""
    import ctypes
    from eunet import _lib
    lib = _lib.load()
    for n, h, w, c, dtc, stage in [(1, 1, 1, 32, _lib.EUNET_BF16, 64), (1, 7, 9, 512, _lib.EUNET_F32, 32),
                                   (4, 512, 512, 128, _lib.EUNET_BF16, 64), (4, 128, 128, 512, _lib.EUNET_BF16, 64),
                                   (2, 3, 5, 96, _lib.EUNET_F32, 32)]:
        y = _lib.Act(0x1000, n, h, w, c, c, 0, dtc)
        s = ctypes.c_int()
        assert lib.eunet_upconv2x2_wgrad_splits(ctypes.byref(y), dtc, ctypes.byref(s)) == 0
        stages = -(-(n * h * w) // stage)
        assert 1 <= s.value <= stages
        per = -(-stages // s.value)
        assert -(-stages // per) == s.value
        assert s.value * 4 * c * c * 4 <= 256 << 20


# ---- the restatement against plain torch.nn --------------------------------------------------------------
def _dc(cin, cout):
    return nn.Sequential(nn.Conv2d(cin, cout, 3, padding=1), nn.BatchNorm2d(cout), nn.ReLU(),
                         nn.Conv2d(cout, cout, 3, padding=1), nn.BatchNorm2d(cout), nn.ReLU())


class _Plain(nn.Module):
    """The transpose-upsample network as plain modules, named as the state_dict names them."""

    def __init__(self, name, b, cin, K):
        super().__init__()
        m = nn.Module()
        m.enc1, m.enc2, m.enc3, m.enc4 = _dc(cin, b), _dc(b, 2 * b), _dc(2 * b, 4 * b), _dc(4 * b, 8 * b)
        m.dec4, m.dec3, m.dec2 = _dc(12 * b, 4 * b), _dc(6 * b, 2 * b), _dc(3 * b, b)
        m.dec1 = nn.Conv2d(b, K, 1)
        m.up4, m.up3, m.up2 = (nn.ConvTranspose2d(c, c, 2, stride=2) for c in (8 * b, 4 * b, 2 * b))
        self.model = m
        if name == "enhanced_unet":
            self.enhance = nn.Sequential(nn.Conv2d(K, 64, 3, padding=1), nn.BatchNorm2d(64), nn.ReLU(), nn.Conv2d(64, K, 1))
        self.pool = nn.MaxPool2d(2)
        self.up = nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False)

    def forward(self, x):
        m = self.model
        e1 = m.enc1(x)
        e2 = m.enc2(self.pool(e1))
        e3 = m.enc3(self.pool(e2))
        e4 = m.enc4(self.pool(e3))
        d4 = m.dec4(torch.cat([m.up4(e4), e3], 1))
        d3 = m.dec3(torch.cat([m.up3(d4), e2], 1))
        d2 = m.dec2(torch.cat([m.up2(d3), e1], 1))
        u = m.dec1(self.up(d2))
        return u + self.enhance(u) if hasattr(self, "enhance") else u


@pytest.mark.parametrize("name", ["enhanced_unet", "unet"])
def test_restatement_equals_plain_modules(name):
    """Forward, loss, every parameter gradient and the BN running statistics of the restatement equal a plain
    torch.nn module with the same weights to 1e-10 (fp64, train mode), and the eval forward as well."""
    b, cin, K = 16, 1, 2
    g = torch.Generator().manual_seed(5)
    x = torch.rand(2, cin, 32, 32, generator=g, dtype=torch.float64)
    msk = torch.randint(0, K, (2, 32, 32), generator=g)
    net = _Plain(name, b, cin, K).double()
    net.load_state_dict(U.formula_weights(name, b, cin, K))
    net.train()
    out = net(x)
    loss = U.batch_loss(name, out, msk)
    loss.backward()
    S = U.formula_weights(name, b, cin, K)
    for k in S:
        if S[k].is_floating_point() and "running" not in k:
            S[k].requires_grad_(True)
    out_r = U.forward(name, S, x, True)
    loss_r = U.batch_loss(name, out_r, msk)
    loss_r.backward()

    def close(a, r):
        return float((a - r).abs().max()) <= 1e-10 * max(1.0, float(r.abs().max()))

    assert close(out.detach(), out_r.detach()) and close(loss.detach(), loss_r.detach())
    for k, p in net.named_parameters():
        assert close(p.grad, S[k].grad), k
    assert all(float(net.get_parameter(k).grad.abs().max()) > 0 for k in ("model.up4.weight", "model.up2.bias"))
    for k, v in net.state_dict().items():
        if "running" in k:
            assert close(v, S[k]), k
    net.eval()
    with torch.no_grad():
        assert close(net(x), U.forward(name, S, x, False))
