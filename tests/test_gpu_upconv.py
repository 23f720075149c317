"""upconv.hip kernel by kernel through the C-ABI against fp64 PyTorch (GPU only).

Bounds are tests/test_gpu_ops.py's gate(): fp32 1e-4 max|ref|; bf16 per element 2^-8 |ref| + 1e-5 max|ref|
against the fp64 result of the operands as the kernels see them (inputs and weights rounded to bf16, the
BN+ReLU operand d formed by that file's tf()).  The weight and bias gradient use the same gate, as its
test_conv3x3_dgrad_wgrad does.

Shapes: C = 32 (the smallest the models produce), 96 (no multiple of 64; 4C = 384 = three column tiles, the
second of which straddles two output parities), 128, 512 (the longest K loop, the widest 4C); pixel counts
M = N h w around the kernels' pixel tile UT = 128 rows per block (127 / 128 / 129: one below, equal, one
above -- two blocks with a one-row second tile) and around the weight gradient's pixel stage (64 bf16 /
32 fp32 pixels: 30, 63, 65, 127 .. 129), plus M = 1, where the split count the weight gradient would like
(512 blocks' worth) exceeds its single pixel stage.  out and g live in channels [0, C) of a buffer with
ctot = C + C/2 whose other channels hold a sentinel.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from test_gpu_ops import DEV, gate, nchw, nhwc, tf

pytestmark = pytest.mark.gpu

UT = 128  # upconv.hip UT: the forward's / data gradient's pixel tile (GEMM rows per block)
STAGE = {torch.bfloat16: 64, torch.float32: 32}  # the weight gradient's pixel stage (upconv_kernel BK)
CS = (32, 96, 128, 512)
SHAPES = ((1, 1, 1), (2, 3, 5), (1, 7, 9), (1, 5, 13), (1, 1, UT - 1), (1, 8, UT // 8), (1, 3, 43))
SENTINEL = -1536.0  # exactly representable in bf16


def _ops():
    from eunet import ops
    return ops


_CASES = {}


def _case(C, shape, dt):
    """Operands (as the kernels see them) and the fp64 results of one (C, shape, dtype), computed once."""
    key = (C, shape, dt)
    if key in _CASES:
        return _CASES[key]
    N, h, w = shape
    g = torch.Generator().manual_seed(1000 * C + 100 * h + w + (7 if dt == torch.bfloat16 else 0))
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    y = rnd(N, h, w, C).to(dt).double()
    sc = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).float().double()
    sh = (rnd(C) * 0.3).float().double()
    W = (rnd(C, C, 2, 2) / math.sqrt(C)).to(dt).double()
    bias = rnd(C).float().double()
    gup = rnd(N, 2 * h, 2 * w, C).to(dt).double()
    d = nchw(tf(y, sc, sh, dt)).requires_grad_(True)
    Wt, bt = W.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    out = F.conv_transpose2d(d, Wt, bt, stride=2)
    out.backward(nchw(gup))
    ref = dict(y=y, sc=sc, sh=sh, W=W, bias=bias, gup=gup, out=nhwc(out.detach()), gd=nhwc(d.grad), dW=Wt.grad,
               db=bt.grad)
    _CASES[key] = ref
    return ref


def _view(vals, C, dt):
    """vals [N,H,W,C] in channels [0, C) of a sentinel-filled buffer with ctot = C + C/2."""
    N, H, Wd, _ = vals.shape
    buf = torch.full((N, H, Wd, C + C // 2), SENTINEL, dtype=dt, device=DEV)
    buf[..., :C] = vals.to(DEV, dt)
    return buf


def _untouched(buf, C):
    return bool((buf[..., C:] == SENTINEL).all())


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("C", CS)
def test_upconv_forward(C, shape, dt):
    ops = _ops()
    r = _case(C, shape, dt)
    N, h, w = shape
    wp = ops.upconv2x2_pack(r["W"].float().to(DEV), dt)
    out = torch.full((N, 2 * h, 2 * w, C + C // 2), SENTINEL, dtype=dt, device=DEV)
    ops.bnrelu_upconv2x2(ops.act(r["y"].to(DEV, dt)), r["sc"].float().to(DEV), r["sh"].float().to(DEV), wp,
                         r["bias"].float().to(DEV), ops.act(out, 0, C))
    torch.cuda.synchronize()
    assert _untouched(out, C), "channels outside the view were written"
    got = out[..., :C]
    print("fwd", C, shape, dt, "gate", gate(got, r["out"], dt))
    assert gate(got, r["out"], dt) <= 1.0
    for a in (0, 1):  # each output parity on its own (its own weight slice, the bias in all four)
        for b in (0, 1):
            assert gate(got[:, a::2, b::2], r["out"][:, a::2, b::2], dt) <= 1.0, (a, b)
    # the bias really is in every parity: without it the result is off by O(|bias|)
    nob = r["out"] - r["bias"]
    assert all(gate(got[:, a::2, b::2], nob[:, a::2, b::2], dt) > 1.0 for a in (0, 1) for b in (0, 1))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("C", CS)
def test_upconv_dgrad(C, shape, dt):
    ops = _ops()
    r = _case(C, shape, dt)
    N, h, w = shape
    wp = ops.upconv2x2_pack(r["W"].float().to(DEV), dt)
    gbuf = _view(r["gup"], C, dt)
    gd = torch.full((N, h, w, C + C // 2), SENTINEL, dtype=dt, device=DEV)
    ops.upconv2x2_dgrad(ops.act(gbuf, 0, C), wp, ops.act(gd, 0, C))
    torch.cuda.synchronize()
    assert _untouched(gd, C) and _untouched(gbuf, C)
    print("dgrad", C, shape, dt, "gate", gate(gd[..., :C], r["gd"], dt))
    assert gate(gd[..., :C], r["gd"], dt) <= 1.0


def _wgrad(ops, r, C, dt, gbuf):
    ya = ops.act(r["y"].to(DEV, dt))
    ns = ops.upconv2x2_wgrad_splits(ya, dt)
    dwp = torch.full((ns * 4 * C * C,), float("nan"), device=DEV)
    dbp = torch.full((ns * 4 * C,), float("nan"), device=DEV)
    ops.upconv2x2_wgrad(ya, r["sc"].float().to(DEV), r["sh"].float().to(DEV), ops.act(gbuf, 0, C), dwp, dbp, ns)
    dw = torch.empty(C, C, 2, 2, device=DEV)
    db = torch.empty(C, device=DEV)
    ops.wgrad_reduce(dwp, None, ns, C, C, 4, dw, None)
    ops.colsum(dbp, ns * 4, C, db)
    return ns, dw, db


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("C", CS)
def test_upconv_wgrad(C, shape, dt):
    from eunet import EunetError
    ops = _ops()
    r = _case(C, shape, dt)
    N, h, w = shape
    gbuf = _view(r["gup"], C, dt)
    ns, dw, db = _wgrad(ops, r, C, dt, gbuf)
    ns2, dw2, db2 = _wgrad(ops, r, C, dt, gbuf)
    torch.cuda.synchronize()
    stages = -(-(N * h * w) // STAGE[dt])
    assert 1 <= ns <= stages and ns2 == ns
    if N * h * w == 1:
        assert ns == 1  # the split the launch would like exceeds the one pixel stage there is
    assert _untouched(gbuf, C)
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "two runs must be bit-identical"
    print("wgrad", C, shape, dt, "splits", ns, "gates", gate(dw, r["dW"], dt), gate(db, r["db"], dt))
    assert gate(dw, r["dW"], dt) <= 1.0
    assert gate(db, r["db"], dt) <= 1.0
    # a split count that is not the query's (here: more splits than pixel stages) is refused, not run
    bad = stages + 1
    with pytest.raises(EunetError):
        ops.upconv2x2_wgrad(ops.act(r["y"].to(DEV, dt)), r["sc"].float().to(DEV), r["sh"].float().to(DEV),
                            ops.act(gbuf, 0, C), torch.empty(bad * 4 * C * C, device=DEV), None, bad)


def test_upconv_forward_view_past_2_31_elements():
    """bf16, C = 32 in ctot = 48, h = w = 3360, N = 1: the output view has 6720^2 x 48 = 2 167 603 200 > 2^31
    elements.  Checked at the first, the last and 64 seeded output pixels against fp64 of those pixels only."""
    ops = _ops()
    C, ct, h = 32, 48, 3360
    dt = torch.bfloat16
    g = torch.Generator(device=DEV).manual_seed(11)
    y = torch.randn(1, h, h, C, generator=g, device=DEV, dtype=torch.float32).to(dt)
    gc = torch.Generator().manual_seed(12)
    sc = torch.rand(C, generator=gc) + 0.5
    sh = torch.randn(C, generator=gc) * 0.3
    W = (torch.randn(C, C, 2, 2, generator=gc) / math.sqrt(C)).to(dt).float()
    bias = torch.randn(C, generator=gc)
    out = torch.full((1, 2 * h, 2 * h, ct), SENTINEL, dtype=dt, device=DEV)
    assert out.numel() > 2 ** 31
    ops.bnrelu_upconv2x2(ops.act(y), sc.to(DEV), sh.to(DEV), ops.upconv2x2_pack(W.to(DEV), dt), bias.to(DEV),
                         ops.act(out, 0, C))
    torch.cuda.synchronize()
    pix = torch.randint(0, 2 * h, (64, 2), generator=gc).tolist() + [[0, 0], [2 * h - 1, 2 * h - 1]]
    worst = 0.0
    for Y, X in pix:
        d = tf(y[0, Y // 2, X // 2].double().cpu(), sc.double(), sh.double(), dt)
        ref = bias.double() + d @ W.double()[:, :, Y % 2, X % 2]
        got = out[0, Y, X].double().cpu()
        assert bool((got[C:] == SENTINEL).all()), (Y, X)
        worst = max(worst, gate(got[:C], ref, dt))
    print("2^31 view: worst gate over 66 pixels", worst)
    assert worst <= 1.0


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_unsupported_arguments_raise(dt):
    """C that is no multiple of 32, a channel-changing view, a wrong 2x shape and mixed dtypes are EunetError."""
    from eunet import EunetError
    ops = _ops()
    other = torch.float32 if dt == torch.bfloat16 else torch.bfloat16
    z = lambda *s, d=dt: torch.zeros(*s, dtype=d, device=DEV)  # noqa: E731
    f = lambda n: torch.zeros(n, device=DEV)  # noqa: E731
    for C in (48, 16, 40):
        with pytest.raises(EunetError):
            ops.upconv2x2_pack(torch.zeros(C, C, 2, 2, device=DEV), dt)
        wp = z(8 * C * C)
        with pytest.raises(EunetError):
            ops.bnrelu_upconv2x2(ops.act(z(1, 2, 2, C)), f(C), f(C), wp, f(C), ops.act(z(1, 4, 4, C)))
        with pytest.raises(EunetError):
            ops.upconv2x2_dgrad(ops.act(z(1, 4, 4, C)), wp, ops.act(z(1, 2, 2, C)))
        with pytest.raises(EunetError):
            ops.upconv2x2_wgrad(ops.act(z(1, 2, 2, C)), f(C), f(C), ops.act(z(1, 4, 4, C)), f(4 * C * C), None, 1)
    C = 32
    wp = ops.upconv2x2_pack(torch.zeros(C, C, 2, 2, device=DEV), dt)
    with pytest.raises(EunetError):  # 2x shape
        ops.bnrelu_upconv2x2(ops.act(z(1, 2, 2, C)), f(C), f(C), wp, f(C), ops.act(z(1, 4, 5, C)))
    with pytest.raises(EunetError):  # channel count changes
        ops.bnrelu_upconv2x2(ops.act(z(1, 2, 2, C)), f(C), f(C), wp, f(C), ops.act(z(1, 4, 4, 2 * C)))
    with pytest.raises(EunetError):  # dtype of the output
        ops.bnrelu_upconv2x2(ops.act(z(1, 2, 2, C)), f(C), f(C), wp, f(C), ops.act(z(1, 4, 4, C, d=other)))
    with pytest.raises(EunetError):  # packed for the other dtype
        ops.upconv2x2_dgrad(ops.act(z(1, 4, 4, C)), ops.upconv2x2_pack(torch.zeros(C, C, 2, 2, device=DEV), other),
                            ops.act(z(1, 2, 2, C)))
    with pytest.raises(EunetError):  # not a transposed-convolution weight
        ops.upconv2x2_pack(torch.zeros(C, C, 3, 3, device=DEV), dt)
    torch.cuda.synchronize()
