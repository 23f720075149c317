"""baselines.hip kernel by kernel against fp64 references (GPU only), with the buffers, sentinels and two-run
check of tests/test_gpu_bnpool.py and its upsample shapes.

ktail_fwd / ktail_bwd fp32, K = 1..3, both modes.  Forward |err| <= 1e-6 x the same linear combination of |z|
                      (weights are exact binary fractions; <= 9 fma / 4 products + 3 adds of fp32 roundings, 2^-24
                      each).  Backward: <ktail_fwd(z), g> = <z, ktail_bwd(g)> in fp64 to 1e-6 x sum|terms|, and
                      elementwise against autograd of the fp64 forward to 1e-6 x the adjoint of |g|.
                      h = 1 / w = 1 shapes have both edges in one row / column (doubled edge weights); 9 and 13
                      rows, 7 and 21 columns have interior and edge rows and several blocks of 256 threads.
"""
import pytest
import torch
import torch.nn.functional as F

import test_gpu_bnpool as BP
from test_gpu_bnpool import DEV, UP_SHAPES, Outs, _twice, nchw

pytestmark = pytest.mark.gpu


def _ops():
    from eunet import ops
    return ops


# ---- ktail --------------------------------------------------------------------------------------------------
UP2, SMOOTH = 0, 1


def _ktail_ref(mode, z_lo):
    """fp64 NHWC input -> NCHW output, as the header states the modes."""
    up = F.interpolate(nchw(z_lo), scale_factor=2, mode="bilinear", align_corners=False)
    return up if mode == UP2 else F.avg_pool2d(up, 2)


def _ktail_input(shape, K, seed):
    N, h, w = shape
    return torch.randn(N, h, w, K, generator=torch.Generator().manual_seed(seed)).double()


kt = pytest.mark.parametrize("mode", [UP2, SMOOTH], ids=["up2", "smooth"])


@kt
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("shape", UP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ktail_fwd(shape, K, mode):
    ops = _ops()
    N, h, w = shape
    s = 2 if mode == UP2 else 1
    z_lo = _ktail_input(shape, K, 1300 + 11 * N * h * w + K)

    def run():
        o = Outs()
        out = o.new((N, K, s * h, s * w))
        ops.ktail_fwd(mode, z_lo.float().to(DEV), out)
        o.check()
        return [out]

    (out,) = _twice(run)
    ref, mag = _ktail_ref(mode, z_lo), _ktail_ref(mode, z_lo.abs())
    err = (out.double() - ref).abs()
    print(f"ktail_fwd mode {mode}: worst err / (1e-6 mag) {float((err / (1e-6 * mag).clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= 1e-6 * mag).all())


@kt
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("shape", UP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ktail_bwd(shape, K, mode):
    ops = _ops()
    N, h, w = shape
    s = 2 if mode == UP2 else 1
    z_lo = _ktail_input(shape, K, 1700 + 11 * N * h * w + K)
    gen = torch.Generator().manual_seed(1900 + N * h * w + K)
    g = torch.randn(N, K, s * h, s * w, generator=gen).double()

    def run():
        o = Outs()
        gz_lo = o.new((N, h, w, K))
        ops.ktail_bwd(mode, g.float().to(DEV), gz_lo)
        o.check()
        return [gz_lo]

    gz_lo = _twice(run)[0].double()
    # the adjoint identity on the kernel's own forward: <fwd(z), g> = <z, bwd(g)>
    out = torch.empty(N, K, s * h, s * w, device=DEV)
    ops.ktail_fwd(mode, z_lo.float().to(DEV), out)
    lhs, rhs = float((out.double().cpu() * g).sum()), float((z_lo * gz_lo).sum())
    terms = float((_ktail_ref(mode, z_lo.abs()) * g.abs()).sum())
    print(f"ktail adjoint identity mode {mode}: |lhs - rhs| / (1e-6 terms) {abs(lhs - rhs) / (1e-6 * terms):.3f}")
    assert abs(lhs - rhs) <= 1e-6 * terms
    # against autograd of the fp64 forward
    zl = z_lo.clone().requires_grad_(True)
    (_ktail_ref(mode, zl) * g).sum().backward()
    za = z_lo.clone().requires_grad_(True)
    (_ktail_ref(mode, za) * g.abs()).sum().backward()  # the adjoint of |g|: sum of |terms| per element
    err = (gz_lo - zl.grad).abs()
    assert bool((err <= 1e-6 * za.grad).all()), float((err / (1e-6 * za.grad).clamp_min(1e-300)).max())


def test_ktail_rejects():
    ops, Err = _ops(), BP._err()
    z = torch.zeros(1, 3, 5, 3, device=DEV)
    ops.ktail_fwd(UP2, z, torch.empty(1, 3, 6, 10, device=DEV))
    ops.ktail_fwd(SMOOTH, z, torch.empty(1, 3, 3, 5, device=DEV))
    with pytest.raises(Err):  # K = 4
        ops.ktail_fwd(UP2, torch.zeros(1, 3, 5, 4, device=DEV), torch.empty(1, 4, 6, 10, device=DEV))
    with pytest.raises(Err):  # output of the other mode's size
        ops.ktail_fwd(UP2, z, torch.empty(1, 3, 3, 5, device=DEV))
    with pytest.raises(Err):  # not fp32
        ops.ktail_fwd(UP2, z.bfloat16(), torch.empty(1, 3, 6, 10, device=DEV))
    with pytest.raises(Err):  # unknown mode
        ops.ktail_fwd(2, z, torch.empty(1, 3, 3, 5, device=DEV))
    with pytest.raises(Err):  # gradient of the other mode's size
        ops.ktail_bwd(UP2, torch.zeros(1, 3, 3, 5, device=DEV), torch.empty(1, 3, 5, 3, device=DEV))
    with pytest.raises(Err):
        ops.ktail_bwd(SMOOTH, torch.zeros(1, 3, 6, 10, device=DEV), torch.empty(1, 3, 5, 3, device=DEV))
    torch.cuda.synchronize()
