"""sdf.hip, the boundary loss: eunet.losses.boundary_loss forward and backward at the edges of their launches.

bl_fwd_kernel reduces 1024 pixels of one sample per block (16-byte loads when H*W is a multiple of 4, scalar ones
otherwise), bl_finalize_kernel combines a sample's tiles (256 threads striding over them, then a 128-wide LDS tree) and
the batch's samples, bl_bwd_kernel is per pixel with the softmax recomputed.  The pixel count sits on either side of a
tile (1, 1023, 1024, 1025 px and 5x7: the scalar path four times, the vector path at 1024), one sample has 257 tiles
(513x512, the vector path, so the finalize's stride wraps).

Everything goes through boundary_loss(..., return_parts=True) and (loss * 3.7).backward().  There is no reference
implementation: the comparison is with tests/_sdf_ref.py, the definition of include/eunet.h restated in fp64 on the
fp32 inputs as stored (tests/test_sdf_host.py holds its gradient to a finite difference).

Value and parts: |got - ref| <= 1e-5 A, with A the restatement's sum of |summands| over the same denominator -- not
relative to |ref|, because the sum cancels by construction (the map has both signs).  Derivation: a few fp32
roundings per product, at most 4 K additions per thread, a 6-level wave tree and 4 wave partials before fp64 takes
over: about 2e-6 A, with a factor-5 margin.  Both bounds carry one absolute term, FLT_MIN = 2^-126, which comes from
the storage format alone: loss, parts and gradient are fp32, and where every logit of a sample is saturated (one
pixel at scale 100) the fp64 reference is a number like 1e-68 that no fp32 holds.  Gradients: the project's loss gates (tests/test_gpu_bce_dice.py), within
1e-4 of the largest reference gradient and per element within 1e-3 relative with a floor of 1e-3 of the largest."""
import itertools

import pytest
import torch

import _sdf_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
GSCALE = 3.7
WEIGHTS = [(1.0, 1.0, 1.0), (0.0, 1.0, 1.0), (0.0, 1.0, 0.0)]
MODES = [("sigmoid", 1), ("sigmoid", 2), ("sigmoid", 3), ("softmax", 2), ("softmax", 3)]


def _gpu(x32, d32, activation, cw):
    from eunet.losses import boundary_loss
    x = x32.to(DEV).requires_grad_(True)
    loss, parts = boundary_loss(x, d32.to(DEV), activation=activation, class_weight=cw, return_parts=True)
    (loss * GSCALE).backward()
    torch.cuda.synchronize()
    return loss.item(), parts.double().cpu(), x.grad.double().cpu()


FLT_MIN = 2.0 ** -126  # the smallest normal fp32


def _grad_close(name, got, ref):
    """tests/test_gpu_bce_dice.py's gates.  One term is added, from the number format and not from any run: the
    gradient is stored in fp32, which holds nothing below its normal range at full precision, so an error of up to
    FLT_MIN = 1.2e-38 is allowed in absolute terms.  It only matters where every logit of a case is saturated (1 and
    35 pixels at scale 100: a sigmoid gradient of exp(-200) is 1e-87 in the fp64 reference and 0 in any fp32)."""
    assert bool(torch.isfinite(got).all()), name
    scale = float(ref.abs().max())
    if scale == 0.0:
        assert float(got.abs().max()) == 0.0, name
        return 0.0, 0.0
    err = (got - ref).abs() - FLT_MIN
    mx = float(err.max()) / scale
    per = float((err / ref.abs().clamp_min(1e-3 * scale)).max())
    assert mx <= 1e-4, (name, mx)
    assert per <= 1e-3, (name, per)
    return mx, per


def _check(name, x32, d32, activation, cw):
    v_ref, p_ref, g_ref, a, p_a = S.boundary_loss(x32, d32, activation, cw, g=GSCALE)
    v, parts, g = _gpu(x32, d32, activation, cw)
    mx, per = _grad_close(name, g, g_ref)
    rel = abs(v - v_ref) / a if a else abs(v - v_ref)
    print(f"{name}: value {v:.8g} (ref {v_ref:.8g}, A {a:.4g}, err / A {rel:.2e}), grad err / max {mx:.2e}, "
          f"worst element {per:.2e}")
    assert v == v and abs(v) != float("inf"), name
    assert abs(v - v_ref) <= 1e-5 * a + FLT_MIN, (name, v, v_ref, a)
    assert parts.shape == p_ref.shape
    for n in range(p_ref.shape[0]):
        assert abs(float(parts[n]) - float(p_ref[n])) <= 1e-5 * float(p_a[n]) + FLT_MIN, \
            (name, n, float(parts[n]), float(p_ref[n]))
    return v, parts, g


def _signed_map(N, K, H, W, seed):
    """The real map of a blob target, from the device op (tests/test_gpu_sdf.py holds it to the restatement)."""
    from eunet import ops
    t = torch.from_numpy(S.blobs(N, H, W, (0, 1, 2) if K == 1 else tuple(range(K)), seed=seed))
    return ops.signed_distance_map(t.to(DEV), K).cpu()


def _logits(N, K, H, W, seed, scale):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, K, H, W, generator=g, dtype=torch.float64) * scale).float(), g


@pytest.mark.parametrize("activation,K", MODES)
@pytest.mark.parametrize("H,W", [(1, 1), (31, 33), (32, 32), (25, 41), (5, 7)])
def test_pixel_counts_around_one_tile(H, W, activation, K):
    """1, 1023, 1024, 1025 and 35 px per sample; N = 1 and 3; the three class-weight sets; the map from
    signed_distance_map and from randn with mixed signs; logits scaled by 2 and by 100 (saturated)."""
    for N, cw, kind, scale in itertools.product((1, 3), WEIGHTS, ("sdf", "randn"), (2.0, 100.0)):
        x, g = _logits(N, K, H, W, seed=100 + H + K + N, scale=scale)
        if kind == "sdf":
            d = _signed_map(N, K, H, W, seed=H * W + K)
        else:
            d = torch.randn(N, K, H, W, generator=g) * 4
            assert H * W == 1 or (bool((d > 0).any()) and bool((d < 0).any()))
        _check(f"{H}x{W} {activation} K{K} N{N} w{cw[:K]} {kind} x{scale:g}", x, d, activation, cw[:K])


@pytest.mark.parametrize("activation,K", [("sigmoid", 1), ("softmax", 3)])
def test_257_tiles_in_one_sample(activation, K):
    """513x512 = 262 656 px = 257 tiles: thread 0 of the finalize reads two tiles and every slot of its LDS tree holds
    a partial.  N = 1; value, parts and the gradient of every pixel, on the real signed map of 5x5 blobs."""
    x, _ = _logits(1, K, 513, 512, seed=7, scale=2.0)
    _check(f"513x512 {activation}", x, _signed_map(1, K, 513, 512, seed=9), activation, None)


def test_batch_of_64_and_65():
    from eunet._lib import EunetError
    from eunet.losses import boundary_loss
    x, g = _logits(65, 3, 5, 7, seed=11, scale=2.0)
    d = torch.randn(65, 3, 5, 7, generator=g) * 4
    _check("N=64", x[:64].contiguous(), d[:64].contiguous(), "softmax", None)
    with pytest.raises(EunetError):
        boundary_loss(x.to(DEV), d.to(DEV))


@pytest.mark.parametrize("activation,K", MODES)
def test_zero_map_gives_exact_zeros(activation, K):
    x, _ = _logits(3, K, 25, 41, seed=13, scale=2.0)
    v, parts, g = _gpu(x, torch.zeros_like(x), activation, None)
    assert v == 0.0 and float(parts.abs().max()) == 0.0 and float(g.abs().max()) == 0.0


def test_gradient_adds_to_the_combined_loss():
    """d (combined_loss + 0.01 boundary_loss) = d combined_loss + d (0.01 boundary_loss)."""
    from eunet.losses import boundary_loss, combined_loss
    x, g = _logits(3, 3, 25, 41, seed=17, scale=2.0)
    t = torch.randint(0, 3, (3, 25, 41), generator=g).to(DEV)
    d = _signed_map(3, 3, 25, 41, seed=19).to(DEV)
    grads = []
    for f in (lambda z: combined_loss(z, t, track_targets=False) + 0.01 * boundary_loss(z, d, class_weight=(0, 1, 1)),
              lambda z: combined_loss(z, t, track_targets=False),
              lambda z: 0.01 * boundary_loss(z, d, class_weight=(0, 1, 1))):
        z = x.to(DEV).requires_grad_(True)
        f(z).backward()
        grads.append(z.grad)
    assert float(grads[2].abs().max()) > 0.0
    assert torch.allclose(grads[0], grads[1] + grads[2], rtol=1e-6, atol=0.0)


def test_gloss_scaling_module_and_bit_identical_runs():
    """(loss * GSCALE).backward() is GSCALE times loss.backward() within the gradient gates; BoundaryLoss(weight) is
    weight times the function; two runs give the same bits in value, parts and gradient."""
    from eunet.losses import BoundaryLoss
    x, _ = _logits(3, 3, 25, 41, seed=23, scale=2.0)
    d = _signed_map(3, 3, 25, 41, seed=29)
    v, parts, g = _gpu(x, d, "softmax", (0, 1, 1))
    v2, parts2, g2 = _gpu(x, d, "softmax", (0, 1, 1))
    assert v == v2 and torch.equal(parts, parts2) and torch.equal(g, g2)
    z = x.to(DEV).requires_grad_(True)
    mod = BoundaryLoss(class_weight=(0, 1, 1), weight=0.5)
    out = mod(z, d.to(DEV))
    out.backward()
    assert abs(out.item() - 0.5 * v) <= 1e-7 * abs(v)
    _grad_close("gloss scaling", z.grad.double().cpu() * (GSCALE / 0.5), g)


@pytest.mark.parametrize("activation", ["softmax", "sigmoid"])
def test_vector_and_scalar_paths_agree(activation):
    """31x32 = 992 px takes the 16-byte path; the same maps padded by one column (31x33 = 1023 px, dist = 0 there)
    take the scalar path.  The padded column adds nothing, so loss * H * W and grad * H * W agree on the common pixels
    within the sum of both bounds, and the column's own gradient is exactly 0."""
    x, g = _logits(3, 3, 31, 32, seed=31, scale=2.0)
    d = torch.randn(3, 3, 31, 32, generator=g) * 4
    xp = torch.cat([x, torch.randn(3, 3, 31, 1, generator=g)], dim=3).contiguous()
    dp = torch.cat([d, torch.zeros(3, 3, 31, 1)], dim=3).contiguous()
    v, parts, gr = _check("31x32 vector", x, d, activation, None)
    vp, partsp, grp = _check("31x33 scalar", xp, dp, activation, None)
    a = S.boundary_loss(x, d, activation, None)[3]
    assert abs(v * 992 - vp * 1023) <= 2e-5 * a * 992
    assert float(grp[..., 32].abs().max()) == 0.0
    _grad_close("vector against scalar", grp[..., :32] * 1023, gr * 992)


def test_descent_moves_the_contour_the_right_way():
    """A sign check, not a convergence claim: 20 plain gradient-descent steps on a free logit tensor with the boundary
    loss alone, on the signed map of a 32x32 disc, never increase the restatement's loss and end below the start.
    Step 100: the loss is a pixel mean of softmax-weighted distances of at most ~23 px over Kw = 2, so its Hessian
    is below 23 * 0.5 / 2048, far under 2 / step."""
    from eunet import ops
    from eunet.losses import boundary_loss
    t = torch.from_numpy(S.discs(32, 32, [(16, 15, 9)]))[None]
    d = ops.signed_distance_map(t.to(DEV), 2)
    z = torch.zeros(1, 2, 32, 32, device=DEV, requires_grad=True)
    dc = d.cpu()
    trace = [S.boundary_loss(z.detach().cpu(), dc, "softmax")[0]]
    for _ in range(20):
        z.grad = None
        boundary_loss(z, d).backward()
        with torch.no_grad():
            z -= 100.0 * z.grad
        trace.append(S.boundary_loss(z.detach().cpu(), dc, "softmax")[0])
    print("loss trace:", " ".join(f"{v:.5f}" for v in trace))
    assert all(b <= a for a, b in zip(trace, trace[1:])), trace
    assert trace[-1] < trace[0]
    # the probability of the disc has grown inside it and shrunk outside
    p1 = torch.softmax(z.detach(), 1)[0, 1].cpu()
    assert float(p1[t[0] == 1].min()) >= 0.5 and float(p1[t[0] == 0].max()) <= 0.5
