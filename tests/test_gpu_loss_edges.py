"""loss.hip past one tile: the combined loss per pixel against the fp64 oracle at the edges of its launch.

loss_fwd_kernel reduces LPIX = 1024 pixels of one sample per block and loss_finalize_kernel combines a
sample's tiles (256 threads striding over them, then a 128-wide LDS tree) and the batch's samples (at most
64).  The other loss tests stay below one tile per sample; here the pixel count sits on either side of a
tile (1, 1023, 1024, 1025 px), one sample has 257 tiles (513x512), the batch is at and past its limit
(64, 65 samples), and K = 1, an upstream gradient other than 1, every branch of focal_pow, ignore_index
together with the Dice / Tversky terms, degenerate targets, saturated logits and out-of-range targets in
two tiles are each compared with the oracle.

Everything goes through eunet.losses.combined_loss(..., params=make_params(...), return_parts=True) and
(loss * 3.7).backward().  The reference is oracle/eunet_ref.py in fp64 on the fp32 logits as stored:
combined_loss per sample, summed and divided by N, for the reference configuration; for any other
parameter set w_focal * focal_loss(batch) + (1/N) sum_n (w_dice dice_loss(n) + w_tversky tversky_loss(n)).
A pixel at ignore_index has (target == c) false for every c in the oracle's Dice and Tversky, which is
what the kernel documents (its probabilities still count in S).

Gates (those of tests/test_gpu_loss_api.py): value and the three parts of every sample within 1e-5
relative (1e-7 absolute for a term that is exactly 0, such as the focal term at K = 1); gradients within
1e-4 of the largest reference gradient, and per element within 1e-3 relative with a floor of 1e-3 of the
largest.
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import eunet_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GSCALE = 3.7  # upstream gradient: (loss * 3.7).backward()
IGN = 255


class Spec:
    """One loss configuration: the kernel's parameters (params()) and the oracle's arguments."""

    def __init__(self, ce_weight=R.CE_WEIGHT, alpha=R.FOCAL_ALPHA, gamma=R.GAMMA, ignore_index=None, nc=3,
                 tv_alpha=R.TV_ALPHA, w=(R.W_FOCAL, R.W_DICE, R.W_TV), focal_norm=0):
        self.ce_weight, self.alpha, self.gamma, self.ignore_index = ce_weight, alpha, gamma, ignore_index
        self.nc, self.tv_alpha, self.w, self.focal_norm = nc, tv_alpha, w, focal_norm

    def params(self):
        from eunet.losses import make_params
        return make_params(ce_weight=None if self.ce_weight is None else list(self.ce_weight),
                           alpha=None if self.alpha is None else list(self.alpha), gamma=self.gamma,
                           ignore_index=self.ignore_index,
                           dice_weight=[R.DICE_W[c] if c < self.nc else 0.0 for c in range(3)],
                           tversky_weight=[R.TVERSKY_W[c] if c < self.nc else 0.0 for c in range(3)],
                           tversky_alpha=self.tv_alpha, w_focal=self.w[0], w_dice=self.w[1], w_tversky=self.w[2],
                           class_div=float(self.nc), focal_norm=self.focal_norm)

    def focal(self, lg, tg):
        cw = None if self.ce_weight is None else torch.tensor(list(self.ce_weight)[:lg.shape[1]], dtype=lg.dtype)
        if self.focal_norm:
            return F.cross_entropy(lg, tg, weight=cw, reduction="mean",
                                   ignore_index=-100 if self.ignore_index is None else self.ignore_index)
        return R.focal_loss(lg, tg, alpha=None if self.alpha is None else list(self.alpha), gamma=self.gamma,
                            ignore_index=self.ignore_index, class_weights=cw)


REFERENCE = Spec()


def _reference(x32, target, spec, oracle_combined):
    """(value, parts [N][3], d (GSCALE * value) / d logits) in fp64 on the logits as stored."""
    x = x32.double().clone().requires_grad_(True)
    N = x.shape[0]
    parts = []
    if oracle_combined:  # the reference configuration: the oracle's own combined_loss per sample
        tot = x.new_zeros(())
        for n in range(N):
            t, p = R.combined_loss(x[n], target[n], parts=True)
            tot = tot + t
            parts.append([p["focal"].item(), p["dice"].item(), p["tversky"].item()])
        tot = tot / N
    else:
        tot = spec.w[0] * spec.focal(x, target)
        for n in range(N):
            lg, tg = x[n:n + 1], target[n:n + 1]
            d, tv = R.dice_loss(lg, tg, spec.nc), R.tversky_loss(lg, tg, spec.nc, spec.tv_alpha)
            tot = tot + (spec.w[1] * d + spec.w[2] * tv) / N
            parts.append([spec.focal(lg, tg).item(), d.item(), tv.item()])
    (tot * GSCALE).backward()
    return tot.item(), parts, x.grad


def _gpu(x32, target, spec):
    from eunet.losses import combined_loss
    x = x32.to(DEV).requires_grad_(True)
    loss, parts = combined_loss(x, target.to(DEV), return_parts=True, params=spec.params(), track_targets=False)
    (loss * GSCALE).backward()
    torch.cuda.synchronize()
    return loss.item(), parts.double().cpu(), x.grad.double().cpu()


def _close(name, got, ref):
    tol = 1e-5 * abs(ref) if ref != 0.0 else 1e-7
    assert abs(got - ref) <= tol, (name, got, ref)


def _grad_close(name, got, ref):
    assert bool(torch.isfinite(got).all()), name
    scale = float(ref.abs().max())
    if scale == 0.0:  # K = 1: the softmax of one logit is constant, the gradient is exactly 0
        assert float(got.abs().max()) == 0.0, name
        return 0.0, 0.0
    err = (got - ref).abs()
    mx = float(err.max()) / scale
    per = float((err / ref.abs().clamp_min(1e-3 * scale)).max())
    assert mx <= 1e-4, (name, mx)
    assert per <= 1e-3, (name, per)
    return mx, per


def _check(name, x32, target, spec=REFERENCE, oracle_combined=None, ref_target=None, ref_spec=None):
    """ref_target / ref_spec: what the oracle sees where it differs from what the kernel is given."""
    if oracle_combined is None:
        oracle_combined = spec is REFERENCE and ref_spec is None
    v_ref, p_ref, g_ref = _reference(x32, target if ref_target is None else ref_target, ref_spec or spec,
                                     oracle_combined)
    v, parts, g = _gpu(x32, target, spec)
    mx, per = _grad_close(name, g, g_ref)
    print(f"{name}: value {v:.8g} (ref {v_ref:.8g}), grad err / max {mx:.2e}, worst element {per:.2e}")
    assert v == v and abs(v) != float("inf"), name
    _close(name + " value", v, v_ref)
    for n, row in enumerate(p_ref):
        for i, term in enumerate(("focal", "dice", "tversky")):
            _close(f"{name} parts[{n}].{term}", float(parts[n, i]), row[i])


def _inputs(N, K, H, W, seed, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(N, K, H, W, generator=g, dtype=torch.float64) * scale).float()
    t = torch.randint(0, K, (N, H, W), generator=g)
    return x, t, g


def _ignore_some(t, g, frac=0.1):
    t = t.clone()
    t[torch.rand(t.shape, generator=g) < frac] = IGN
    return t


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (31, 33), (32, 32), (25, 41)])
def test_pixel_counts_around_one_tile(H, W, K):
    """1, 1023, 1024 and 1025 px per sample (the second tile of 25x41 holds one pixel), N = 3, K = 1..3.
    K = 1 is the same formulas: the focal term is 0, Dice and Tversky are not once a pixel is not of
    class 0.  Its only valid label is 0 (then every term is exactly 0), so K = 1 also runs with every
    seventh pixel at ignore_index, against the oracle's single-class Dice / Tversky."""
    x, t, _ = _inputs(3, K, H, W, seed=100 + H + K)
    _check(f"{H}x{W} K{K}", x, t)
    if K == 1:
        t.view(-1)[::7] = IGN
        _check(f"{H}x{W} K1 ignore", x, t, Spec(ignore_index=IGN, nc=1), oracle_combined=False)


def test_257_tiles_in_one_sample():
    """513x512 = 262 656 px = 257 tiles: thread 0 of the finalize reads two tiles and every slot of its
    LDS tree holds a partial.  Value, parts and the gradient of every pixel."""
    x, t, _ = _inputs(1, 3, 513, 512, seed=7)
    _check("513x512", x, t)


def test_batch_of_64_and_65():
    """64 samples is the limit of the finalize's per-sample LDS arrays; 65 is refused by the library."""
    from eunet._lib import EunetError
    from eunet.losses import combined_loss
    x, t, _ = _inputs(65, 3, 5, 7, seed=11)
    _check("N=64", x[:64].contiguous(), t[:64].contiguous())
    with pytest.raises(EunetError):
        combined_loss(x.to(DEV), t.to(DEV), params=REFERENCE.params(), track_targets=False)


def test_entry_points_share_the_shape_rule():
    """The one shape rule of the loss entry points (include/eunet.h, "per-pixel losses") holds for eunet_loss_fwd
    and eunet_loss_bwd too: an empty plane and a backward over 65 samples are refused before any launch."""
    from eunet import ops
    from eunet._lib import EunetError
    x, t, _ = _inputs(65, 3, 5, 7, seed=11)
    x, t = x.to(DEV), t.to(DEV)
    sums = torch.zeros(ops.loss_sums_len(65, 3), device=DEV)
    loss, parts = torch.zeros((), device=DEV), torch.zeros(65, 3, device=DEV)
    ws = torch.zeros(ops.loss_workspace_bytes(65, 3, 5, 7), dtype=torch.uint8, device=DEV)
    # "bad args" is the shape rule's message: the refusal comes from the argument check, not from a failed launch
    with pytest.raises(EunetError, match="loss_fwd: bad args"):
        ops.loss_fwd(x[:3, :, :0], t[:3, :0], None, sums, loss, parts, ws)  # h = 0
    with pytest.raises(EunetError, match="loss_bwd: bad args"):
        ops.loss_bwd(x, t, None, sums, torch.ones(1, device=DEV), torch.empty_like(x))


PARAM_SETS = {
    "reference": REFERENCE,
    "gamma0": Spec(gamma=0.0),
    "gamma1": Spec(gamma=1.0),
    "gamma2": Spec(gamma=2.0),
    "gamma8": Spec(gamma=8.0),   # the last of focal_pow's repeated products
    "gamma9": Spec(gamma=9.0),   # the first integer on its powf branch
    "gamma1.5": Spec(gamma=1.5),
    "ignore255": Spec(ignore_index=IGN),
    "ce_mean": Spec(ce_weight=(2.0, 1.0, 3.0), alpha=None, gamma=0.0, ignore_index=IGN, w=(1.0, 0.0, 0.0),
                    focal_norm=1),
    "tversky_a0.3": Spec(tv_alpha=0.3),
    "class_div2": Spec(nc=2),
}


@pytest.mark.parametrize("name", list(PARAM_SETS))
def test_parameter_sets(name):
    """3 x 25x41 (two tiles per sample), K = 3.  ignore255: about 10 % of the pixels ignored with all
    three terms on; ce_mean: focal_norm = 1 with class weights and ignored pixels, against
    F.cross_entropy(weight, ignore_index, reduction='mean'); class_div2: the third Dice / Tversky weights 0."""
    spec = PARAM_SETS[name]
    x, t, g = _inputs(3, 3, 25, 41, seed=21)
    if spec.ignore_index is not None:
        t = _ignore_some(t, g)
        assert 0.05 < float((t == IGN).float().mean()) < 0.15
    _check(name, x, t, spec, oracle_combined=False)
    if spec is REFERENCE:
        _check(name + " (oracle combined_loss)", x, t)


def test_degenerate_targets():
    """A sample in which class 2 never occurs (T_2 = 0) and a sample that is class 2 throughout."""
    x, t, g = _inputs(3, 3, 25, 41, seed=31)
    t[1] = torch.randint(0, 2, (25, 41), generator=g)
    t[2] = 2
    _check("degenerate targets", x, t)


def test_saturated_logits():
    """Logits spread over +-40: the softmax saturates, pt rounds to 1 where the target wins and to 0 where
    it loses by a wide margin.  Loss and gradients stay finite and within the gates."""
    g = torch.Generator().manual_seed(41)
    x = ((torch.rand(3, 3, 25, 41, generator=g, dtype=torch.float64) * 2 - 1) * 40).float()
    t = torch.randint(0, 3, (3, 25, 41), generator=g)
    assert float(x.abs().max()) > 39.0
    _check("saturated", x, t)
    _check("saturated gamma1.5", x, t, PARAM_SETS["gamma1.5"], oracle_combined=False)


def test_out_of_range_targets_in_both_tiles():
    """25x41, K = 3: 7 targets of value K in the first tiles and 5 in the second tiles.  The second tile of
    a 1025 px sample is one pixel, so the batch has 5 samples and the last pixel of each is out of range.
    sums[-1] counts all 12; the loss and the gradient are those of the oracle with the 12 pixels ignored."""
    from eunet import ops
    N, K, H, W = 5, 3, 25, 41
    x, t, g = _inputs(N, K, H, W, seed=51)
    bad = t.clone()
    flat = bad.view(N, -1)
    flat[:, 1024] = K
    for n, p in ((0, 0), (0, 1023), (1, 517), (2, 255), (2, 256), (3, 640), (4, 3)):
        flat[n, p] = K
    assert int((bad == K).sum()) == 12 and int((flat[:, :1024] == K).sum()) == 7
    ign = bad.clone()
    ign[bad == K] = IGN
    prm = REFERENCE.params()
    xd, td = x.to(DEV), bad.to(DEV)
    sums = torch.empty(ops.loss_sums_len(N, K), dtype=torch.float32, device=DEV)
    loss = torch.empty((), dtype=torch.float32, device=DEV)
    parts = torch.empty(N, 3, dtype=torch.float32, device=DEV)
    ws = torch.empty(ops.loss_workspace_bytes(N, K, H, W), dtype=torch.uint8, device=DEV)
    ops.loss_fwd(xd, td, prm, sums, loss, parts, ws)
    torch.cuda.synchronize()
    assert sums[-1].item() == 12.0
    assert sums[-2].item() == float(N * H * W)  # the focal denominator still counts every pixel
    _check("out of range", x, bad, ref_target=ign, ref_spec=Spec(ignore_index=IGN), oracle_combined=False)
