"""The pixel-weighted entry points of loss.hip and bce_dice.hip (eunet_loss_fwd_w / _bwd_w,
eunet_bce_dice_fwd_w / _bwd_w) against the fp64 restatements of tests/_wmap_ref.py.

The weight is one more per-pixel stream of kernels whose logic is per pixel and whose tile is 1024 pixels, so
the pixel count sits on either side of a tile (1, 1023, 1024, 1025 px: the scalar path three times, the
16-byte path at 1024), one sample has 257 tiles (513x512, the 16-byte path) and the batch is at its limit of
64.  Weights are drawn from U[0, 12) with some exact zeros; ignored pixels carry a huge weight and must
contribute nothing; an out-of-range target under a weight is counted as without one.

Everything goes through eunet.losses.combined_loss / bce_dice_loss(..., pixel_weight=m, return_parts=True)
and (loss * 3.7).backward().

Gates (the project's loss gates, tests/test_gpu_loss_edges.py and tests/test_gpu_bce_dice.py): value and
every part within 1e-5 relative (1e-7 absolute where the reference is exactly 0); gradients within 1e-4 of
the largest reference gradient, and per element within 1e-3 relative with a floor of 1e-3 of the largest.
With pixel_weight = ones the weighted entry points give the unweighted ones' value, parts, sums and
gradient bit for bit.
"""
import pytest
import torch

import _bce_ref as B
import _wmap_ref as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
GSCALE = 3.7
IGN = 255


def _close(name, got, ref):
    tol = 1e-5 * abs(ref) if ref != 0.0 else 1e-7
    assert abs(got - ref) <= tol, (name, got, ref)


def _grad_close(name, got, ref):
    assert bool(torch.isfinite(got).all()), name
    scale = float(ref.abs().max())
    if scale == 0.0:
        assert float(got.abs().max()) == 0.0, name
        return 0.0, 0.0
    err = (got - ref).abs()
    mx = float(err.max()) / scale
    per = float((err / ref.abs().clamp_min(1e-3 * scale)).max())
    assert mx <= 1e-4, (name, mx)
    assert per <= 1e-3, (name, per)
    return mx, per


def _inputs(N, K, H, W, seed, kind):
    """Logits, targets (K = 1 of the BCE loss draws from {0, 1, 2}: foreground maps 2 -> 1) and weights from
    U[0, 12) with every fifth exactly 0."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(N, K, H, W, generator=g, dtype=torch.float64) * 2).float()
    t = torch.randint(0, 3 if (K == 1 and kind == "bce") else K, (N, H, W), generator=g)
    m = (torch.rand(N, H, W, generator=g, dtype=torch.float64) * 12).float()
    m.view(-1)[::5] = 0.0
    return x, t, m


def _bce_params(s):
    from eunet.losses import make_bce_dice_params
    return make_bce_dice_params(pos_weight=list(s["pos_weight"]), class_weight=list(s["class_weight"]),
                                dice_weight=list(s["dice_weight"]), w_bce=s["w_bce"], w_dice=s["w_dice"],
                                smooth=s["smooth"], ignore_index=s["ignore_index"], target_mode=s["target_mode"])


def _combined_params(s):
    from eunet.losses import make_params
    return make_params(ce_weight=list(s["ce_weight"]), alpha=list(s["alpha"]), gamma=s["gamma"],
                       ignore_index=s["ignore_index"], dice_weight=list(s["dice_weight"]),
                       tversky_weight=list(s["tversky_weight"]), tversky_alpha=s["tversky_alpha"], w_focal=s["w_focal"],
                       w_dice=s["w_dice"], w_tversky=s["w_tversky"], class_div=s["class_div"])


def _gpu(kind, x32, target, m, params, weighted=True):
    from eunet.losses import bce_dice_loss, combined_loss
    fn = bce_dice_loss if kind == "bce" else combined_loss
    x = x32.to(DEV).requires_grad_(True)
    kw = dict(pixel_weight=m.to(DEV)) if weighted else {}
    loss, parts = fn(x, target.to(DEV), return_parts=True, params=params, track_targets=False, **kw)
    (loss * GSCALE).backward()
    torch.cuda.synchronize()
    return loss, parts, x.grad


def _check(kind, name, x32, target, m, s=None, ref_target=None):
    """ref_target: what the restatement sees where it differs from what the kernel is given."""
    if kind == "bce":
        s = s or B.spec()
        ref = M.bce_dice_w(x32, target if ref_target is None else ref_target, m, g=GSCALE, **s)
        params = _bce_params(s)
    else:
        s = s or M.combined_spec()
        ref = M.combined_w(x32, target if ref_target is None else ref_target, m, g=GSCALE, **s)
        params = _combined_params(s)
    v_ref, p_ref, g_ref = ref
    loss, parts, grad = _gpu(kind, x32, target, m, params)
    v, parts, grad = loss.item(), parts.double().cpu(), grad.double().cpu()
    mx, per = _grad_close(name, grad, g_ref)
    print(f"{kind} {name}: value {v:.8g} (ref {v_ref:.8g}), grad err / max {mx:.2e}, worst element {per:.2e}")
    assert v == v and abs(v) != float("inf"), name
    _close(name + " value", v, v_ref)
    assert parts.shape == p_ref.shape
    for n in range(p_ref.shape[0]):
        for i in range(p_ref.shape[1]):
            _close(f"{name} parts[{n}][{i}]", float(parts[n, i]), float(p_ref[n, i]))
    return v, grad


@pytest.mark.parametrize("kind", ["combined", "bce"])
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (31, 33), (32, 32), (25, 41)])
def test_pixel_counts_around_one_tile(H, W, K, kind):
    """1, 1023, 1024 and 1025 px per sample, N = 3, K = 1..3, both losses."""
    x, t, m = _inputs(3, K, H, W, seed=200 + H + K, kind=kind)
    _check(kind, f"{H}x{W} K{K}", x, t, m)


@pytest.mark.parametrize("kind,K", [("combined", 3), ("bce", 1)])
def test_257_tiles_in_one_sample(kind, K):
    """513x512 = 262 656 px = 257 tiles of one sample, on the 16-byte path."""
    x, t, m = _inputs(1, K, 513, 512, seed=7, kind=kind)
    _check(kind, "513x512", x, t, m)


@pytest.mark.parametrize("kind,K", [("combined", 3), ("bce", 2)])
def test_batch_of_64(kind, K):
    x, t, m = _inputs(64, K, 5, 7, seed=11, kind=kind)
    _check(kind, "N=64", x, t, m)


@pytest.mark.parametrize("kind", ["combined", "bce"])
@pytest.mark.parametrize("H,W", [(25, 41), (32, 32)])
def test_ignored_pixels_with_a_large_weight_contribute_nothing(kind, H, W):
    """Every seventh pixel at ignore index 255 carries the weight 1e30 (inf and nan on two of them): the loss
    is finite and equals the restatement's, and equals, bit for bit, the loss with those weights at 0."""
    x, t, m = _inputs(3, 3, H, W, seed=31 + H, kind=kind)
    t.view(-1)[::7] = IGN
    m[t == IGN] = 1e30
    m.view(-1)[0], m.view(-1)[7] = float("inf"), float("nan")
    s = B.spec(ignore_index=IGN, class_weight=(2.0, 1.0, 3.0)) if kind == "bce" else M.combined_spec(ignore_index=IGN)
    v, g = _check(kind, f"{H}x{W} ignore", x, t, m, s)
    m0 = torch.where(t == IGN, torch.zeros_like(m), m)
    v0, g0 = _check(kind, f"{H}x{W} ignore, weight 0", x, t, m0, s)
    assert v == v0 and torch.equal(g, g0)
    if kind == "bce":  # there an ignored pixel counts nowhere (the combined loss keeps its probabilities in S)
        assert float(g[t.unsqueeze(1).expand_as(g) == IGN].abs().max()) == 0.0


@pytest.mark.parametrize("kind", ["combined", "bce"])
def test_out_of_range_target_under_a_weight_is_counted(kind):
    """Targets 7 and -3 in both tiles of a 25x41 sample: they contribute nothing to the weighted term (the
    restatement sees them as ignored) and are counted where the unweighted call counts them."""
    from eunet import losses
    x, t, m = _inputs(2, 3, 25, 41, seed=41, kind=kind)
    bad = t.clone()
    bad[0, 0, 3], bad[0, 24, 40], bad[1, 12, 5] = 7, -3, 7
    m[0, 0, 3] = 1e30
    ref_t = torch.where((bad < 0) | (bad > 2), torch.full_like(bad, IGN), bad)
    s = B.spec(ignore_index=IGN) if kind == "bce" else M.combined_spec(ignore_index=IGN)
    _check(kind, "out of range", x, bad, m, s, ref_target=ref_t)
    fn = losses.bce_dice_loss if kind == "bce" else losses.combined_loss
    try:
        losses.check_targets()  # start from a clean counter, whatever ran before
    except ValueError:
        pass
    fn(x.to(DEV), bad.to(DEV), pixel_weight=m.to(DEV))
    with pytest.raises(ValueError, match="3 target value"):
        losses.check_targets()


PATHS = [(25, 41), (32, 32), (31, 33), (64, 48)]  # HW % 4: 1, 0, 3, 0


@pytest.mark.parametrize("kind", ["combined", "bce"])
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("H,W", PATHS)
def test_weight_of_ones_is_the_unweighted_call_bit_for_bit(H, W, K, kind):
    """Value, parts, sums and gradient of the weighted entry points at m = 1 equal the unweighted ones', bit for
    bit, on the scalar and on the 16-byte path; non-default parameters, some pixels ignored."""
    from eunet import ops
    x, t, _ = _inputs(3, K, H, W, seed=51 + H + K, kind=kind)
    if H * W > 8:
        t.view(-1)[::9] = IGN
    ones = torch.ones(3, H, W)
    if kind == "bce":
        params = _bce_params(B.spec(pos_weight=(1.5, 3.0, 0.5), class_weight=(2.0, 1.0, 3.0),
                                    dice_weight=(1.0, 15.0, 8.0), w_bce=0.7, w_dice=1.3, ignore_index=IGN))
    else:
        params = _combined_params(M.combined_spec(ignore_index=IGN))
    lw, pw, gw = _gpu(kind, x, t, ones, params)
    lu, pu, gu = _gpu(kind, x, t, ones, params, weighted=False)
    assert torch.equal(lw, lu) and torch.equal(pw, pu) and torch.equal(gw, gu), (kind, H, W, K)
    # the saved sums, through the ops layer
    xd, td, od = x.to(DEV), t.to(DEV), ones.to(DEV)
    if kind == "bce":
        n_sums, n_ws = ops.bce_dice_sums_len(3, K), ops.bce_dice_workspace_bytes(3, K, H, W)
        fwd_w, fwd = ops.bce_dice_fwd_w, ops.bce_dice_fwd
    else:
        n_sums, n_ws = ops.loss_sums_len(3, K), ops.loss_workspace_bytes(3, K, H, W)
        fwd_w, fwd = ops.loss_fwd_w, ops.loss_fwd
    outs = []
    for weighted in (True, False):
        sums = torch.empty(n_sums, device=DEV)
        loss, parts = torch.empty((), device=DEV), torch.empty(3, 2 if kind == "bce" else 3, device=DEV)
        ws = torch.empty(n_ws, dtype=torch.uint8, device=DEV)
        if weighted:
            fwd_w(xd, td, od, params, sums, loss, parts, ws)
        else:
            fwd(xd, td, params, sums, loss, parts, ws)
        outs.append((sums, loss, parts))
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_function_apply_as_called_before_the_weight_argument():
    """BCEDiceFunction.apply(logits, target, params, track_targets), the four-argument call from before pixel_weight
    became its optional fifth, is bce_dice_loss(logits, target): value, parts and gradient bit for bit (3x25x41,
    K = 2)."""
    from eunet.losses import BCEDiceFunction, bce_dice_loss
    x, t, _ = _inputs(3, 2, 25, 41, seed=77, kind="bce")
    outs = []
    for call in (lambda xd, td: BCEDiceFunction.apply(xd, td, None, False),
                 lambda xd, td: bce_dice_loss(xd, td, return_parts=True, track_targets=False)):
        xd = x.to(DEV).requires_grad_(True)
        loss, parts = call(xd, t.to(DEV))
        loss.backward()
        outs.append((loss.detach(), parts, xd.grad))
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_library_refusals():
    """focal_norm = 1 with a weight and a null weight are EUNET_ERR_INVALID in the library itself."""
    from eunet import _lib, ops
    from eunet.losses import make_params
    x = torch.randn(2, 3, 4, 5, device=DEV)
    t = torch.randint(0, 3, (2, 4, 5), device=DEV)
    m = torch.ones(2, 4, 5, device=DEV)
    sums = torch.empty(ops.loss_sums_len(2, 3), device=DEV)
    loss, parts = torch.empty((), device=DEV), torch.empty(2, 3, device=DEV)
    ws = torch.empty(ops.loss_workspace_bytes(2, 3, 4, 5), dtype=torch.uint8, device=DEV)
    p = make_params(focal_norm=1)
    with pytest.raises(_lib.EunetError, match="focal_norm"):
        ops.loss_fwd_w(x, t, m, p, sums, loss, parts, ws)
    with pytest.raises(_lib.EunetError, match="focal_norm"):
        ops.loss_bwd_w(x, t, m, p, sums, torch.ones(1, device=DEV), torch.empty_like(x))
    with pytest.raises(_lib.EunetError):
        ops.loss_fwd_w(x, t, None, None, sums, loss, parts, ws)
    with pytest.raises(_lib.EunetError):
        _lib.call("eunet_bce_dice_fwd_w", x.data_ptr(), t.data_ptr(), None, 2, 3, 4, 5, None, sums.data_ptr(),
                  loss.data_ptr(), None, ws.data_ptr(), None)
    torch.cuda.synchronize()
