"""lovasz.hip, the losses: ops.lovasz_errors, eunet.losses.lovasz_loss forward and backward, against tests/_lovasz_ref.py
(the definition of include/eunet.h restated in fp64 on the fp32 inputs as stored; tests/test_lovasz_host.py holds it to
the definition of the Lovasz extension by brute force).

Errors.  The existing tests state a bound for sigmoid_terms' probability (tests/test_gpu_bce_dice.py, 4 x torch's own
fp32 error, 3.4e-7) but none for softmax_px, and the hinge error uses neither.  So the worst deviation of the device's
errors from the fp64 restatement was measured on these inputs (N(0, 2^2) logits): MEASURED_ERR below, per activation.
The bound is 4 x that and no looser than 2^-20 (softmax 5.32e-7, hinge 9.54e-7); it guards against a wrong formula, not
against rounding.

Forward.  The Lovasz extension has g >= 0 and sum g <= 1, so |l(e) - l(e')| <= max |e - e'|: the bound on every
segment loss (and on the loss, a mean of means of them) is the case's own max |e_dev - e_fp64| plus 1e-7, computed by
the test.  An order that differs between the fp32 and the fp64 errors is inside that bound.

Gradients: the gates of tests/test_gpu_boundary_loss.py -- within 1e-4 of the largest reference gradient, per element
within 1e-3 relative with a floor of 1e-3 of the largest."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _lovasz_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGN = 255
GSCALE = 3.7
MODES = [("softmax", 2), ("softmax", 3), ("hinge", 1), ("hinge", 2), ("hinge", 3)]
# worst |e_dev - e_fp64| over test_errors_and_flags' cases, as measured on an MI355X (softmax: 32x32, K = 3; hinge:
# 2^-21, half an ulp of an error in [8, 16), the single rounding of 1 - z s)
MEASURED_ERR = {"softmax": 1.33e-7, "hinge": 4.77e-7}
ERR_BOUND = {a: min(4.0 * v, 2.0 ** -20) for a, v in MEASURED_ERR.items()}


def _grad_close(name, got, ref):
    """tests/test_gpu_boundary_loss.py's gates (without its FLT_MIN term: no logit here is saturated)."""
    assert bool(torch.isfinite(got).all()), name
    scale = float(ref.abs().max())
    if scale == 0.0:
        assert float(got.abs().max()) == 0.0, name
        return 0.0, 0.0
    err = (got - ref).abs()
    mx = float(err.max()) / scale
    per = float((err / ref.abs().clamp_min(1e-3 * scale)).max())
    print(f"{name}: grad err / max {mx:.2e}, worst element {per:.2e}")
    assert mx <= 1e-4, (name, mx)
    assert per <= 1e-3, (name, per)
    return mx, per


def _inputs(N, K, H, W, seed, scale=2.0, ignore=True, bad=False):
    """randn logits; a target of random classes with an ignored stripe (the first column) and, with bad, one
    out-of-range value."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(N, K, H, W, generator=g, dtype=torch.float64) * scale).float()
    t = torch.randint(0, max(K, 2), (N, H, W), generator=g)
    if ignore:
        t[:, :, 0] = IGN
    if bad:
        t[N - 1, H - 1, W - 1] = -7
    return x, t


def _fwd_raw(x, t, activation, per_image, mode, mask, ign):
    """ops.lovasz_fwd on device tensors -> weights, factor, loss, parts, counts, bad."""
    from eunet import ops
    n, k, h, w = x.shape
    s, l = ops.lovasz_segments(n, k, h, w, per_image)
    weights = torch.empty_like(x)
    factor = torch.empty(s, device=DEV)
    loss = torch.empty((), device=DEV)
    parts = torch.empty(s, device=DEV)
    counts = torch.empty(s, 2, dtype=torch.int64, device=DEV)
    bad = torch.empty(1, device=DEV)
    ws = torch.empty(ops.lovasz_workspace_bytes(s, l), dtype=torch.uint8, device=DEV)
    ops.lovasz_fwd(x, t, ops.LOVASZ_ACTIVATIONS[activation], per_image, mode, mask, ign, weights, factor, loss, parts,
                   counts, bad, ws)
    return weights, factor, loss, parts, counts, bad


# ---- errors and flags ---------------------------------------------------------------------------
@pytest.mark.parametrize("activation,K", MODES)
@pytest.mark.parametrize("H,W", [(1, 1), (1, 37), (5, 7), (31, 33), (32, 32)])
def test_errors_and_flags(H, W, activation, K):
    """1, 37, 35, 1023 and 1024 px per sample, N = 2, with an ignored stripe and an out-of-range target."""
    from eunet import ops
    x, t = _inputs(2, K, H, W, seed=H * W + K, bad=True)
    e_ref, f_ref = R.errors_flags(x, t, activation, IGN)
    e, f = ops.lovasz_errors(x.to(DEV), t.to(DEV), activation, ignore_index=IGN)
    assert e.dtype == torch.float32 and f.dtype == torch.uint8 and e.shape == x.shape and f.shape == x.shape
    worst = float(np.abs(e.double().cpu().numpy() - e_ref).max())
    print(f"{H}x{W} {activation} K{K}: worst |e - e_fp64| {worst:.3e} (bound {ERR_BOUND[activation]:.3e})")
    assert np.array_equal(f.cpu().numpy(), f_ref)
    assert (f_ref == 2).any()
    assert worst <= ERR_BOUND[activation]


# ---- forward ----------------------------------------------------------------------------------------
def _mixed(K, seed):
    """N = 3 of 9 x 11 with unequal content: sample 0 has no foreground (all class 0), sample 1 is ignored entirely,
    sample 2 is random with an ignored stripe."""
    x, t = _inputs(3, K, 9, 11, seed=seed)
    t[0] = 0
    t[1] = IGN
    return x, t


_REF = {}


def _reference(key, x, t, activation, classes, per_image):
    """The restatement of a case, computed once."""
    if key not in _REF:
        _REF[key] = R.loss(x, t, activation, classes, per_image, IGN)
    return _REF[key]


@pytest.mark.parametrize("activation,K", [("softmax", 2), ("softmax", 3), ("hinge", 2), ("hinge", 3)])
@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("classes", ["present", "all", [1], None])
def test_forward_against_the_restatement(activation, K, per_image, classes):
    from eunet import ops
    from eunet.losses import lovasz_loss
    x, t = _mixed(K, seed=10 + K)
    ref = _reference((activation, K, per_image, str(classes)), x, t, activation, classes, per_image)
    xd, td = x.to(DEV), t.to(DEV)
    e_dev, _ = ops.lovasz_errors(xd, td, activation, ignore_index=IGN)
    bound = float(np.abs(e_dev.double().cpu().numpy() - ref["errors"]).max()) + 1e-7
    loss, parts = lovasz_loss(xd, td, activation=activation, classes=classes, per_image=per_image, ignore_index=IGN,
                              return_parts=True)
    parts = parts.double().cpu().numpy()
    assert parts.shape == ref["parts"].shape == ((3 * K,) if per_image else (K,))
    assert np.array_equal(np.isnan(parts), np.isnan(ref["parts"])), (parts, ref["parts"])
    sel = ~np.isnan(parts)
    worst = float(np.abs(parts[sel] - ref["parts"][sel]).max()) if sel.any() else 0.0
    print(f"{activation} K{K} per_image {per_image} classes {classes}: loss {loss.item():.8g} (ref {ref['loss']:.8g}), "
          f"worst segment {worst:.2e}, bound {bound:.2e}")
    assert worst <= bound
    assert abs(loss.item() - ref["loss"]) <= bound
    if per_image:
        assert np.isnan(parts[K:2 * K]).all()  # the ignored sample selects nothing, whatever the classes


def test_an_entirely_ignored_batch_gives_zero_loss_and_zero_gradient():
    from eunet.losses import lovasz_loss
    x, t = _inputs(2, 3, 5, 7, seed=3)
    t[:] = IGN
    for activation, per_image in itertools.product(("softmax", "hinge"), (False, True)):
        xd = x.to(DEV).requires_grad_(True)
        loss = lovasz_loss(xd, t.to(DEV), activation=activation, classes="all", per_image=per_image, ignore_index=IGN)
        loss.backward()
        assert loss.item() == 0.0 and float(xd.grad.abs().max()) == 0.0


def test_out_of_range_targets_are_counted():
    from eunet.losses import check_targets, lovasz_loss
    x, t = _inputs(2, 2, 5, 7, seed=4, bad=True)
    check_targets()
    lovasz_loss(x.to(DEV), t.to(DEV), ignore_index=IGN)
    with pytest.raises(ValueError, match="1 target value"):
        check_targets()


# ---- backward ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("activation,K", MODES)
@pytest.mark.parametrize("H,W", [(5, 7), (31, 33), (32, 32)])
def test_backward_layer_from_the_device_weights(H, W, activation, K):
    """The device's weights (g times the factor of its segment) fed to the fp64 backward formula, against the device
    gradient: the scalar path (35 and 1023 px) and the 16-byte path (1024 px)."""
    from eunet import _lib, ops
    for per_image in (False, True):
        x, t = _inputs(3, K, H, W, seed=H + K)
        xd, td = x.to(DEV), t.to(DEV)
        weights, factor, *_ = _fwd_raw(xd, td, activation, per_image, _lib.LOVASZ_ALL, 0, IGN)
        glog = torch.empty_like(xd)
        ops.lovasz_bwd(xd, td, ops.LOVASZ_ACTIVATIONS[activation], per_image, weights, factor,
                       torch.full((1,), GSCALE, device=DEV), glog)
        f = factor.double().cpu()
        wfull = weights.double().cpu() * (f.reshape(3, K, 1, 1) if per_image else f.reshape(1, K, 1, 1))
        ref = R.backward_from_weights(x, t, wfull.numpy(), activation, gloss=GSCALE)
        _grad_close(f"{H}x{W} {activation} K{K} per_image {per_image}", glog.double().cpu(), ref)
        assert float(glog[:, :, :, 0].abs().max()) == 0.0  # the ignored stripe


def _ramp(K):
    """N = 2 of 5 x 7 logits on ramps chosen so that no two errors of a segment come close, and a striped target."""
    n, hw = 2, 35
    i = torch.arange(n * hw, dtype=torch.float64).reshape(n, 1, 5, 7)
    x = torch.zeros(n, K, 5, 7, dtype=torch.float64)
    x[:, 1:2] = -2.0 + 0.0571 * i + 0.013
    if K == 3:
        x[:, 2:3] = 1.3 - 0.0379 * i
    t = ((torch.arange(n * hw).reshape(n, 5, 7) * 7) % 10 % K).long()
    return x.float(), t


@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("per_image", [False, True])
def test_end_to_end_against_fp64_autograd(K, per_image):
    from eunet.losses import lovasz_loss
    x, t = _ramp(K)
    e, f = R.errors_flags(x, t, "softmax")
    for seg in R.segments(e, per_image):  # a condition of the test: the fp32 errors cannot order differently
        assert float(np.diff(np.sort(seg)).min()) >= 1e-4
    v_ref, g_ref = R.autograd_loss(x, t, "softmax", None, per_image, None, gloss=GSCALE)
    xd = x.to(DEV).requires_grad_(True)
    loss = lovasz_loss(xd, t.to(DEV), per_image=per_image)
    (loss * GSCALE).backward()
    assert abs(loss.item() - v_ref) <= 1e-6
    _grad_close(f"ramp K{K} per_image {per_image}", xd.grad.double().cpu(), g_ref)


def test_ties_are_broken_by_index_and_runs_are_bit_identical():
    """All-zero logits: p = 1/2 exactly on both sides, every error of K = 2 is 1/2 and the index order alone decides
    the gradient."""
    from eunet.losses import lovasz_loss
    x = torch.zeros(2, 2, 9, 11)
    g = torch.Generator().manual_seed(5)
    t = torch.randint(0, 2, (2, 9, 11), generator=g)
    v_ref, g_ref = R.autograd_loss(x, t, "softmax", "all", False, None, gloss=GSCALE)
    runs = []
    for _ in range(2):
        xd = x.to(DEV).requires_grad_(True)
        loss = lovasz_loss(xd, t.to(DEV), classes="all")
        (loss * GSCALE).backward()
        runs.append((loss.detach().cpu(), xd.grad.cpu()))
    assert abs(runs[0][0].item() - v_ref) <= 1e-6
    _grad_close("ties", runs[0][1].double(), g_ref)
    assert torch.equal(runs[0][0], runs[1][0])
    assert np.array_equal(runs[0][1].numpy().view(np.uint32), runs[1][1].numpy().view(np.uint32))


def test_hinge_binary():
    """K = 1: against the restatement, and a mask with no foreground -- under the default classes ("all") the largest
    hinge error is penalised, under "present" the loss is 0."""
    from eunet import ops
    from eunet.losses import lovasz_loss
    x, t = _inputs(2, 1, 9, 11, seed=6)
    for per_image in (False, True):
        ref = R.loss(x, t, "hinge", None, per_image, IGN)
        _, g_ref = R.autograd_loss(x, t, "hinge", None, per_image, IGN, gloss=GSCALE)
        xd = x.to(DEV).requires_grad_(True)
        e_dev, _ = ops.lovasz_errors(xd.detach(), t.to(DEV), "hinge", ignore_index=IGN)
        bound = float(np.abs(e_dev.double().cpu().numpy() - ref["errors"]).max()) + 1e-7
        loss = lovasz_loss(xd, t.to(DEV), activation="hinge", per_image=per_image, ignore_index=IGN)
        (loss * GSCALE).backward()
        assert abs(loss.item() - ref["loss"]) <= bound
        _grad_close(f"hinge K1 per_image {per_image}", xd.grad.double().cpu(), g_ref)
    t0 = torch.zeros_like(t)
    xd = x.to(DEV)
    worst = float(torch.relu(1.0 + x.double()).max())
    assert worst > 0
    assert abs(lovasz_loss(xd, t0.to(DEV), activation="hinge").item() - worst) <= 1e-6
    assert lovasz_loss(xd, t0.to(DEV), activation="hinge", classes="present").item() == 0.0


def test_fused_route_equals_the_three_ops():
    """lovasz_errors -> lovasz_sort -> dot gives the bits of the fused forward: the gradient at every element and
    the segment losses (the dot in fp64 on the host, rounded once)."""
    from eunet import _lib, ops
    for (activation, K), per_image in itertools.product(MODES, (False, True)):
        x, t = _inputs(2, K, 31, 33, seed=20 + K)
        xd, td = x.to(DEV), t.to(DEV)
        weights, factor, loss, parts, counts, bad = _fwd_raw(xd, td, activation, per_image, _lib.LOVASZ_ALL, 0, IGN)
        e, f = ops.lovasz_errors(xd, td, activation, ignore_index=IGN)
        if per_image:
            es, fs = e.reshape(2 * K, -1), f.reshape(2 * K, -1)
        else:
            es, fs = (a.permute(1, 0, 2, 3).reshape(K, -1).contiguous() for a in (e, f))
        order, grad, cnt = ops.lovasz_sort(es, fs)
        g = grad.reshape(2, K, 31, 33) if per_image else grad.reshape(K, 2, 31, 33).permute(1, 0, 2, 3)
        assert torch.equal(g.contiguous().view(torch.int32), weights.view(torch.int32)), (activation, K, per_image)
        assert torch.equal(cnt, counts)
        eb = es.double().clamp_min(0.0) if activation == "hinge" else es.double()
        dot = (eb * grad.double()).sum(dim=1).float()
        assert torch.equal(dot.view(torch.int32), parts.view(torch.int32)), (activation, K, per_image, dot, parts)
        assert bad.item() == 0.0


# ---- the debug build --------------------------------------------------------------------------------
CHILD = r'''
import sys, torch
sys.path[:0] = [ROOT, ROOT + "/enhanced-unet_amd"]
from eunet import _lib
from eunet.losses import lovasz_loss
assert _lib.load().eunet_debug_enabled() == 1, "not the debug build"
torch.manual_seed(0)
t = torch.randint(0, 3, (2, 31, 33), device="cuda")
t[:, :, 0] = 255
for activation, per_image in (("softmax", False), ("softmax", True), ("hinge", False), ("hinge", True)):
    x = torch.randn(2, 3, 31, 33, device="cuda", requires_grad=True)
    lovasz_loss(x, t, activation=activation, per_image=per_image, ignore_index=255).backward()
    st = _lib.debug_status()
    print(activation, per_image, "debug status", st)
    assert st == (0, 0), (activation, per_image, st)
print("DEBUG_OK")
'''


def test_debug_build_checks_pass():
    """A forward and backward at 31 x 33 in a child process whose EUNET_LIB points at the bounds-checked build (as
    tests/test_gpu_debug.py runs the other losses): none of lovasz.hip's device checks fails."""
    lib = os.path.join(ROOT, "enhanced-unet_amd", "eunet", "libeunet_hip_debug.so")
    assert os.path.exists(lib), "build it: make -C enhanced-unet_amd debug"
    r = subprocess.run([sys.executable, "-c", CHILD.replace("ROOT", repr(ROOT))], env=dict(os.environ, EUNET_LIB=lib),
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0 and "DEBUG_OK" in r.stdout


# ---- descent ----------------------------------------------------------------------------------------
def test_descent_lowers_the_loss_and_raises_the_iou():
    """30 plain SGD steps on the logits of a 32 x 32 two-disc target: a sanity check, strictly better than at step 0."""
    from eunet.losses import lovasz_loss
    yy, xx = torch.meshgrid(torch.arange(32), torch.arange(32), indexing="ij")
    t = (((yy - 9) ** 2 + (xx - 10) ** 2 <= 36) | ((yy - 22) ** 2 + (xx - 21) ** 2 <= 25)).long()[None].to(DEV)
    g = torch.Generator().manual_seed(8)
    x = (torch.randn(1, 2, 32, 32, generator=g) * 0.1).to(DEV).requires_grad_(True)

    def iou(z):
        pred = z.argmax(1)
        return float(((pred == 1) & (t == 1)).sum()) / float(((pred == 1) | (t == 1)).sum())

    first = last = None
    iou0 = iou(x.detach())
    for step in range(31):
        loss = lovasz_loss(x, t)
        if step == 0:
            first = loss.item()
        last = loss.item()
        if step == 30:
            break
        (grad,) = torch.autograd.grad(loss, x)
        with torch.no_grad():
            x -= 100.0 * grad
    print(f"loss {first:.4f} -> {last:.4f}, IoU {iou0:.4f} -> {iou(x.detach()):.4f}")
    assert last < first and iou(x.detach()) > iou0
