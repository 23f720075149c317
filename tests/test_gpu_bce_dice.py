"""bce_dice.hip: the sigmoid BCE + soft Dice loss and the evaluator's sigmoid ops at the edges of their launches.

bce_dice_fwd_kernel reduces 1024 pixels of one sample per block (16-byte loads when H*W is a multiple of
4, scalar ones otherwise), bce_dice_finalize_kernel combines a sample's tiles (256 threads striding over
them, then a 128-wide LDS tree) and the batch's samples (at most 64), bce_dice_bwd_kernel is per pixel.  The
pixel count sits on either side of a tile (1, 1023, 1024, 1025 px: the scalar path three times, the vector
path at 1024), one sample has 257 tiles (513x512, the vector path), the batch is at and past its limit.

Everything goes through eunet.losses.bce_dice_loss(..., return_parts=True) and (loss * 3.7).backward().
There is no reference implementation: the comparison is with tests/_bce_ref.py, the definition of
include/eunet.h restated in fp64 on the fp32 logits as stored (tests/test_bce_dice_host.py holds it to
torch's own BCE and an autograd Dice within 1e-12).

Gates (the project's loss gates, tests/test_gpu_loss_edges.py): value and every part within 1e-5 relative
(1e-7 absolute where the reference is exactly 0); gradients within 1e-4 of the largest reference gradient,
and per element within 1e-3 relative with a floor of 1e-3 of the largest.
"""
import pytest
import torch
import torch.nn.functional as F

import _bce_ref as B

pytestmark = pytest.mark.gpu
DEV = "cuda"
GSCALE = 3.7
IGN = 255


def _params(s):
    from eunet.losses import make_bce_dice_params
    return make_bce_dice_params(pos_weight=list(s["pos_weight"]), class_weight=list(s["class_weight"]),
                                dice_weight=list(s["dice_weight"]), w_bce=s["w_bce"], w_dice=s["w_dice"],
                                smooth=s["smooth"], ignore_index=s["ignore_index"], target_mode=s["target_mode"])


def _gpu(x32, target, s):
    from eunet.losses import bce_dice_loss
    x = x32.to(DEV).requires_grad_(True)
    loss, parts = bce_dice_loss(x, target.to(DEV), return_parts=True, params=_params(s), track_targets=False)
    (loss * GSCALE).backward()
    torch.cuda.synchronize()
    return loss.item(), parts.double().cpu(), x.grad.double().cpu()


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


def _check(name, x32, target, s=None, ref_target=None, ref_spec=None):
    """ref_target / ref_spec: what the restatement sees where it differs from what the kernel is given."""
    s = s or B.spec()
    v_ref, p_ref, g_ref = B.bce_dice(x32, target if ref_target is None else ref_target, g=GSCALE, **(ref_spec or s))
    v, parts, g = _gpu(x32, target, s)
    mx, per = _grad_close(name, g, g_ref)
    print(f"{name}: value {v:.8g} (ref {v_ref:.8g}), grad err / max {mx:.2e}, worst element {per:.2e}")
    assert v == v and abs(v) != float("inf"), name
    _close(name + " value", v, v_ref)
    assert parts.shape == p_ref.shape
    for n in range(p_ref.shape[0]):
        for i, term in enumerate(("bce", "dice")):
            _close(f"{name} parts[{n}].{term}", float(parts[n, i]), float(p_ref[n, i]))
    return v, g


def _inputs(N, K, H, W, seed, scale=2.0):
    """K = 1 draws targets from {0, 1, 2}: the foreground mode maps 2 -> 1."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(N, K, H, W, generator=g, dtype=torch.float64) * scale).float()
    t = torch.randint(0, 3 if K == 1 else K, (N, H, W), generator=g)
    return x, t, g


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (31, 33), (32, 32), (25, 41)])
def test_pixel_counts_around_one_tile(H, W, K):
    """1, 1023, 1024 and 1025 px per sample (the second tile of 25x41 holds one pixel), N = 3, K = 1..3.
    K = 1 runs again with every seventh pixel at ignore index 255."""
    x, t, _ = _inputs(3, K, H, W, seed=100 + H + K)
    if K == 1 and H * W > 1:
        assert int((t == 2).sum()) > 0
    _check(f"{H}x{W} K{K}", x, t)
    if K == 1:
        t.view(-1)[::7] = IGN
        _check(f"{H}x{W} K1 ignore", x, t, B.spec(ignore_index=IGN))


def test_257_tiles_in_one_sample():
    """513x512 = 262 656 px = 257 tiles: thread 0 of the finalize reads two tiles and every slot of its LDS
    tree holds a partial.  N = 1, K = 1; value, parts and the gradient of every pixel."""
    x, t, _ = _inputs(1, 1, 513, 512, seed=7)
    _check("513x512", x, t)


def test_batch_of_64_and_65():
    """64 samples is the limit of the finalize's per-sample LDS arrays; 65 is refused by the library."""
    from eunet._lib import EunetError
    from eunet.losses import bce_dice_loss
    x, t, _ = _inputs(65, 3, 5, 7, seed=11)
    _check("N=64", x[:64].contiguous(), t[:64].contiguous())
    with pytest.raises(EunetError):
        bce_dice_loss(x.to(DEV), t.to(DEV), track_targets=False)


PARAM_SETS = {
    "defaults": B.spec(),
    "pos_weight": B.spec(pos_weight=(1.5, 3.0, 0.5)),
    "class_weight": B.spec(class_weight=(2.0, 1.0, 3.0)),
    "dice_weight": B.spec(dice_weight=(1.0, 15.0, 8.0)),
    "bce_only": B.spec(pos_weight=(1.5, 3.0, 0.5), class_weight=(2.0, 1.0, 3.0), w_dice=0.0),
    "dice_only": B.spec(w_bce=0.0),
    "smooth1": B.spec(smooth=1.0),
    "ignore255": B.spec(ignore_index=IGN),
}


@pytest.mark.parametrize("name", list(PARAM_SETS))
def test_parameter_sets(name):
    """3 x 25x41 (two tiles per sample), K = 3.  bce_only (w_dice = 0) is also compared directly with
    F.binary_cross_entropy_with_logits(weight, pos_weight) in fp64; ignore255: about 10 % of the pixels."""
    s = PARAM_SETS[name]
    g = torch.Generator().manual_seed(21)
    x = (torch.randn(3, 3, 25, 41, generator=g, dtype=torch.float64) * 2).float()
    t = torch.randint(0, 3, (3, 25, 41), generator=g)
    if s["ignore_index"] is not None:
        t = t.clone()
        t[torch.rand(t.shape, generator=g) < 0.1] = IGN
        assert 0.05 < float((t == IGN).float().mean()) < 0.15
    v, grad = _check(name, x, t, s)
    if name == "bce_only":
        xd = x.double().requires_grad_(True)
        ref = F.binary_cross_entropy_with_logits(
            xd, F.one_hot(t, 3).movedim(-1, 1).double(),
            weight=torch.tensor(s["class_weight"], dtype=torch.float64).view(1, 3, 1, 1),
            pos_weight=torch.tensor(s["pos_weight"], dtype=torch.float64).view(1, 3, 1, 1))
        (ref * GSCALE).backward()
        _close("bce_only against torch", v, ref.item())
        _grad_close("bce_only against torch", grad, xd.grad)


def test_degenerate_targets():
    """A sample in which class 2 never occurs (T_2 = 0), a sample that is class 2 throughout, one fully
    ignored sample among valid ones."""
    x, t, g = _inputs(4, 3, 25, 41, seed=31)
    t[1] = torch.randint(0, 2, (25, 41), generator=g)
    t[2] = 2
    _check("degenerate targets", x, t)
    t[3] = IGN
    v, grad = _check("one ignored sample", x, t, B.spec(ignore_index=IGN))
    assert float(grad[3].abs().max()) == 0.0


@pytest.mark.parametrize("K", [1, 3])
def test_fully_ignored_batch_is_exactly_zero(K):
    from eunet.losses import bce_dice_loss, make_bce_dice_params
    x, _, _ = _inputs(3, K, 25, 41, seed=33)
    xd = x.to(DEV).requires_grad_(True)
    t = torch.full((3, 25, 41), IGN, device=DEV)
    loss, parts = bce_dice_loss(xd, t, return_parts=True, params=make_bce_dice_params(ignore_index=IGN),
                                track_targets=False)
    (loss * GSCALE).backward()
    assert loss.item() == 0.0
    assert float(parts.abs().max()) == 0.0
    assert float(xd.grad.abs().max()) == 0.0


@pytest.mark.parametrize("span", [40.0, 100.0])
def test_saturated_logits(span):
    """Logits uniform in +-40 and +-100: exp(-|x|) underflows, sp and the sigmoid pair neither overflow nor
    cancel.  Loss and gradients stay finite and within the gates."""
    g = torch.Generator().manual_seed(41)
    x = ((torch.rand(3, 3, 25, 41, generator=g, dtype=torch.float64) * 2 - 1) * span).float()
    t = torch.randint(0, 3, (3, 25, 41), generator=g)
    assert float(x.abs().max()) > span - 1.0
    _check(f"saturated {span}", x, t, B.spec(pos_weight=(1.5, 3.0, 0.5)))
    x1 = x[:, :1].contiguous()
    _check(f"saturated {span} K1", x1, t)


@pytest.mark.parametrize("K,badval", [(3, 3), (1, -3)])
def test_out_of_range_targets_in_both_tiles(K, badval):
    """25x41: 7 bad targets in the first tiles and 5 in the second tiles (value K in onehot mode, -3 in
    foreground mode).  The second tile of a 1025 px sample is one pixel, so the batch has 5 samples and the
    last pixel of each is out of range.  sums[-1] counts all 12; the loss and the gradient are those of the
    restatement with the 12 pixels ignored; check_targets() raises."""
    from eunet import losses, ops
    N, H, W = 5, 25, 41
    x, t, g = _inputs(N, K, H, W, seed=51)
    bad = t.clone()
    flat = bad.view(N, -1)
    flat[:, 1024] = badval
    for n, p in ((0, 0), (0, 1023), (1, 517), (2, 255), (2, 256), (3, 640), (4, 3)):
        flat[n, p] = badval
    assert int((bad == badval).sum()) == 12 and int((flat[:, :1024] == badval).sum()) == 7
    ign = bad.clone()
    ign[bad == badval] = IGN
    xd, td = x.to(DEV), bad.to(DEV)
    sums = torch.empty(ops.bce_dice_sums_len(N, K), dtype=torch.float32, device=DEV)
    loss = torch.empty((), dtype=torch.float32, device=DEV)
    parts = torch.empty(N, 2, dtype=torch.float32, device=DEV)
    ws = torch.empty(ops.bce_dice_workspace_bytes(N, K, H, W), dtype=torch.uint8, device=DEV)
    ops.bce_dice_fwd(xd, td, None, sums, loss, parts, ws)
    torch.cuda.synchronize()
    assert sums[-1].item() == 12.0
    assert sums[-2].item() == float(N * H * W - 12)  # V: the valid pixels
    _check("out of range", x, bad, ref_target=ign, ref_spec=B.spec(ignore_index=IGN))
    try:  # start from a clean count, whatever ran before in this process (_check does not track)
        losses.check_targets()
    except ValueError:
        pass
    losses.bce_dice_loss(xd, td)
    with pytest.raises(ValueError):
        losses.check_targets()
    losses.check_targets()  # the count was cleared


def test_library_refuses_bad_modes_and_smooth():
    from eunet import _lib, ops
    from eunet._lib import EunetError
    x = torch.zeros(1, 2, 4, 4, device=DEV)
    t = torch.zeros(1, 4, 4, dtype=torch.long, device=DEV)
    sums = torch.empty(ops.bce_dice_sums_len(1, 2), device=DEV)
    loss, parts = torch.empty((), device=DEV), torch.empty(1, 2, device=DEV)
    ws = torch.empty(ops.bce_dice_workspace_bytes(1, 2, 4, 4), dtype=torch.uint8, device=DEV)
    p = ops.bce_dice_default_params()
    p.target_mode = _lib.BCE_TARGET_FOREGROUND
    with pytest.raises(EunetError):
        ops.bce_dice_fwd(x, t, p, sums, loss, parts, ws)
    p = ops.bce_dice_default_params()
    p.smooth = 0.0
    with pytest.raises(EunetError):
        ops.bce_dice_fwd(x, t, p, sums, loss, parts, ws)
    with pytest.raises(EunetError):
        ops.bce_dice_bwd(x, t, p, sums, torch.ones(1, device=DEV), torch.empty_like(x))


# ---- the evaluator's ops ---------------------------------------------------------------------------
def _crop_inputs(K):
    g = torch.Generator().manual_seed(61 + K)
    return (torch.randn(K, 32, 40, generator=g, dtype=torch.float64) * 4).float()


@pytest.mark.parametrize("K", [1, 2, 3])
def test_sigmoid_crop(K):
    """A 32x40 plane cropped to 29x31, each flip combination, against torch.sigmoid in fp64 with the same
    crop and flips.  The bound is 4 x the largest error of torch's own fp32 sigmoid (on the CPU) against fp64
    on these inputs (N(0, 4^2) logits, seeds 62..64), measured again on every run.  Measured: torch's error
    8.45e-8 / 8.63e-8 / 8.62e-8 for K = 1 / 2 / 3, so the bounds are 3.38e-7 / 3.45e-7 / 3.45e-7."""
    from eunet import ops
    x = _crop_inputs(K)
    own, bound = B.sigmoid_bound(x)
    print(f"K{K}: torch fp32 sigmoid err {own:.3e}, bound {bound:.3e}")
    assert own > 0.0
    xd = x.to(DEV)
    for fh in (False, True):
        for fw in (False, True):
            p = ops.sigmoid_crop(xd, 29, 31, flip_h=fh, flip_w=fw).double().cpu()
            ref = torch.sigmoid(x.double())[:, :29, :31]
            if fh:
                ref = ref.flip(1)
            if fw:
                ref = ref.flip(2)
            assert p.shape == (K, 29, 31)
            err = float((p - ref).abs().max())
            print(f"  flips {fh} {fw}: err {err:.3e}")
            assert err <= bound, (K, fh, fw, err, bound)


def test_probs_threshold_one_logit_is_exact():
    from eunet import ops
    g = torch.Generator().manual_seed(71)
    p = torch.rand(1, 29, 31, generator=g)
    for thr in (0.5, 0.3):
        q = p.clone()
        q.view(-1)[::5] = thr  # planted values exactly at the threshold
        q.view(-1)[1::5] = float(torch.nextafter(torch.tensor(thr), torch.tensor(0.0)))
        m = ops.probs_threshold(q.to(DEV), thr).cpu()
        assert m.dtype == torch.int64 and m.shape == (29, 31)
        assert torch.equal(m, (q[0] >= torch.tensor(thr)).long())
        assert int(m.view(-1)[::5].min()) == 1 and int(m.view(-1)[1::5].max()) == 0


@pytest.mark.parametrize("K", [2, 3])
def test_probs_threshold_argmax_first_maximum(K):
    from eunet import ops
    g = torch.Generator().manual_seed(72 + K)
    p = torch.rand(K, 29, 31, generator=g)
    flat = p.view(K, -1)
    flat[:, ::4] = flat[0, ::4].clone()  # all classes tie: class 0
    flat[K - 1, 1::4] = flat[1, 1::4] = 2.0  # the largest value twice (K = 2: once): the first holder
    if K == 3:
        flat[2, 2::4] = flat[1, 2::4] = 3.0  # classes 1 and 2 tie above class 0: class 1
    first = torch.zeros(p.shape[1:], dtype=torch.long)
    best = p[0].clone()
    for k in range(1, K):
        take = p[k] > best
        first[take] = k
        best = torch.where(take, p[k], best)
    m = ops.probs_threshold(p.to(DEV), 0.5).cpu()
    assert torch.equal(m, first)
    assert int(m.view(-1)[::4].max()) == 0
    assert int(m.view(-1)[1::4].min()) == 1 and int(m.view(-1)[1::4].max()) == 1
