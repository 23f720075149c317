"""Host side of the sigmoid BCE + Dice loss: the fp64 restatement the GPU tests compare with
(tests/_bce_ref.py) against torch's own BCE and an autograd Dice, and the Python layer's argument
handling (make_bce_dice_params, BCEDiceLoss, the Evaluator's keywords), none of which needs a GPU."""
import pytest
import torch
import torch.nn.functional as F

import _bce_ref as B

IGN = 255
G = 3.7


def _autograd(x32, target, s):
    """F.binary_cross_entropy_with_logits(weight, pos_weight) over the valid pixels + a Dice written with
    torch ops, in fp64; the gradient of G * loss by autograd."""
    x = x32.double().clone().requires_grad_(True)
    N, K = x.shape[:2]
    t, valid, _ = B.targets(target, K, s["ignore_index"], s["target_mode"])
    pw = torch.tensor(s["pos_weight"][:K], dtype=torch.float64)
    cw = torch.tensor(s["class_weight"][:K], dtype=torch.float64)
    xs, ts = x.movedim(1, -1)[valid], t.movedim(1, -1)[valid]  # [V, K]
    if xs.numel():
        bce = F.binary_cross_entropy_with_logits(xs, ts, weight=cw, pos_weight=pw, reduction="mean")
    else:
        bce = x.sum() * 0.0
    dice = x.new_zeros(())
    for n in range(N):
        for c in range(K):
            p = torch.sigmoid(x[n, c])[valid[n]]
            tt = t[n, c][valid[n]]
            dice = dice + s["dice_weight"][c] * (1 - (2 * (p * tt).sum() + s["smooth"]) /
                                                 (p.sum() + tt.sum() + s["smooth"])) / K
    loss = s["w_bce"] * bce + s["w_dice"] * dice / N
    (loss * G).backward()
    return float(loss.detach()), x.grad


@pytest.mark.parametrize("ignore", [False, True])
@pytest.mark.parametrize("K,mode", [(1, None), (1, "foreground"), (2, None), (2, "onehot"), (3, "onehot")])
def test_restatement_equals_torch_bce_plus_autograd_dice(K, mode, ignore):
    g = torch.Generator().manual_seed(5 + K)
    x = (torch.randn(3, K, 9, 11, generator=g, dtype=torch.float64) * 2).float()
    target = torch.randint(0, 3 if K == 1 else K, (3, 9, 11), generator=g)
    if ignore:
        target.view(-1)[::7] = IGN
        target[2] = IGN  # one sample without a valid pixel
    s = B.spec(pos_weight=(1.5, 3.0, 0.5), class_weight=(2.0, 1.0, 3.0), dice_weight=(1.0, 15.0, 8.0), w_bce=0.7,
               w_dice=1.3, ignore_index=IGN if ignore else None, target_mode=mode)
    v_ref, g_ref = _autograd(x, target, s)
    v, parts, grad = B.bce_dice(x, target, g=G, **s)
    assert abs(v - v_ref) <= 1e-12 * max(1.0, abs(v_ref)), (v, v_ref)
    assert float((grad - g_ref).abs().max()) <= 1e-12
    assert parts.shape == (3, 2)
    if ignore:
        assert float(parts[2].abs().max()) == 0.0
        assert float(grad[2].abs().max()) == 0.0


def test_restatement_all_ignored_is_exactly_zero():
    x = torch.randn(2, 1, 4, 5)
    v, parts, grad = B.bce_dice(x, torch.full((2, 4, 5), IGN), ignore_index=IGN)
    assert v == 0.0 and float(parts.abs().max()) == 0.0 and float(grad.abs().max()) == 0.0


def test_make_bce_dice_params_tables():
    from eunet import _lib
    from eunet.losses import NO_IGNORE, BCEDiceLoss, make_bce_dice_params
    p = make_bce_dice_params()
    assert list(p.pos_weight) == list(p.class_weight) == list(p.dice_weight) == [1.0, 1.0, 1.0]
    assert (p.w_bce, p.w_dice, p.ignore_index, p.target_mode) == (1.0, 1.0, NO_IGNORE, _lib.BCE_TARGET_AUTO)
    assert abs(p.smooth - 1e-6) < 1e-12
    p = make_bce_dice_params(pos_weight=2.0, class_weight=[2.0, 1.0], dice_weight=torch.tensor([1.0, 15.0, 8.0]),
                             w_bce=0.5, w_dice=0.0, smooth=1.0, ignore_index=255, target_mode="onehot")
    assert list(p.pos_weight) == [2.0, 2.0, 2.0]
    assert list(p.class_weight) == [2.0, 1.0, 0.0]
    assert list(p.dice_weight) == [1.0, 15.0, 8.0]
    assert (p.w_bce, p.w_dice, p.smooth, p.ignore_index, p.target_mode) == (0.5, 0.0, 1.0, 255,
                                                                            _lib.BCE_TARGET_ONEHOT)
    with pytest.raises(ValueError):
        make_bce_dice_params(pos_weight=[1.0, 2.0, 3.0, 4.0])
    with pytest.raises(ValueError):
        make_bce_dice_params(target_mode="binary")
    with pytest.raises(ValueError):
        make_bce_dice_params(smooth=0.0)
    # the default mode follows K at call time; foreground is K = 1's mode and its only one
    m = BCEDiceLoss(pos_weight=[3.0])
    assert m.params(1).target_mode == _lib.BCE_TARGET_FOREGROUND
    assert m.params(2).target_mode == _lib.BCE_TARGET_ONEHOT
    assert m.params().target_mode == _lib.BCE_TARGET_AUTO
    with pytest.raises(ValueError):
        BCEDiceLoss(target_mode="foreground").params(2)
    with pytest.raises(ValueError):
        BCEDiceLoss(target_mode="onehot").params(1)
    m.pos_weight = [5.0]
    assert bytes(m.params(1)) != bytes(BCEDiceLoss(pos_weight=[3.0]).params(1))


def test_foreground_with_two_logits_is_refused_before_the_device():
    from eunet.losses import bce_dice_loss, make_bce_dice_params
    with pytest.raises(ValueError):
        bce_dice_loss(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long),
                      params=make_bce_dice_params(target_mode="foreground"))


def test_bce_dice_loss_on_cpu_tensors_raises():
    from eunet import EunetError
    from eunet.losses import BCEDiceLoss, bce_dice_loss
    x, t = torch.zeros(1, 1, 4, 4, requires_grad=True), torch.zeros(1, 4, 4, dtype=torch.long)
    with pytest.raises(EunetError):
        bce_dice_loss(x, t)
    with pytest.raises(EunetError):
        BCEDiceLoss()(x, t)


def test_evaluator_activation_keyword():
    from eunet.evaluator import Evaluator
    from eunet.models import EnhancedUNet
    m = EnhancedUNet(num_classes=3, in_channels=1, base_ch=16)
    e = Evaluator(m, "cpu", "enhanced_unet")
    assert e.activation == "softmax"
    e = Evaluator(m, "cpu", "enhanced_unet", activation="sigmoid", threshold=0.4)
    assert e.activation == "sigmoid" and e.threshold == 0.4
    with pytest.raises(ValueError):
        Evaluator(m, "cpu", "enhanced_unet", activation="tanh")
    with pytest.raises(ValueError):
        e.evaluate_binary([])  # three logits
    with pytest.raises(ValueError):
        Evaluator(m, "cpu", "enhanced_unet").evaluate_binary([])


def test_new_ops_are_dispatcher_ops_and_refuse_cpu_tensors():
    from eunet import EunetError, ops
    assert {"bce_dice_fwd", "bce_dice_bwd", "sigmoid_crop", "probs_threshold"} <= set(ops.DISPATCHED)
    with pytest.raises(EunetError):
        ops.sigmoid_crop(torch.zeros(1, 4, 4), 3, 3)
    with pytest.raises(EunetError):
        ops.probs_threshold(torch.zeros(1, 4, 4))
