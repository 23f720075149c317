"""The sigmoid BCE + Dice loss on a model, and the Evaluator's sigmoid path.

Every case: enhanced_unet, base 16, 1 channel, K = 1, 32x32, batch 2, fp32 (bf16 where said).  Images are
seeded uniform noise and the masks seeded labels in {0, 1, 2}: with one logit the loss trains "cell"
([target >= 1]).

The Trainer switch (loss="bce_dice") and its step-graph key are not in the tree, so the cases that went through
Trainer.step are not here either: in the whole GPU suite a replay of an existing test's captured step ended in a
segmentation fault inside the HIP runtime's graph launch while the switch was in, the cause was not found, and
train_eval.py stays as it was.  The training cases below call bce_dice_loss in a loop of their own.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _bce_ref as B

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _model(dtype="fp32", seed=3):
    from eunet.models import EnhancedUNet
    torch.manual_seed(seed)
    return EnhancedUNet(num_classes=1, in_channels=1, base_ch=16, dtype=dtype).to(DEV)


def _batch(i=0, h=32, w=32):
    g = torch.Generator().manual_seed(200 + i)
    x = torch.rand(2, 1, h, w, generator=g)
    m = torch.randint(0, 3, (2, h, w), generator=g)
    return x.to(DEV), m.to(DEV)


def _train_forward(model, i):
    """One train-mode forward: the BN running statistics leave (0, 1)."""
    x, _ = _batch(i)
    with torch.no_grad():
        model.train().forward_lowres(x)


def test_one_logit_model_trains_with_the_sigmoid_loss():
    """A one-logit model has a gradient under bce_dice_loss (under the softmax loss it is exactly 0): every
    parameter that can have one gets a finite, nonzero gradient, and five AdamW steps lower the loss."""
    from eunet.losses import bce_dice_loss
    x, m = _batch()
    model = _model().train()
    opt = torch.optim.AdamW(model.parameters(), lr=4e-3)
    losses = []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        loss = bce_dice_loss(model.forward_lowres(x), m)
        loss.backward()
        if not losses:
            zero = [k for k, p in model.named_parameters() if p.grad is None or float(p.grad.abs().max()) == 0.0]
            # a conv bias ahead of a BatchNorm has a true gradient of 0
            assert all(k.endswith(".bias") for k in zero), zero
            assert any(float(p.grad.abs().max()) > 0 for k, p in model.named_parameters() if k.endswith(".weight"))
            assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None)
        opt.step()
        losses.append(loss.item())
    print("losses", losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_bf16_model_gives_a_finite_loss_and_gradients():
    from eunet.losses import bce_dice_loss
    x, m = _batch(1)
    model = _model("bf16").train()
    loss = bce_dice_loss(model.forward_lowres(x), m)
    loss.backward()
    print("bf16 loss", loss.item())
    assert np.isfinite(loss.item())
    assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None)


def _eval_logits(model, img):
    h, w = img.shape[1:]
    xp = F.pad(img[None].to(DEV), (0, (32 - w % 32) % 32, 0, (32 - h % 32) % 32), mode="reflect")
    with torch.no_grad():
        return model.eval().forward_lowres(xp)[0, :, :h, :w].float().cpu()


def test_evaluator_sigmoid_prediction():
    """predict_semantic_mask of a 29x31 image (one forward: TTA off) equals thresholding torch.sigmoid (fp64)
    of the model's own eval logits after the same reflect pad and crop.  A pixel may disagree only if its
    probability lies within the sigmoid bound (4 x torch's own fp32 sigmoid error on these logits,
    tests/_bce_ref.sigmoid_bound) of the threshold, and fewer than 1 % of the pixels lie there.  The threshold
    is the median probability, so both labels occur.  With TTA on the mask is still a {0, 1} mask."""
    from eunet.train_eval import Evaluator
    model = _model()
    _train_forward(model, 30)
    g = torch.Generator().manual_seed(31)
    img = torch.rand(1, 29, 31, generator=g)
    lg = _eval_logits(model, img)
    p64 = torch.sigmoid(lg.double())[0]
    thr = float(p64.median().float())
    own, bound = B.sigmoid_bound(lg)
    ev = Evaluator(model, DEV, "enhanced_unet", preprocess=None, activation="sigmoid", threshold=thr)
    ev.enable_tta = False
    mask = ev.predict_semantic_mask(img)
    assert mask.shape == (29, 31) and mask.dtype == np.int64
    ref = (p64 >= thr).long().numpy()
    near = ((p64 - thr).abs() <= bound).numpy()
    print(f"threshold {thr:.6f}, sigmoid err {own:.2e}, bound {bound:.2e}, near pixels {int(near.sum())}, "
          f"foreground {int(ref.sum())} / {ref.size}")
    assert near.mean() < 0.01
    assert 0 < int(ref.sum()) < ref.size
    assert not ((mask != ref) & ~near).any()
    ev.enable_tta = True
    tta = ev.predict_semantic_mask(img)
    assert tta.shape == (29, 31) and set(np.unique(tta)) <= {0, 1}


def test_evaluate_binary_is_the_mean_of_the_two_metrics():
    from eunet.metrics import calculate_dice, calculate_iou
    from eunet.train_eval import Evaluator
    model = _model()
    _train_forward(model, 40)
    g = torch.Generator().manual_seed(41)
    imgs = [torch.rand(1, 29, 31, generator=g), torch.rand(1, 32, 32, generator=g)]
    gts = [torch.randint(0, 3, (29, 31), generator=g), torch.randint(0, 3, (32, 32), generator=g)]
    thr = float(torch.sigmoid(_eval_logits(model, imgs[0])).median())
    ev = Evaluator(model, DEV, "enhanced_unet", preprocess=None, activation="sigmoid", threshold=thr)
    ev.enable_tta = False
    loader = [{"images": imgs, "batch_items": [{"semantic_mask": t} for t in gts]}]
    res = ev.evaluate_binary(loader)
    assert set(res) == {"bin_iou", "bin_dice"}
    preds = [ev.predict_semantic_mask(im) for im in imgs]
    ious, dices = [], []
    for p, t in zip(preds, gts):  # by hand, on the host
        a, b = p == 1, t.numpy() > 0
        ious.append((a & b).sum() / (a | b).sum())
        dices.append(2.0 * (a & b).sum() / (a.sum() + b.sum()))
        assert abs(calculate_iou(a, b) - ious[-1]) < 1e-12 and abs(calculate_dice(a, b) - dices[-1]) < 1e-12
    print("bin_iou", res["bin_iou"], "bin_dice", res["bin_dice"])
    assert abs(res["bin_iou"] - float(np.mean(ious))) < 1e-12
    assert abs(res["bin_dice"] - float(np.mean(dices))) < 1e-12
    assert 0.0 < res["bin_iou"] < 1.0
