"""unet on the GPU, whole model: the HIP engine (eunet/baselines.py) against the reference's
fixtures and the fp64 restatement (tests/_baseline_ref.py).  Gates and helpers are those of
tests/test_gpu_model.py (its module docstring states them)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _baseline_ref as BR
from test_gpu_model import DEV, _load, _rel, _rel_l2, _rel_px

pytestmark = pytest.mark.gpu
NAMES = ("unet",)


def _model(name, base=64, cin=3, K=3, dtype="fp32"):
    from eunet.models import get_model
    m = get_model(name, num_classes=K, in_channels=cin, base_ch=base, dtype=dtype)
    sd = {k: (v.float() if v.is_floating_point() else v) for k, v in BR.formula_weights(name, base, cin, K).items()}
    m.load_state_dict(sd)
    return m.to(DEV)


def _lowres(name, out):
    """The training loop's logits at mask size (train_eval.py:306-310): unet's 2H output resized, an exact 2x2 mean."""
    return F.avg_pool2d(out, 2)


def _pre_bn_bias(k):
    return k.endswith((".0.bias", ".3.bias"))


# ---- 6. forward -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_forward_matches_reference_fixture(golden_dir, name):
    g = _load(golden_dir, f"{name}_c3k3.npz")
    m = _model(name)
    x = torch.from_numpy(g["x"]).to(DEV)
    m.train()
    with torch.no_grad():
        out = m(x)
    assert out.shape == g["out_train"].shape
    S64 = BR.formula_weights(name, 64, 3, 3)
    with torch.no_grad():
        ref64 = BR.forward(name, S64, torch.from_numpy(g["x"]).double(), training=True)
        ref64_eval = BR.forward(name, S64, torch.from_numpy(g["x"]).double(), training=False)
    print(name, "train: vs fixture", _rel(out, g["out_train"]), "per pixel vs fp64 (floor 1e-2)", _rel_px(out, ref64),
          "| reference fp32 vs fp64", _rel_px(g["out_train"], ref64))
    assert _rel(out, g["out_train"]) < 1e-3
    assert _rel_px(out, ref64) < 1e-3
    sd = m.state_dict()
    for k in g.files:
        if k.startswith("bn:"):
            assert _rel(sd[k[3:]], g[k]) < 1e-3, k
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1, k
    m.eval()
    with torch.no_grad():
        out_e = m(x)
        low_e = m.forward_lowres(x)
    print(name, "eval: vs fixture", _rel(out_e, g["out_eval"]), "per pixel vs fp64", _rel_px(out_e, ref64_eval))
    assert _rel(out_e, g["out_eval"]) < 1e-3
    assert _rel_px(out_e, ref64_eval) < 1e-3
    # forward_lowres: the 2x2 mean of the 2H output
    want = _lowres(name, out_e.double())
    assert low_e.shape == want.shape
    assert float((low_e.double() - want).abs().max()) <= 1e-6 * float(out_e.abs().max())
    m.train()
    with torch.no_grad():  # train mode without grad: the same kernels, batch statistics
        low_t = m.forward_lowres(x)
    assert float((low_t.double() - _lowres(name, out.double())).abs().max()) <= 1e-6 * float(out.abs().max())


# ---- 7. one training step against the branch-pinned restatement ------------------------------------------
def _gpu_step(name, m, x, msk):
    """Forward + loss (the model's Trainer row) + backward with the engine's state kept; returns
    (logits, loss, pins of the branches the kernels took)."""
    import _pins
    from eunet.losses import combined_loss
    from eunet.train_eval import Trainer
    prm = Trainer(m, DEV, name, total_epochs=50).loss_params()
    _pins.keep(m)
    m.train()
    logits = m.forward_lowres(x.to(DEV))
    loss = combined_loss(logits, msk.to(DEV), params=prm)
    loss.backward()
    torch.cuda.synchronize()
    eng = m._engine
    pins = _pins.trunk_pins(eng.last_state, eng.dtype)
    _pins.keep(m, False)
    eng.last_state = None
    return logits.detach(), loss, pins


def _ref_grads(name, base, cin, K, x, msk, dtype, pins, label=None):
    import _pins
    S = BR.formula_weights(name, base, cin, K, dtype=dtype)
    for k in S:
        if S[k].is_floating_point() and "running" not in k:
            S[k].requires_grad_(True)
    rec = {} if label else None
    loss = BR.batch_loss(name, BR.forward(name, S, x.to(dtype), True, pins=pins, record=rec), msk)
    if rec is not None:
        _pins.audit(pins, rec, "fp32", label=label)
    loss.backward()
    return S, loss


@pytest.mark.parametrize("base,cin,K,H", [(64, 3, 3, 32), (16, 1, 2, 64)])
@pytest.mark.parametrize("name", NAMES)
def test_train_grads_match_restatement(name, base, cin, K, H):
    """Loss and every parameter gradient of one train step vs the fp64 restatement evaluated on the branch
    configuration the GPU took (gate of test_gpu_model.test_train_grads_match_oracle)."""
    from eunet import synth
    x, msk = synth.batch(2, H, H, start_index=7, num_classes=K, in_channels=cin)
    m = _model(name, base, cin, K)
    _, loss, pins = _gpu_step(name, m, x, msk)
    S, loss_ref = _ref_grads(name, base, cin, K, x, msk, torch.float64, pins, label=f"{name} b{base} c{cin} K{K} {H}^2")
    S32, _ = _ref_grads(name, base, cin, K, x, msk, torch.float32, pins)
    print(name, "loss", loss.item(), "restatement", loss_ref.item())
    assert abs(loss.item() - loss_ref.item()) < 1e-4 * abs(loss_ref.item())
    scale = max(float(S[k].grad.abs().max()) for k in S if S[k].grad is not None)
    rows = []
    for k, p in m.named_parameters():
        ref = S[k].grad
        assert p.grad is not None, k
        if _pre_bn_bias(k):  # exactly-zero true gradient: compare against the global gradient scale
            assert float((p.grad.double().cpu() - ref).abs().max()) < 1e-4 * scale, k
            continue
        tol = max(1e-3, 3.0 * _rel_l2(S32[k].grad, ref))
        rows.append((_rel_l2(p.grad, ref) / tol, k, _rel_l2(p.grad, ref), tol))
    for r in sorted(rows, reverse=True)[:4]:
        print(f"grads {name} b{base} c{cin} K{K} {H}^2 (ratio, name, err, tol):", r)
    assert all(r[0] < 1.0 for r in rows), sorted(rows, reverse=True)[:3]
    for k, v in m.state_dict().items():
        if "running" in k:
            assert _rel(v, S[k]) < 1e-3, k


# ---- 8. Trainer.step against the reference's step ----------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_trainer_step_matches_reference_fixture(golden_dir, name):
    """Trainer.step on the fixture batch: lr, loss and the post-AdamW
    parameters under the tolerance formula of test_gpu_model.test_trainer_step_matches_reference_fixture."""
    from eunet.train_eval import Trainer
    g = _load(golden_dir, f"step_{name}_c3k3.npz")
    m = _model(name)
    tr = Trainer(m, DEV, name, total_epochs=50)
    lr = tr.epoch_lr_step(0)
    assert abs(lr - float(g["lr"])) < 1e-12
    loss = tr.step(torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["m"]).to(DEV))
    print(name, "step loss", loss, "reference", float(g["loss"]))
    assert abs(loss - float(g["loss"])) < 1e-4 * abs(float(g["loss"]))
    sd = m.state_dict()
    for k in sd:
        if "num_batches" in k:
            continue
        post = sd[k].double().cpu().reshape(-1)
        if f"post:{k}" in g.files:
            ref = torch.from_numpy(np.asarray(g[f"post:{k}"])).reshape(-1)
            gref = torch.from_numpy(np.asarray(g[f"grad:{k}"])).reshape(-1) if f"grad:{k}" in g.files else None
        else:
            idx = torch.from_numpy(g[f"post_idx:{k}"])
            post, ref = post[idx], torch.from_numpy(g[f"post_val:{k}"])
            gref = torch.from_numpy(g[f"grad_val:{k}"]).reshape(-1) if f"grad_val:{k}" in g.files else None
        if _pre_bn_bias(k):
            assert float((post - ref).abs().max()) < 2.0 * lr, k
            continue
        tol = 0.05 * lr + 1e-6 * ref.abs().max()
        if gref is not None:
            eps = 1e-8
            ga = gref.double().abs()
            dg = 2e-3 * float(ga.max())
            lin = lr * eps * dg / ((ga - dg).clamp_min(0) + eps) ** 2
            tol = tol + torch.where(ga <= dg, torch.full_like(ga, 2.0 * lr), lin)
        assert bool(((post - ref).abs() < tol).all()), (k, float((post - ref).abs().max()))


# ---- 9. bf16 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_bf16_forward_vs_fp32_restatement(name):
    """bf16 forward_lowres (base 64, c 1, K 2, 128^2, B 2) vs the fp32 restatement, judged against what CPU bf16
    autocast of the restatement itself achieves (gate of test_gpu_model.test_bf16_forward_dice_vs_fp32_cpu)."""
    from eunet import synth
    x, _ = synth.batch(2, 128, 128, start_index=3, num_classes=2, in_channels=1)
    with torch.no_grad():
        ref = _lowres(name, BR.forward(name, BR.formula_weights(name, 64, 1, 2, dtype=torch.float32), x, True)).double()
        with torch.autocast("cpu", dtype=torch.bfloat16):
            ac = BR.forward(name, BR.formula_weights(name, 64, 1, 2, dtype=torch.float32), x, True)
        ac = _lowres(name, ac.float())
    m = _model(name, 64, 1, 2, dtype="bf16").train()
    with torch.no_grad():
        out = m.forward_lowres(x.to(DEV)).double().cpu()

    def metrics(o):
        o = o.double()
        return float((o - ref).norm() / ref.norm()), (o.argmax(1) == ref.argmax(1)).double().mean().item()

    ours, auto = metrics(out), metrics(ac)
    print(name, "bf16 ours (relL2, agree):", ours, "autocast:", auto)
    assert ours[0] < max(2.0 * auto[0], 0.02), (ours, auto)
    assert ours[1] > min(0.97, auto[1] - 0.02), (ours, auto)


@pytest.mark.parametrize("name", NAMES)
def test_bf16_train_step_runs_and_is_finite(name):
    """The bf16 backward end to end (base 16: 16 / 32 / 64 channels, 2 / 4 / 8 bf16 units): the
    loss within 1e-2 of the fp32 engine's (the bf16 loss floor of test_gpu_model's bf16 gradient test), every
    gradient finite and nearer to the fp32 engine's than to zero (rel L2 < 1: a sanity bound on a wrong operand or
    slot, not an accuracy gate -- bf16 storage alone costs the deep encoder weights 0.3-0.5, as that test
    documents; biases ahead of a BatchNorm, whose true gradient is 0, excluded).  Figures printed."""
    from eunet import synth
    from eunet.losses import combined_loss
    x, msk = synth.batch(2, 64, 64, start_index=13, num_classes=2, in_channels=1)
    grads, losses = {}, {}
    for dt in ("fp32", "bf16"):
        m = _model(name, 16, 1, 2, dtype=dt).train()
        loss = combined_loss(m.forward_lowres(x.to(DEV)), msk.to(DEV))
        loss.backward()
        torch.cuda.synchronize()
        losses[dt] = loss.item()
        grads[dt] = {k: p.grad.detach().double().cpu() for k, p in m.named_parameters()}
    print(name, "bf16 / fp32 loss", losses["bf16"], losses["fp32"])
    assert abs(losses["bf16"] - losses["fp32"]) < 1e-2 * abs(losses["fp32"])
    rows = []
    for k, gb in grads["bf16"].items():
        assert bool(torch.isfinite(gb).all()), k
        if not _pre_bn_bias(k):
            rows.append((_rel_l2(gb, grads["fp32"][k]), k))
    print(name, "bf16 vs fp32 engine gradients, worst rel L2:", sorted(rows, reverse=True)[:4])
    assert all(r[0] < 1.0 for r in rows), sorted(rows, reverse=True)[:3]


# ---- 10. schedules ------------------------------------------------------------------------------------------
def test_step_graph_replay_is_exact(name="unet"):
    """Trainer.step_graph with unet: 2 eager warm-up steps, a capture and two replays against eager steps from the
    same weights -- losses, parameters, AdamW moments and BN statistics bit for bit (fp32)."""
    from eunet import synth
    from eunet.train_eval import Trainer
    batches = []
    for i in range(4):
        x, msk = synth.batch(2, 64, 96, start_index=5 * i + 1, num_classes=3, in_channels=3)
        batches.append((x.to(DEV), msk.to(DEV)))
    ta = Trainer(_model(name, 16, 3, 3), DEV, name, total_epochs=12)
    tb = Trainer(_model(name, 16, 3, 3), DEV, name, total_epochs=12)
    tb.step_graph = True
    for i, (x, m) in enumerate(batches):
        assert torch.equal(ta.step(x, m, sync_loss=False), tb.step(x, m, sync_loss=False)), i
    assert tb._graph is not None and tb.graph_captures == 1
    for (k, p), q in zip(ta.model.named_parameters(), tb.model.parameters()):
        assert torch.equal(p, q), k
        sa, sb = ta.optimizer.state[p], tb.optimizer.state[q]
        for s in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(sa[s], sb[s]), (k, s)
    for (k, a), b in zip(ta.model.named_buffers(), tb.model.buffers()):
        assert torch.equal(a, b), k


@pytest.mark.parametrize("name", NAMES)
def test_sink_sees_parameters_in_backward_order(name):
    """A recording sink: ready() reports follow backward_param_order() (eunet.dp's bucket layout) -- the reports,
    each a set of finished parameters, are consecutive runs of that order -- and name every parameter once."""
    from eunet import synth
    from eunet.dp import backward_order
    from eunet.engine import GradSink
    from eunet.losses import combined_loss

    class Rec(GradSink):
        reports = []

        def ready(self, names):
            Rec.reports.append(list(names))

    m = _model(name, 16, 1, 2).train()
    m.grad_sink_factory = lambda: Rec(DEV)
    x, msk = synth.batch(2, 32, 32, start_index=2, num_classes=2, in_channels=1)
    combined_loss(m.forward_lowres(x.to(DEV)), msk.to(DEV)).backward()
    torch.cuda.synchronize()
    order = backward_order(m)
    flat = [n for r in Rec.reports for n in r]
    assert sorted(flat) == sorted(n for n, _ in m.named_parameters()) and len(set(flat)) == len(flat)
    pos = {n: i for i, n in enumerate(order)}
    lo = 0
    for r in Rec.reports:
        assert sorted(pos[n] for n in r) == list(range(lo, lo + len(r))), (r, lo)
        lo += len(r)
    for k, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k


# ---- 11. Evaluator and train_model -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_evaluator_single_forward(name):
    """Evaluator(m, 'cuda', name, preprocess=None): no TTA for the baseline (train_eval.py:604-652), one forward;
    _run_model_single on a 40x56 image (reflect pad to 64x64 and crop) vs the restatement's fp64 softmax."""
    from eunet.train_eval import Evaluator
    g = torch.Generator().manual_seed(71)
    xw = torch.rand(2, 3, 64, 64, generator=g)
    img = torch.rand(3, 40, 56, generator=g)
    m = _model(name).train()
    with torch.no_grad():
        m(xw.to(DEV))  # one train forward: BN running statistics away from (0, 1)
    S = BR.formula_weights(name, 64, 3, 3)
    with torch.no_grad():
        BR.forward(name, S, xw.double(), True)
        xp = F.pad(img.double()[None], (0, 8, 0, 24), mode="reflect")
        ref = torch.softmax(_lowres(name, BR.forward(name, S, xp, False))[0], 0)[:, :40, :56]
    m.eval()
    ev = Evaluator(m, DEV, name, preprocess=None)
    assert ev.enable_tta is False
    calls = []
    h = m.register_forward_hook(lambda *a: calls.append(1))
    fl, n_low = m.forward_lowres, []
    m.forward_lowres = lambda t: (n_low.append(1), fl(t))[1]
    try:
        with torch.no_grad():
            p = ev._run_model_single(ev._prepare_image_tensor(img))
            p_tta = ev._run_tta_inference(ev._prepare_image_tensor(img))
    finally:
        h.remove()
        del m.forward_lowres
    assert len(calls) + len(n_low) == 2  # one network forward per call
    assert tuple(p.shape) == (3, 40, 56) and torch.equal(p, p_tta)
    print(name, "evaluator probabilities, max abs err:", float((p.double().cpu() - ref).abs().max()))
    assert float((p.double().cpu() - ref).abs().max()) < 1e-3
    assert ev.predict_semantic_mask(img).shape == (40, 56)


@pytest.mark.parametrize("name,num_epochs,ran", [("unet", 3, 3)])
def test_train_model_writes_reference_checkpoint(tmp_path, monkeypatch, name, num_epochs, ran):
    """train_model on a synthetic loader at 64^2.  The first checkpoint can only be written at the first
    validation (every third epoch), so it runs three epochs."""
    from eunet import synth, train_eval
    from eunet.models import get_model
    from eunet.train_eval import CHECKPOINT_KEYS, load_checkpoint, train_model
    epochs = []
    inner = train_eval.Trainer.train_epoch
    monkeypatch.setattr(train_eval.Trainer, "train_epoch", lambda self, dl: (epochs.append(1), inner(self, dl))[1])
    loader = synth.loader(1, 2, 64, 64, start_index=40, num_classes=3, in_channels=3)
    path = train_model(name, device=DEV, num_epochs=num_epochs, train_loader=loader, save_dir=str(tmp_path),
                       verbose=False, base_ch=16)
    assert len(epochs) == ran
    assert os.path.exists(path)
    m = get_model(name, num_classes=3, base_ch=16)
    ck = load_checkpoint(m, path)
    assert tuple(ck.keys()) == CHECKPOINT_KEYS
    assert len(ck["history"]["train_loss"]) == ck["epoch"] and ck["epoch"] % 3 == 0 and ck["epoch"] <= ran
    assert all(np.isfinite(v) for v in ck["history"]["train_loss"])
