"""Host-side checks of the unet baseline: schema, Trainer table, and the CPU restatement
(tests/_baseline_ref.py) against the reference's fixtures (tests/golden/gen_golden_baselines.py)."""
import os

import numpy as np
import pytest
import torch

import _baseline_ref as BR

NAMES = ("unet",)
N_PARAMS = {"unet": 7788675}
N_KEYS = {"unet": 100}


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name), allow_pickle=False)


def _rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.mark.parametrize("name", NAMES)
def test_schema_counts_and_cpu_error(golden_dir, name):
    from eunet import EunetError
    from eunet.models import get_model
    g = _load(golden_dir, f"{name}_c3k3.npz")
    m = get_model(name, num_classes=3)
    keys = list(m.state_dict().keys())
    assert keys == [str(k) for k in g["keys"]]
    assert len(keys) == N_KEYS[name]
    assert keys == [k for k, _, _ in BR.SPECS[name](64, 3, 3)]
    assert sum(p.numel() for p in m.parameters()) == N_PARAMS[name] == int(g["n_params"])
    with pytest.raises(EunetError):
        m(torch.rand(1, 3, 32, 32))
    m.eval()
    with pytest.raises(EunetError):
        m.forward_lowres(torch.rand(1, 3, 32, 32))
    order = m.backward_param_order()
    if order is not None:
        assert sorted(order) == sorted(n for n, _ in m.named_parameters()) and len(set(order)) == len(order)


@pytest.mark.parametrize("name", ["fcn", "pspnet", "segnet", "linknet", "deeplab"])
def test_unbuilt_names_raise(name):
    from eunet.models import get_model
    with pytest.raises(ValueError):
        get_model(name)


def test_model_limits():
    from eunet.models import UNet
    for cls in (UNet,):
        for kw in (dict(num_classes=4), dict(num_classes=0), dict(in_channels=5), dict(base_ch=24)):
            with pytest.raises(ValueError):
                cls(**kw)
        m = cls(num_classes=2, in_channels=1, base_ch=16, dtype="bf16")
        assert m.compute_dtype == torch.bfloat16 and m._engine.dtype == torch.bfloat16
        assert m.set_dtype("fp32")._engine.dtype == torch.float32


@pytest.mark.parametrize("name,weights,base_lr", [("unet", (1.5, 1.5, 0.5), 2e-3)])
def test_trainer_table_and_schedule(golden_dir, name, weights, base_lr):
    """train_eval.py:82-119: loss-term weights, base lr, no auxiliary supervision; the LR trajectory for
    E = 50, whose first epoch is the step fixture's recorded lr."""
    from eunet.models import get_model
    from eunet.train_eval import Trainer
    tr = Trainer(get_model(name, num_classes=2, in_channels=1, base_ch=16), "cpu", name, total_epochs=50)
    assert (tr.dice_loss_weight, tr.focal_loss_weight, tr.tversky_loss_weight) == weights
    assert tr.optimizer.param_groups[0]["initial_lr"] == base_lr
    assert tr.aux_branch_weights == {} and tr.consistency_weight == 0.0
    lrs = [tr.epoch_lr_step(e) for e in range(50)]
    ref = BR.lr_trajectory(name, 50)
    assert max(abs(a - b) for a, b in zip(lrs, ref)) < 1e-12
    g = _load(golden_dir, f"step_{name}_c3k3.npz")
    assert abs(lrs[0] - float(g["lr"])) < 1e-12
    for other in ("fcn", "linknet", "segnet"):
        with pytest.raises(ValueError):
            Trainer(torch.nn.Linear(1, 1), "cpu", other)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_forward_matches_reference(golden_dir, name):
    """fp64 restatement vs the reference's fp32 logits: the reference's own fp32 noise, at the bound
    tests/test_oracle.py holds the fp64 Enhanced-UNet restatement to (2e-5 of max|logit|)."""
    g = _load(golden_dir, f"{name}_c3k3.npz")
    S = BR.formula_weights(name, 64, 3, 3)
    x = torch.from_numpy(g["x"]).double()
    with torch.no_grad():
        out = BR.forward(name, S, x, training=True)
    assert out.shape == g["out_train"].shape
    e_train = _rel(out.numpy(), g["out_train"])
    for k in g.files:
        if k.startswith("bn:"):
            assert _rel(S[k[3:]].numpy(), g[k]) < 1e-4, k
    with torch.no_grad():
        out_e = BR.forward(name, S, x, training=False)
    e_eval = _rel(out_e.numpy(), g["out_eval"])
    print(f"{name} restatement vs reference: train {e_train:.2e} eval {e_eval:.2e}")
    assert e_train < 2e-5 and e_eval < 2e-5


def _feeds_bn(key):
    return key.endswith((".0.bias", ".3.bias"))


@pytest.mark.parametrize("name", NAMES)
def test_restatement_step_matches_reference(golden_dir, name):
    """One train_epoch step vs the reference's.  lr and loss in fp64; gradients and post-step parameters with the gates and the fp32
    run of tests/test_oracle.py's step test (the step is discontinuous at ReLU kinks and pool ties,
    and AdamW's first update is lr * sign(g): an fp64 run is a different function at those elements)."""
    g = _load(golden_dir, f"step_{name}_c3k3.npz")
    lr, loss, _ = BR.step(name, BR.formula_weights(name, 64, 3, 3), torch.from_numpy(g["x"]).double(),
                          torch.from_numpy(g["m"]))
    assert abs(lr - float(g["lr"])) < 1e-12
    print(f"{name} step loss {loss} reference {float(g['loss'])}")
    assert abs(loss - float(g["loss"])) < 1e-5 * abs(float(g["loss"]))
    S = BR.formula_weights(name, 64, 3, 3, dtype=torch.float32)
    _, loss32, grads = BR.step(name, S, torch.from_numpy(g["x"]), torch.from_numpy(g["m"]))
    assert abs(loss32 - float(g["loss"])) < 1e-5 * abs(float(g["loss"]))
    # the fixture's gradients are the clipped ones (train_epoch clips in place before the step)
    for k, gr in grads.items():
        for tag, arr in (("grad", gr.numpy()), ("post", S[k].detach().numpy())):
            if f"{tag}:{k}" in g.files:
                ref = g[f"{tag}:{k}"]
                scale = max(np.abs(ref).max(), 1e-12)
                floor = 2.0 * lr if tag == "post" and _feeds_bn(k) else 1e-6
                assert np.abs(arr.reshape(ref.shape) - ref).max() < 2e-3 * scale + floor, (tag, k)
            else:
                flat = arr.reshape(-1)
                ref_norm = float(g[f"{tag}_norm:{k}"])
                assert abs(np.sqrt((flat ** 2).sum()) - ref_norm) < 1e-3 * ref_norm, (tag, k)
                idx, ref_v = g[f"{tag}_idx:{k}"], g[f"{tag}_val:{k}"]
                assert np.abs(flat[idx] - ref_v).max() < 2e-3 * max(np.abs(ref_v).max(), 1e-12), (tag, k)
    for k in S:
        if k.endswith(("running_mean", "running_var")):
            assert _rel(S[k].numpy(), g[f"post:{k}"]) < 1e-4, k


def test_new_entry_points_declared_bound_and_dispatched():
    from eunet import _lib, ops
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "eunet.h")).read()
    for name, cite in (("eunet_ktail_fwd", "models.py:236"), ("eunet_ktail_bwd", "train_eval.py:306-310")):
        assert name in src and cite in src
        assert name in _lib.exported_symbols() and hasattr(_lib.load(), name)
        assert name[len("eunet_"):] in ops.DISPATCHED
    sch = str(torch.ops.eunet.ktail_fwd.default._schema)
    assert sch == "eunet::ktail_fwd(int mode, Tensor z_lo, Tensor(a!) out) -> ()", sch
