"""Generate the unet baseline's golden fixtures by running the REFERENCE implementation (build
container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_baselines.py [name ...]

Imports the reference's models.py / train_eval.py exactly as gen_golden.py does (read-only, never
copied, inert stubs for the libraries the training path never uses; SMP absent, so get_model builds
BasicUNet).  Formula weights (oracle/weights.py) over the state_spec rows without enhance.*.

  unet_c3k3.npz       input 2x3x32x32 (seed as gen_golden.gen_forward): train logits, BN running statistics
                      after, eval logits, and the model's state_dict key list
  step_unet_c3k3.npz  one Trainer.train_epoch after warmup_scheduler.step() at 32x32: lr, loss, post-step
                      parameters and gradients (summarised as step_c3k3.npz).  The batch is the first seed at
                      which the reference's own step is stable under fp32 rounding of its input (stable_seed)
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as G  # noqa: E402  (stubs, reference import, _inputs, _bn_stats, _summaries)
from oracle.weights import formula_state_dict  # noqa: E402
from oracle.eunet_ref import state_spec  # noqa: E402


def spec_of(name):
    assert name == "unet"
    return [r for r in state_spec(64, 3, 3) if not r[0].startswith("enhance.")]


def _model(ref_models, name):
    model = ref_models.get_model(name, num_classes=3, device="cpu")
    sd = formula_state_dict(spec_of(name))
    ref_sd = model.state_dict()
    assert list(ref_sd.keys()) == list(sd.keys()), f"{name}: state_dict schema mismatch"
    model.load_state_dict({k: (torch.tensor(0, dtype=torch.long) if k.endswith("num_batches_tracked") else
                               torch.from_numpy(np.asarray(v)).float().reshape(ref_sd[k].shape))
                           for k, v in sd.items()})
    return model


def gen_forward(ref_models, name):
    torch.manual_seed(0)
    model = _model(ref_models, name)
    x, _ = G._inputs(2, 3, 32, 32, 3, seed=11)
    model.train()
    with torch.no_grad():
        out_train = model(x)
    stats = G._bn_stats(model)
    model.eval()
    with torch.no_grad():
        out_eval = model(x)
    np.savez_compressed(os.path.join(HERE, f"{name}_c3k3.npz"), x=x.numpy(), out_train=out_train.numpy(),
                        out_eval=out_eval.numpy(), keys=np.array(list(model.state_dict().keys())),
                        n_params=sum(p.numel() for p in model.parameters()),
                        **{"bn:" + k: v for k, v in stats.items()})


def _ref_step(ref_models, ref_te, name, x, m):
    model = _model(ref_models, name)
    batch = {"images": x, "batch_items": [{"semantic_mask": m[i]} for i in range(2)]}
    tr = ref_te.Trainer(model, "cpu", name, total_epochs=50)
    tr.warmup_scheduler.step()  # train_model epoch 0 (train_eval.py:1104-1105)
    lr = tr.optimizer.param_groups[0]["lr"]
    loss = tr.train_epoch([batch])
    return model, lr, loss


STABLE_DG = 2e-3   # the gradient accuracy the GPU step test's tolerance formula assumes (of a tensor's largest entry)
STABLE_TRIALS = 6


def stable_seed(ref_models, ref_te, name, H, W, first):
    """The step is discontinuous at ReLU kinks and max-pool ties, and with these inputs (uniform noise, focal
    gamma 5: few pixels carry the loss) ONE branch within fp32 rounding of its kink moves whole gradient tensors
    by 1e-2 of their scale -- five times what the fp32 step test allows any implementation (STABLE_DG).  Such an
    input pins nothing: the reference's own step changes by that much when its input moves by one fp32 rounding.
    So the fixture takes the first seed >= first at which the REFERENCE's step is stable: under STABLE_TRIALS
    perturbations of the images by 1e-7 relative (seeded), no parameter gradient (biases ahead of a BatchNorm,
    whose true gradient is 0, aside) moves by more than STABLE_DG of its largest entry.  Decided by the
    reference alone."""
    def grads(x, m):
        model, _, _ = _ref_step(ref_models, ref_te, name, x, m)
        return {k: p.grad.detach().clone() for k, p in model.named_parameters()
                if not k.endswith((".0.bias", ".3.bias"))}

    for seed in range(first, first + 64):
        x, m = G._inputs(2, 3, H, W, 3, seed=seed)
        g0 = grads(x, m)
        worst = 0.0
        for t in range(STABLE_TRIALS):
            gen = torch.Generator().manual_seed(1000 * seed + t)
            xp = (x * (1 + 1e-7 * torch.randn(x.shape, generator=gen))).float()
            g1 = grads(xp, m)
            worst = max(worst, max(float((g1[k] - g0[k]).abs().max() / g0[k].abs().max()) for k in g0))
            if worst > STABLE_DG:
                break
        print(f"{name} {H}x{W} seed {seed}: the reference's gradients move {worst:.2e} of their scale under "
              f"1e-7 input perturbations" + ("" if worst <= STABLE_DG else " -- not used"))
        if worst <= STABLE_DG:
            return seed
    raise RuntimeError("no stable seed found")


def gen_step(ref_models, ref_te, name, H, W, first_seed):
    seed = stable_seed(ref_models, ref_te, name, H, W, first_seed)
    x, m = G._inputs(2, 3, H, W, 3, seed=seed)
    model, lr, loss = _ref_step(ref_models, ref_te, name, x, m)
    sd = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    grads = {k: p.grad.detach().numpy().copy() for k, p in model.named_parameters()}
    np.savez_compressed(os.path.join(HERE, f"step_{name}_c3k3.npz"), x=x.numpy(), m=m.numpy(), lr=lr, loss=loss,
                        seed=seed, **G._summaries("post", sd), **G._summaries("grad", grads))


def main(only=()):
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    ref_models, ref_te = G._import_reference()
    jobs = {
        "unet_c3k3": lambda: gen_forward(ref_models, "unet"),
        "step_unet_c3k3": lambda: gen_step(ref_models, ref_te, "unet", 32, 32, first_seed=45),
    }
    for name, job in jobs.items():
        if not only or name in only:
            job()
    print("fixtures written to", HERE)


if __name__ == "__main__":
    main(tuple(sys.argv[1:]))
