"""upsample="transpose" on the GPU, whole model: the HIP engine against the fp64 restatement
(tests/_upconv_ref.py) evaluated on the branches the kernels took (tests/_pins.py).  Gates and helpers are
those of tests/test_gpu_model.py and tests/test_gpu_baselines_model.py."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

import _upconv_ref as U
from test_gpu_model import DEV, _rel, _rel_l2

pytestmark = pytest.mark.gpu
UP_KEYS = [f"model.{u}.{w}" for u in ("up4", "up3", "up2") for w in ("weight", "bias")]


def _model(name, base, cin, K, dtype="fp32"):
    from eunet.models import get_model
    m = get_model(name, num_classes=K, in_channels=cin, base_ch=base, dtype=dtype, upsample="transpose")
    sd = {k: (v.float() if v.is_floating_point() else v) for k, v in U.formula_weights(name, base, cin, K).items()}
    m.load_state_dict(sd)
    return m.to(DEV)


def _pre_bn_bias(k):
    return k.endswith((".0.bias", ".3.bias")) and not k.startswith("enhance.3")


def _head_pin(m):
    """The 2H head's ReLU branches as the engine took them.  tests/_pins.py leaves that ReLU to the oracle (its
    input is recomputed inside the head kernels, never stored) -- but the oracle evaluates it on ITS z, which the
    engine's fp32 trunk output matches only to ~3e-6, and one element of the half million that lands on the other
    side of the kink moves every upstream gradient by a finite amount (measured at base 64, 32^2: a single element
    2.9e-7 max|h| from the kink, relative L2 1.2e-3 on the encoder gradients).  So the head is pinned like the trunk,
    from the engine's own saved state: z = dec1(d2) [N,H,W,K] and the batch statistics (mean, invstd) the head
    kernel kept for its backward, through head.hip's expression fma(gamma, (conv(up2(z)) - mean) invstd, beta) > 0
    in fp64.  What is left is the rounding of the head's own fp32 conv (27 products), ~1e-7; _pins.audit holds
    every pin that disagrees with the restatement's own branch to 1e-5 max|h| of the kink."""
    S = m._engine.last_state
    P = {k: v.detach().double().cpu() for k, v in m.named_parameters()}
    z = S["z"].detach().double().cpu().permute(0, 3, 1, 2)
    u = F.interpolate(z, scale_factor=2, mode="bilinear", align_corners=False)
    h = F.conv2d(u, P["enhance.0.weight"], P["enhance.0.bias"], padding=1)
    c = lambda t: t.detach().double().cpu()[None, :, None, None]  # noqa: E731
    xh = (h - c(S["hmean"])) * c(S["hinv"])
    return (P["enhance.1.weight"][None, :, None, None] * xh + P["enhance.1.bias"][None, :, None, None]) > 0


def _model_pins(name, m):
    import _pins
    pins = _pins.model_pins(m)
    if name == "enhanced_unet":
        pins["enhance.1"] = _head_pin(m)
    return pins


def _gpu_step(name, m, x, msk):
    """Forward + the model's Trainer-row loss + backward with the engine's state kept: (loss, pins)."""
    import _pins
    from eunet.losses import combined_loss
    from eunet.train_eval import Trainer
    prm = Trainer(m, DEV, name, total_epochs=50).loss_params()
    _pins.keep(m)
    m.train()
    loss = combined_loss(m.forward_lowres(x.to(DEV)), msk.to(DEV), params=prm)
    loss.backward()
    torch.cuda.synchronize()
    pins = _model_pins(name, m)
    _pins.keep(m, False)
    m._engine.last_state = None
    return loss, pins


@pytest.mark.parametrize("name,base,cin,K,H", [("enhanced_unet", 16, 1, 2, 64), ("enhanced_unet", 64, 3, 3, 32),
                                               ("unet", 16, 1, 2, 64)])
def test_train_grads_match_restatement(name, base, cin, K, H):
    """Loss and every parameter gradient of one train step vs the fp64 restatement on the GPU's own branches:
    relative L2 per tensor <= max(1e-3, 3 x the pinned fp32 restatement's own error); running statistics 1e-3
    (the gate of test_gpu_model.test_train_grads_match_oracle)."""
    import _pins
    from eunet import synth
    x, msk = synth.batch(2, H, H, start_index=7, num_classes=K, in_channels=cin)
    m = _model(name, base, cin, K)
    loss, pins = _gpu_step(name, m, x, msk)
    rec = {}
    S, loss_ref = U.grads(name, base, cin, K, x, msk, torch.float64, pins, record=rec)
    _pins.audit(pins, rec, "fp32", label=f"transpose {name} b{base} c{cin} K{K} {H}^2")
    S32, _ = U.grads(name, base, cin, K, x, msk, torch.float32, pins)
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
    assert all(any(r[1] == k for r in rows) for k in UP_KEYS)
    for r in sorted(rows, reverse=True)[:4] + [r for r in rows if r[1] in UP_KEYS]:
        print(f"grads {name} b{base} c{cin} K{K} {H}^2 (ratio, name, err, tol):", r)
    assert all(r[0] < 1.0 for r in rows), sorted(rows, reverse=True)[:3]
    for k, v in m.state_dict().items():
        if "running" in k:
            assert _rel(v, S[k]) < 1e-3, k


@pytest.mark.parametrize("name", ["enhanced_unet", "unet"])
def test_eval_forward_matches_restatement(name):
    """Eval-mode forward (after one train forward moved the running statistics) within 1e-3 of max|logit|."""
    from eunet import synth
    base, cin, K = 16, 1, 2
    x, _ = synth.batch(2, 64, 64, start_index=21, num_classes=K, in_channels=cin)
    x2, _ = synth.batch(2, 40, 56, start_index=23, num_classes=K, in_channels=cin)
    m = _model(name, base, cin, K).train()
    S = U.formula_weights(name, base, cin, K)
    with torch.no_grad():
        m(x.to(DEV))
        U.forward(name, S, x.double(), True)
        ref = U.forward(name, S, x2.double(), False)
        m.eval()
        out = m(x2.to(DEV))
        low = m.forward_lowres(x2.to(DEV))
    print(name, "eval forward vs restatement:", _rel(out, ref))
    assert out.shape == ref.shape and _rel(out, ref) < 1e-3
    assert float((low.double() - F.avg_pool2d(out.double(), 2)).abs().max()) <= 1e-6 * float(out.abs().max())


@pytest.mark.parametrize("name", ["enhanced_unet", "unet"])
def test_bf16_train_step(name):
    """bf16 end to end (base 16, 1-ch, K 2, 64^2, the shape and bound of test_gpu_baselines_model's bf16 step test):
    the loss within 1e-2 of the fp32 engine's, every gradient finite, every up* gradient nearer to the fp32
    engine's than to zero."""
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
    print(name, "transpose bf16 / fp32 loss", losses["bf16"], losses["fp32"])
    assert abs(losses["bf16"] - losses["fp32"]) < 1e-2 * abs(losses["fp32"])
    for k, gb in grads["bf16"].items():
        assert bool(torch.isfinite(gb).all()), k
    rows = [(_rel_l2(grads["bf16"][k], grads["fp32"][k]), k) for k in UP_KEYS]
    print(name, "up* bf16 vs fp32 engine gradients, rel L2:", rows)
    assert all(float(grads["bf16"][k].abs().max()) > 0 for k in UP_KEYS)
    assert all(r[0] < 1.0 for r in rows), rows


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_step_graph_replay_is_exact(dtype):
    """Trainer.step eager against Trainer.step_graph (2 eager warm-up steps, a capture, two replays): losses,
    parameters, AdamW moments and BN statistics bit for bit; the graph's key separates the two variants."""
    from eunet import synth
    from eunet.models import get_model
    from eunet.train_eval import StepGraph, Trainer
    batches = []
    for i in range(5):
        x, msk = synth.batch(2, 64, 96, start_index=5 * i + 1, num_classes=3, in_channels=3)
        batches.append((x.to(DEV), msk.to(DEV)))
    ta = Trainer(_model("enhanced_unet", 16, 3, 3, dtype), DEV, "enhanced_unet", total_epochs=12)
    tb = Trainer(_model("enhanced_unet", 16, 3, 3, dtype), DEV, "enhanced_unet", total_epochs=12)
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
    assert all(float((p - q).abs().max()) > 0 for (k, p), q in
               zip(ta.model.named_parameters(), _model("enhanced_unet", 16, 3, 3, dtype).parameters()) if k in UP_KEYS)
    tc = Trainer(get_model("enhanced_unet", num_classes=3, base_ch=16, dtype=dtype).to(DEV), DEV, "enhanced_unet")
    x, m = batches[0]
    assert StepGraph.key(ta, x, m) != StepGraph.key(tc, x, m)


def test_state_dict_round_trip_and_bilinear_checkpoint():
    """A transpose model's state_dict reloads into a fresh one bit for bit (same forward); a bilinear model's
    loads with strict=False, leaving up* at their initialisation, and the model still runs."""
    from eunet import synth
    from eunet.models import get_model
    x, _ = synth.batch(2, 32, 32, start_index=3, num_classes=2, in_channels=1)
    a = _model("enhanced_unet", 16, 1, 2).eval()
    b = get_model("enhanced_unet", num_classes=2, in_channels=1, base_ch=16, upsample="transpose")
    b.load_state_dict(a.state_dict())
    b = b.to(DEV).eval()
    assert list(a.state_dict()) == list(b.state_dict())
    with torch.no_grad():
        assert torch.equal(a(x.to(DEV)), b(x.to(DEV)))
    src = get_model("enhanced_unet", num_classes=2, in_channels=1, base_ch=16)
    init = {k: b.state_dict()[k].clone() for k in UP_KEYS}
    res = b.load_state_dict(src.state_dict(), strict=False)
    assert sorted(res.missing_keys) == sorted(UP_KEYS)
    assert all(torch.equal(b.state_dict()[k], init[k]) for k in UP_KEYS)
    with torch.no_grad():
        assert bool(torch.isfinite(b(x.to(DEV))).all())


# ---- data parallel: world 2 on one GPU (gloo carries the collectives) -------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _dp_worker(rank, world, port, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "enhanced-unet_amd"), os.path.join(root, "tests")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import _pins
        import _upconv_ref as U
        from eunet import synth
        from eunet.dp import DataParallel
        from eunet.losses import combined_loss
        name, base, cin, K = "enhanced_unet", 16, 1, 2
        x, msk = synth.batch(2, 64, 64, start_index=100 + 2 * rank, num_classes=K, in_channels=cin, device="cuda")
        model = _model(name, base, cin, K).train()
        dp = DataParallel(model, bucket_mb=0.05)
        dp.before_forward()
        _pins.keep(model)
        combined_loss(model.forward_lowres(x), msk).backward()
        torch.cuda.synchronize()
        pins = _model_pins(name, model)
        out = dict(rank=rank, buckets=len(dp.buckets), order_ok=dp.order == model.backward_param_order(),
                   bucketed=[k for k in UP_KEYS if any(k in members for _, _, members in dp.buckets)],
                   grads={k: p.grad.detach().double().cpu().numpy() for k, p in model.named_parameters()})
        for odt, key in ((torch.float64, "ref64"), (torch.float32, "ref32")):
            S, _ = U.grads(name, base, cin, K, x.cpu(), msk.cpu(), odt, pins)
            out[key] = {k: S[k].grad.double().numpy() for k in out["grads"]}
        q.put(out)
    except Exception:  # report instead of hanging the parent on q.get
        import traceback
        q.put(dict(rank=rank, error=traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_dp_world2_gradients_are_the_mean_of_the_shards():
    """World 2 on one GPU: every rank's bucketed, all-reduced gradients -- the up* ones included -- equal the mean
    over the shards of each shard's branch-pinned restatement gradient, within max(1e-3, 3 x the fp32
    restatement's error) relative L2 per tensor; both ranks hold identical gradients."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in procs:
            r = q.get(timeout=500)
            res.append(r)
            assert "error" not in r, r["error"]
    finally:
        for p in procs:
            p.join(timeout=60 if all("error" not in r for r in res) else 1)
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
    assert all(p.exitcode == 0 for p in procs)
    res.sort(key=lambda r: r["rank"])
    for r in res:
        assert r["buckets"] > 3 and r["order_ok"] and r["bucketed"] == UP_KEYS, (r["buckets"], r["order_ok"], r["bucketed"])
        for key in ("grads", "ref64", "ref32"):
            r[key] = {k: torch.from_numpy(v) for k, v in r[key].items()}
    ref = {k: sum(r["ref64"][k] for r in res) / world for k in res[0]["grads"]}
    ref32 = {k: sum(r["ref32"][k] for r in res) / world for k in res[0]["grads"]}
    scale = max(float(v.abs().max()) for v in ref.values())
    rows = []
    for k, g in res[0]["grads"].items():
        assert torch.equal(g, res[1]["grads"][k]), k
        if _pre_bn_bias(k):
            assert float((g - ref[k]).abs().max()) < 1e-4 * scale, k
            continue
        tol = max(1e-3, 3 * _rel_l2(ref32[k], ref[k]))
        rows.append((_rel_l2(g, ref[k]) / tol, k, _rel_l2(g, ref[k]), tol))
    for r in sorted(rows, reverse=True)[:3] + [r for r in rows if r[1] in UP_KEYS]:
        print("world-2 mean-of-shards grad (ratio, name, err, tol):", r)
    assert all(r[0] < 1.0 for r in rows), sorted(rows, reverse=True)[:3]
