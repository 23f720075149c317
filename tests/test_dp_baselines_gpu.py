"""eunet.dp with the unet baseline: bucketed all-reduce from inside its backward (GPU only).
One spawned process, world size 1 on the RCCL backend (the pattern of tests/test_dp_gpu.py): with one rank
the averaged gradients and the replicated Trainer steps must equal the plain ones bit for bit."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(port, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "enhanced-unet_amd"), os.path.join(root, "tests")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        import _baseline_ref as BR
        from eunet import synth
        from eunet.dp import DataParallel
        from eunet.losses import combined_loss
        from eunet.models import get_model
        from eunet.train_eval import Trainer
        x, m = synth.batch(2, 64, 64, start_index=200, num_classes=2, in_channels=1, device="cuda")
        res = {}
        for name in ("unet",):
            sd = {k: v.float() if v.is_floating_point() else v for k, v in BR.formula_weights(name, 16, 1, 2).items()}

            def fresh():
                mod = get_model(name, num_classes=2, in_channels=1, base_ch=16, dtype="bf16")
                mod.load_state_dict(sd)
                return mod.cuda().train()

            ref = fresh()
            combined_loss(ref.forward_lowres(x), m).backward()
            model = fresh()
            dp = DataParallel(model, bucket_mb=0.02)
            dp.before_forward()
            combined_loss(model.forward_lowres(x), m).backward()
            torch.cuda.synchronize()
            grads_equal = all(torch.equal(p.grad, q.grad) for p, q in zip(model.parameters(), ref.parameters()))
            ta, tb = Trainer(fresh(), "cuda", name), Trainer(fresh(), "cuda", name)
            ta.dp = DataParallel(ta.model, bucket_mb=0.02)
            la = [ta.step(x, m) for _ in range(3)]
            lb = [tb.step(x, m) for _ in range(3)]
            same_step = la == lb and all(torch.equal(p, q) for p, q in zip(ta.model.state_dict().values(),
                                                                             tb.model.state_dict().values()))
            res[name] = dict(buckets=len(dp.buckets), order_ok=dp.order == (model.backward_param_order() or dp.order),
                             grads_equal=grads_equal, same_step=same_step)
        q.put(res)
    except Exception as e:  # report instead of hanging the parent on q.get
        q.put(dict(error=repr(e)))
    finally:
        dist.destroy_process_group()


def test_dp_world1_baselines():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_worker, args=(_free_port(), q))
    p.start()
    res = q.get(timeout=300)
    p.join(timeout=120)
    print("RCCL world-1 DP, baselines:", res)
    assert "error" not in res, res
    assert p.exitcode == 0
    for name in ("unet",):
        r = res[name]
        assert r["buckets"] > 1 and r["order_ok"], (name, r)
        assert r["grads_equal"], f"{name}: RCCL-averaged gradients (world 1) must equal the plain backward"
        assert r["same_step"], f"{name}: Trainer steps with DataParallel(world 1) must equal the plain steps"
