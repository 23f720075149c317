"""bench.py's driver contract on the GPU box: `bench.py --gpus 2` starts two ranks by itself (the
driver's command shape), each timing the per-rank workload with max-over-ranks timing and rank 0 printing
one JSON line that reports the real process-group size (BASELINE configs[3]: train_eval.py:337-343 per
rank).  gloo carries the collectives so that two ranks can share the one GPU of the box.  A plain run
(no --full) reports the headline figure alone and --dump-outputs writes the last timed step's outputs."""
import json
import math
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra, env=None, timeout=240):
    e = dict(os.environ, **(env or {}))
    cmd = [sys.executable, "-u", os.path.join(ROOT, "bench.py"), *extra]
    return subprocess.run(cmd, cwd=ROOT, env=e, capture_output=True, text=True, timeout=timeout)


@pytest.mark.gpu
def test_bench_gpus2_runs_two_ranks():
    r = _bench("--gpus", "2", "--size", "256", "--batch", "1", "--steps", "2", "--warmup", "1",
               "--no-cpu-baseline", "--dice-size", "0", "--no-fp32-leg", env={"EUNET_DIST_BACKEND": "gloo"})
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]  # rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["world"]["size"] == 2 and d["world"]["backend"] == "gloo"
    assert d["config"]["parallelism"] == "dp2" and d["config"]["global_batch"] == 2
    assert d["steps"] == 2 and d["value"] > 0
    # value = images of all ranks / the max-over-ranks time
    assert abs(d["value"] - 2 * 1 * 2 / (d["ms_per_step"] * 2e-3)) / d["value"] < 1e-2
    # per rank: its own step time, the communication its backward left exposed, the bucket count
    pr = d["world"]["per_rank"]
    assert [r["rank"] for r in pr] == [0, 1], pr
    for r in pr:
        assert r["steps"] == 2 and r["buckets"] >= 1, r
        for k in ("ms_per_step", "exposed_comm_ms", "last_bucket_ms"):
            assert isinstance(r[k], float) and math.isfinite(r[k]) and r[k] >= 0.0, (k, r)
    assert max(r["ms_per_step"] for r in pr) <= d["ms_per_step"] * 1.01


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """A plain run (no --full) times exactly --steps steps, leaves every leg that takes a run of its own
    null, and --dump-outputs writes the last timed step's loss and the model state as float32 / float64
    .npy files within the 64 MB budget."""
    import numpy as np
    out = tmp_path / "dump"
    r = _bench("--gpus", "1", "--size", "64", "--batch", "2", "--base", "16", "--steps", "3", "--warmup", "1",
               "--dump-outputs", str(out))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["full"] is False and d["steps"] == 3 and d["warmup"] == 1 and d["dtype"] == "bf16"
    assert d["unit"] == "img/s" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0 and abs(d["value"] - 2 * 1e3 / d["ms_per_step"]) / d["value"] < 1e-2
    assert d["steps_diag"]["step_ms"]["min"] > 0 and "step_kernel_busy_ms" not in d["steps_diag"]
    for leg in ("dp_world1", "fp32_configs1", "dual_configs4", "cpu_baseline", "logits_rel_err_vs_cpu",
                "dice_vs_cpu_ref"):
        assert d[leg] is None, leg
    files = sorted(p.name for p in out.iterdir())
    assert "loss.npy" in files and all(f.endswith(".npy") for f in files)
    from eunet.models import EnhancedUNet
    keys = EnhancedUNet(num_classes=2, in_channels=1, base_ch=16, dtype="bf16").state_dict()
    assert set(files) == {"loss.npy"} | {f"state.{k}.npy" for k in keys}
    total = 0
    for f in files:
        a = np.load(out / f)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
        total += a.nbytes
        if f != "loss.npy":
            assert a.shape == tuple(keys[f[len("state."):-len(".npy")]].shape), f
    assert total <= 64 * 10 ** 6
    assert np.load(out / "loss.npy").shape == () and float(np.load(out / "loss.npy")) > 0
    # three optimisation steps ran on this model: 1 warm-up + 3 timed
    assert float(np.load(out / "state.model.enc1.1.num_batches_tracked.npy")) == 4


def test_write_outputs_budget_and_seeded_sample(tmp_path):
    """bench.write_outputs: whole arrays while they fit the budget; above it every large array is cut to
    the same seeded sample of its elements (identical from call to call), small ones stay whole, and the
    bytes written stay within the budget.  CPU-only."""
    import numpy as np
    import torch
    import bench
    big = torch.arange(100000, dtype=torch.float32).reshape(100, 1000)
    named = [("loss", torch.tensor(1.5)), ("big", big), ("count", torch.tensor(7)),
             ("small", torch.ones(10, dtype=torch.bfloat16)), ("wide", torch.full((3,), 0.1, dtype=torch.float64))]
    n = bench.write_outputs(str(tmp_path / "a"), named)
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k, _ in named}
    assert n == sum(a.nbytes for a in got.values()) <= bench.DUMP_BUDGET
    assert got["big"].shape == (100, 1000) and got["big"].dtype == np.float32 and (got["big"] == big.numpy()).all()
    assert got["count"].dtype == np.float64 and got["count"] == 7 and got["wide"].dtype == np.float64
    assert got["small"].dtype == np.float32 and got["loss"].dtype == np.float32 and got["loss"] == 1.5
    budget = 40000
    for sub in ("b", "c"):
        assert bench.write_outputs(str(tmp_path / sub), named, budget=budget) <= budget
    b, c = np.load(tmp_path / "b" / "big.npy"), np.load(tmp_path / "c" / "big.npy")
    assert b.ndim == 1 and 9000 < b.size < 10000 and (b == c).all()
    assert (np.diff(b) > 0).all()  # sorted indices without replacement of arange: strictly increasing values
    assert np.load(tmp_path / "b" / "small.npy").shape == (10,)


def test_bench_rejects_world_size_mismatch():
    """Under a launcher whose WORLD_SIZE differs from --gpus, bench.py exits non-zero before any GPU
    work (CPU-only: the check precedes device selection)."""
    r = _bench("--gpus", "2", env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"}, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr
