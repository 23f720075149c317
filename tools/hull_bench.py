"""Time of the per-cell convex hulls (csrc/hull.hip: ops.cell_hulls) next to the per-cell sums of the same planes
(csrc/cellprops.hip: ops.cell_stats, the tree's yardstick for one pass over a label map).

    python tools/hull_bench.py [--size 1024] [--reps 10] [--rounds 5] [--out profiles/hull_bench.txt]

One process, the routes alternating over the rounds; per line the median [min, max] of the rounds.
The maps are the [S, S] eunet.synth tile (3 classes, instances=True) as one id map per class (live, dead), as in
tools/cellprops_bench.py.
  * cell_hulls of the two class planes, int32 and int64 ids: the device time (the init, extents and chain kernels,
    from kprof's events around the C-ABI call) and the whole call on a host clock (the row layout is formed in numpy
    and uploaded, the tables are read back: the call synchronises);
  * cell_stats of the same planes without an image, the same two figures;
  * the worst case of the chain: one label of torch.randint(0, 2) noise covering the plane, S rows for a single wave.
Recorded, not gated.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "enhanced-unet_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from eunet import kprof, ops, synth  # noqa: E402

DEV = "cuda"
WARMUP = 3


def host_timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / reps


def row(name, v):
    return f"{name:66s} {statistics.median(v):11.1f} [{min(v):.1f}, {max(v):.1f}] us"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hull_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hull_bench: needs the GPU (nothing is measured without one)")
    S = a.size
    _, sem, inst = synth.tile(S, S, 0, num_classes=3, instances=True)
    gt_np = np.stack([np.where(sem == c, inst, 0) for c in (1, 2)])
    n = int(gt_np.max())
    ids64 = torch.from_numpy(gt_np).to(DEV)
    ids32 = ids64.int()
    noise = torch.randint(0, 2, (1, S, S), device=DEV, dtype=torch.int32)
    st32, st64, st_noise = ops.cell_stats(ids32, n), ops.cell_stats(ids64, n), ops.cell_stats(noise, 1)
    verts = int(ops.cell_hulls(ids32, st32)["hull"][:, :, 0].sum())
    noise_verts = int(ops.cell_hulls(noise, st_noise)["hull"][0, 1, 0])

    calls = {
        "cell_hulls int32": (lambda: ops.cell_hulls(ids32, st32), "cell_hulls"),
        "cell_hulls int64": (lambda: ops.cell_hulls(ids64, st64), "cell_hulls"),
        "cell_stats int32, no image": (lambda: ops.cell_stats(ids32, n), "cell_stats"),
        "cell_stats int64, no image": (lambda: ops.cell_stats(ids64, n), "cell_stats"),
        f"cell_hulls of one randint(0, 2) noise label, {S} rows": (lambda: ops.cell_hulls(noise, st_noise),
                                                                  "cell_hulls"),
        "cell_stats of the same noise plane, n = 1": (lambda: ops.cell_stats(noise, 1), "cell_stats"),
    }
    for fn, _ in calls.values():
        for _ in range(WARMUP):
            fn()
    us = {f"{k}, {part}": [] for k in calls for part in ("device time", "whole call")}
    for _ in range(a.rounds):
        for name, (fn, fam) in calls.items():
            us[f"{name}, whole call"].append(host_timed(fn, a.reps))
            with kprof.KernelTimer() as kt:  # the launches alone, bracketed by events: a run of its own
                for _ in range(a.reps):
                    fn()
            s = kt.summary()[fam]
            us[f"{name}, device time"].append(1e3 * s["ms"] / s["launches"])
    med = {k: statistics.median(v) for k, v in us.items()}
    cells = [int((np.unique(p) > 0).sum()) for p in gt_np]
    lines = [f"# tools/hull_bench.py: [{S}, {S}] eunet.synth tile (3 classes) as two class planes of ids, n = {n}; "
             f"{a.reps} calls per round, {a.rounds} alternating rounds, {WARMUP} warm-up calls; "
             f"{torch.cuda.get_device_name(0)}",
             f"# cells (live, dead): {cells}; hull vertices of all cells {verts}; box rows of all cells "
             f"{int(ops.cell_hulls(ids32, st32)['row_off'][-1])}; the noise label's hull has {noise_verts} vertices",
             f"{'call':66s} {'median [min, max]':>30s}"]
    lines += [row(k, v) for k, v in us.items()]
    lines.append("# ratios of the medians")
    names = list(calls)
    for hull, stats in ((names[0], names[2]), (names[1], names[3]), (names[4], names[5])):
        lines.append(f"{hull} / {stats}: device time {med[hull + ', device time'] / med[stats + ', device time']:.2f}, "
                     f"whole call {med[hull + ', whole call'] / med[stats + ', whole call']:.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
