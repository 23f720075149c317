"""Time of the distance-transform watershed (csrc/watershed.hip, ops.watershed_from_distance) pass by pass, of its
host merge, and of Evaluator.semantic_to_instances with split="watershed" next to the erosion ladder.

    python tools/watershed_bench.py [--size 1024] [--reps 10] [--rounds 5] [--out profiles/watershed_bench.txt]

One process, the routes alternating over the rounds; per line the median [min, max] of the rounds.
The mask is the [S, S] eunet.synth tile (3 classes); the distance planes are distance_transform_sq(mask, [1, 2], "ne").
  * the device passes of watershed_from_distance on the two planes at the default depth, from kprof's events around
    each C-ABI call (basins: up, pointer jumping, first pixels, numbering; peaks; saddles; relabel), per call;
  * the host merge (ops.merge_basins) of the same calls, a host clock, with the basin and saddle-pair counts;
  * watershed_from_distance as a whole: a host clock around the call (it synchronises three times: the basin
    counts, the saddle table, the peaks), so the copies and the waits are in it;
  * distance_transform_sq "ne" of the two classes and ops.label_components of the live class mask (the one-pass
    yardstick: what the erosion route starts with), device events;
  * semantic_to_instances on the mask with split="watershed" and split="erosion": a host clock around the call,
    the mask resident on the device;
  * the instances both routes return per class next to the cells the tile holds (the distinct ids of the synth
    instance map: a cell painted over completely by later ones is gone).
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
from eunet.evaluator import Evaluator  # noqa: E402

DEV = "cuda"
WARMUP = 3
PASSES = ("watershed_basins", "watershed_peaks", "watershed_saddles", "watershed_relabel")


def timed(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps  # us per call


def host_timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / reps


def row(name, v):
    return f"{name:58s} {statistics.median(v):11.1f} [{min(v):.1f}, {max(v):.1f}] us"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "watershed_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("watershed_bench: needs the GPU (nothing is measured without one)")
    S = a.size
    _, sem, inst = synth.tile(S, S, 0, num_classes=3, instances=True)
    true_cells = [len(np.unique(inst[(inst > 0) & (sem == c)])) for c in (1, 2)]
    mask = torch.from_numpy(sem).to(DEV)
    dist = ops.distance_transform_sq(mask, [1, 2], "ne")
    dist_out = torch.empty_like(dist)
    ids_out = torch.empty_like(dist)
    live, _ = ops.mask_eq(mask, 1)
    ev = {s: Evaluator(None, DEV, "enhanced_unet", preprocess=None, split=s) for s in ("watershed", "erosion")}

    merge_us, graph = [], []
    merge = ops.merge_basins

    def timed_merge(peak, root, offs, ea, eb, saddle, depth):
        t0 = time.perf_counter()
        out = merge(peak, root, offs, ea, eb, saddle, depth)
        merge_us.append(1e6 * (time.perf_counter() - t0))
        graph.append((len(peak), len(ea)))
        return out

    ops.merge_basins = timed_merge
    routes = {
        "watershed_from_distance, 2 planes, whole call": lambda: ops.watershed_from_distance(dist, 1.0, out=ids_out),
        "semantic_to_instances split=watershed": lambda: ev["watershed"].semantic_to_instances(mask),
        "semantic_to_instances split=erosion": lambda: ev["erosion"].semantic_to_instances(mask),
    }
    device = {
        "distance_transform_sq ne, 2 classes": lambda: ops.distance_transform_sq(mask, [1, 2], "ne", out=dist_out),
        "label_components of the live mask": lambda: ops.label_components(live),
    }
    for fn in list(routes.values()) + list(device.values()):
        for _ in range(WARMUP):
            fn()
    us = {k: [] for k in list(routes) + list(device) + list(PASSES) + ["host merge (ops.merge_basins)"]}
    for _ in range(a.rounds):
        for name, fn in device.items():
            us[name].append(timed(fn, a.reps))
        for name, fn in routes.items():
            us[name].append(host_timed(fn, a.reps))
        del merge_us[:]
        with kprof.KernelTimer() as kt:  # the passes of the same call, bracketed by events: a run of its own
            for _ in range(a.reps):
                ops.watershed_from_distance(dist, 1.0, out=ids_out)
        s = kt.summary()
        for p in PASSES:
            us[p].append(1e3 * s[p]["ms"] / a.reps)
        us["host merge (ops.merge_basins)"].append(sum(merge_us) / a.reps)
    ops.merge_basins = merge

    counts = {}
    for sname, e in ev.items():
        _, labels, _ = e.semantic_to_instances(mask)
        counts[sname] = [sum(1 for l in labels if l == c) for c in (0, 1)]
    _, n_regions, _ = ops.watershed_from_distance(dist, 1.0)
    nb, ne = graph[-1]
    lines = [f"# tools/watershed_bench.py: [{S}, {S}] eunet.synth mask (3 classes); {a.reps} calls per round, {a.rounds} "
             f"alternating rounds, {WARMUP} warm-up calls; {torch.cuda.get_device_name(0)}",
             f"{'call':58s} {'median [min, max]':>30s}"]
    lines += [row(k, us[k]) for k in device]
    lines.append("# watershed_from_distance on the two class planes, depth 1.0: device time of each pass (events around the "
                 "C-ABI call), per call")
    lines += [row("  " + p, us[p]) for p in PASSES]
    lines.append(row(f"  host merge (ops.merge_basins): {nb} basins, {ne} pairs", us["host merge (ops.merge_basins)"]))
    lines += [row(k, us[k]) for k in routes]
    med = {k: statistics.median(v) for k, v in us.items()}
    dev_sum = sum(med[p] for p in PASSES)
    whole = med["watershed_from_distance, 2 planes, whole call"]
    lines.append("# ratios of the medians")
    lines.append(f"device passes in all: {dev_sum:.1f} us; whole call - passes - merge (copies, waits, allocation): "
                 f"{whole - dev_sum - med['host merge (ops.merge_basins)']:.1f} us")
    lines.append(f"basins pass / label_components (one plane each way: basins runs two): "
                 f"{med['watershed_basins'] / 2 / med['label_components of the live mask']:.2f}")
    lines.append(f"semantic_to_instances watershed / erosion: time "
                 f"{med['semantic_to_instances split=watershed'] / med['semantic_to_instances split=erosion']:.2f}")
    lines.append(f"# regions of the two planes at depth 1.0 before the area limits: {n_regions.tolist()}")
    lines.append(f"# instances (live, dead): cells in the tile {true_cells}, split=watershed {counts['watershed']}, "
                 f"split=erosion {counts['erosion']}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
