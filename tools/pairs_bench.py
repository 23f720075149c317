"""Time of the label-map instance metrics (csrc/pairs.hip: ops.label_pairs, ops.labels_from_stack; the 4-connected
ops.label_components) next to the routes they replace or are measured against.

    python tools/pairs_bench.py [--size 1024] [--reps 10] [--rounds 5] [--out profiles/pairs_bench.txt]

One process, the routes alternating over the rounds; per line the median [min, max] of the rounds.
The ground truth is the [S, S] eunet.synth tile (3 classes, instances=True) as one id map per class (live, dead); the
prediction is a perturbed copy (shifted by (3, 2) pixels, every seventh cell removed).
  * label_pairs of the two class planes, int32 / int32 and int64 / int64: the device pass (the table's clear
    included) from kprof's events around the C-ABI call, per launch, with the bytes it reads per second, and the whole
    call on a host clock (the table is read back: the call synchronises);
  * ops.semantic_counts on the same int64 pair, the project's one-pass yardstick (16 bytes per pixel as well);
  * metrics.instance_counts on the equivalent mask stacks (stack + pack + all-pairs overlap), the route it replaces,
    per class, with the stacks' bytes next to the maps';
  * labels_from_stack of the ground-truth stack (one class selected);
  * 4- against 8-connected label_components of the live class mask;
  * the per-image metric part of evaluate_panoptic (semantic_to_instance_maps, the ground-truth maps, label_pairs,
    instance_stats_from_pairs) against semantic_to_instances + calculate_instance_metrics on the same predicted
    semantic mask, split="watershed", host clocks; and the two metric parts alone, from maps and stacks that exist;
  * the worst case: torch.randint noise maps, where every pixel is a run of its own and inserts for itself.
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
from eunet import kprof, metrics, ops, synth  # noqa: E402
from eunet.evaluator import Evaluator  # noqa: E402

DEV = "cuda"
WARMUP = 3


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
    return f"{name:66s} {statistics.median(v):11.1f} [{min(v):.1f}, {max(v):.1f}] us"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pairs_bench: needs the GPU (nothing is measured without one)")
    S = a.size
    _, sem, inst = synth.tile(S, S, 0, num_classes=3, instances=True)
    gt_np = np.stack([np.where(sem == c, inst, 0) for c in (1, 2)])
    pred_np = np.roll(gt_np, (3, 2), axis=(1, 2))
    pred_np[(pred_np % 7) == 3] = 0
    pred_sem_np = np.where(pred_np[0] > 0, 1, np.where(pred_np[1] > 0, 2, 0)).astype(np.int64)
    gt64, pred64 = torch.from_numpy(gt_np).to(DEV), torch.from_numpy(pred_np).to(DEV)
    gt32, pred32 = gt64.int(), pred64.int()
    pred_sem = torch.from_numpy(pred_sem_np).to(DEV)

    def stacks(ids):
        out = []
        for plane in ids:
            keep = [j for j in np.unique(plane) if j > 0]
            out.append(torch.from_numpy(np.stack([plane == j for j in keep]).astype(np.uint8)).to(DEV))
        return out

    gt_stacks, pred_stacks = stacks(gt_np), stacks(pred_np)
    gt_masks = [m for s in gt_stacks for m in s]
    gt_labels = [c for c, s in enumerate(gt_stacks) for _ in s]
    item = {"semantic_mask": torch.from_numpy(sem).to(DEV), "instance_masks": gt_masks, "instance_labels": gt_labels}
    all_gt = torch.cat(gt_stacks)
    live_ids = [j + 1 if l == 0 else 0 for j, l in enumerate(gt_labels)]
    live, _ = ops.mask_eq(torch.from_numpy(sem).to(DEV), 1)
    ev = Evaluator(None, DEV, "enhanced_unet", preprocess=None, split="watershed")
    noise = {n: (torch.randint(0, n, (2, S, S), device=DEV, dtype=torch.int32),
                 torch.randint(0, n, (2, S, S), device=DEV, dtype=torch.int32)) for n in (50, 1000)}

    def panoptic_image():
        ids, _, _ = ev.semantic_to_instance_maps(pred_sem)
        g, _ = ev._gt_instance_maps(item, ids.shape[1:], ids.device)
        return metrics.instance_stats_from_pairs(ops.label_pairs(ids, g), 2)

    def reference_image():
        masks, labels, scores = ev.semantic_to_instances(pred_sem)
        return metrics.calculate_instance_metrics(masks, labels, scores, gt_masks, gt_labels)

    pm, pl, ps = ev.semantic_to_instances(pred_sem)
    device = {
        "semantic_counts of the two int64 planes": lambda: ops.semantic_counts(pred64.view(2, -1), gt64.view(2, -1)),
        "label_components of the live mask, 8-connected": lambda: ops.label_components(live),
        "label_components of the live mask, 4-connected": lambda: ops.label_components(live, connectivity=4),
        f"labels_from_stack, {len(all_gt)} planes, one class selected": lambda: ops.labels_from_stack(all_gt, live_ids),
    }
    host = {
        "label_pairs int32 / int32, whole call": lambda: ops.label_pairs(pred32, gt32),
        "label_pairs int64 / int64, whole call": lambda: ops.label_pairs(pred64, gt64),
        "instance_counts on the mask stacks, both classes": lambda: [metrics.instance_counts(p, g)
                                                                     for p, g in zip(pred_stacks, gt_stacks)],
        "metric part from the maps: label_pairs + instance_stats_from_pairs":
            lambda: metrics.instance_stats_from_pairs(ops.label_pairs(pred32, gt32), 2),
        "metric part from the stacks: calculate_instance_metrics":
            lambda: metrics.calculate_instance_metrics(pm, pl, ps, gt_masks, gt_labels),
        "evaluate_panoptic's image: maps + ground-truth maps + pairs + stats": panoptic_image,
        "evaluate's image: semantic_to_instances + calculate_instance_metrics": reference_image,
        "label_pairs of randint(0, 50) noise, int32, whole call": lambda: ops.label_pairs(*noise[50]),
        "label_pairs of randint(0, 1000) noise, int32, whole call": lambda: ops.label_pairs(*noise[1000]),
    }
    kernel = {
        "label_pairs int32 / int32, device pass": (lambda: ops.label_pairs(pred32, gt32), 2 * S * S * 8),
        "label_pairs int64 / int64, device pass": (lambda: ops.label_pairs(pred64, gt64), 2 * S * S * 16),
        "label_pairs of randint(0, 50) noise, device pass": (lambda: ops.label_pairs(*noise[50]), 2 * S * S * 8),
    }
    for fn in list(device.values()) + list(host.values()):
        for _ in range(WARMUP):
            fn()
    us = {k: [] for k in list(device) + list(host) + list(kernel)}
    for _ in range(a.rounds):
        for name, fn in device.items():
            us[name].append(timed(fn, a.reps))
        for name, fn in host.items():
            us[name].append(host_timed(fn, a.reps))
        for name, (fn, _) in kernel.items():
            with kprof.KernelTimer() as kt:  # the pass alone, bracketed by events: a run of its own
                for _ in range(a.reps):
                    fn()
            s = kt.summary()["label_pairs"]
            us[name].append(1e3 * s["ms"] / s["launches"])  # per launch: a call whose table regrows launches again
    med = {k: statistics.median(v) for k, v in us.items()}
    rows = {k: len(ops.label_pairs(*v)) for k, v in noise.items()}
    n_rows = len(ops.label_pairs(pred32, gt32))
    stack_bytes = sum(s.numel() for s in gt_stacks + pred_stacks)
    lines = [f"# tools/pairs_bench.py: [{S}, {S}] eunet.synth tile (3 classes) as two class planes of ids against a "
             f"perturbed copy; {a.reps} calls per round, {a.rounds} alternating rounds, {WARMUP} warm-up calls; "
             f"{torch.cuda.get_device_name(0)}",
             f"# instances (live, dead): ground truth {[len(s) for s in gt_stacks]}, prediction "
             f"{[len(s) for s in pred_stacks]}; the table of the pair holds {n_rows} rows",
             f"{'call':66s} {'median [min, max]':>30s}"]
    lines += [row(k, us[k]) for k in kernel]
    lines += [row(k, us[k]) for k in device]
    lines += [row(k, us[k]) for k in host]
    lines.append("# ratios of the medians")
    for name, (_, nbytes) in kernel.items():
        lines.append(f"{name}: {nbytes / 1e6:.1f} MB read, {nbytes / med[name] / 1e3:.1f} GB/s")
    lines.append("semantic_counts of the two int64 planes: "
                 f"{2 * S * S * 16 / med['semantic_counts of the two int64 planes'] / 1e3:.1f} GB/s")
    lines.append(f"bytes of the four mask stacks {stack_bytes / 1e6:.1f} MB against the int32 maps' {2 * 2 * S * S * 4 / 1e6:.1f} MB")
    lines.append("instance_counts on the stacks / label_pairs int32 whole call: "
                 f"{med['instance_counts on the mask stacks, both classes'] / med['label_pairs int32 / int32, whole call']:.1f}")
    lines.append("metric part from the stacks / from the maps: "
                 f"{med['metric part from the stacks: calculate_instance_metrics'] / med['metric part from the maps: label_pairs + instance_stats_from_pairs']:.2f}")
    lines.append("label_components 4-connected / 8-connected: "
                 f"{med['label_components of the live mask, 4-connected'] / med['label_components of the live mask, 8-connected']:.2f}")
    lines.append(f"# worst case, every pixel its own run: randint(0, 50) gives {rows[50]} rows, randint(0, 1000) "
                 f"{rows[1000]} rows (the table regrows from {ops.PAIRS_FIRST_CAPACITY} slots on every call)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
