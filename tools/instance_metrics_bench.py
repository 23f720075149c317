"""Time eunet.metrics.calculate_instance_metrics against the reference's per-pair numpy method.

    python tools/instance_metrics_bench.py [--size 1024] [--cells 300] [--repeats 20] [--out FILE]

Inputs: `cells` predicted and `cells` true discs of radius 6-10 on a size x size image (seeded; ~70 % live),
the true ones jittered copies of the predicted ones, as [h, w] uint8 masks.

GPU figure: the whole calculate_instance_metrics call on device tensors (the form semantic_to_instances and
CellDataset produce) -- host clock around the call, which ends in the device-to-host copy of the count
matrices, i.e. a synchronise.  3 warm-up calls, then `repeats` timed ones: median and [min, max].  The same
with numpy inputs (adds the host-to-device copy of the masks), and the two kernels alone from device events.

CPU figure: the reference evaluates calculate_iou -- np.logical_and(a, b).sum() and np.logical_or(a, b).sum()
on the two full-size masks (metrics.py:12-18) -- once per (prediction, unmatched ground truth) pair.  All of
them would take minutes, so `--pairs` seeded random pairs are timed (median of 3 passes) and scaled to the
number of pairs the greedy loop visits on these inputs (counted exactly from the GPU's count matrices).
The intersections of the sampled pairs are compared with the GPU's: they must be equal.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "enhanced-unet_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def make_inputs(size, cells, seed=11):
    g = np.random.default_rng(seed)
    yy, xx = np.ogrid[:size, :size]

    def disc(cy, cx, r):
        return ((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r).astype(np.uint8)

    cy, cx = g.integers(12, size - 12, cells), g.integers(12, size - 12, cells)
    r = g.integers(6, 11, cells)
    labels = (g.random(cells) > 0.7).astype(int).tolist()
    pred = [disc(cy[i], cx[i], r[i]) for i in range(cells)]
    gt = [disc(cy[i] + g.integers(-4, 5), cx[i] + g.integers(-4, 5), g.integers(6, 11)) for i in range(cells)]
    scores = g.random(cells).tolist()
    return pred, labels, scores, gt, list(labels)


def visited_pairs(inter, ap, ag, scores, thr=0.05):
    """Number of calculate_iou calls of the reference's greedy loop for one class."""
    order = sorted(range(len(ap)), key=lambda i: scores[i], reverse=True)
    matched, calls = set(), 0
    for p in order:
        best, best_g = 0.0, -1
        for g in range(len(ag)):
            if g in matched:
                continue
            calls += 1
            u = int(ap[p]) + int(ag[g]) - int(inter[p, g])
            iou = 1.0 if u == 0 else int(inter[p, g]) / u
            if iou > best:
                best, best_g = iou, g
        if best >= thr and best_g >= 0:
            matched.add(best_g)
    return calls


def timed(fn, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "n": len(ts)}


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--size", type=int, default=1024)
    ap_.add_argument("--cells", type=int, default=300)
    ap_.add_argument("--repeats", type=int, default=20)
    ap_.add_argument("--pairs", type=int, default=300)
    ap_.add_argument("--out", default=None)
    a = ap_.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("instance_metrics_bench: needs the GPU (no CPU fallback)")
    from eunet import metrics, ops

    pred, pl, sc, gt, gl = make_inputs(a.size, a.cells)
    dpred = [torch.from_numpy(m).cuda() for m in pred]
    dgt = [torch.from_numpy(m).cuda() for m in gt]
    res = {"size": a.size, "pred": len(pred), "gt": len(gt), "device": torch.cuda.get_device_name(0)}
    res["gpu_device_inputs"] = timed(lambda: metrics.calculate_instance_metrics(dpred, pl, sc, dgt, gl), a.repeats)
    res["gpu_numpy_inputs"] = timed(lambda: metrics.calculate_instance_metrics(pred, pl, sc, gt, gl), a.repeats)

    sp, sg = torch.stack(dpred), torch.stack(dgt)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ks = []
    for i in range(3 + a.repeats):
        ev[0].record()
        pp, _ = ops.pack_masks(sp)
        pg, _ = ops.pack_masks(sg)
        inter = ops.pairwise_overlap(pp, pg)
        ev[1].record()
        torch.cuda.synchronize()
        if i >= 3:
            ks.append(ev[0].elapsed_time(ev[1]))
    res["kernels_pack2_overlap_all_pairs"] = {"median_ms": statistics.median(ks), "min_ms": min(ks), "max_ms": max(ks)}
    inter = inter.cpu().numpy()

    # the reference's per-pair cost on this host's CPU, sampled
    g = np.random.default_rng(5)
    pairs = [(int(g.integers(len(pred))), int(g.integers(len(gt)))) for _ in range(a.pairs)]
    passes = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = []
        for p, q in pairs:
            i = np.logical_and(pred[p], gt[q]).sum()
            u = np.logical_or(pred[p], gt[q]).sum()
            got.append((i, u))
        passes.append((time.perf_counter() - t0) / len(pairs) * 1e3)
    assert all(int(i) == int(inter[p, q]) for (p, q), (i, _) in zip(pairs, got)), "GPU and numpy intersections differ"
    calls = 0
    for cid in (0, 1):
        ip = [i for i, l in enumerate(pl) if l == cid]
        ig = [i for i, l in enumerate(gl) if l == cid]
        if ig:
            sub = inter[np.ix_(ip, ig)]
            calls += visited_pairs(sub, [pred[i].sum() for i in ip], [gt[i].sum() for i in ig], [sc[i] for i in ip])
    per_pair = statistics.median(passes)
    res["cpu_reference_method"] = {"per_pair_ms_median": per_pair, "per_pair_ms_passes": passes, "sampled_pairs": len(pairs),
                                   "pairs_visited": calls, "projected_s": per_pair * calls / 1e3,
                                   "cpu_threads": torch.get_num_threads()}
    res["speedup_projected"] = per_pair * calls / res["gpu_device_inputs"]["median_ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
