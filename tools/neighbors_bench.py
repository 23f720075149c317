"""Time of the nearest-cell transform, the label expansion and the contact table (csrc/neighbors.hip) next to the
tree's kernels they are siblings of.

    python tools/neighbors_bench.py [--size 1024] [--reps 10] [--rounds 5] [--out profiles/neighbors_bench.txt]

One process, the routes alternating over the rounds; per line the median [min, max] of the rounds.  Device times are
kprof's events around the C-ABI call, whole calls a host clock around calls that end in a read-back or a synchronise.
The map is the [S, S] eunet.synth tile (3 classes, instances=True) as ONE pooled id map, as Evaluator.measure_neighbors
forms it.
  * nearest_site (int32 and int64 ids) next to distance_transform_sq(ids, [0], "ne") of the same plane: the same
    sites, the parent's two kernels, 4 bytes fewer written per pixel and no index carried through the row scan;
  * expand_label_map without a limit (the Voronoi partition) and with distance 8;
  * label_contacts (connectivity 4 and 8) of the Voronoi partition, which is what measure_neighbors counts, next to
    the device pass of label_pairs of the map against a perturbed copy, the one-pass hash-table yardstick;
  * the whole Evaluator.measure_neighbors call after the mask (the prediction is stubbed with the tile's mask);
  * the worst cases: a plane with a single site in a corner, where every pixel's row scan runs to the site's column,
    and torch.randint(1, 51) noise ids, where every pixel inserts into the table.
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
    return f"{name:74s} {statistics.median(v):11.1f} [{min(v):.1f}, {max(v):.1f}] us"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbors_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("neighbors_bench: needs the GPU (nothing is measured without one)")
    S = a.size
    x, sem, inst = synth.tile(S, S, 0, num_classes=3, instances=True)
    pooled_np = np.where(np.asarray(sem) > 0, np.asarray(inst), 0).astype(np.int64)
    other_np = np.roll(pooled_np, (3, 2), axis=(0, 1))
    other_np[(other_np % 7) == 3] = 0
    ids64 = torch.from_numpy(pooled_np).to(DEV)
    ids32, other32 = ids64.int(), torch.from_numpy(other_np).to(DEV).int()
    voronoi = ops.expand_label_map(ids32)
    single = torch.zeros(S, S, dtype=torch.int32, device=DEV)
    single[S - 1, S - 1] = 1
    noise = torch.randint(1, 51, (S, S), device=DEV, dtype=torch.int32)
    edt_in = ids64.unsqueeze(0).contiguous()

    # the transform's distances are the parent's
    dist, site = ops.nearest_site(ids32)
    assert torch.equal(dist, ops.distance_transform_sq(edt_in, [0], "ne")[0, 0]), "nearest_site and edt_sq disagree"
    assert torch.equal(voronoi, ids32.reshape(-1)[site.reshape(-1).long()].reshape(S, S)), "expansion is not the gather"

    from eunet.evaluator import Evaluator
    from eunet.models import EnhancedUNet
    torch.manual_seed(0)
    ev = Evaluator(EnhancedUNet(num_classes=3, in_channels=3, base_ch=16).to(DEV).eval(), DEV, "enhanced_unet",
                   preprocess=None, split="watershed")
    mask = torch.from_numpy(np.ascontiguousarray(sem).astype(np.int64)).to(DEV)
    ev._predict_mask_device = lambda image: mask
    image = torch.from_numpy(np.asarray(x))

    calls = {
        "nearest_site int32": (lambda: ops.nearest_site(ids32), "nearest_site"),
        "nearest_site int64": (lambda: ops.nearest_site(ids64), "nearest_site"),
        'distance_transform_sq(ids, [0], "ne") int64': (lambda: ops.distance_transform_sq(edt_in, [0], "ne"), "edt_sq"),
        "expand_label_map int32, no limit (Voronoi)": (lambda: ops.expand_label_map(ids32), "expand_label_map"),
        "expand_label_map int32, distance 8": (lambda: ops.expand_label_map(ids32, 8), "expand_label_map"),
        "label_contacts int32 of the Voronoi partition, connectivity 4": (lambda: ops.label_contacts(voronoi, 4),
                                                                          "label_contacts"),
        "label_contacts int32 of the Voronoi partition, connectivity 8": (lambda: ops.label_contacts(voronoi, 8),
                                                                          "label_contacts"),
        "label_contacts int32 of the cells themselves, connectivity 4": (lambda: ops.label_contacts(ids32, 4),
                                                                         "label_contacts"),
        "label_pairs int32 / int32": (lambda: ops.label_pairs(other32, ids32), "label_pairs"),
        "worst case: nearest_site of a single site in the last corner": (lambda: ops.nearest_site(single),
                                                                        "nearest_site"),
        'worst case: distance_transform_sq "ne" of the same single site': (
            lambda: ops.distance_transform_sq(single.long().unsqueeze(0), [0], "ne"), "edt_sq"),
        "worst case: label_contacts of randint(1, 51) noise, connectivity 4": (lambda: ops.label_contacts(noise, 4),
                                                                              "label_contacts"),
        "worst case: label_contacts of randint(1, 51) noise, connectivity 8": (lambda: ops.label_contacts(noise, 8),
                                                                              "label_contacts"),
    }
    whole = {"measure_neighbors after the mask (Voronoi, connectivity 4), whole call":
             lambda: ev.measure_neighbors(image)}
    for fn in [c[0] for c in calls.values()] + list(whole.values()):
        for _ in range(WARMUP):
            fn()
    us = {f"{k}, {part}": [] for k in calls for part in ("device time", "whole call")}
    us.update({k: [] for k in whole})
    for _ in range(a.rounds):
        for name, (fn, fam) in calls.items():
            us[f"{name}, whole call"].append(host_timed(fn, a.reps))
            with kprof.KernelTimer() as kt:  # the launches alone, bracketed by events: a run of its own
                for _ in range(a.reps):
                    fn()
            s = kt.summary()[fam]
            us[f"{name}, device time"].append(1e3 * s["ms"] / s["launches"])
        for name, fn in whole.items():
            us[name].append(host_timed(fn, max(1, a.reps // 5)))
    med = {k: statistics.median(v) for k, v in us.items()}
    got = ev.measure_neighbors(image)
    lines = [f"# tools/neighbors_bench.py: [{S}, {S}] eunet.synth tile (3 classes) as one pooled id map; {a.reps} "
             f"calls per round, {a.rounds} alternating rounds, {WARMUP} warm-up calls; {torch.cuda.get_device_name(0)}",
             f"# cells {int((np.unique(pooled_np) > 0).sum())}; foreground pixels {int((pooled_np > 0).sum())} of "
             f"{pooled_np.size}; contact rows of the Voronoi partition {len(ops.label_contacts(voronoi, 4))} (4), "
             f"{len(ops.label_contacts(voronoi, 8))} (8); measure_neighbors: {got['n_live']} live, {got['n_dead']} "
             "dead",
             f"{'call':74s} {'median [min, max]':>30s}"]
    lines += [row(k, v) for k, v in us.items()]
    lines.append("# ratios of the medians, device time")

    def ratio(a_, b_):
        return med[a_ + ", device time"] / med[b_ + ", device time"]

    edt = 'distance_transform_sq(ids, [0], "ne") int64'
    lines.append(f"nearest_site int32 / distance_transform_sq: {ratio('nearest_site int32', edt):.2f}")
    lines.append(f"nearest_site int64 / distance_transform_sq: {ratio('nearest_site int64', edt):.2f}")
    lines.append("expand_label_map (Voronoi) / nearest_site int32: "
                 f"{ratio('expand_label_map int32, no limit (Voronoi)', 'nearest_site int32'):.2f}")
    lines.append("expand_label_map (distance 8) / nearest_site int32: "
                 f"{ratio('expand_label_map int32, distance 8', 'nearest_site int32'):.2f}")
    for c in (4, 8):
        k = f"label_contacts int32 of the Voronoi partition, connectivity {c}"
        lines.append(f"label_contacts (Voronoi, {c}) / label_pairs: {ratio(k, 'label_pairs int32 / int32'):.2f}")
        k = f"worst case: label_contacts of randint(1, 51) noise, connectivity {c}"
        lines.append(f"label_contacts (noise, {c}) / label_pairs: {ratio(k, 'label_pairs int32 / int32'):.2f}")
    one, one_edt = [k for k in calls if "single site" in k]
    lines.append(f"single site: nearest_site / distance_transform_sq: {ratio(one, one_edt):.2f}")
    lines.append(f"single site / the tile, nearest_site: {ratio(one, 'nearest_site int32'):.1f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
