"""Device time of the score histogram (csrc/curves.hip) next to the project's one-pass streaming yardstick and a
torch-only route.

    python tools/curves_bench.py [--size 1024] [--reps 200] [--rounds 5] [--out profiles/curves_bench.txt]

One process, device events, the routes alternating over the rounds.  Reported per line: median [min, max] of the
rounds' us/call, the bytes the call has to move (computed from the shapes, below) and bytes / median time.
  * score_hist of [3, S, S] probabilities and the [S, S] int64 mask into a resident (hist, invalid) pair, 1208 bins
    (metrics.curve_edges): 12 + 8 bytes per pixel (each class's blocks read the mask again: 36 bytes per pixel
    leave the caches).  Three maps: "saturated", the softmax of 24 x the one-hot eunet.synth mask plus unit noise
    (fp32 rounds it to 0 and 1: the end bins, whole waves on one address); "tails", the same with 12 x (scores
    within 1e-4 of 0 and 1, spread over the log-spaced tail bins by the noise); and "uniform", torch.rand (every
    lane its own bin).
  * score_hist with out=None on the saturated map: the same plus the allocation and zeroing of the outputs.
  * ops.semantic_counts of the mask against itself: 16 bytes per pixel, one pass, block-level integer sums.
  * torch only, on the device: per class torch.bucketize (right=True) of the plane, the key 2 bin + truth, and
    one torch.bincount; the confidence sums and the invalid / ignored rules are left out (it does less).
  The ratio saturated / uniform of score_hist shows whether the wave aggregation holds: without it the saturated
  map serialises 64 same-address atomics per wave and is the slower one.
Recorded, not gated.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "enhanced-unet_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from eunet import ops, synth  # noqa: E402
from eunet.metrics import curve_edges, curve_metrics_from_hist  # noqa: E402

DEV = "cuda"
WARMUP = 10


def timed(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps  # us per call


def alternate(fns, reps, rounds):
    for fn in fns.values():
        for _ in range(WARMUP):
            fn()
    us = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            us[name].append(timed(fn, reps))
    return us


def row(name, v, nbytes):
    m = statistics.median(v)
    return f"{name:46s} {m:9.1f} [{min(v):.1f}, {max(v):.1f}] us  {nbytes / 1e6:9.2f} MB  {nbytes / m / 1e6:6.3f} TB/s"


def torch_route(probs, mask, edges_dev, bins):
    out = []
    for c in range(probs.shape[0]):
        b = (torch.bucketize(probs[c].reshape(-1), edges_dev, right=True) - 1).clamp_(0, bins - 1)
        key = 2 * b + (mask.reshape(-1) == c)
        out.append(torch.bincount(key, minlength=2 * bins))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "curves_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("curves_bench: needs the GPU (nothing is measured without one)")
    S = a.size
    px = S * S
    sem = synth.tile(S, S, 0, num_classes=3)[1]
    mask = torch.from_numpy(sem).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    onehot = torch.nn.functional.one_hot(mask, 3).permute(2, 0, 1).float()
    noise = torch.randn(3, S, S, device=DEV, generator=g)
    sat = torch.softmax(24.0 * onehot + noise, 0).contiguous()
    tails = torch.softmax(12.0 * onehot + noise, 0).contiguous()
    uni = torch.rand(3, S, S, device=DEV, generator=g)
    e = curve_edges()
    bins = len(e) - 1
    ed = torch.from_numpy(e).to(DEV)
    end = float(((sat < e[1]) | (sat >= e[-2])).float().mean())
    lines = [f"# tools/curves_bench.py: [3, {S}, {S}] probabilities, {bins} bins; saturated map: {100 * end:.1f} % of the "
             f"scores in the two end bins; {a.reps} calls per round, {a.rounds} alternating rounds, {WARMUP} warm-up "
             f"calls; {torch.cuda.get_device_name(0)}",
             f"{'call':46s} {'median [min, max]':>28s} {'bytes':>13s} {'bytes / median':>12s}"]
    acc_s = ops.score_hist(sat, mask, ed)
    acc_u = ops.score_hist(uni, mask, ed)
    acc_t = ops.score_hist(tails, mask, ed)
    fns = {
        "score_hist saturated": (lambda: ops.score_hist(sat, mask, ed, out=acc_s), 20 * px),
        "score_hist tails": (lambda: ops.score_hist(tails, mask, ed, out=acc_t), 20 * px),
        "score_hist uniform": (lambda: ops.score_hist(uni, mask, ed, out=acc_u), 20 * px),
        "score_hist saturated, out=None": (lambda: ops.score_hist(sat, mask, ed), 20 * px),
        "semantic_counts": (lambda: ops.semantic_counts(mask[None], mask[None]), 16 * px),
        "torch bucketize + bincount saturated": (lambda: torch_route(sat, mask, ed, bins), 20 * px),
        "torch bucketize + bincount uniform": (lambda: torch_route(uni, mask, ed, bins), 20 * px),
    }
    us = alternate({k: v[0] for k, v in fns.items()}, a.reps, a.rounds)
    lines += [row(k, us[k], fns[k][1]) for k in fns]
    med = {k: statistics.median(v) for k, v in us.items()}
    lines.append("# ratios of the medians")
    lines.append(f"score_hist saturated / uniform: {med['score_hist saturated'] / med['score_hist uniform']:.3f}")
    for m in ("saturated", "uniform"):
        lines.append(f"score_hist {m} / semantic_counts: time {med['score_hist ' + m] / med['semantic_counts']:.3f}   "
                     f"bytes/s {(20 / med['score_hist ' + m]) / (16 / med['semantic_counts']):.3f}")
        lines.append(f"torch route {m} / score_hist {m}: time "
                     f"{med['torch bucketize + bincount ' + m] / med['score_hist ' + m]:.2f}")
    # what the timed calls computed is the restatement's (fresh outputs, on the timed tensors), and the torch
    # route's counts are the histogram's
    import _curves_ref as R
    ok = True
    for p in (sat, tails, uni):
        hist, inv = ops.score_hist(p, mask, ed)
        ref, rinv = R.score_hist_ref(p.cpu().numpy(), sem, e)
        ok = ok and np.array_equal(hist.cpu().numpy(), ref) and int(inv.item()) == rinv
        t = torch.stack(torch_route(p, mask, ed, bins)).reshape(3, bins, 2)
        ok = ok and torch.equal(t, hist[:, :, :2])
    lines.append(f"# fresh score_hist calls equal the numpy restatement and the torch route's counts on these tensors: {ok}")
    r = curve_metrics_from_hist(ops.score_hist(sat, mask, ed)[0], e)
    lines.append("# saturated map: " + ", ".join(f"{n} auc {v['auc']:.6f} +- {v['auc_resolution']:.1e} ap {v['ap']:.6f} "
                                                 f"ece {v['ece']:.4f}" for n, v in r.items()))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
