"""Device time of the exact distance transform and the boundary statistics (csrc/boundary.hip) next to the project's
one-pass streaming yardstick, its other distance kernel and the host route the reference would take.

    python tools/boundary_bench.py [--size 1024] [--reps 50] [--rounds 5] [--out profiles/boundary_bench.txt]

One process, device events, the routes alternating over the rounds.  Reported per line: median [min, max] of the
rounds' us/call, the bytes the call has to move (computed from the shapes, below) and bytes / median time.
The ground truth is the [S, S] eunet.synth mask (3 classes); the prediction is a perturbed copy: shifted by
(1, 2) pixels with 1 % of its pixels relabelled at random.
  * distance_transform_sq "edge" of the 3 classes into a resident buffer: per class the map is read once (8 B per
    pixel; its neighbours come from the caches), the plane is written, re-read and rewritten by the column pass and
    read and written once more by the row pass: 3 x (8 + 4 x 4) bytes per pixel.
  * the same transform ("eq", one value) of a map with a single site: the row pass's outward scan runs to the site
    from every pixel, its worst case; 8 + 16 bytes per pixel.  Reported next to the realistic case, not in its place.
  * boundary_stats into resident outputs (cap 64, radius 2): the two 3-class transforms, the 13-pixel pass over both
    maps (16 bytes per pixel) and the statistics pass (per class both maps and both transforms: 24 bytes per pixel),
    with the allocation of the workspace.
  * metrics.calculate_boundary_stats end to end with out=None: the same plus the zeroed outputs.
  * ops.semantic_counts of the mask against the prediction: 16 bytes per pixel, one pass.
  * ops.border_weight_map at its default radius (28) on the synth instance map: 8 bytes read, 4 written per pixel.
  * the host route: both masks copied to the host; per class scipy.ndimage.binary_erosion for the edges and
    distance_transform_edt of both, then numpy for the same histogram, maximum, sum and band counts (the reference
    rows are left out: it does less).  A host clock around the whole, masks resident on the device before.
Recorded, not gated.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "enhanced-unet_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from eunet import metrics, ops, synth  # noqa: E402

DEV = "cuda"
WARMUP = 5


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


def row(name, v, nbytes):
    m = statistics.median(v)
    return f"{name:50s} {m:10.1f} [{min(v):.1f}, {max(v):.1f}] us  {nbytes / 1e6:9.2f} MB  {nbytes / m / 1e6:6.3f} TB/s"


def host_route(pred_dev, gt_dev, cap=64, radius=2, ignore=255):
    """What the reference's tools give: scipy morphology and distance transforms on the host, numpy statistics."""
    from scipy import ndimage as nd
    pred, gt = pred_dev.cpu().numpy(), gt_dev.cpu().numpy()
    pred = np.where(gt == ignore, ignore, pred)
    cap2 = cap * cap
    surf = np.zeros((3, 2, cap2 + 5), np.int64)
    band = np.zeros((3, 1, 3), np.int64)
    for c in range(3):
        rp, rg = pred == c, gt == c
        ep, eg = rp & ~nd.binary_erosion(rp), rg & ~nd.binary_erosion(rg)
        if not ep.any() or not eg.any():
            continue  # the benchmark's maps hold every class on both sides
        dp = np.rint(nd.distance_transform_edt(~ep) ** 2).astype(np.int64)
        dg = np.rint(nd.distance_transform_edt(~eg) ** 2).astype(np.int64)
        for d, (own, other) in enumerate(((ep, dg), (eg, dp))):
            d2 = other[own]
            surf[c, d, :cap2 + 1] = np.bincount(d2[d2 <= cap2], minlength=cap2 + 1)
            surf[c, d, cap2 + 1] = int((d2 > cap2).sum())
            surf[c, d, cap2 + 3] = int(d2.max())
            surf[c, d, cap2 + 4] = int(np.floor(np.sqrt(d2.astype(np.float64)) * 65536.0).sum())  # no integer fix-up
        bp, bg = rp & (dp <= radius * radius), rg & (dg <= radius * radius)
        band[c, 0] = (bp.sum(), bg.sum(), (bp & bg).sum())
    return surf, band


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boundary_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("boundary_bench: needs the GPU (nothing is measured without one)")
    S = a.size
    px = S * S
    _, sem, inst = synth.tile(S, S, 0, num_classes=3, instances=True)
    rng = np.random.default_rng(0)
    pert = np.roll(sem, (1, 2), axis=(0, 1))
    flip = rng.random((S, S)) < 0.01
    pert[flip] = rng.integers(0, 3, int(flip.sum()))
    gt, pred = torch.from_numpy(sem).to(DEV), torch.from_numpy(pert).to(DEV)
    labels = torch.from_numpy(inst).to(DEV)
    one = torch.zeros(S, S, dtype=torch.int64, device=DEV)
    one[S // 3, S // 5] = 1
    edge_out = torch.empty(3, S, S, dtype=torch.int32, device=DEV)
    one_out = torch.empty(1, S, S, dtype=torch.int32, device=DEV)
    acc = ops.boundary_stats(pred, gt)
    wmap_out = ops.border_weight_map(labels, gt)
    edt_b, stats_b = 3 * 24 * px, (2 * 3 * 24 + 16 + 3 * 24) * px
    fns = {
        "distance_transform_sq edge, 3 classes": (lambda: ops.distance_transform_sq(gt, [0, 1, 2], "edge", out=edge_out), edt_b),
        "distance_transform_sq eq, a single site": (lambda: ops.distance_transform_sq(one, [1], "eq", out=one_out), 24 * px),
        "boundary_stats (2 transforms + rows + statistics)": (lambda: ops.boundary_stats(pred, gt, out=acc), stats_b),
        "calculate_boundary_stats, out=None": (lambda: metrics.calculate_boundary_stats(pred, gt), stats_b),
        "semantic_counts": (lambda: ops.semantic_counts(pred[None], gt[None]), 16 * px),
        "border_weight_map, default radius": (lambda: ops.border_weight_map(labels, gt, out=wmap_out), 12 * px),
    }
    for fn, _ in fns.values():
        for _ in range(WARMUP):
            fn()
    host_route(pred, gt)
    us = {name: [] for name in list(fns) + ["host route: scipy + numpy"]}
    for _ in range(a.rounds):
        for name, (fn, _) in fns.items():
            us[name].append(timed(fn, a.reps))
        us["host route: scipy + numpy"].append(host_timed(lambda: host_route(pred, gt), a.host_reps))
    med = {k: statistics.median(v) for k, v in us.items()}
    n_edge = int((ops.distance_transform_sq(gt, [0, 1, 2], "edge") == 0).sum())
    lines = [f"# tools/boundary_bench.py: [{S}, {S}] eunet.synth mask (3 classes, {n_edge} edge pixels) against a perturbed "
             f"copy; {a.reps} calls per round ({a.host_reps} of the host route), {a.rounds} alternating rounds, {WARMUP} "
             f"warm-up calls; {torch.cuda.get_device_name(0)}",
             f"{'call':50s} {'median [min, max]':>29s} {'bytes':>13s} {'bytes / median':>12s}"]
    lines += [row(k, us[k], v[1]) for k, v in fns.items()]
    lines.append(row("host route: scipy + numpy", us["host route: scipy + numpy"], 16 * px))
    lines.append("# ratios of the medians")
    t_edt, t_stats = med["distance_transform_sq edge, 3 classes"], med["boundary_stats (2 transforms + rows + statistics)"]
    lines.append(f"boundary_stats - 2 x transform (the reference rows, the statistics pass, the workspace): "
                 f"{t_stats - 2 * t_edt:.1f} us")
    lines.append(f"single site / realistic transform, per plane: "
                 f"{med['distance_transform_sq eq, a single site'] / (t_edt / 3):.1f}")
    lines.append(f"transform (3 classes) / semantic_counts: time {t_edt / med['semantic_counts']:.2f}")
    lines.append(f"transform (3 classes) / border_weight_map: time {t_edt / med['border_weight_map, default radius']:.2f}")
    lines.append(f"host route / boundary_stats: time {med['host route: scipy + numpy'] / t_stats:.1f}")
    # what the timed calls computed: the resident accumulator holds a whole number of copies of one fresh call,
    # the fresh call equals the numpy restatement (at a size the restatement can afford) and the host route
    import _boundary_ref as R
    fresh = ops.boundary_stats(pred, gt)
    hs, hb = host_route(pred, gt)
    c2 = 64 * 64
    ok_host = np.array_equal(fresh[0][:, :, :c2 + 4].cpu().numpy(), hs[:, :, :c2 + 4]) and \
        np.array_equal(fresh[1].cpu().numpy(), hb)
    q = 256
    small = ops.boundary_stats(pred[:q, :q].contiguous(), gt[:q, :q].contiguous(), band_radii=(0, 2))
    ref = R.boundary_stats(pert[:q, :q], sem[:q, :q], radii=(0, 2))
    ok_ref = all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(small, ref))
    lines.append(f"# a fresh boundary_stats equals the host route's histogram, counts, maximum and band: {ok_host}; "
                 f"the {q} x {q} corner equals the numpy restatement: {ok_ref}")
    m = metrics.boundary_metrics_from_stats({"surf": fresh[0], "band": fresh[1], "refrows": fresh[2], "cap": 64,
                                             "band_radii": (2,)})
    lines.append("# " + ", ".join(f"{n}: nsd@2 {m[n]['nsd'][2]:.4f} hd {m[n]['hd']:.2f} hd95 {m[n]['hd95']:.2f} assd "
                                  f"{m[n]['assd']:.4f} biou@2 {m[n]['boundary_iou'][2]:.4f}" for n in metrics.CLASS_NAMES))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
