"""Device time of the elastic / affine warp (csrc/warp.hip) next to the flips that move the same tensors.

    python tools/warp_bench.py [--size 1024] [--reps 200] [--rounds 5] [--out profiles/warp_bench.txt]

One process, device events, the routes alternating over the rounds.  Reported per line: median [min, max] of the
rounds' us/call, the bytes the call has to move (computed from the shapes, below) and bytes / median time.
  * elastic_grid [S, S, 2] from a resident 3 x 3 control grid and a rotation + zoom: 8 S^2 bytes written.
  * warp_u8 of an [S, S, 3] image through that map against flip_u8 of the same image: map 8 + source 3 + output 3
    bytes per pixel against 3 + 3.
  * warp_labels of the tile's int64 class mask against flip_mask: 8 + 8 + 8 against 8 + 8.
  * warp_labels of a per-instance uint8 stack [N, S, S] (one plane per drawn cell of eunet.synth tiles 0 and 1,
    the first --planes = 264 of them) against flip_u8 of the same bytes viewed as [N S, S, 1]: 2 N bytes per pixel each; the warp reads the map once
    per 64 planes on top (8 ceil(N / 64)).
  The source bytes count every source pixel once: a smooth map reads each about once, from cache lines that
  neighbouring pixels share.
  * the map's largest error against the fp64 restatement (tests/_warp_ref.py) at the suite's shapes and at S^2 with
    a 45 degree rotation at scale 0.7, in units of 2^-23 max(h, w, max |grid|) (the suite's bound is 8 units), and
    with control displacements of three image sizes, where the weights' own rounding shows.
  * CellDataset.__getitem__ on one LabelMe item of S x S written to a temporary directory, with and without
    elastic=, host clock around the item and a device synchronise, the same `random` seed before every item.
Recorded, not gated.
"""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "enhanced-unet_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from eunet import ops, synth  # noqa: E402
from eunet.data import CellDataset, warp_matrix  # noqa: E402

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


def map_error(h, w, gh, gw, angle, scale, sigma, seed):
    import _warp_ref as R
    ctrl = np.random.default_rng(seed).normal(0.0, sigma, (2, gh, gw)).astype(np.float32)
    m = warp_matrix(h, w, angle, scale)
    got = ops.elastic_grid(h, w, ctrl, m, device=DEV).double().cpu().numpy()
    ref = R.grid_ref(h, w, ctrl.astype(np.float64), m.astype(np.float32).astype(np.float64))
    return float(np.abs(got - ref).max()) / (2.0 ** -23 * max(h, w, float(np.abs(ref).max())))


def write_item(d, size, n_cells=60):
    """One S x S LabelMe item (ten files, so that the train split holds seven): a synth tile and octagonal cells."""
    from PIL import Image
    rng = np.random.default_rng(7)
    img = (synth.tile(size, size, 0, in_channels=3)[0].transpose(1, 2, 0) * 255).astype(np.uint8)
    shapes = []
    for j in range(n_cells):
        cx, cy, r = rng.uniform(20, size - 20), rng.uniform(20, size - 20), rng.uniform(6, 16)
        pts = [[cx + r * np.cos(a), cy + r * np.sin(a)] for a in np.linspace(0, 2 * np.pi, 8, endpoint=False)]
        shapes.append({"label": "live" if j % 3 else "dead", "points": pts})
    for i in range(10):
        Image.fromarray(img).save(os.path.join(d, f"b{i:02d}.jpg"), quality=95)
        with open(os.path.join(d, f"b{i:02d}.json"), "w") as f:
            json.dump({"shapes": shapes}, f)


def item_times(ds_by_name, reps, rounds):
    def one(ds):
        random.seed(0)
        np.random.seed(0)
        t0 = time.perf_counter()
        ds[0]
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)  # ms
    for ds in ds_by_name.values():
        for _ in range(3):
            one(ds)
    ms = {name: [] for name in ds_by_name}
    for _ in range(rounds):
        for name, ds in ds_by_name.items():
            ms[name].append(statistics.median(one(ds) for _ in range(reps)))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--planes", type=int, default=264)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("warp_bench: needs the GPU (nothing is measured without one)")
    S = a.size
    x, sem, inst = synth.tile(S, S, 0, num_classes=3, in_channels=3, instances=True)
    img = torch.from_numpy((x.transpose(1, 2, 0) * 255).astype(np.uint8)).contiguous().to(DEV)
    mask = torch.from_numpy(sem).to(DEV)
    planes = [(inst == i).astype(np.uint8) for i in np.unique(inst).tolist() if i]
    inst1 = synth.tile(S, S, 1, num_classes=3, instances=True)[2]  # topped up from tile 1 to a.planes planes
    planes += [(inst1 == i).astype(np.uint8) for i in np.unique(inst1).tolist() if i]
    stack = torch.from_numpy(np.stack(planes[:a.planes])).to(DEV)
    N = stack.shape[0]
    ctrl = torch.from_numpy(np.random.default_rng(0).normal(0.0, 10.0, (2, 3, 3)).astype(np.float32)).to(DEV)
    m = warp_matrix(S, S, 20.0, 1.1)
    grid = ops.elastic_grid(S, S, ctrl, m, device=DEV)
    px = S * S
    lines = [f"# tools/warp_bench.py: {S}^2, eunet.synth tile 0 ({N} instance planes, topped up from tile 1); map: 3 x 3 control grid sigma 10, rotation "
             f"20 degrees, zoom 1.1, border reflect; {a.reps} calls per round, {a.rounds} alternating rounds, {WARMUP} "
             f"warm-up calls; {torch.cuda.get_device_name(0)}",
             f"{'call':46s} {'median [min, max]':>28s} {'bytes':>13s} {'bytes / median':>12s}"]
    flat = stack.reshape(N * S, S, 1)
    fns = {
        "elastic_grid": (lambda: ops.elastic_grid(S, S, ctrl, m, device=DEV), 8 * px),
        f"warp_u8 [{S},{S},3]": (lambda: ops.warp_u8(img, grid), 14 * px),
        f"flip_u8 [{S},{S},3]": (lambda: ops.flip_u8(img, 1), 6 * px),
        f"warp_labels int64 [{S},{S}]": (lambda: ops.warp_labels(mask, grid), 24 * px),
        f"flip_mask int64 [{S},{S}]": (lambda: ops.flip_mask(mask, 1), 16 * px),
        f"warp_labels uint8 [{N},{S},{S}]": (lambda: ops.warp_labels(stack, grid), (2 * N + 8 * -(-N // 64)) * px),
        f"flip_u8 of the stack as [{N}*{S},{S},1]": (lambda: ops.flip_u8(flat, 1), 2 * N * px),
    }
    us = alternate({k: v[0] for k, v in fns.items()}, a.reps, a.rounds)
    lines += [row(k, us[k], fns[k][1]) for k in fns]
    names = list(fns)
    lines.append("# ratios of the medians, warp / flip: time, and bytes per second")
    for wn, fn_ in ((names[1], names[2]), (names[3], names[4]), (names[5], names[6])):
        tw, tf = statistics.median(us[wn]), statistics.median(us[fn_])
        lines.append(f"{wn + ' / ' + fn_:78s} time {tw / tf:6.3f}   bytes/s {(fns[wn][1] / tw) / (fns[fn_][1] / tf):6.3f}")
    # the results the timed calls produced are the restatement's (one check per route, on the timed tensors)
    import _warp_ref as R
    gh = grid.cpu().numpy()
    ok = (np.array_equal(ops.warp_u8(img, grid).cpu().numpy(), R.warp_u8_ref(img.cpu().numpy(), gh)) and
          np.array_equal(ops.warp_labels(mask, grid).cpu().numpy(), R.warp_labels_ref(sem, gh)) and
          np.array_equal(ops.warp_labels(stack[:40], grid).cpu().numpy(), R.warp_labels_ref(stack[:40].cpu().numpy(), gh)))
    lines.append(f"# timed warps equal the integer restatement on these tensors: {ok}")
    errs = {}
    for (h, w) in ((1, 1), (7, 5), (33, 65), (96, 128), (256, 256)):
        for (gh_, gw_) in ((2, 2), (3, 3), (4, 7), (16, 16)):
            for k, (ang, sc, sg) in enumerate(((0.0, 1.0, 10.0), (33.0, 0.5, 4.0), (-10.0, 2.0, 2.0), (45.0, 0.7, 10.0))):
                errs[(h, w)] = max(errs.get((h, w), 0.0), map_error(h, w, gh_, gw_, ang, sc, sg, h + w + gh_ + k))
    errs[(S, S)] = max(map_error(S, S, g, g, 45.0, 0.7, 10.0, g) for g in (2, 3, 16))
    far = max(map_error(h, w, g, g, 45.0, 0.7, 3.0 * max(h, w), g) for (h, w) in ((7, 5), (33, 65), (96, 128), (256, 256))
              for g in (2, 3, 16))
    lines.append("# elastic_grid against the fp64 restatement, largest error in units of 2^-23 max(h, w, max |grid|) (suite bound: 8):")
    lines.append("#   " + ", ".join(f"{h}x{w}: {e:.2f}" for (h, w), e in errs.items()) + f"; overall {max(errs.values()):.2f}")
    lines.append(f"#   with control displacements of sigma = three image sizes (7x5 .. 256x256): {far:.2f}")
    with tempfile.TemporaryDirectory() as d:
        write_item(d, S)
        cfg = dict(sigma=10.0, grid=3, rotate=20.0, scale=(0.9, 1.1), seed=0)
        dss = {"plain": CellDataset(d, split="train", device=DEV),
               "elastic": CellDataset(d, split="train", device=DEV, elastic=dict(cfg)),
               "plain + weight_map": CellDataset(d, split="train", device=DEV, weight_map={}),
               "elastic + weight_map": CellDataset(d, split="train", device=DEV, weight_map={}, elastic=dict(cfg))}
        ms = item_times(dss, 5, a.rounds)
    lines.append(f"# CellDataset.__getitem__ of one {S} x {S} LabelMe item (60 polygons), ms per item (host clock, device "
                 f"synchronised), median [min, max] over {a.rounds} alternating rounds of 5 items")
    for name, v in ms.items():
        lines.append(f"{'__getitem__ ' + name:46s} {statistics.median(v):9.2f} [{min(v):.2f}, {max(v):.2f}] ms")
    for base in ("plain", "plain + weight_map"):
        el = base.replace("plain", "elastic")
        lines.append(f"    {el} / {base} (medians): {statistics.median(ms[el]) / statistics.median(ms[base]):.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
