"""Whole-image against overlap-tile inference on one large image (Evaluator._run_model_single, csrc/tiling.hip).

    python tools/tiled_infer_bench.py [--size 2048] [--tiles 512 1024] [--base 64] [--dtype bf16]
                                      [--reps 3] [--rounds 5] [--out profiles/tiled_infer_bench.txt]

One process, device events.  Enhanced-UNet, 3 channels -> 3 classes, eval mode, a size x size image resident on
the device, preprocess off: a call is one _run_model_single (reflect pad, forward_lowres, softmax + crop for the
whole-image route; tile_gather, forward_lowres per tile_batch tiles, one tile_blend for the tiled routes, blend
"crop" with the default margin).  The routes alternate over the rounds after 2 warm-up calls each; reported: median
[min, max] of the rounds' ms/image, and whether the tiled probabilities are bit-equal to the whole-image ones.
Then one extra call per tiled route under eunet.kprof.KernelTimer: the device time of tile_gather (all launches of
the call) and tile_blend against their bytes (gather: every tile element read and written once; blend: every tile
logit read once, every probability written once).  Inflation = (N th tw) / (hp wp), the area pushed through the
network over the padded image's, beside its large-image limit (tile / stride)^2.  Recorded, not gated.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "enhanced-unet_amd")]
import torch  # noqa: E402
from eunet import kprof, tiling  # noqa: E402
from eunet.evaluator import Evaluator  # noqa: E402
from eunet.models import EnhancedUNet  # noqa: E402

DEV = "cuda"
WARMUP = 2


def timed(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps  # ms per call


def med(v):
    return f"{statistics.median(v):9.2f} [{min(v):.2f}, {max(v):.2f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--tiles", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--base", type=int, default=64)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--tile-batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiled_infer_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tiled_infer_bench: needs the GPU (nothing is measured without one)")
    torch.manual_seed(0)
    m = EnhancedUNet(num_classes=3, in_channels=3, base_ch=a.base, dtype=a.dtype)
    g = torch.Generator().manual_seed(1)
    for k, v in m.state_dict().items():  # BatchNorm statistics off (0, 1): eval mode is a real affine
        if k.endswith("running_mean"):
            v.copy_(0.1 * torch.randn(v.shape, generator=g))
        elif k.endswith("running_var"):
            v.copy_(0.5 + torch.rand(v.shape, generator=g))
    m = m.to(DEV).eval()
    img = torch.rand(3, a.size, a.size, generator=g).to(DEV)
    routes = {"whole": Evaluator(m, DEV, "enhanced_unet", preprocess=None)}
    for t in a.tiles:
        routes[f"tile {t}"] = Evaluator(m, DEV, "enhanced_unet", preprocess=None, tile=t, tile_batch=a.tile_batch)
    lines = [f"# tools/tiled_infer_bench.py: Evaluator._run_model_single, Enhanced-UNet base {a.base}, 3 -> 3, "
             f"{a.dtype}, {a.size}^2 image, blend crop, margin {tiling.RECEPTIVE_MARGIN}, tile_batch {a.tile_batch}; "
             f"{a.reps} calls per round, {a.rounds} alternating rounds, {WARMUP} warm-up calls; "
             f"{torch.cuda.get_device_name(0)}",
             f"{'route':12s} {'ms/image median [min, max]':>32s} {'tiles':>8s} {'inflation':>10s} {'limit':>6s} "
             f"{'bit-equal':>10s}"]
    fns = {name: (lambda ev=ev: ev._run_model_single(img)) for name, ev in routes.items()}
    ref = None
    equal = {}
    for name, fn in fns.items():
        for _ in range(WARMUP):
            out = fn()
        if name == "whole":
            ref = out.clone()
        else:
            equal[name] = bool(torch.equal(out, ref))
    ms = {name: [] for name in fns}
    for _ in range(a.rounds):
        for name, fn in fns.items():
            ms[name].append(timed(fn, a.reps))
    for name, ev in routes.items():
        if ev.tile is None:
            lines.append(f"{name:12s} {med(ms[name]):>32s} {'-':>8s} {1.0:10.2f} {'-':>6s} {'-':>10s}")
        else:
            p = ev._tile_plan(a.size, a.size)
            lines.append(f"{name:12s} {med(ms[name]):>32s} {f'{p.ny}x{p.nx}':>8s} {p.inflation:10.2f} "
                         f"{(p.tile / p.stride) ** 2:6.2f} {str(equal[name]):>10s}")
    lines.append(f"{'kernel (device events, 1 call)':32s} {'launches':>9s} {'ms':>9s} {'MB':>9s} {'TB/s':>7s}")
    for name, ev in routes.items():
        if ev.tile is None:
            continue
        with kprof.KernelTimer() as kt:
            fns[name]()
        s = kt.summary()
        for fam in ("tile_gather", "tile_blend"):
            r = s[fam]
            lines.append(f"{name + ' ' + fam:32s} {r['launches']:9d} {r['ms']:9.3f} {r['bytes'] / 1e6:9.1f} "
                         f"{r['bytes'] / 1e9 / r['ms']:7.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
