"""Times of the U-Net border weight map (csrc/weightmap.hip), of separate_instances, and of the two losses with
and without a pixel weight (csrc/loss.hip, csrc/bce_dice.hip).

    python tools/weight_map_bench.py [--size 1024] [--batch 4] [--parent-lib PATH] [--out profiles/weight_map_bench.txt]

One process, device events, eunet.synth tiles (tile(..., instances=True): one id per drawn cell).  Reported per
line: median [min, max] of the rounds' us/call.
  * border_weight_map at sigma = 5 (R = 28) on the batch's label maps, with the number of instances and the
    fraction of background pixels that have two ids in reach (counted from a map at the same R with a sigma so
    large that no border term underflows), and at radius 48.
  * separate_instances on the same maps.
  * forward + backward of each loss through eunet.losses on resident tensors, weighted against unweighted,
    alternating over the rounds (the weight is the map above).
  * the unweighted C-ABI entry points (forward + backward, called through ctypes on preallocated buffers, no
    autograd) of this build against another build of the library (--parent-lib: libeunet_hip.so built from the
    parent commit), alternating; the parent is timed in two interleaved series ("parent", "parent again") so its own
    spread stands next to the difference.  Without --parent-lib that section says so.
Recorded, not gated.
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "enhanced-unet_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from eunet import _lib, ops, synth  # noqa: E402
from eunet.losses import bce_dice_loss, combined_loss  # noqa: E402

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


def med(v):
    return f"{statistics.median(v):10.1f} [{min(v):.1f}, {max(v):.1f}]"


def alternate(fns, reps, rounds):
    for fn in fns.values():
        for _ in range(WARMUP):
            fn()
    us = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            us[name].append(timed(fn, reps))
    return us


def raw_entries(lib, kind, x, t, k):
    """fwd + bwd of the unweighted entry points of `lib` (a ctypes.CDLL) on preallocated buffers."""
    n, _, h, w = x.shape
    pre = "eunet_bce_dice" if kind == "bce" else "eunet_loss"
    ln, nb = ctypes.c_int(), ctypes.c_size_t()
    getattr(lib, pre + "_sums_len")(n, k, ctypes.byref(ln))
    getattr(lib, pre + "_workspace_bytes")(n, k, h, w, ctypes.byref(nb))
    sums = torch.empty(ln.value, device=DEV)
    ws = torch.empty(nb.value, dtype=torch.uint8, device=DEV)
    loss, parts = torch.empty((), device=DEV), torch.empty(n, 3, device=DEV)
    gl, gx = torch.ones(1, device=DEV), torch.empty_like(x)
    fwd, bwd = getattr(lib, pre + "_fwd"), getattr(lib, pre + "_bwd")
    vp = ctypes.c_void_p
    fwd.argtypes = [vp, vp] + [ctypes.c_int] * 4 + [vp] * 6
    bwd.argtypes = [vp, vp] + [ctypes.c_int] * 4 + [vp] * 5
    st = torch.cuda.current_stream().cuda_stream
    a = (x.data_ptr(), t.data_ptr(), n, k, h, w, None)

    def call():
        if fwd(*a, sums.data_ptr(), loss.data_ptr(), parts.data_ptr(), ws.data_ptr(), st) or \
                bwd(*a, sums.data_ptr(), gl.data_ptr(), gx.data_ptr(), st):
            raise SystemExit(f"{pre}: entry point failed")

    call.keep = (sums, ws, loss, parts, gl, gx)
    call.result = lambda: (loss.clone(), gx.clone())
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weight_map_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("weight_map_bench: needs the GPU (nothing is measured without one)")
    B, S = a.batch, a.size
    tiles = [synth.tile(S, S, i, num_classes=3, instances=True) for i in range(B)]
    sem = torch.from_numpy(np.stack([t[1] for t in tiles])).to(DEV)
    lab = torch.from_numpy(np.stack([t[2] for t in tiles])).to(DEV)
    n_inst = sum(int(torch.unique(lab[i]).numel()) - 1 for i in range(B))
    reach = ops.border_weight_map(lab, w0=1.0, sigma=1e3, radius=28)
    bg = lab == 0
    frac = float(((reach > 1.0) & bg).sum()) / float(bg.sum())
    lines = [f"# tools/weight_map_bench.py: B {B}, {S}^2, eunet.synth tiles 0..{B - 1}; {a.reps} calls per round, "
             f"{a.rounds} alternating rounds, {WARMUP} warm-up calls; {torch.cuda.get_device_name(0)}",
             f"# {n_inst} instances in the batch; {100 * bg.float().mean().item():.1f} % of the pixels are background, "
             f"{100 * frac:.1f} % of those have two ids within R = 28",
             f"{'call':44s} {'us/call median [min, max]':>36s}"]
    out = torch.empty(B, S, S, device=DEV)
    cw = (1.0, 3.0, 2.0)
    us = alternate({
        "border_weight_map sigma 5 (R 28)": lambda: ops.border_weight_map(lab, sem, class_weight=cw, out=out),
        "border_weight_map sigma 5, radius 48": lambda: ops.border_weight_map(lab, sem, class_weight=cw, radius=48, out=out),
        "border_weight_map, no instance (base only)": lambda: ops.border_weight_map(torch.zeros_like(lab), sem, out=out),
        "separate_instances": lambda: ops.separate_instances(lab, sem),
    }, max(10, a.reps // 4), a.rounds)
    lines += [f"{name:44s} {med(v):>36s}" for name, v in us.items()]
    wm = ops.border_weight_map(lab, sem, class_weight=cw)
    g = torch.Generator().manual_seed(0)
    medians = {}
    for kind, k, fn in (("combined", 3, combined_loss), ("bce_dice", 2, bce_dice_loss), ("bce_dice", 1, bce_dice_loss)):
        x = (torch.randn(B, k, S, S, generator=g) * 2).to(DEV).requires_grad_(True)
        t = sem.clamp(max=k - 1) if k > 1 else sem

        def call(pw, x=x, t=t, fn=fn):
            x.grad = None
            fn(x, t, track_targets=False, pixel_weight=pw).backward()

        us = alternate({"unweighted": lambda: call(None), "weighted": lambda: call(wm)}, a.reps, a.rounds)
        for name, v in us.items():
            medians[(kind, k, name)] = statistics.median(v)
            lines.append(f"{f'{kind} fwd+bwd [{B},{k},{S},{S}] {name}':44s} {med(v):>36s}")
        lines.append(f"{'':4s}weighted / unweighted (medians): "
                     f"{medians[(kind, k, 'weighted')] / medians[(kind, k, 'unweighted')]:.3f}")
    lines.append(f"# unweighted C-ABI entry points (fwd + bwd, ctypes, no autograd): this build against "
                 f"{'the --parent-lib build' if a.parent_lib else 'no --parent-lib given: not measured'}")
    if a.parent_lib:
        _lib.load()
        new, old = ctypes.CDLL(_lib.LIB_PATH), ctypes.CDLL(os.path.abspath(a.parent_lib))  # handles of their own
        for kind, k in (("combined", 3), ("bce", 2)):
            x = (torch.randn(B, k, S, S, generator=g) * 2).to(DEV)
            t = sem.clamp(max=k - 1)
            fns = {"parent": raw_entries(old, kind, x, t, k), "this build": raw_entries(new, kind, x, t, k),
                   "parent again": raw_entries(old, kind, x, t, k)}
            us = alternate(fns, a.reps, a.rounds)
            same = all(torch.equal(u, v) for u, v in zip(fns["parent"].result(), fns["this build"].result()))
            for name, v in us.items():
                lines.append(f"{f'{kind} K={k} {name}':44s} {med(v):>36s}")
            lines.append(f"{'':4s}loss and gradient of the two builds bit-identical: {same}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
