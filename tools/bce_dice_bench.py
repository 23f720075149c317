"""Forward + backward time of the sigmoid BCE + Dice loss (csrc/bce_dice.hip) beside the combined softmax loss
(csrc/loss.hip) on the same logits, and where the new kernels stand against their byte counts.

    python tools/bce_dice_bench.py [--size 1024] [--batch 4] [--reps 2000] [--out profiles/bce_dice_bench.txt]

One process, device events.  A call = loss(logits, target) + loss.backward() on resident tensors: the forward
partial kernel, the finalize and the per-pixel backward (plus autograd's host work, the same for both).  At
[B,2,S,S] bce_dice_loss and combined_loss alternate over the rounds after 20 warm-up calls each; at [B,1,S,S] the
BCE loss runs alone (a softmax over one logit has no gradient).  Reported: median [min, max] of the rounds'
us/call.  The algorithmic bytes of a call are logits and target read twice (forward, backward) and the gradient
written once: (2 * (4K + 8) + 4K) bytes per pixel; TB/s = those bytes over the call time, a lower bound on the
kernels' own rate (the call time holds the launch gaps and, where the kernels are shorter than autograd's host work
per call, that host work).  Then an extra pass per loss under eunet.kprof.BusyTimer: events around each C-ABI call,
i.e. the device time of the forward entry (partial kernel + finalize) and of the backward entry, against their own
bytes (forward 4K + 8 per pixel, backward 8K + 8).  Recorded, not gated.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "enhanced-unet_amd")]
import torch  # noqa: E402
from eunet import kprof  # noqa: E402
from eunet.losses import bce_dice_loss, combined_loss  # noqa: E402

DEV = "cuda"
WARMUP = 20


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
    return f"{statistics.median(v):9.1f} [{min(v):.1f}, {max(v):.1f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bce_dice_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bce_dice_bench: needs the GPU (nothing is measured without one)")
    g = torch.Generator().manual_seed(0)
    px = a.batch * a.size * a.size
    lines = [f"# tools/bce_dice_bench.py: loss forward + backward, B {a.batch}, {a.size}^2, fp32 logits, int64 target; "
             f"{a.reps} calls per round, {a.rounds} alternating rounds, {WARMUP} warm-up calls; "
             f"{torch.cuda.get_device_name(0)}",
             f"{'loss':28s} {'us/call median [min, max]':>34s} {'MB/call':>9s} {'TB/s':>7s}"]
    medians, entries = {}, []
    for k in (2, 1):
        x = (torch.randn(a.batch, k, a.size, a.size, generator=g) * 2).to(DEV).requires_grad_(True)
        t = torch.randint(0, 2, (a.batch, a.size, a.size), generator=g).to(DEV)

        def call(loss_fn):
            x.grad = None
            loss_fn(x, t, track_targets=False).backward()

        fns = {"bce_dice": lambda: call(bce_dice_loss)}
        if k == 2:
            fns["combined"] = lambda: call(combined_loss)
        for fn in fns.values():
            for _ in range(WARMUP):
                fn()
        us = {name: [] for name in fns}
        for _ in range(a.rounds):
            for name, fn in fns.items():
                us[name].append(timed(fn, a.reps))
        mb = px * (2 * (4 * k + 8) + 4 * k) / 1e6
        for name in fns:
            m = statistics.median(us[name])
            medians[(name, k)] = m
            lines.append(f"{name + f' [{a.batch},{k},{a.size},{a.size}]':28s} {med(us[name]):>34s} {mb:9.1f} "
                         f"{mb / m:7.3f}")
        for name, fn in fns.items():  # device time per entry point: the calls alternate forward, backward
            with kprof.BusyTimer() as bt:
                for _ in range(50):
                    fn()
            torch.cuda.synchronize()
            spans = [1e3 * e0.elapsed_time(e1) for e0, e1 in bt.iv]
            for part, sel, b in (("fwd", spans[0::2], 4 * k + 8), ("bwd", spans[1::2], 8 * k + 8)):
                entries.append(f"{name + ' ' + part + f' K={k}':28s} {med(sel):>34s} {px * b / 1e6:9.1f} "
                               f"{px * b / 1e6 / statistics.median(sel):7.3f}")
    lines.append(f"bce_dice / combined call time at K = 2 (medians): "
                 f"{medians[('bce_dice', 2)] / medians[('combined', 2)]:.3f}")
    lines.append(f"{'entry point (device events)':28s} {'us median [min, max] of 50':>34s} {'MB':>9s} {'TB/s':>7s}")
    lines += entries
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
