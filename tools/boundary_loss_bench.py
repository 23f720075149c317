"""Device time of the signed distance map and the boundary loss (csrc/sdf.hip) next to the tree's nearest stream,
the sigmoid BCE + Dice loss, and the distance transform the map is built on.

    python tools/boundary_loss_bench.py [--size 1024] [--batch 4] [--reps 200] [--rounds 5]
                                        [--out profiles/boundary_loss_bench.txt]

One process, device events, the routes alternating over the rounds after warm-up calls of each.  Reported per line:
median [min, max] of the rounds' us/call, the bytes the call has to move (computed from the shapes, below) and bytes /
median time.  The target is the [S, S] eunet.synth mask (3 classes) repeated over the batch; logits are randn * 2.
  * signed_distance_map, K = 3, into a resident buffer (the workspace is allocated per call): two transforms of
    3 x (8 + 4 x 4) bytes per pixel each (distance_transform_sq's count) and the combine kernel: the target (8), two
    int32 planes per class in and one fp32 plane out, 8 + 3 x 12 bytes per pixel.
  * distance_transform_sq "eq" and "ne" of the same planes into resident buffers: the two transforms on their own.
    The combine kernel's time is reported as the whole call minus the two (it has no entry point of its own; the
    difference also holds the workspace allocation).
  * boundary_loss (softmax, K = 3) and bce_dice_loss (K = 3) as a call = loss(...) + loss.backward() on resident
    tensors.  Bytes: boundary forward 8K per pixel (logits and map), backward 12K (both again, the gradient out);
    bce_dice forward 4K + 8, backward 8K + 8.
  * the same four entry points under eunet.kprof.BusyTimer in an extra pass: events around each C-ABI call, i.e. the
    device time of the forward entry (partial kernel + finalize) and of the backward entry.
Recorded, not gated.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "enhanced-unet_amd")]
import torch  # noqa: E402
from eunet import kprof, ops, synth  # noqa: E402
from eunet.losses import bce_dice_loss, boundary_loss  # noqa: E402

DEV = "cuda"
WARMUP = 10
K = 3


def timed(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps  # us per call


def row(name, v, nbytes):
    m = statistics.median(v)
    return f"{name:44s} {m:10.1f} [{min(v):.1f}, {max(v):.1f}] us  {nbytes / 1e6:9.2f} MB  {nbytes / m / 1e6:6.3f} TB/s"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boundary_loss_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("boundary_loss_bench: needs the GPU (nothing is measured without one)")
    S, B = a.size, a.batch
    px = B * S * S
    _, sem = synth.tile(S, S, 0, num_classes=3)[:2]
    target = torch.from_numpy(sem).to(DEV)[None].repeat(B, 1, 1).contiguous()
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(B, K, S, S, generator=g) * 2).to(DEV).requires_grad_(True)
    phi = torch.empty(B, K, S, S, device=DEV)
    d_eq = torch.empty(B, K, S, S, dtype=torch.int32, device=DEV)
    d_ne = torch.empty(B, K, S, S, dtype=torch.int32, device=DEV)
    ops.signed_distance_map(target, K, out=phi)

    def loss_call(fn, second):
        x.grad = None
        fn(x, second).backward()

    edt_b = K * 24 * px
    sdf_b = 2 * edt_b + (8 + K * 12) * px
    fns = {
        "signed_distance_map K=3": (lambda: ops.signed_distance_map(target, K, out=phi), sdf_b),
        "distance_transform_sq eq, 3 classes": (lambda: ops.distance_transform_sq(target, [0, 1, 2], "eq", out=d_eq), edt_b),
        "distance_transform_sq ne, 3 classes": (lambda: ops.distance_transform_sq(target, [0, 1, 2], "ne", out=d_ne), edt_b),
        "boundary_loss fwd + bwd (softmax, K=3)": (lambda: loss_call(boundary_loss, phi), 20 * K * px),
        "bce_dice_loss fwd + bwd (K=3)": (lambda: loss_call(lambda z, t: bce_dice_loss(z, t, track_targets=False), target),
                                          (12 * K + 16) * px),
    }
    for fn, _ in fns.values():
        for _ in range(WARMUP):
            fn()
    us = {name: [] for name in fns}
    for _ in range(a.rounds):
        for name, (fn, _) in fns.items():
            us[name].append(timed(fn, a.reps))
    med = {k: statistics.median(v) for k, v in us.items()}
    lines = [f"# tools/boundary_loss_bench.py: B {B}, {S}^2 eunet.synth mask, K = {K}, fp32 logits; {a.reps} calls per "
             f"round, {a.rounds} alternating rounds, {WARMUP} warm-up calls; {torch.cuda.get_device_name(0)}",
             f"{'call':44s} {'median [min, max]':>29s} {'bytes':>13s} {'bytes / median':>12s}"]
    lines += [row(k, us[k], v[1]) for k, v in fns.items()]
    t_comb = med["signed_distance_map K=3"] - med["distance_transform_sq eq, 3 classes"] - \
        med["distance_transform_sq ne, 3 classes"]
    comb_b = (8 + K * 12) * px
    lines.append(f"signed_distance_map - eq - ne (the combine kernel and the workspace allocation): {t_comb:.1f} us for "
                 f"{comb_b / 1e6:.2f} MB, {comb_b / t_comb / 1e6 if t_comb > 0 else float('nan'):.3f} TB/s")
    lines.append(f"{'entry point (device events)':44s} {'median [min, max] of 50':>29s} {'bytes':>13s} {'bytes / median':>12s}")
    rates = {}
    for name, fn, bf, bb in (("boundary_loss", fns["boundary_loss fwd + bwd (softmax, K=3)"][0], 8 * K, 12 * K),
                             ("bce_dice_loss", fns["bce_dice_loss fwd + bwd (K=3)"][0], 4 * K + 8, 8 * K + 8)):
        with kprof.BusyTimer() as bt:
            for _ in range(50):
                fn()
        torch.cuda.synchronize()
        spans = [1e3 * e0.elapsed_time(e1) for e0, e1 in bt.iv]
        for part, sel, b in (("fwd", spans[0::2], bf), ("bwd", spans[1::2], bb)):
            lines.append(row(f"{name} {part}", sel, b * px))
            rates[(name, part)] = b * px / statistics.median(sel)
    lines.append("# boundary_loss / bce_dice_loss, bytes per second: "
                 f"fwd {rates[('boundary_loss', 'fwd')] / rates[('bce_dice_loss', 'fwd')]:.2f}, "
                 f"bwd {rates[('boundary_loss', 'bwd')] / rates[('bce_dice_loss', 'bwd')]:.2f}; whole call "
                 f"{(20 * K / med['boundary_loss fwd + bwd (softmax, K=3)']) / ((12 * K + 16) / med['bce_dice_loss fwd + bwd (K=3)']):.2f}")
    # what the timed calls computed: the resident map equals a fresh one, and its transforms are the timed ones
    fresh = ops.signed_distance_map(target, K)
    ok = torch.equal(fresh, phi)
    out_r = torch.where(target[:, None] == torch.arange(K, device=DEV).view(1, K, 1, 1), 1.0 - d_ne.double().sqrt(),
                        d_eq.double().sqrt()).float()
    lines.append(f"# the resident map equals a fresh call: {ok}; equals sqrt of the timed transforms: "
                 f"{torch.equal(out_r, phi)}; range [{float(phi.min()):.2f}, {float(phi.max()):.2f}]")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
