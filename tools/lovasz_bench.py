"""Device time of the Lovasz loss (csrc/lovasz.hip) next to two yardsticks in the same process: the torch-only route
on the same tensors and the combined loss.

    timeout -k 10 600 python tools/lovasz_bench.py [--size 1024] [--batch 4] [--reps 20] [--rounds 5]
                                                   [--out profiles/lovasz_bench.txt]

One process, device events, the routes alternating over the rounds after warm-up calls of each; run it under a
`timeout` of its own.  The target is the [S, S] eunet.synth mask (3 classes) repeated over the batch, K = 3, softmax,
per_image off (3 segments of B S^2 elements).  Two logit sets:
  * saturated: (randn + 3 onehot(target)) * 5, a trained net's -- most errors are below 1e-4, so most keys share
    their high digits
  * randn: torch.randn, every digit of every pass populated
Per set, median [min, max] of the rounds' us/call of
  * lovasz_loss fwd + bwd: loss = lovasz_loss(x, t); loss.backward() on resident tensors (the workspace, weights and
    gradient are allocated per call, as in training)
  * ops.lovasz_errors and ops.lovasz_sort on their own (the sort op on the errors op's output, one segment per plane:
    the keys kernel, the four passes, the scan and the gradient)
  * torch-only fwd + bwd: softmax, abs, torch.sort(descending=True), cumsum, gather (indexing by the permutation),
    dot, autograd -- Berman's lovasz_softmax_flat without its host-side `present` test
  * combined_loss fwd + bwd (focal + Dice + Tversky, csrc/loss.hip)
and, from torch.profiler's kernel records of five further native calls, the device time per kernel group: errors, each
of the four sort passes (histogram + row scan + scatter), scan + gradient, finalize, backward.  Where the profiler
returns no kernel records the groups are reported as not measured.  Recorded, not gated.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "enhanced-unet_amd")]
import torch  # noqa: E402
from eunet import ops, synth  # noqa: E402
from eunet.losses import combined_loss, lovasz_loss  # noqa: E402

DEV = "cuda"
WARMUP = 3
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


def row(name, v):
    return f"{name:44s} {statistics.median(v):10.1f} [{min(v):.1f}, {max(v):.1f}] us"


def torch_lovasz(x, t):
    """Berman's lovasz_softmax (classes over the batch), every class taken as present."""
    p = x.softmax(1)
    losses = []
    for c in range(K):
        fg = (t == c).float().reshape(-1)
        err = (fg - p[:, c].reshape(-1)).abs()
        es, perm = torch.sort(err, 0, descending=True)
        fgs = fg[perm]
        gts = fgs.sum()
        jac = 1.0 - (gts - fgs.cumsum(0)) / (gts + (1.0 - fgs).cumsum(0))
        jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
        losses.append(torch.dot(es, jac))
    return torch.stack(losses).mean()


def kernel_groups(fn, calls=5):
    """us per call of each kernel group of fn (a native forward + backward), from torch.profiler's kernel records in
    launch order; None if it returns none."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    ev = sorted((e for e in prof.events() if "kernel" in e.name.lower() or e.name.startswith("_ZN")),
                key=lambda e: e.time_range.start)
    names = [e.name for e in ev]
    if not any("lz_scatter_kernel" in n for n in names):
        return None
    groups = {}
    passes = fg_scan = 0
    for e in ev:
        n, us = e.name, e.time_range.end - e.time_range.start
        if "lz_errors_kernel" in n:
            g, passes, fg_scan = "errors", 0, 0
        elif "lz_hist_kernel" in n:
            passes += 1
            g = f"sort pass {passes} (bits {8 * passes - 8}..{8 * passes - 1})"
        elif "lz_scatter_kernel" in n:
            g = f"sort pass {passes} (bits {8 * passes - 8}..{8 * passes - 1})"
        elif "scan_block_counts_kernel" in n:
            g = f"sort pass {passes} (bits {8 * passes - 8}..{8 * passes - 1})" if not fg_scan else "scan + gradient"
        elif "lz_fgcount_kernel" in n:
            g, fg_scan = "scan + gradient", 1
        elif "lz_grad_kernel" in n:
            g = "scan + gradient"
        elif "lz_finalize_kernel" in n:
            g = "finalize"
        elif "lz_bwd_kernel" in n:
            g = "backward"
        else:
            continue
        groups[g] = groups.get(g, 0.0) + us / calls
    return groups


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lovasz_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lovasz_bench: needs the GPU (nothing is measured without one)")
    S, B = a.size, a.batch
    _, sem = synth.tile(S, S, 0, num_classes=3)[:2]
    target = torch.from_numpy(sem).to(DEV)[None].repeat(B, 1, 1).contiguous()
    g = torch.Generator().manual_seed(0)
    noise = torch.randn(B, K, S, S, generator=g).to(DEV)
    onehot = (target[:, None] == torch.arange(K, device=DEV).view(1, K, 1, 1)).float()
    sets = {"saturated": ((noise + 3.0 * onehot) * 5.0).contiguous(), "randn": noise}
    segs, seglen = ops.lovasz_segments(B, K, S, S, False)
    ws_bytes = ops.lovasz_workspace_bytes(segs, seglen)
    lines = [f"# tools/lovasz_bench.py: B {B}, {S}^2 eunet.synth mask, K = {K}, fp32 logits, softmax, per_image off "
             f"({segs} segments of {seglen} elements); {a.reps} calls per round, {a.rounds} alternating rounds, {WARMUP} "
             f"warm-up calls; {torch.cuda.get_device_name(0)}",
             f"# workspace of one forward call: {ws_bytes} bytes ({ws_bytes / 2 ** 20:.1f} MiB), "
             f"{ws_bytes / (segs * seglen):.2f} bytes per element; saved for the backward: weights "
             f"{4 * segs * seglen} bytes"]
    for label, logits in sets.items():
        x = logits.clone().requires_grad_(True)

        def call(fn):
            x.grad = None
            fn(x, target).backward()

        e, f = ops.lovasz_errors(logits, target, "softmax")
        small = float((e < 1e-4).float().mean())
        es, fs = e.reshape(B * K, S * S), f.reshape(B * K, S * S)
        fns = {
            "lovasz_loss fwd + bwd": lambda: call(lambda z, t: lovasz_loss(z, t, track_targets=False)),
            "ops.lovasz_errors": lambda: ops.lovasz_errors(logits, target, "softmax"),
            f"ops.lovasz_sort [{B * K}, {S * S}]": lambda: ops.lovasz_sort(es, fs),
            "torch-only fwd + bwd": lambda: call(torch_lovasz),
            "combined_loss fwd + bwd": lambda: call(lambda z, t: combined_loss(z, t, track_targets=False)),
        }
        for fn in fns.values():
            for _ in range(WARMUP):
                fn()
        us = {name: [] for name in fns}
        for _ in range(a.rounds):
            for name, fn in fns.items():
                us[name].append(timed(fn, a.reps))
        med = {k: statistics.median(v) for k, v in us.items()}
        native = lovasz_loss(x, target).item()
        ref = torch_lovasz(x.detach(), target).item()
        lines.append(f"## {label} logits: {100 * small:.1f} % of the errors below 1e-4; loss {native:.6f}, torch-only "
                     f"route {ref:.6f}")
        lines.append(f"{'call':44s} {'median [min, max]':>29s}")
        lines += [row(k, v) for k, v in us.items()]
        lines.append(f"# torch-only / native: {med['torch-only fwd + bwd'] / med['lovasz_loss fwd + bwd']:.2f}; native / "
                     f"combined_loss: {med['lovasz_loss fwd + bwd'] / med['combined_loss fwd + bwd']:.2f}")
        try:
            groups = kernel_groups(fns["lovasz_loss fwd + bwd"])
        except Exception as exc:  # the profiler is optional: the rows above stand without it
            groups = None
            lines.append(f"# torch.profiler failed: {type(exc).__name__}: {exc}")
        if groups is None:
            lines.append("# kernel groups: not measured (torch.profiler returned no kernel records)")
        else:
            lines.append(f"{'kernel group (torch.profiler, 5 calls)':44s} {'us per call':>12s}")
            lines += [f"{k:44s} {v:12.1f}" for k, v in groups.items()]
            lines.append(f"{'sum of the groups':44s} {sum(groups.values()):12.1f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
