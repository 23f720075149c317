"""Train-step rate of enhanced_unet and the unet baseline.

    python tools/baseline_bench.py [--size 1024] [--batch 4] [--steps 10] [--out profiles/baselines_bench.txt]

One process, profiler off, device events, 3 warm-up steps per model.  Train step = Trainer.step (forward, loss,
backward, clip + AdamW) at base 64, 3 input channels, 3 classes, bf16, deferred loss.  The models alternate
over three rounds; reported: median [min, max] of the rounds' ms/step and img/s.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "enhanced-unet_amd")]
import torch  # noqa: E402
from eunet import synth  # noqa: E402
from eunet.models import get_model  # noqa: E402
from eunet.train_eval import Trainer  # noqa: E402

DEV = "cuda"
NAMES = ("enhanced_unet", "unet")


def timed(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def med(v):
    return f"{statistics.median(v):8.2f} [{min(v):.2f}, {max(v):.2f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "baselines_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("baseline_bench: needs the GPU (nothing is measured without one)")
    lines = [f"# tools/baseline_bench.py: base 64, c3, K3, {a.size}^2, B {a.batch}, bf16; {a.steps} steps per round, "
             f"{a.rounds} alternating rounds, 3 warm-up steps; {torch.cuda.get_device_name(0)}"]
    torch.manual_seed(0)
    x, m = synth.batch(a.batch, a.size, a.size, start_index=100, num_classes=3, in_channels=3, device=DEV)
    trainers = {}
    for name in NAMES:
        model = get_model(name, num_classes=3, in_channels=3, base_ch=64, dtype="bf16").to(DEV)
        trainers[name] = Trainer(model, DEV, name, total_epochs=50)
        for _ in range(3):
            trainers[name].step(x, m, sync_loss=False)
    ms = {n: [] for n in NAMES}
    for _ in range(a.rounds):
        for name in NAMES:
            ms[name].append(timed(lambda: trainers[name].step(x, m, sync_loss=False), a.steps))
    lines.append(f"{'model':14s} {'ms/step median [min, max]':>32s} {'img/s median [min, max]':>34s}")
    for name in NAMES:
        lines.append(f"{name:14s} {med(ms[name]):>32s} {med([1e3 * a.batch / t for t in ms[name]]):>34s}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
