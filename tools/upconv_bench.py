"""Train-step rate of enhanced_unet with the bilinear and with the learned (transposed-convolution) decoder
upsample, and where the upconv2x2 kernels stand against their byte and FLOP counts.

    python tools/upconv_bench.py [--size 1024] [--batch 4] [--steps 10] [--out profiles/upconv_bench.txt]

One process, device events, 3 warm-up steps per model.  Train step = Trainer.step (forward, loss, backward,
clip + AdamW) at base 64, 3 input channels, 3 classes, bf16, deferred loss.  The two models alternate over three
rounds; reported: median [min, max] of the rounds' ms/step and img/s.  The yardstick of the transpose model is the
bilinear step in the same process.  Then one extra, untimed-for-the-rate pass of the transpose model under
eunet.kprof: per launch of the upconv2x2 family (pack, forward, data gradient, weight gradient of the three
layers) the time, the achieved TB/s against the algorithmic bytes and the fraction of the bf16 dense MFMA peak
against the algorithmic FLOPs (the counts of eunet/ops.py).  Recorded, not gated.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "enhanced-unet_amd")]
import torch  # noqa: E402
from eunet import kprof, synth  # noqa: E402
from eunet.models import get_model  # noqa: E402
from eunet.train_eval import Trainer  # noqa: E402

DEV = "cuda"
VARIANTS = ("bilinear", "transpose")
PEAK_TFLOPS_BF16 = 2500.0  # dense MFMA peak, as bench.py's PEAK_TFLOPS


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upconv_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("upconv_bench: needs the GPU (nothing is measured without one)")
    lines = [f"# tools/upconv_bench.py: enhanced_unet base 64, c3, K3, {a.size}^2, B {a.batch}, bf16; {a.steps} steps per "
             f"round, {a.rounds} alternating rounds, 3 warm-up steps; {torch.cuda.get_device_name(0)}"]
    torch.manual_seed(0)
    x, m = synth.batch(a.batch, a.size, a.size, start_index=100, num_classes=3, in_channels=3, device=DEV)
    trainers = {}
    for v in VARIANTS:
        model = get_model("enhanced_unet", num_classes=3, in_channels=3, base_ch=64, dtype="bf16", upsample=v).to(DEV)
        trainers[v] = Trainer(model, DEV, "enhanced_unet", total_epochs=50)
        for _ in range(3):
            trainers[v].step(x, m, sync_loss=False)
    ms = {v: [] for v in VARIANTS}
    for _ in range(a.rounds):
        for v in VARIANTS:
            ms[v].append(timed(lambda: trainers[v].step(x, m, sync_loss=False), a.steps))
    lines.append(f"{'upsample':14s} {'ms/step median [min, max]':>32s} {'img/s median [min, max]':>34s}")
    for v in VARIANTS:
        lines.append(f"{v:14s} {med(ms[v]):>32s} {med([1e3 * a.batch / t for t in ms[v]]):>34s}")
    lines.append(f"transpose / bilinear step time (medians): {statistics.median(ms['transpose']) / statistics.median(ms['bilinear']):.3f}")
    # the upconv2x2 family under kprof (events around every launch; the weight gradients run on the side stream,
    # so their spans overlap the launch stream's kernels)
    with kprof.KernelTimer() as kt:
        for _ in range(a.steps):
            trainers["transpose"].step(x, m, sync_loss=False)
        torch.cuda.synchronize()
    fam = kt.summary().get("upconv2x2")
    if fam:
        per = fam["ms"] / fam["launches"]
        lines.append(f"upconv2x2 family over {a.steps} steps: {fam['launches']} launches, {fam['ms'] / a.steps:.3f} ms/step summed "
                     f"spans, {1e3 * per:.1f} us/launch, {fam['bytes'] / (fam['ms'] * 1e-3) / 1e12:.3f} TB/s algorithmic, "
                     f"{fam['flops'] / (fam['ms'] * 1e-3) / 1e12:.1f} TFLOP/s = "
                     f"{fam['flops'] / (fam['ms'] * 1e-3) / 1e12 / PEAK_TFLOPS_BF16:.4f} of the bf16 peak")
        recs = kt.records["upconv2x2"]
        n = len(recs) // a.steps  # launches per step, in issue order: 3 packs, 3 forwards, then per layer dgrad + wgrad
        lines.append(f"{'launch (issue order in a step)':32s} {'us median':>10s} {'GB':>8s} {'GFLOP':>8s} {'TB/s':>7s} {'of peak':>8s}")
        for i in range(n):
            ts = [recs[s * n + i][0].elapsed_time(recs[s * n + i][1]) for s in range(a.steps)]
            t, fl, by = statistics.median(ts), recs[i][2], recs[i][3]
            lines.append(f"{i:3d} {'':28s} {1e3 * t:10.1f} {by / 1e9:8.3f} {fl / 1e9:8.1f} {by / (t * 1e-3) / 1e12:7.3f} "
                         f"{fl / (t * 1e-3) / 1e12 / PEAK_TFLOPS_BF16:8.4f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
