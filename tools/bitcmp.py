"""Bit-identity check between library builds: two bf16 Trainer steps of the bench model (default: the bench
size), then a SHA-256 over every parameter, gradient and BN running statistic, one line per build.

    python tools/bitcmp.py LIB [LIB ...] [--size 1024 --batch 4]
    python tools/bitcmp.py --losses LIB [LIB ...]

Each build runs in its own child process (EUNET_LIB); equal digests = bit-identical steps.

--losses: instead, every per-pixel loss entry point (combined, BCE + Dice, boundary; forward and backward, with and
without a pixel weight) at the tile and vector-path edges, one SHA-256 per case over loss, parts, sums and glogits.
The exit status is 1 when a case differs between the builds."""
import argparse
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "enhanced-unet_amd")]


def digest(a):
    import torch
    from eunet import synth
    from eunet.models import EnhancedUNet
    from eunet.train_eval import Trainer
    torch.manual_seed(0)
    model = EnhancedUNet(num_classes=2, in_channels=1, base_ch=64, dtype="bf16").cuda()
    tr = Trainer(model, "cuda", "enhanced_unet", total_epochs=50)
    tr.epoch_lr_step(0)
    for i in range(2):
        x, m = synth.batch(a.batch, a.size, a.size, start_index=3 + i, num_classes=2, in_channels=1)
        tr.step(x.cuda(), m.cuda(), sync_loss=False)
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for k, t in list(model.state_dict().items()) + [(k + ".grad", p.grad) for k, p in model.named_parameters()]:
        h.update(k.encode())
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


# (N, H, W): 1, 1023, 1024, 1025 and 3072 pixels (H W % 4 = 1, 3, 0, 1, 0), 257 tiles (the finalize's thread 0 reads
# two), the largest batch
LOSS_SHAPES = [(3, 1, 1), (3, 31, 33), (3, 32, 32), (3, 25, 41), (3, 64, 48), (1, 513, 512), (64, 5, 7)]
IGNORE = 255


def loss_digests():
    """[(case, sha256)] of every loss entry point over LOSS_SHAPES x K x {unweighted, weighted}, and one case with the
    logits 4 bytes off a 16-byte boundary (the scalar path at H W % 4 = 0)."""
    import torch
    from eunet import ops
    from eunet.losses import make_bce_dice_params, make_params

    def sha(*ts):
        h = hashlib.sha256()
        for t in ts:
            h.update(t.detach().contiguous().cpu().numpy().tobytes())
        return h.hexdigest()[:16]

    def run(name, sums_len, ws_bytes, n_parts, fwd, bwd, x, t, prm, pw):
        n, k, h, w = x.shape
        sums = torch.zeros(sums_len(n, k), device="cuda")
        loss, parts = torch.zeros((), device="cuda"), torch.zeros(n, n_parts, device="cuda")
        ws = torch.zeros(ws_bytes(n, k, h, w), dtype=torch.uint8, device="cuda")
        g = torch.full((1,), 0.75, device="cuda")
        gl = torch.zeros_like(x)
        lead = (x, t) if pw is None else (x, t, pw)
        fwd[pw is not None](*lead, prm, sums, loss, parts, ws)
        bwd[pw is not None](*lead, prm, sums, g, gl)
        return name, sha(loss, parts, sums, gl)

    out = []
    cases = [(s, False) for s in LOSS_SHAPES] + [((3, 32, 32), True)]
    for (n, h, w), off in cases:
        for k in (1, 2, 3):
            gen = torch.Generator().manual_seed(1000 * n + 10 * h + k)
            flat = torch.empty(n * k * h * w + 1, device="cuda")
            x = flat[1:] if off else flat[:-1]  # a 4-byte offset keeps the view contiguous
            x = x.view(n, k, h, w).copy_((4.0 * torch.randn(n, k, h, w, generator=gen)).cuda())
            t = torch.randint(0, max(k, 2) + (k == 1), (n, h, w), generator=gen)
            t[torch.rand(n, h, w, generator=gen) < 0.1] = IGNORE
            t = t.cuda()
            tl = t.clamp(max=k - 1).where(t != IGNORE, t) if k == 1 else t  # the combined loss takes [0, K)
            pwt = (0.25 + 3.0 * torch.rand(n, h, w, generator=gen)).cuda()
            d = (6.0 * torch.randn(n, k, h, w, generator=gen)).cuda()
            tag = f"n{n}_{h}x{w}_k{k}" + ("_off4" if off else "")
            lp = [None, make_params(ce_weight=[1.0, 2.5, 0.7], alpha=[0.9, 1.3, 2.1], gamma=3.0, ignore_index=IGNORE,
                                    dice_weight=[1.0, 3.0, 2.0], tversky_weight=[0.5, 4.0, 1.5], tversky_alpha=0.6,
                                    w_focal=1.7, w_dice=0.8, w_tversky=1.1, class_div=float(k)),
                  make_params(gamma=2.5, ignore_index=IGNORE)]
            bp = [make_bce_dice_params(ignore_index=IGNORE),
                  make_bce_dice_params(pos_weight=[2.0, 0.5, 1.5], class_weight=[1.0, 2.5, 0.7],
                                       dice_weight=[1.0, 3.0, 2.0], w_bce=0.7, w_dice=1.3, smooth=1e-3,
                                       ignore_index=IGNORE)]
            for pw in (None, pwt):
                wt = "_w" if pw is not None else ""
                for i, p in enumerate(lp):
                    out.append(run(f"loss{wt}_p{i}_{tag}", ops.loss_sums_len, ops.loss_workspace_bytes, 3,
                                   (ops.loss_fwd, ops.loss_fwd_w), (ops.loss_bwd, ops.loss_bwd_w), x, tl, p, pw))
                for i, p in enumerate(bp):
                    out.append(run(f"bce_dice{wt}_p{i}_{tag}", ops.bce_dice_sums_len, ops.bce_dice_workspace_bytes, 2,
                                   (ops.bce_dice_fwd, ops.bce_dice_fwd_w), (ops.bce_dice_bwd, ops.bce_dice_bwd_w),
                                   x, t, p, pw))
            for act in ("softmax", "sigmoid"):
                if act == "softmax" and k == 1:
                    continue
                for cw in ((1.0, 1.0, 1.0), (0.0, 1.5, 0.5)):
                    a = ops.BOUNDARY_ACTIVATIONS[act]
                    loss, parts = torch.zeros((), device="cuda"), torch.zeros(n, device="cuda")
                    ws = torch.zeros(ops.boundary_loss_workspace_bytes(n, h, w), dtype=torch.uint8, device="cuda")
                    gl = torch.zeros_like(x)
                    ops.boundary_loss_fwd(x, d, a, *cw, loss, parts, ws)
                    ops.boundary_loss_bwd(x, d, a, *cw, torch.full((1,), 0.75, device="cuda"), gl)
                    out.append((f"boundary_{act}_cw{cw[0]:g}_{tag}", sha(loss, parts, ws, gl)))
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--losses", action="store_true")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        if a.losses:
            for name, dg in loss_digests():
                print(f"case {name} {dg}", flush=True)
        else:
            print(digest(a), flush=True)
        return
    per_lib = []
    for lib in a.libs:
        r = subprocess.run([sys.executable, __file__, "--child", "--size", str(a.size), "--batch", str(a.batch)] +
                           (["--losses"] if a.losses else []),
                           env=dict(os.environ, EUNET_LIB=lib), capture_output=True, text=True, timeout=300)
        if r.returncode:
            sys.stderr.write(r.stderr[-3000:])
            raise SystemExit(f"{lib}: rc {r.returncode}")
        if not a.losses:
            print(f"bitcmp {lib} {r.stdout.strip().splitlines()[-1]}", flush=True)
            continue
        cases = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("case ")]
        per_lib.append(dict(cases))
        print(f"bitcmp --losses {lib} {len(cases)} cases, all: "
              f"{hashlib.sha256(' '.join(d for _, d in cases).encode()).hexdigest()}", flush=True)
    if a.losses and len(per_lib) > 1:
        bad = [k for k in per_lib[0] if any(p.get(k) != per_lib[0][k] for p in per_lib[1:])]
        for k in bad:
            print(f"DIFFERS {k} " + " ".join(p.get(k, "-") for p in per_lib), flush=True)
        families = sorted({k.split("_n")[0] for k in per_lib[0]})
        for f in families:
            ks = [k for k in per_lib[0] if k.split("_n")[0] == f]
            print(f"  {f}: {len(ks)} cases, {sum(k in bad for k in ks)} differ")
        print("bitcmp --losses: " + ("EQUAL" if not bad else f"{len(bad)} of {len(per_lib[0])} cases differ"))
        raise SystemExit(1 if bad else 0)


if __name__ == "__main__":
    main()
