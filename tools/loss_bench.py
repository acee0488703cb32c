"""Time StandardDiffusionLoss.get_loss, forward + backward, under the torch and the hip loss engine in one process.

    python tools/loss_bench.py [--rounds 15] [--iters 20] [--step 2500]

Two shapes: cfg4's 28 frames of 4 x 32 x 48 latents without class weights, and the same with the ParallelDomain class
weights (person x7, vehicle x3) on 28 x 3 x 256 x 384 semantic-map frames.  A window is `iters` calls of get_loss(...).mean()
+ backward() between two device synchronisations, timed with the host clock; the engines alternate window by window, and
the table gives the median, the fastest and the slowest window per call.  Needs an MI355X: there is no CPU path."""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from gcd_amd import training as TR      # noqa: E402

BT, C, H, W = 28, 4, 32, 48
FRAME_HW = (256, 384)


def semantic_frames(n, hw, gen, dev):
    """A random background with rectangles in exact class colours: what batch['jpg'] of the ParallelDomain set looks like."""
    img = torch.rand(n, 3, *hw, generator=gen) * 2.0 - 1.0
    palette = list(TR.PD_PERSON_RGB.values()) + list(TR.PD_VEHICLE_RGB.values())
    for b in range(n):
        for k in range(12):
            rgb = palette[(b + k) % len(palette)]
            y0, x0 = int(torch.randint(0, hw[0] - 64, (1,), generator=gen)), int(torch.randint(0, hw[1] - 96, (1,), generator=gen))
            hh, ww = int(torch.randint(8, 64, (1,), generator=gen)), int(torch.randint(8, 96, (1,), generator=gen))
            img[b, :, y0:y0 + hh, x0:x0 + ww] = (torch.tensor(rgb, dtype=torch.float32) / 127.5 - 1.0)[:, None, None]
    return img.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step", type=int, default=2500, help="global_step: 2500 is the middle of the annealing (keep 55 %%)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/loss_bench.py needs an MI355X; there is no CPU path for the product")
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(0)
    out = torch.randn(BT, C, H, W, generator=gen).to(dev).requires_grad_(True)
    tgt = torch.randn(BT, C, H, W, generator=gen).to(dev)
    w = (torch.rand(BT, generator=gen) + 0.5).to(dev)[:, None, None, None]
    cfg = dict(sigma_sampler_config={"target": "gcd_amd.training.EDMSampling", "params": {}},
               loss_weighting_config={"target": "gcd_amd.training.EDMWeighting", "params": {}}, focus_top=0.1, focus_steps=5000)
    shapes = [("28x4x32x48, no class weights", TR.StandardDiffusionLoss(**cfg), {"global_step": args.step}),
              ("28x4x32x48, person x7 vehicle x3 on 28x3x256x384", TR.StandardDiffusionLoss(**cfg, pd_person_weight=7.0, pd_vehicle_weight=3.0),
               {"global_step": args.step, "jpg": semantic_frames(BT, FRAME_HW, gen, dev)})]
    old = TR.LOSS_ENGINE

    def window(loss_fn, batch, engine, iters):
        TR.set_loss_engine(engine)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(iters):
            out.grad = None
            loss_fn.get_loss(out, tgt, w, batch).mean().backward()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / iters

    rows = []
    try:
        for name, loss_fn, batch in shapes:
            values, grads = {}, {}
            for engine in ("torch", "hip"):                       # warm-up of every shape, and the values to compare
                window(loss_fn, batch, engine, 3)
                values[engine], grads[engine] = float(loss_fn.get_loss(out, tgt, w, batch).mean().detach()), out.grad.clone()
            times = {"torch": [], "hip": []}
            for _ in range(args.rounds):
                for engine in ("torch", "hip"):
                    times[engine].append(window(loss_fn, batch, engine, args.iters))
            rel = float((grads["hip"] - grads["torch"]).double().norm() / grads["torch"].double().norm())
            for engine in ("torch", "hip"):
                t = sorted(times[engine])
                rows.append((name, engine, t[len(t) // 2] * 1e6, t[0] * 1e6, t[-1] * 1e6, values[engine], rel))
    finally:
        TR.set_loss_engine(old)
    print(f"get_loss(...).mean() + backward(), global_step {args.step}; per call, {args.rounds} windows of {args.iters} calls, "
          f"engines alternating; {torch.cuda.get_device_name(dev)}")
    print(f"{'shape':<52} {'engine':<6} {'median us':>10} {'min us':>9} {'max us':>9} {'loss':>13} {'grad rel-L2 hip vs torch':>25}")
    for name, engine, med, lo, hi, value, rel in rows:
        print(f"{name:<52} {engine:<6} {med:>10.1f} {lo:>9.1f} {hi:>9.1f} {value:>13.8f} {rel:>25.2e}")
    for i in range(0, len(rows), 2):
        print(f"{rows[i][0]}: torch / hip = {rows[i][2] / rows[i + 1][2]:.2f}x")


if __name__ == "__main__":
    main()
