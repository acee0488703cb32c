"""Time the optimizer step on the full-width VideoUNet's parameter shapes (no forward pass): the default path
(`gcd_adam_step_multi` through `AdamHIP.step()`) against the device-resident step of include/gcd_amd_train_optim.h with its
options switched on one at a time.

    python tools/optim_bench.py [--repeats 25] [--warmup 3] [--out profiles/r10_optim_step.txt]

One process, device events around each `step()`, the variants ALTERNATED inside every repeat, the median over >= 20
repeats.  Per variant: time, the bytes the shapes imply (28 B per parameter for the update, 36 B with an EMA shadow, 4 B for
the reduction), the resulting TB/s, and the number of kernel launches.
Gate 1: the median of (b) — the new path with every option off — is no slower than the SLOWEST of (a)'s own repeats in the
same run.  Exit status 1 when it fails."""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r10_optim_step.txt"))
    args = ap.parse_args()
    assert args.repeats >= 20, "the median is taken over at least 20 repeats"
    from gcd_amd import _lib
    from gcd_amd.ema import LitEma
    from gcd_amd.training import AdamHIP
    from gcd_amd.video_model import VideoUNet
    from oracle import svd_unet_ref as O
    _lib.load()
    dev = torch.device("cuda:0")
    with torch.device("meta"):
        net = VideoUNet(**O.KUBRIC.as_reference_kwargs())
    shapes = [tuple(p.shape) for p in net.parameters() if p.requires_grad]

    class Bag(torch.nn.Module):
        def __init__(self):
            super().__init__()
            g = torch.Generator(device=dev).manual_seed(0)
            self.ps = torch.nn.ParameterList(
                [torch.nn.Parameter(torch.randn(s, device=dev, generator=g) * 0.02) for s in shapes])

    bag = Bag()
    params = list(bag.parameters())
    g = torch.Generator(device=dev).manual_seed(1)
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=g) * 1e-3
    n_par = sum(p.numel() for p in params)
    n_multi = 0          # launches of gcd_adam_step_multi: 48 tensors or 65535 chunks each
    cnt = blocks = 0
    for p in params:
        ch = -(-p.numel() // _lib.OPTIM_CHUNK)
        if cnt == 48 or (cnt and blocks + ch > 65535):
            n_multi, cnt, blocks = n_multi + 1, 0, 0
        cnt, blocks = cnt + 1, blocks + ch
    n_multi += 1
    hyper = dict(lr=2e-5, betas=(0.9, 0.999), eps=1e-8)
    variants = [
        ("a", "default path: gcd_adam_step_multi", AdamHIP(params, **hyper), 28, n_multi),
        ("b", "device state, every option off", AdamHIP(params, device_state=True, **hyper), 28, 2),
        ("c", "+ clipping", AdamHIP(params, max_grad_norm=1.0, **hyper), 32, 3),
        ("d", "+ dynamic loss scaling", AdamHIP(params, max_grad_norm=1.0, loss_scale="dynamic", init_scale=1.0, **hyper), 32, 3),
        ("e", "+ EMA", AdamHIP(params, max_grad_norm=1.0, loss_scale="dynamic", init_scale=1.0, ema=LitEma(bag), **hyper),
         40, 3),
    ]
    times = {k: [] for k, *_ in variants}
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in variants]
    for rep in range(args.warmup + args.repeats):
        for (k, _, opt, _, _), (e0, e1) in zip(variants, ev):
            e0.record()
            opt.step()
            e1.record()
        torch.cuda.synchronize()
        if rep >= args.warmup:
            for (k, *_), (e0, e1) in zip(variants, ev):
                times[k].append(e0.elapsed_time(e1) * 1e-3)
    lines = [f"optimizer step on the full-width VideoUNet's shapes: {len(params)} tensors, {n_par} parameters "
             f"({sum(-(-p.numel() // _lib.OPTIM_CHUNK) for p in params)} chunks of {_lib.OPTIM_CHUNK}); {torch.cuda.get_device_name(0)}",
             f"device events around step(), variants alternated, {args.warmup} warm-up + {args.repeats} repeats; "
             "B/param from the shapes (update 28, EMA + 8, reduction + 4)",
             f"{'':2}{'variant':42} {'median ms':>10} {'min ms':>9} {'max ms':>9} {'B/param':>8} {'TB/s':>7} {'launches':>9}"]
    med = {}
    for k, name, opt, bpp, launches in variants:
        t = times[k]
        med[k] = statistics.median(t)
        if k != "a":
            assert opt.launches_per_step == launches, (k, opt.launches_per_step)
        lines.append(f"{k:2}{name:42} {med[k] * 1e3:10.3f} {min(t) * 1e3:9.3f} {max(t) * 1e3:9.3f} {bpp:8d} "
                     f"{n_par * bpp / med[k] / 1e12:7.3f} {launches:9d}")
    rate_b = n_par * 28 / med["b"]
    for k, _, _, bpp, _ in variants[2:]:
        lines.append(f"({k}) costs {med[k] / med['b']:.3f} x (b); its bytes at (b)'s rate would cost {bpp / 28:.3f} x "
                     f"({n_par * bpp / rate_b * 1e3:.3f} ms)")
    ok = med["b"] <= max(times["a"])
    lines.append(f"gate 1: median (b) {med['b'] * 1e3:.3f} ms <= slowest repeat of (a) {max(times['a']) * 1e3:.3f} ms: "
                 f"{'PASS' if ok else 'FAIL'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
