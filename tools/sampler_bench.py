"""Time the fused sampler family on the full-width network at 14x72x128 latents (a record, not a gate).

    python tools/sampler_bench.py [--latent 72x128] [--repeats 5] [--out FILE]

One process, device events on the loop's stream, the variants interleaved inside every repeat, median over the repeats.
A variant is a sampler at the step count a user would pick for it: 25 Euler steps (the unchanged FusedEulerLoop and
gcd_cfg_euler_step), 15 DPM++ 2M steps, 13 Heun steps (25 network evaluations), and for completeness Euler with churn,
Euler ancestral and DPM++ 2S ancestral at Euler's and Heun's counts.  Per repeat a variant builds its loop, runs the eager
stage and the capturing stage (not timed), then one clip's worth of stages (timed) — for the stochastic samplers the timed
region contains their noise draws.  Reported: ms per network evaluation and ms per clip.

Whether 15 DPM++ 2M steps match 25 Euler steps in QUALITY needs trained weights; this tool says nothing about it.
"""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

import bench  # noqa: E402

CHURN = dict(s_churn=10.0, s_tmin=0.05, s_tmax=50.0, s_noise=1.003)
# name, class, keywords, steps
VARIANTS = [
    ("euler (FusedEulerLoop)", "EulerEDMSampler", {}, 25),
    ("dpmpp2m", "DPMPP2MSampler", {}, 15),
    ("heun", "HeunEDMSampler", {}, 13),
    ("euler + churn", "EulerEDMSampler", CHURN, 25),
    ("euler ancestral", "EulerAncestralSampler", {}, 25),
    ("dpmpp2s ancestral", "DPMPP2SAncestralSampler", {}, 13),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--latent", default="72x128")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from gcd_amd import sampling
    from gcd_amd.denoiser import Denoiser
    from gcd_amd.wrappers import OpenAIWrapper
    dev = torch.device("cuda:0")
    T = 14
    h, w = (int(v) for v in args.latent.split("x"))
    net = bench.build_model(dev, seed=0)
    noise, c, uc = bench.synth_inputs(dev, T, h, w, seed=100, cond=bench.pose_conditioner(dev))
    fd = sampling.FusedDenoiser(Denoiser({"target": "gcd_amd.denoiser_scaling.VScalingWithEDMcNoise"}), OpenAIWrapper(net),
                                num_video_frames=T, image_only_indicator=torch.zeros(2, T, device=dev))

    def make(cls, kw, steps):
        return getattr(sampling, cls)(
            discretization_config={"target": "gcd_amd.discretizer.EDMDiscretization", "params": {"sigma_max": 700.0}},
            num_steps=steps, device="cuda",
            guider_config={"target": "gcd_amd.guiders.LinearPredictionGuider",
                           "params": {"num_frames": T, "max_scale": 1.5, "min_scale": 1.0}}, **kw)

    def one_clip(sampler):
        """(ms, launches) of one clip's stages on a warmed loop with its graph captured."""
        assert sampler._can_fuse(fd, noise, c, uc)
        loop = sampler._fused_loop_class()(sampler, fd, noise.clone(), c, uc)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        try:
            with loop:
                loop.step(0)
                loop.step(1)
                loop.side.synchronize()
                e0.record(loop.side)
                for i in range(loop.num_launches):
                    loop.step(2 + i)
                e1.record(loop.side)
                loop.side.synchronize()
        finally:
            loop.close()
        assert bool(torch.isfinite(loop.x).all())
        return e0.elapsed_time(e1), loop.num_launches, type(loop).__name__

    samplers = [(name, make(cls, kw, steps), steps) for name, cls, kw, steps in VARIANTS]
    for _, s, _ in samplers:                     # one untimed pass: packing, workspace, allocator
        one_clip(s)
    times = {name: [] for name, _, _ in samplers}
    info = {}
    for _ in range(args.repeats):
        for name, s, steps in samplers:          # interleaved: drift of the box hits every variant alike
            ms, launches, loop_name = one_clip(s)
            times[name].append(ms)
            info[name] = (steps, launches, loop_name)
    lines = [f"sampler family at 14x{h}x{w} latents, full-width network, {torch.cuda.get_device_name(0)}; "
             f"median of {args.repeats} (min .. max), device events, variants interleaved",
             f"{'variant':<24}{'loop':<16}{'steps':>6}{'evals':>6}{'ms / eval':>12}{'ms / clip':>12}   (min .. max ms / clip)"]
    for name, _, _ in samplers:
        steps, launches, loop_name = info[name]
        med = statistics.median(times[name])
        lines.append(f"{name:<24}{loop_name:<16}{steps:>6}{launches:>6}{med / launches:>12.3f}{med:>12.1f}   "
                     f"({min(times[name]):.1f} .. {max(times[name]):.1f})")
    text = "\n".join(lines)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
