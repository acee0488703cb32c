"""tools/lora_bench.py — the `time_lora` fine-tune step against the `everything` step, at BASELINE.json cfg4's per-GPU shape
(2 clips x 14 frames of 32 x 48 latents, the full-width Kubric VideoUNet), fp16 and bf16 GEMM operands.

In ONE process, on two networks with the same weights, the two steps ALTERNATE (everything, time_lora, everything, ...),
each timed in phases as tools/train_step_bench.py times its step (forward / backward / optimizer, a synchronisation after
each); the median of `--steps` (5) after `--warmup` (2) is reported.  The optimizer phase of the LoRA step is
project_grads + AdamHIP over the adapters + merge.  Then the two new kernels alone (hip events around 10 calls): the bytes
each has to move over the time, against the HBM peak.  Peak memory of a mode is what torch's allocator peaked at during that
mode's steps minus what the other mode's objects held at the time.  No figure is fixed in advance.

    python tools/lora_bench.py [--steps 5] [--warmup 2] [--out profiles/r18_lora_bench.txt]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from bench import build_model  # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s, MI355X data sheet (DESIGN.md §11.4 quotes fractions of this figure)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--latent", default="32x48")
    ap.add_argument("--clips", type=int, default=2)
    ap.add_argument("--frames", type=int, default=14)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from gcd_amd import autograd_ops as AO, lora as L, training as TR
    dev = torch.device("cuda:0")
    T = a.frames
    h, w = (int(v) for v in a.latent.split("x"))
    BT = a.clips * T
    lines = []

    def say(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    den = TR.TrainDenoiser({"target": "gcd_amd.denoiser_scaling.VScalingWithEDMcNoise"}, use_checkpoint=None)
    loss_fn = TR.StandardDiffusionLoss(
        sigma_sampler_config={"target": "gcd_amd.training.EDMSampling", "params": {"p_mean": 1.0, "p_std": 1.6}},
        loss_weighting_config={"target": "gcd_amd.training.EDMWeighting", "params": {"sigma_data": 1.0}},
        focus_top=0.1, focus_steps=5000, batch2model_keys=["image_only_indicator", "num_video_frames"])
    g = torch.Generator(device=dev).manual_seed(1)
    x0 = torch.randn(BT, 4, h, w, generator=g, device=dev)
    cond = {"crossattn": torch.randn(BT, 1, 1024, generator=g, device=dev),
            "concat": torch.randn(BT, 4, h, w, generator=g, device=dev) * 0.8,
            "vector": torch.randn(BT, 896, generator=g, device=dev).clamp(-1, 1)}
    batch = {"global_step": 2500, "num_video_frames": T, "image_only_indicator": torch.zeros(a.clips, T, device=dev)}
    scale = 1024.0

    held0 = torch.cuda.memory_allocated()
    net_e = build_model(dev, seed=0).train()
    opt_e = TR.AdamHIP(net_e.parameters(), lr=2e-5)
    held_e = torch.cuda.memory_allocated() - held0
    net_l = build_model(dev, seed=0).train()
    lora = L.apply_ft_strategy(net_l, "time_lora", generator=torch.Generator().manual_seed(2))
    with torch.no_grad():                      # B away from its zero start: dA is not identically zero either
        for b in lora.lora_B:
            b.normal_(0.0, 0.02)
    lora.merge()
    opt_l = TR.AdamHIP(lora.parameters(), lr=2e-5)
    held_l = torch.cuda.memory_allocated() - held0 - held_e

    def step(mode):
        net, opt = (net_e, opt_e) if mode == "everything" else (net_l, opt_l)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = loss_fn._forward(net, den, cond, x0, batch).mean()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        opt.zero_grad()
        (loss * scale).backward()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if mode == "everything":
            opt.step(grad_scale=1.0 / scale)
        else:
            lora.step(opt, grad_scale=1.0 / scale)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        return (t1 - t0, t2 - t1, t3 - t2), bool(torch.isfinite(loss))

    for dtype in ("fp16", "bf16"):
        AO.set_train_dtype(dtype)
        AO.PACK.clear()
        times = {"everything": [], "time_lora": []}
        peak = {"everything": 0, "time_lora": 0}
        finite = True
        for it in range(a.warmup + a.steps):
            for mode in ("everything", "time_lora"):
                torch.cuda.reset_peak_memory_stats()
                t, ok = step(mode)
                finite = finite and ok
                peak[mode] = max(peak[mode], torch.cuda.max_memory_allocated())
                if it >= a.warmup:
                    times[mode].append(t)
        res = {}
        for mode, ts in times.items():
            f, b, o = (sorted(t[i] for t in ts)[len(ts) // 2] for i in range(3))
            tot = sorted(sum(t) for t in ts)[len(ts) // 2]
            other = held_l if mode == "everything" else held_e
            res[mode] = {"forward_s": round(f, 4), "backward_s": round(b, 4), "optimizer_s": round(o, 4), "step_s": round(tot, 4),
                         "peak_mem_gib": round((peak[mode] - held0 - other) / 2 ** 30, 1)}
        say({"what": "fine-tune step, full-width Kubric VideoUNet, alternating in one process", "gemm_operands": dtype,
             "frames": BT, "latent": [h, w], "median_of": a.steps, "engine": TR.TRAIN_ENGINE, "loss_finite": finite, **res,
             "lora_over_everything": round(res["time_lora"]["step_s"] / res["everything"]["step_s"], 3)})
    AO.set_train_dtype("fp16")

    # ---- the two kernels alone ----
    nk = sum(w_.numel() for w_ in lora.weights())
    for w_ in lora.weights():                  # a dW for every layer (also the ones the backward pass never reaches)
        if w_.grad is None:
            w_.grad = torch.randn_like(w_) * 1e-3
    lora.project_grads()
    scratch_bytes = 4 * lora._scratch.numel()
    adapters = 4 * sum(p.numel() for p in lora.parameters())
    for name, fn, nbytes in (("gcd_lora_merge", lora.merge, 2 * 4 * nk + adapters),
                             ("gcd_lora_project", lora.project_grads, 4 * nk + 2 * scratch_bytes + 2 * adapters)):
        fn()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(11)]
        ev[0].record()
        for i in range(10):
            fn()
            ev[i + 1].record()
        torch.cuda.synchronize()
        ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(10))[5]
        say({"kernel": name, "layers": len(lora.names), "weight_elements": nk, "rank": lora.r, "median_ms_of_10": round(ms, 3),
             "bytes_moved": nbytes, "tb_per_s": round(nbytes / (ms * 1e-3) / 1e12, 2),
             "fraction_of_hbm_peak": round(nbytes / (ms * 1e-3) / HBM_PEAK, 3), "includes_host_side_of_the_call": True})
    if a.out:
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
