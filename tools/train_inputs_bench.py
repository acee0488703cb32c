"""tools/train_inputs_bench.py — the fine-tune step of cfg4 as the reference's config really runs it: `vector` comes out of a
TRAINABLE SphericalEmbedder (configs/train_kubric_max90.yaml:116-121), so the UNet's `y` requires grad.  Full-width Kubric
VideoUNet, 2 clips x 14 frames at 32x48 latents; GeneralConditioner -> TrainDenoiser -> StandardDiffusionLoss -> backward ->
AdamHIP over the UNet's and the embedder's parameters together.  Three ways to run that step, in ONE process, alternated
step by step, median of `--steps` each, for fp16 and bf16 operands:

    switch_on   planned engine with input gradients (train_plan.set_input_grads / GCD_TRAIN_INPUT_GRADS=1)
    fallback    switch off: the planned entry hands the step to the operator-level tape engine (what ran before)
    frozen      the conditioner's outputs fed as plain data: the planned step `bench.py --train` measures (no bar: the gap
                to it is what the input gradients cost)

Condition: switch_on must not be slower than fallback.  Writes profiles/r14_train_input_grads.json.

    python tools/train_inputs_bench.py [--steps 5] [--out profiles/r14_train_input_grads.json]
"""
import argparse
import json
import sys
import time
import warnings
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from bench import build_model  # noqa: E402

MODES = ("switch_on", "fallback", "frozen")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--latent", default="32x48")
    ap.add_argument("--clips", type=int, default=2)
    ap.add_argument("--frames", type=int, default=14)
    ap.add_argument("--dtypes", default="fp16,bf16")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r14_train_input_grads.json"))
    a = ap.parse_args()
    from gcd_amd import autograd_ops as AO, training as TR
    from gcd_amd.conditioning import GeneralConditioner
    dev = torch.device("cuda:0")
    T = a.frames
    h, w = (int(v) for v in a.latent.split("x"))
    BT = a.clips * T
    net = build_model(dev, seed=0).train()
    adm, aux = net.adm_in_channels, net.aux_emb_dim
    ident = "gcd_amd.conditioning.IdentityEncoder"
    torch.manual_seed(0)
    cond = GeneralConditioner([
        {"target": ident, "input_key": "ids"},
        {"target": "gcd_amd.conditioning.SphericalEmbedder", "is_trainable": True, "input_key": "pose",
         "params": {"embed_dim": aux}},
        {"target": ident, "input_key": "clip"}, {"target": ident, "input_key": "cond_latents"}]).to(dev).train()
    scaling = {"target": "gcd_amd.denoiser_scaling.VScalingWithEDMcNoise"}
    dens = {"switch_on": TR.TrainDenoiser(scaling, engine="planned", input_grads=True),
            "fallback": TR.TrainDenoiser(scaling, engine="planned", input_grads=False),
            "frozen": TR.TrainDenoiser(scaling, engine="planned", input_grads=False)}
    loss_fn = TR.StandardDiffusionLoss(
        sigma_sampler_config={"target": "gcd_amd.training.EDMSampling", "params": {"p_mean": 1.0, "p_std": 1.6}},
        loss_weighting_config={"target": "gcd_amd.training.EDMWeighting", "params": {"sigma_data": 1.0}},
        focus_top=0.1, focus_steps=5000, batch2model_keys=["image_only_indicator", "num_video_frames"])
    opt = TR.AdamHIP(list(net.parameters()) + list(cond.parameters()), lr=2e-5)
    g = torch.Generator(device=dev).manual_seed(1)
    x0 = torch.randn(BT, 4, h, w, generator=g, device=dev)
    batch = {"ids": torch.randn(BT, adm, generator=g, device=dev).clamp(-1, 1),
             "pose": torch.rand(BT, 3, generator=g, device=dev) * 2 - 1,
             "clip": torch.randn(BT, 1, 1024, generator=g, device=dev),
             "cond_latents": torch.randn(BT, 4, h, w, generator=g, device=dev) * 0.8,
             "global_step": 2500, "num_video_frames": T, "image_only_indicator": torch.zeros(a.clips, T, device=dev)}
    proj = cond.embedders[1].proj
    scale = 1024.0

    def step(mode):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c = cond(batch)
        if mode == "frozen":
            c = {k: v.detach() for k, v in c.items()}
        loss = loss_fn._forward(net, dens[mode], c, x0, batch).mean()
        opt.zero_grad()
        (loss * scale).backward()
        got = proj.weight.grad is not None
        opt.step(grad_scale=1.0 / scale)
        torch.cuda.synchronize()
        assert got == (mode != "frozen") and bool(torch.isfinite(loss))
        return time.perf_counter() - t0

    res = {"what": "cfg4 fine-tune step with a trainable SphericalEmbedder behind cond['vector'], full-width Kubric VideoUNet",
           "frames": BT, "latent": [h, w], "steps": a.steps, "warmup": a.warmup, "order": "alternated in one process",
           "note": "bench.py --train still measures the frozen-conditioner planned step (`frozen` here)"}
    ok = True
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for dt in a.dtypes.split(","):
            AO.set_train_dtype(dt)
            AO.PACK.clear()
            times = {m: [] for m in MODES}
            for it in range(a.warmup + a.steps):
                for m in MODES:
                    t = step(m)
                    if it >= a.warmup:
                        times[m].append(t)
            med = {m: sorted(v)[len(v) // 2] for m, v in times.items()}
            r = {m + "_s": round(med[m], 4) for m in MODES}
            r["all_s"] = {m: [round(t, 4) for t in v] for m, v in times.items()}
            r["switch_on_over_fallback"] = round(med["switch_on"] / med["fallback"], 3)
            r["switch_on_minus_frozen_s"] = round(med["switch_on"] - med["frozen"], 4)
            r["not_slower_than_fallback"] = bool(med["switch_on"] <= med["fallback"])
            ok = ok and r["not_slower_than_fallback"]
            res[dt] = r
    res["condition_met"] = ok
    res["peak_mem_gib"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: v for k, v in res.items() if k != "note"}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
