"""Generate tests/golden/samplers_tiny.pt: the UNMODIFIED reference samplers (through oracle/ref_shim.py) on the TINY
network and procedural weights / inputs of oracle/make_golden.py's sampler fixture (T = 4, 8x8 latents, 5 steps, input
seed 3, sigma_max = 700).  Needs the reference tree; run with:  python -m tools.make_golden_samplers

Per case: the state after every step (`trace`), `final`, and every noise tensor the reference drew, in order (`noise`):
a seeded recorder is the `noise_sampler` of the ancestral samplers, and stands in for torch.randn_like around the call
of the churn case.

Bars from the reference alone: every case, and plain Euler, is also run with every floating tensor of the state dict
rounded once to fp16; sens[case] = rel_l2(final_fp16w, final_fp32w) says how much the sampler amplifies operand rounding.
The GPU bar of a case is 1.5 * TOL_LOOP * max(1, sens[case] / sens["euler"]) — 1.5 * TOL_LOOP being the project's bar
for plain Euler on this very loop (tests/test_unet_gpu.py::test_sampler_vs_reference_golden).
"""
from __future__ import annotations

import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from oracle import ref_shim, svd_unet_ref as O, weights  # noqa: E402
from oracle.make_golden import build_reference_unet  # noqa: E402

OUT = ROOT / "tests" / "golden" / "samplers_tiny.pt"
T, H, W, STEPS, INPUT_SEED, NOISE_SEED = 4, 8, 8, 5, 3, 1234
TOL_LOOP = 1e-3
LINEAR = ("LinearPredictionGuider", {"num_frames": T, "max_scale": 1.5, "min_scale": 1.0})
VANILLA = ("VanillaCFG", {"scale": 1.25})
CHURN = dict(s_churn=1.0, s_tmin=0.05, s_tmax=50.0, s_noise=1.003)
# name -> (sampler class, extra keywords, guider)
CASES = {
    "euler": ("EulerEDMSampler", {}, LINEAR),
    "heun": ("HeunEDMSampler", {}, LINEAR),
    "euler_churn": ("EulerEDMSampler", CHURN, LINEAR),
    "euler_ancestral": ("EulerAncestralSampler", {}, LINEAR),
    "dpmpp2s_ancestral": ("DPMPP2SAncestralSampler", {}, LINEAR),
    "dpmpp2m": ("DPMPP2MSampler", {}, LINEAR),
    "heun_vanilla": ("HeunEDMSampler", {}, VANILLA),
    "dpmpp2m_vanilla": ("DPMPP2MSampler", {}, VANILLA),
}


class NoiseRecorder:
    def __init__(self, seed=NOISE_SEED):
        self.gen, self.drawn = torch.Generator().manual_seed(seed), []

    def __call__(self, x):
        z = torch.randn(x.shape, generator=self.gen, dtype=x.dtype)
        self.drawn.append(z.clone())
        return z


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def run_case(name, net):
    ref_shim.install()
    import sgm.modules.diffusionmodules.sampling as S
    from sgm.modules.diffusionmodules.denoiser import Denoiser
    from sgm.modules.diffusionmodules.wrappers import OpenAIWrapper
    cls, kw, (guider, gparams) = CASES[name]
    cfg = O.TINY
    noise, c, uc = weights.synth_inputs(1, T, H, W, cfg.context_dim, cfg.adm_in_channels + cfg.aux_emb_dim, seed=INPUT_SEED)
    sampler = getattr(S, cls)(
        num_steps=STEPS, device="cpu", discretization_config=ref_shim.SAMPLER_CFG["discretization_config"],
        guider_config={"target": "sgm.modules.diffusionmodules.guiders." + guider, "params": dict(gparams)}, **kw)
    den, model = Denoiser(ref_shim.DENOISER_CFG), OpenAIWrapper(net)
    extra = {"num_video_frames": T, "image_only_indicator": torch.zeros(2, T)}
    rec, trace = NoiseRecorder(), []
    if hasattr(sampler, "noise_sampler"):
        sampler.noise_sampler = rec

    def denoiser(inp, sigma, cc):
        return den(model, inp, sigma, cc, **extra)

    orig_step = sampler.sampler_step

    def traced_step(*a, **k):
        r = orig_step(*a, **k)
        trace.append((r[0] if isinstance(r, tuple) else r).detach().clone())
        return r

    sampler.sampler_step = traced_step
    saved = torch.randn_like
    torch.randn_like = lambda x, *a, **k: rec(x)          # the churn noise of EDMSampler.sampler_step
    try:
        with torch.no_grad():
            final = sampler(denoiser, noise.clone(), cond=c, uc=uc)
    finally:
        torch.randn_like = saved
    if name == "euler_churn":                              # a condition on the reference alone: both kinds of row occur
        sig = sampler.discretization(STEPS, device="cpu")
        churns = [bool(sampler.s_tmin <= sig[i] <= sampler.s_tmax) for i in range(STEPS)]
        assert churns == [False, False, True, True, False], (churns, sig.tolist())
        assert len(rec.drawn) == 2
    return {"trace": torch.stack(trace), "final": final, "noise": rec.drawn}


def main():
    torch.manual_seed(0)
    net, _ = build_reference_unet(O.TINY)
    net16, _ = build_reference_unet(O.TINY)
    net16.load_state_dict({k: (v.half().float() if v.is_floating_point() else v) for k, v in net.state_dict().items()})
    cases, sens = {}, {}
    for name in CASES:
        cases[name] = run_case(name, net)
        sens[name] = rel_l2(run_case(name, net16)["final"], cases[name]["final"])
        print(f"{name}: final std {float(cases[name]['final'].std()):.4f}, {len(cases[name]['noise'])} draws, "
              f"fp16-weight sensitivity {sens[name]:.3e}")
    ratios = {k: sens[k] / sens["euler"] for k in CASES if k != "euler"}
    bars = {k: 1.5 * TOL_LOOP * max(1.0, r) for k, r in ratios.items()}
    for k in ratios:
        print(f"{k}: ratio {ratios[k]:.3f} -> bar {bars[k]:.3e}")
    cases.pop("euler")                                     # tests/golden/sampler_tiny.pt holds plain Euler
    torch.save({"config": "TINY", "T": T, "h": H, "w": W, "steps": STEPS, "input_seed": INPUT_SEED,
                "noise_seed": NOISE_SEED, "specs": {k: CASES[k] for k in cases}, "cases": cases, "sens": sens,
                "ratios": ratios, "bars": bars, "tol_loop": TOL_LOOP}, OUT)
    print("wrote", OUT, OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
