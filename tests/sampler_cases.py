"""Shared by the sampler-family tests (a helper module like memcontract.py, not a conftest): the golden fixture of
tools/make_golden_samplers.py, samplers built from its specs, and a noise source that replays recorded draws."""
from pathlib import Path

import torch

GOLD = Path(__file__).resolve().parent / "golden"
DISC = {"target": "gcd_amd.discretizer.EDMDiscretization", "params": {"sigma_max": 700.0}}
CASES = ["heun", "euler_churn", "euler_ancestral", "dpmpp2s_ancestral", "dpmpp2m", "heun_vanilla", "dpmpp2m_vanilla"]
_golden = None
_LIN3 = ("LinearPredictionGuider", {"num_frames": 3, "max_scale": 1.5, "min_scale": 1.0})
_CHURN = dict(s_churn=2.0, s_tmin=0.05, s_tmax=200.0, s_noise=1.003)
# name -> spec in the golden's form, for the tests that need no golden (T = 3)
KINDS = {
    "euler": ("EulerEDMSampler", {}, _LIN3),
    "euler_churn": ("EulerEDMSampler", _CHURN, _LIN3),
    "heun": ("HeunEDMSampler", {}, _LIN3),
    "heun_churn": ("HeunEDMSampler", _CHURN, ("VanillaCFG", {"scale": 1.25})),
    "euler_ancestral": ("EulerAncestralSampler", dict(eta=0.8, s_noise=1.01), _LIN3),
    "dpmpp2s_ancestral": ("DPMPP2SAncestralSampler", {}, _LIN3),
    "dpmpp2m": ("DPMPP2MSampler", {}, ("VanillaCFG", {"scale": 1.25})),
}


def row_kinds():
    """One row of the 7-step stage tables of KINDS per pattern of non-zero coefficients (every kind of row the table
    builder emits), plus a row with every term and both stores on and one that needs no network output at all."""
    from gcd_amd.sampler_stages import stage_table
    out, seen = {}, set()
    for name, spec in KINDS.items():
        s = make_sampler(spec, 7, "cpu")
        rows, _ = stage_table(s, s.discretization(7, device="cpu"))
        for k, r in enumerate(rows):
            pat = tuple((r[1:10] != 0).tolist())
            if pat not in seen:
                seen.add(pat)
                out[f"{name}_stage{k}"] = r.clone()
    out["all_terms"] = torch.tensor([1.7, 0.3, -0.6, 0.8, -0.25, 0.4, 1.0, -0.5, 0.6, 0.7, 0.0, 0.0])
    out["no_network"] = torch.tensor([2.0, 1.0, 0.0, 0.0, 0.0, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    return out


def golden():
    """tests/golden/samplers_tiny.pt, loaded once and never modified."""
    global _golden
    if _golden is None:
        _golden = torch.load(GOLD / "samplers_tiny.pt")
    return _golden


def make_sampler(spec, steps, device, T=None):
    """spec: (class name, extra keywords, (guider class name, guider params)) as the golden stores it."""
    from gcd_amd.util import instantiate_from_config
    cls, kw, (guider, gparams) = spec
    gparams = dict(gparams)
    if T is not None and "num_frames" in gparams:
        gparams["num_frames"] = T
    return instantiate_from_config({
        "target": "gcd_amd.sampling." + cls,
        "params": dict(kw, num_steps=steps, device=device, discretization_config=DISC,
                       guider_config={"target": "gcd_amd.guiders." + guider, "params": gparams})})


class Replay:
    """noise_sampler that hands out recorded tensors in order; `left` says how many were not asked for."""

    def __init__(self, tensors):
        self.tensors, self.i = list(tensors), 0

    def __call__(self, x):
        z = self.tensors[self.i].to(device=x.device, dtype=x.dtype)
        self.i += 1
        assert z.shape == x.shape
        return z

    @property
    def left(self):
        return len(self.tensors) - self.i
