"""CPU: the sampler family beyond plain Euler (Heun, Euler with churn, Euler ancestral, DPM++ 2S ancestral, DPM++ 2M;
VanillaCFG) — plugin surface, the C ABI of libgcd_amd_sampler.so, the generic path against the reference's goldens
(tools/make_golden_samplers.py), the stage table against the generic path, noise-draw order, routing."""
import math
import re
import types
from pathlib import Path

import pytest
import torch

from conftest import rel_l2
import sampler_cases as sc

ROOT = Path(__file__).resolve().parent.parent
KINDS = sc.KINDS


# ------------------------------------------------------------------------------------------------ plugin surface and C ABI
@pytest.mark.parametrize("cls,params", [
    ("HeunEDMSampler", dict(s_churn=0.5, s_tmin=0.1, s_tmax=10.0, s_noise=1.003)),
    ("EulerEDMSampler", dict(s_churn=0.5)),
    ("EulerAncestralSampler", dict(eta=0.9, s_noise=1.01)),
    ("DPMPP2SAncestralSampler", dict(eta=1.0, s_noise=1.0)),
    ("DPMPP2MSampler", {}),
])
def test_new_samplers_instantiate_from_config_with_the_reference_keywords(cls, params):
    from gcd_amd import guiders, sampling
    from gcd_amd.util import instantiate_from_config
    s = instantiate_from_config({
        "target": "gcd_amd.sampling." + cls,
        "params": dict(params, num_steps=15, device="cpu", verbose=False, discretization_config=sc.DISC,
                       guider_config={"target": "gcd_amd.guiders.VanillaCFG", "params": {"scale": 2.5}})})
    assert type(s) is getattr(sampling, cls) and s.num_steps == 15 and type(s.guider) is guiders.VanillaCFG
    assert s.guider.scale == 2.5 and s.use_graph is True and s.last_path is None
    for k, v in params.items():
        assert getattr(s, k) == v
    if isinstance(s, sampling.AncestralSampler):
        assert isinstance(s, sampling.SingleStepDiffusionSampler) and s.noise_sampler(torch.zeros(2, 3)).shape == (2, 3)
    if isinstance(s, sampling.EDMSampler):
        assert isinstance(s, sampling.SingleStepDiffusionSampler) and s.noise_sampler is None


def test_vanilla_cfg_is_the_reference_arithmetic():
    from gcd_amd.guiders import VanillaCFG
    g = VanillaCFG(scale=1.25)
    x = torch.randn(6, 2, generator=torch.Generator().manual_seed(0))
    assert torch.equal(g(x, None), x[:3] + 1.25 * (x[3:] - x[:3]))
    c, uc = {"vector": torch.ones(3, 2), "n": 4}, {"vector": torch.zeros(3, 2), "n": 4}
    xi, si, ci = g.prepare_inputs(x[:3], torch.ones(3), c, uc)
    assert xi.shape[0] == 6 and si.shape[0] == 6 and ci["n"] == 4
    assert torch.equal(ci["vector"], torch.cat((uc["vector"], c["vector"])))


def test_sampler_library_exports_what_its_header_declares_and_validates_arguments():
    from gcd_amd import _lib
    from gcd_amd.csrc import build as b
    header = (ROOT / "include" / "gcd_amd_sampler.h").read_text()
    lib = _lib.load_sampler()                  # header == table == exports, ABI version: tests/test_libraries_host.py
    m = re.search(r"#define GCD_SAMPLER_ROW (\d+)", header)
    assert int(m.group(1)) == _lib.SAMPLER_ROW == 12
    # argument validation happens before any launch, so it is observable without a GPU
    ok = [16, 16, 16, 16, 16, 16, 16]
    for i in range(4):                                     # cur, net, scale, coef are required
        a = list(ok)
        a[i] = None
        assert lib.gcd_sampler_stage_f32(*a, 4, 2, 16, None) != 0
        assert b"null pointer" in lib.gcd_sampler_last_error()
    for nx, T, chw in [(0, 2, 16), (4, 0, 16), (4, 2, 0), (-1, 2, 16), (4, -3, 16), (4, 2, -16)]:
        assert lib.gcd_sampler_stage_f32(*ok, nx, T, chw, None) != 0
        assert b"empty problem" in lib.gcd_sampler_last_error()
    with pytest.raises(_lib.GcdError, match="no CPU"):
        from gcd_amd import sampler_ops
        sampler_ops.sampler_stage(torch.zeros(2, 4), torch.zeros(4, 4), torch.ones(2), torch.zeros(12), 2)
    # a library of its own (its symbols, sources and headers are apart from the others': tests/test_libraries_host.py)
    assert "sampler_stage" not in (ROOT / "include" / "gcd_amd.h").read_text()
    assert b.LIBRARIES["gcd_amd_sampler"].sources == ["sampler_stage.hip"] and "sampler_stage.hip" not in b.SOURCES


# --------------------------------------------------------------------------------------- generic path vs the reference goldens
@pytest.fixture(scope="module")
def oracle_stack():
    from gcd_amd.denoiser import Denoiser
    from gcd_amd.wrappers import OpenAIWrapper
    from oracle import svd_unet_ref as O, weights
    g = sc.golden()
    gu = torch.load(sc.GOLD / "unet_tiny.pt")
    sd = weights.synth_state_dict(gu["state_dict_shapes"])
    T = g["T"]

    class OracleNet(torch.nn.Module):
        def forward(self, x, timesteps=None, context=None, y=None, num_video_frames=None, image_only_indicator=None):
            return O.unet_forward(sd, O.TINY, x, timesteps, context, y, num_video_frames, image_only_indicator)

    noise, c, uc = weights.synth_inputs(1, T, g["h"], g["w"], O.TINY.context_dim,
                                        O.TINY.adm_in_channels + O.TINY.aux_emb_dim, g["input_seed"])
    den = Denoiser({"target": "gcd_amd.denoiser_scaling.VScalingWithEDMcNoise"})
    model = OpenAIWrapper(OracleNet())
    extra = {"num_video_frames": T, "image_only_indicator": torch.zeros(2, T)}
    return noise, c, uc, (lambda i, s, cc: den(model, i, s, cc, **extra))


@pytest.mark.parametrize("name", sc.CASES)
def test_generic_path_reproduces_the_reference_golden_with_the_oracle_network(oracle_stack, name):
    """The drop-in classes (generic torch path, CPU) driving the ORACLE network reproduce the reference's trajectory with
    the reference's own noise, drawn in the reference's order; the stage table plans the same number of draws."""
    from gcd_amd.sampler_stages import stage_table
    g = sc.golden()
    case = g["cases"][name]
    noise, c, uc, denoiser = oracle_stack
    sampler = sc.make_sampler(g["specs"][name], g["steps"], "cpu")
    replay = sc.Replay(case["noise"])
    sampler.noise_sampler = replay if case["noise"] or hasattr(sampler, "eta") else None
    trace, orig = [], sampler.sampler_step

    def traced(*a, **k):
        r = orig(*a, **k)
        trace.append((r[0] if isinstance(r, tuple) else r).detach().clone())
        return r

    sampler.sampler_step = traced
    with torch.no_grad():
        out = sampler(denoiser, noise.clone(), cond=c, uc=uc)
    assert sampler.last_path == "generic" and replay.left == 0 and replay.i == len(case["noise"])
    e_trace = max(rel_l2(t, r) for t, r in zip(trace, case["trace"]))
    e = rel_l2(out, case["final"])
    print(f"{name}: generic path vs reference golden: trace {e_trace:.3e}, final {e:.3e}")
    assert len(trace) == len(case["trace"]) and e_trace < 2e-5 and e < 2e-5
    rows, draws = stage_table(sampler, sampler.discretization(g["steps"], device="cpu"))
    assert len(draws) == len(case["noise"])
    assert [s for s, _, _ in draws] == sorted(s for s, _, _ in draws)


# ----------------------------------------------------------------------------------------- stage table vs the generic path
def _f_u(x, sigma):
    return torch.tanh(x / (sigma * sigma + 1.0) ** 0.5) * 0.7 + 0.1 * torch.sin(x)


def _f_c(x, sigma):
    return torch.tanh(0.8 * x / (sigma * sigma + 1.0) ** 0.5 + 0.2) * 0.9 - 0.05 * torch.cos(2.0 * x)


def _toy_denoiser(inp, sigma, cc):
    """A closed-form non-linear denoiser on the doubled [uc | c] batch."""
    n = inp.shape[0] // 2
    s = sigma.reshape(-1, *([1] * (inp.ndim - 1)))
    return torch.cat((_f_u(inp[:n], s[:n]), _f_c(inp[n:], s[n:])))


def _emulate_stages(rows, draws, x0, scale, T, draw):
    """gcd_sampler_stage_f32 in float32 torch: the network's raw outputs are chosen so that the kernel's affine map
    net * c_out + cur * c_skip gives the toy denoiser back.  h0, h1 and noise start as NaN: a row that reads a buffer
    before one has written it poisons the result."""
    cur = x0.clone()
    nan = torch.full_like(x0, float("nan"))
    h0, h1, noise = nan.clone(), nan.clone(), nan.clone()
    sc_ = scale.reshape(-1)[torch.arange(x0.shape[0]) % T].reshape(-1, *([1] * (x0.ndim - 1)))
    for stage, used, coef in draws:
        if stage < 0:
            cur = cur + draw(cur) * coef
    for k, r in enumerate(rows):
        for stage, used, _ in draws:
            if stage == k:
                z = draw(cur)
                noise = z if used else noise
        sigma = r[0]
        s2 = sigma * sigma + 1.0
        c_skip, c_out = 1.0 / s2, -sigma / s2.sqrt()
        net_u, net_c = (_f_u(cur, sigma) - cur * c_skip) / c_out, (_f_c(cur, sigma) - cur * c_skip) / c_out
        du, dc = net_u * c_out + cur * c_skip, net_c * c_out + cur * c_skip
        D = du + sc_ * (dc - du)
        new = torch.zeros_like(cur)
        for coef, t in ((r[1], cur), (r[2], D), (r[3], h0), (r[4], h1), (r[5], noise)):
            if coef != 0:
                new = new + coef * t
        n0 = r[6] * cur + r[7] * D if (r[6] != 0 or r[7] != 0) else h0
        n1 = r[8] * cur + r[9] * D if (r[8] != 0 or r[9] != 0) else h1
        cur, h0, h1 = new, n0, n1
    return cur


@pytest.mark.parametrize("name", list(KINDS))
def test_stage_table_emulation_equals_the_generic_path(name):
    from gcd_amd.sampler_stages import stage_table
    T, steps = 3, 7
    sampler = sc.make_sampler(KINDS[name], steps, "cpu")
    gen = torch.Generator().manual_seed(5)
    x0 = torch.randn(2 * T, 4, 5, 3, generator=gen)
    drawn = [torch.randn(x0.shape, generator=gen) for _ in range(2 * steps)]
    cond = {"vector": torch.zeros(2 * T, 2), "crossattn": torch.zeros(2 * T, 1, 2), "concat": torch.zeros(2 * T, 1, 5, 3)}
    replay = sc.Replay(drawn)
    if name != "dpmpp2m":
        sampler.noise_sampler = replay
    ref = sampler(_toy_denoiser, x0.clone(), cond=cond, uc=cond)
    assert sampler.last_path == "generic"
    sigmas = sampler.discretization(steps, device="cpu")
    rows, draws = stage_table(sampler, sigmas)
    assert rows.dtype == torch.float32 and rows.shape[1] == 12 and bool(torch.isfinite(rows).all())
    assert float(rows[:, 10:].abs().max()) == 0.0 and len(draws) == replay.i
    if "churn" in name:                                   # both kinds of row occur: steps that churn and steps that do not
        assert 0 < len(draws) < steps
    from gcd_amd.sampling import _guider_scale
    replay2 = sc.Replay(drawn)
    got = _emulate_stages(rows, draws, x0 * torch.sqrt(1.0 + sigmas[0] ** 2.0), _guider_scale(sampler.guider, T), T, replay2)
    e = rel_l2(got, ref)
    print(f"{name}: {rows.shape[0]} stages, {len(draws)} draws, stage emulation vs generic path rel-L2 {e:.3e}")
    assert bool(torch.isfinite(got).all()) and e < 2e-5 and replay2.i == replay.i


@pytest.mark.parametrize("name", list(KINDS))
@pytest.mark.parametrize("steps", [1, 2, 25])
def test_stage_rows_are_finite_and_counted(name, steps):
    """No inf / NaN coefficient, including sigma' = 0 and the first DPM++ 2M step; one stage per network evaluation."""
    from gcd_amd.sampler_stages import stage_table
    sampler = sc.make_sampler(KINDS[name], steps, "cpu")
    rows, draws = stage_table(sampler, sampler.discretization(steps, device="cpu"))
    assert bool(torch.isfinite(rows).all()) and bool((rows[:, 0] > 0).all())
    want = 2 * steps - 1 if name.startswith("heun") else steps          # the last step saves its second evaluation
    if name == "dpmpp2s_ancestral":          # ... and so does every step whose float32 sigma_down vanishes (sampling.py:282)
        from gcd_amd.sampler_stages import get_ancestral_step
        sig = sampler.discretization(steps, device="cpu")
        want = sum(1 + int(not float(get_ancestral_step(sig[i], sig[i + 1], eta=sampler.eta)[0]) < 1e-14)
                   for i in range(steps))
        assert want == 2 * steps - 1 or steps == 2       # [700, 0.002, 0]: sigma_up rounds to sigma', sigma_down to 0
    assert rows.shape[0] == want
    if name == "dpmpp2m":
        assert float(rows[0, 3]) == 0.0 and float(rows[-1, 3]) == 0.0 and not draws      # no history read on those steps
        assert tuple(rows[-1, 1:3].tolist()) == (0.0, 1.0)                               # sigma' = 0: x <- D
    if "ancestral" in name:
        assert len(draws) == steps and draws[-1][1] is False and float(rows[-1, 5]) == 0.0   # drawn, then discarded
    with pytest.raises(ValueError):
        stage_table(sampler, torch.tensor([1.0, 0.0, 0.0]))


# ---------------------------------------------------------------------------------------------------------------- routing
def test_routing_on_cpu_stand_ins():
    """Euler without churn keeps FusedEulerLoop; every other case routes to FusedStageLoop; an unknown guider, or a
    sampler without a stage form, stays on the generic path."""
    from gcd_amd import sampling
    from gcd_amd.denoiser import Denoiser
    from gcd_amd.video_model import VideoUNet
    from gcd_amd.wrappers import OpenAIWrapper
    from oracle import svd_unet_ref as O
    T = 3
    with torch.device("meta"):
        net = VideoUNet(**O.TINY.as_reference_kwargs())
    fd = sampling.FusedDenoiser(Denoiser({"target": "gcd_amd.denoiser_scaling.VScalingWithEDMcNoise"}), OpenAIWrapper(net),
                                num_video_frames=T, image_only_indicator=None)
    x = types.SimpleNamespace(is_cuda=True, dtype=torch.float32, shape=(2 * T, 4, 8, 8))      # a GPU tensor's stand-in
    cond = {"vector": None, "crossattn": None, "concat": types.SimpleNamespace(shape=(2 * T, net.in_channels - 4, 8, 8))}
    for name, spec in KINDS.items():
        s = sc.make_sampler(spec, 5, "cpu")
        assert s._can_fuse(fd, x, cond, cond), name
        want = sampling.FusedEulerLoop if name == "euler" else sampling.FusedStageLoop
        assert s._fused_loop_class() is want, name
        assert not s._can_fuse(fd, types.SimpleNamespace(is_cuda=False, dtype=x.dtype, shape=x.shape), cond, cond)
        assert not s._can_fuse(fd, types.SimpleNamespace(is_cuda=True, dtype=x.dtype, shape=(2 * T + 1, 4, 8, 8)), cond, cond)
        assert not s._can_fuse(lambda i, sg, c: i, x, cond, cond)
        s.guider = types.SimpleNamespace(scale=torch.ones(1, T), num_frames=T, additional_cond_keys=[])   # unknown guider
        assert not s._can_fuse(fd, x, cond, cond), name
    assert issubclass(sampling.FusedStageLoop, sampling.FusedEulerLoop)
    ident = sampling.HeunEDMSampler(discretization_config=sc.DISC, num_steps=5, device="cpu")           # IdentityGuider
    assert not ident._can_fuse(fd, x, cond, cond)
    lin = sc.make_sampler(KINDS["heun"], 5, "cpu")
    lin.guider.additional_cond_keys = ["extra"]
    assert not lin._can_fuse(fd, x, cond, cond)
    other_T = sc.make_sampler(KINDS["heun"], 5, "cpu", T=T + 1)
    assert not other_T._can_fuse(fd, x, cond, cond)
    assert math.isclose(float(sampling._guider_scale(sc.make_sampler(KINDS["dpmpp2m"], 5, "cpu").guider, T)[2]), 1.25)
