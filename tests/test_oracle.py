"""CPU: pin the oracle restatement (oracle/svd_unet_ref.py) against golden tensors produced by the
reference's own modules (oracle/make_golden.py).  Bar: fp32 round-off (rel-L2 <= 2e-5)."""
from pathlib import Path

import pytest
import torch

from conftest import rel_l2
from oracle import svd_unet_ref as O, weights

GOLD = Path(__file__).resolve().parent / "golden"


def _sample(t, n=4096):
    f = t.reshape(-1)
    idx = torch.linspace(0, f.numel() - 1, min(n, f.numel())).long()
    return f[idx]


@pytest.fixture(scope="module")
def tiny_sd():
    g = torch.load(GOLD / "unet_tiny.pt")
    return weights.synth_state_dict(g["state_dict_shapes"]), g


def _unet_inputs(cfg, T, h, w, seed):
    noise, c, uc = weights.synth_inputs(1, T, h, w, cfg.context_dim,
                                        cfg.adm_in_channels + cfg.aux_emb_dim, seed)
    x = torch.cat([torch.cat([noise, uc["concat"]], 1), torch.cat([noise, c["concat"]], 1)])
    ts = torch.linspace(-1.5, 1.63, 2 * T)
    return (x, ts, torch.cat([uc["crossattn"], c["crossattn"]]),
            torch.cat([uc["vector"], c["vector"]]), torch.zeros(2, T))


def test_unet_forward_matches_reference_golden(tiny_sd):
    sd, g = tiny_sd
    x, ts, ctx, y, ioi = _unet_inputs(O.TINY, g["T"], g["h"], g["w"], g["input_seed"])
    taps = {}
    with torch.no_grad():
        out = O.unet_forward(sd, O.TINY, x, ts, ctx, y, g["T"], ioi, taps=taps)
    assert float(g["out"].std()) > 0.1, "golden output is degenerate (zero-init weights?)"
    assert rel_l2(out, g["out"]) < 2e-5
    assert set(taps) == set(g["tap_samples"]) and len(taps) == 25
    for k, v in taps.items():
        assert tuple(v.shape) == g["tap_shapes"][k]
        assert rel_l2(_sample(v), g["tap_samples"][k]) < 2e-5, k
        assert abs(float(v.double().norm()) / g["tap_norms"][k] - 1) < 2e-5, k


@pytest.mark.parametrize("fixture", ["unet_tiny_heavy.pt", "unet_tiny_geglu_range.pt"])
def test_unet_forward_stress_fixtures_match_reference_golden(tiny_sd, fixture):
    """The two stress fixtures (oracle/make_golden_stress.py: Student-t nu = 3 weights; the same with the GEGLU projections
    scaled until the hidden tensor reaches ~half of the fp16 range) pin the oracle too, at fp32 round-off."""
    _, g0 = tiny_sd
    g = torch.load(GOLD / fixture)
    sd = weights.synth_state_dict_heavy(g0["state_dict_shapes"], g["salt"], g["nu"], g["geglu_gain"])
    x, ts, ctx, y, ioi = _unet_inputs(O.TINY, g["T"], g["h"], g["w"], g["input_seed"])
    taps = {}
    with torch.no_grad():
        out = O.unet_forward(sd, O.TINY, x, ts, ctx, y, g["T"], ioi, taps=taps)
    if g["geglu_gain"] > 1.0:
        assert 20000.0 < g["geglu_hidden_absmax"] < 65504.0, "must sit high in the fp16 range without overflow"
    assert g["weight_absmax_over_sigma"] > 20.0, "weights are not heavy-tailed"
    assert rel_l2(out, g["out"]) < 5e-5
    for k, v in taps.items():
        assert rel_l2(_sample(v), g["tap_samples"][k]) < 5e-5, k


def test_sampler_loop_matches_reference_golden(tiny_sd):
    sd, _ = tiny_sd
    g = torch.load(GOLD / "sampler_tiny.pt")
    noise, c, uc = weights.synth_inputs(1, g["T"], g["h"], g["w"], O.TINY.context_dim,
                                        O.TINY.adm_in_channels + O.TINY.aux_emb_dim, g["input_seed"])
    trace = []
    with torch.no_grad():
        final = O.sample_loop(sd, O.TINY, noise, c, uc, g["T"], g["steps"], trace=trace)
    assert len(trace) == g["steps"]
    for i, xi in enumerate(trace):
        assert rel_l2(xi, g["trace"][i]) < 2e-5, f"step {i}"
    assert rel_l2(final, g["final"]) < 2e-5


def test_known_answers():
    k = torch.load(GOLD / "kat.pt")
    sig = O.edm_sigmas(25, sigma_max=700.0)
    assert torch.allclose(sig, k["sigmas_25_700"], rtol=1e-6, atol=0)
    # values quoted in SURVEY.md §8(a3)
    assert abs(float(sig[0]) - 700.000122) < 1e-3 and abs(float(sig[1]) - 545.729492) < 1e-3
    assert float(sig[-1]) == 0.0 and abs(float(sig[-2]) - 0.002) < 1e-8
    assert torch.allclose(O.guider_scale(14)[None], k["guider_scale_14"])
    sc = torch.stack(O.v_scaling_edm_cnoise(k["scaling_sigma"]))
    assert torch.allclose(sc, k["scaling"], rtol=1e-6)
    # sigma = 1 -> (0.5, -0.70710677, 0.70710677, 0)  
    assert torch.allclose(sc[:, 1], torch.tensor([0.5, -0.70710677, 0.70710677, 0.0]), atol=1e-7)
    assert torch.allclose(O.timestep_embedding(k["temb_t"], 320), k["temb_320"], atol=1e-6)


def test_topology_counts():
    """Module census of SURVEY.md Appendix B: 22 VideoResBlocks, 16 transformers, 3 down, 3 up."""
    i, m, o = O.topology(O.KUBRIC)
    flat = [l for blk in i + [m] + o for l in blk]
    assert len(i) == 12 and len(o) == 12
    assert sum(l[0] == "res" for l in flat) == 22
    assert sum(l[0] == "attn" for l in flat) == 16
    assert sum(l[0] == "down" for l in flat) == 3 and sum(l[0] == "up" for l in flat) == 3


def test_random_init_is_vacuous_without_reseeding():
    """zeroing the 61 zero_module tensors makes the network output exactly 0 —
    which is why the fixtures re-draw them."""
    g = torch.load(GOLD / "unet_tiny.pt")
    sd = weights.synth_state_dict(g["state_dict_shapes"])
    zeroed = [k for k in sd if k.endswith("out_layers.3.weight") or k.endswith("out_layers.3.bias")
              or k.endswith("proj_out.weight") or k.endswith("proj_out.bias") or k.startswith("out.2.")]
    assert len([k for k in zeroed if k.endswith(".weight")]) == 61
    for k in zeroed:
        sd[k] = torch.zeros_like(sd[k])
    x, ts, ctx, y, ioi = _unet_inputs(O.TINY, 4, 8, 8, 5)
    with torch.no_grad():
        out = O.unet_forward(sd, O.TINY, x, ts, ctx, y, 4, ioi)
    assert float(out.abs().max()) == 0.0


def test_embedders_against_reference_if_mounted():
    """The restatement against the reference at a second shape / seed, with the image_only_indicator path of
    AlphaBlender: the reference's own forward is recorded in tests/golden/ref_checks_tiny.pt
    (oracle/make_golden_ref_checks.py, which also rebuilds the inputs)."""
    from oracle.make_golden_ref_checks import embedders_inputs
    g = torch.load(GOLD / "ref_checks_tiny.pt")["embedders"]
    cfg = O.TINY
    with torch.device("meta"):
        from gcd_amd.video_model import VideoUNet
        shapes = {k: tuple(v.shape) for k, v in VideoUNet(**cfg.as_reference_kwargs()).state_dict().items()}
    sd = weights.synth_state_dict(shapes, salt=g["salt"])
    x, ts, ctx, y, ioi = embedders_inputs()
    assert float(ioi.abs().sum()) > 0
    with torch.no_grad():
        mine = O.unet_forward(sd, cfg, x, ts, ctx, y, g["T"], ioi)
    assert rel_l2(mine, g["out"]) < 2e-5


def test_oracle_full_width_cfg0_step_vs_reference_golden():
    """BASELINE.json cfg0 at the real width: one EulerEDM sampler_step of the 1.53 B-parameter Kubric
    network on a 14 x 32 x 32 x 4 latent — the oracle restatement against the reference plugin stack's
    own result (oracle/make_golden_fullres.py).  Pins the oracle at the shape bench.py's parity leg
    and cpu_baseline use it."""
    g = torch.load(GOLD / "step_kubric_32x32.pt")
    from gcd_amd.video_model import VideoUNet
    with torch.device("meta"):
        shapes = {k: tuple(v.shape) for k, v in VideoUNet(**O.KUBRIC.as_reference_kwargs()).state_dict().items()}
    sd = weights.synth_state_dict(shapes, g["salt"])
    T, h, w = g["T"], g["h"], g["w"]
    noise, c, uc = weights.synth_inputs(1, T, h, w, O.KUBRIC.context_dim,
                                        O.KUBRIC.adm_in_channels + O.KUBRIC.aux_emb_dim, g["input_seed"])
    st = g["steps"][1]                      # the mid-schedule one (sigma 3 -> 2): x and D weigh alike
    sig, nxt = st["sigma"], st["next_sigma"]
    x = noise * (1.0 + sig ** 2) ** 0.5
    with torch.no_grad():
        got = O.sampler_step(sd, O.KUBRIC, x, sig, nxt, c, uc, T, torch.zeros(2, T), O.guider_scale(T))
    e = rel_l2(got, st["x_next"])
    assert float(st["x_next"].std()) > 0.5 and e < 2e-5, f"oracle vs reference at 14x32x32: {e:.2e}"


def test_oracle_gradients_match_live_reference():
    """The fine-tune step's parity chain (tests/test_backward_gpu.py) compares the HIP gradients with
    torch.autograd over the ORACLE; this pins that reference: autograd through the oracle restatement
    equals autograd through the unmodified reference modules (denoiser + L2 loss, TINY width), for the
    input and for every parameter.  The reference's run is recorded in tests/golden/ref_checks_tiny.pt
    (oracle/make_golden_ref_checks.py: every parameter gradient by its norm, strided samples and seeded
    projections of the whole tensor)."""
    from oracle.make_golden_ref_checks import gradients_inputs, rel_err, unpack
    g = torch.load(GOLD / "ref_checks_tiny.pt")["gradients"]
    cfg = O.TINY
    with torch.device("meta"):
        from gcd_amd.video_model import VideoUNet
        shapes = {k: tuple(v.shape) for k, v in VideoUNet(**cfg.as_reference_kwargs()).state_dict().items()}
    records = unpack(g["param_grads"], shapes)
    sd = weights.synth_state_dict(shapes, salt=g["salt"])
    sdo = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    noise, c, target, sigma, ioi = gradients_inputs()
    x_o = noise.clone().requires_grad_(True)
    out_o = O.denoise(sdo, cfg, x_o, sigma, c, g["T"], ioi)
    ((out_o - target) ** 2).mean().backward()
    assert rel_l2(out_o, g["out"]) < 2e-5 and rel_l2(x_o.grad, g["x_grad"]) < 2e-5
    checked = dead = 0
    for name, rec in records.items():
        go = sdo[name].grad
        # q / k / norm2 of the one-key cross-attention: exactly 0 in exact arithmetic; the reference's SDPA
        # backward leaves ~1e-10 of rounding noise there
        if rec is None or rec["amax"] < 1e-8:
            assert go is None or float(go.abs().max()) < 1e-8, name
            dead += 1
            continue
        # (scalar blend logits are long cancelling sums: fp32 summation order shows at 1e-4)
        assert go is not None and rel_err(go, rec) < (5e-5 if go.numel() > 1 else 1e-3), name
        checked += 1
    assert checked > 1000 and dead >= 64
