"""GPU: end-to-end parity of the HIP VideoUNet / sampler (through the C ABI) with the CPU oracle and
the committed reference goldens.

Tolerances (rel-L2 vs fp32 reference; operands are fp16 with fp32 accumulation and an fp32 residual
stream — SURVEY.md §0.5 measured 1.8e-3 per forward / 8.4e-4 per loop for fp16 autocast):
    single UNet forward      <= 2e-3
    per-block activations    <= 2e-3
    sampler trajectory/final <= 1e-3   (north_star: frames within 1e-3 rel-L2)
"""
from pathlib import Path

import pytest
import torch

from conftest import rel_l2
from oracle import svd_unet_ref as O, weights

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
TOL_FWD = 2e-3
TOL_LOOP = 1e-3
# decoded 576 x 1024 frames of a full loop against the reference loop + reference decoder (measured on procedural
# weights: 1.07e-3 rel-L2, 70.4 dB): the north_star's "within 1e-3" is asserted on latents, pixels are "PSNR-equivalent"
TOL_PIXELS = 1.2e-3
TOL_PSNR_DB = 68.0


def _build(cfg, gpu, salt=0):
    from gcd_amd.video_model import VideoUNet
    with torch.device("meta"):
        net = VideoUNet(**cfg.as_reference_kwargs())
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    sd = weights.synth_state_dict(shapes, salt)
    net = net.to_empty(device=gpu)
    net.load_state_dict(sd)
    return net.eval(), sd


def _unet_inputs(cfg, T, h, w, seed):
    noise, c, uc = weights.synth_inputs(1, T, h, w, cfg.context_dim,
                                        cfg.adm_in_channels + cfg.aux_emb_dim, seed)
    x = torch.cat([torch.cat([noise, uc["concat"]], 1), torch.cat([noise, c["concat"]], 1)])
    ts = torch.linspace(-1.5, 1.63, 2 * T)
    return (x, ts, torch.cat([uc["crossattn"], c["crossattn"]]),
            torch.cat([uc["vector"], c["vector"]]), torch.zeros(2, T))


@pytest.fixture(scope="module")
def tiny(gpu):
    return _build(O.TINY, gpu)


def test_unet_forward_vs_reference_golden(gpu, tiny):
    """Same inputs / weights as the fixture made by the reference modules (oracle/make_golden.py)."""
    net, sd = tiny
    g = torch.load(GOLD / "unet_tiny.pt")
    x, ts, ctx, y, ioi = _unet_inputs(O.TINY, g["T"], g["h"], g["w"], g["input_seed"])
    net.engine.taps = {}
    out = net(x.to(gpu), ts.to(gpu), context=ctx.to(gpu), y=y.to(gpu), num_video_frames=g["T"],
              image_only_indicator=ioi.to(gpu))
    torch.cuda.synchronize()
    taps, net.engine.taps = net.engine.taps, None
    errs = {}
    for k, v in taps.items():
        f = v.reshape(-1).cpu()
        idx = torch.linspace(0, f.numel() - 1, min(4096, f.numel())).long()
        errs[k] = rel_l2(f[idx], g["tap_samples"][k])
    worst = max(errs, key=errs.get)
    print("per-block rel-L2:", {k: f"{e:.2e}" for k, e in errs.items()})
    assert set(taps) == set(g["tap_samples"])
    assert errs[worst] < TOL_FWD, f"block {worst}: rel-L2 {errs[worst]:.3e}"
    e = rel_l2(out, g["out"])
    assert out.shape == g["out"].shape and out.dtype == torch.float32
    assert e < TOL_FWD, f"UNet forward vs reference golden: rel-L2 {e:.3e}"


# (fixture, bar): see oracle/make_golden_stress.py for what each stresses and what was measured (round 5:
# 1.64e-3 and 5.2e-3; the second is operand rounding no longer diluted by the residual, not a range effect).
# Round 6: the range fixture's bar is no longer a number chosen after the result — it is where the UNMODIFIED reference
# itself lands on this fixture under its own inference arithmetic (fp16 torch.autocast, scripts/eval_utils.py:181-186)
# against its fp32 run: tests/golden/autocast_bars.json (oracle/make_autocast_bars.py), 8.02e-3.  The HIP path must not
# be further from the fp32 reference than the reference's own fp16 path is.
def _reference_fp16_autocast_error(fixture):
    import json
    bars = json.loads((GOLD / "autocast_bars.json").read_text())["tiny_forward_reference_autocast_vs_own_fp32"]
    return bars["fixtures"][fixture]["float16"]["output_rel_l2"]


@pytest.mark.parametrize("fixture,bar", [("unet_tiny_heavy.pt", TOL_FWD), ("unet_tiny_geglu_range.pt", None)])
def test_unet_forward_stress_weights_vs_reference_golden(gpu, fixture, bar):
    """fp16 OPERAND stress against the UNMODIFIED reference's fp32 forward (oracle/make_golden_stress.py).
    `unet_tiny_heavy`: Student-t (nu = 3) weights — single weights tens of sigma out — must stay inside the forward bar.
    `unet_tiny_geglu_range`: additionally the GEGLU projections scaled until the hidden tensor value * gelu(gate), which
    this path keeps in fp16 (a plain round-to-nearest conversion in the epilogue: NOT clamped, +-inf from 65520 on, pinned
    by tests/test_conditioning_gpu.py), peaks at 48 % of that range: the forward must stay finite, must not have
    overflowed (no block may jump), and — with every FeedForward now ~500x the residual it lands
    on, so that nothing dilutes the fp16 operand rounding of 48 FeedForwards — stay below 8e-3 (measured 5.2e-3; 4.9e-3
    already at gain 6 where the range plays no role)."""
    from gcd_amd.video_model import VideoUNet
    g = torch.load(GOLD / fixture)
    ref16 = _reference_fp16_autocast_error(fixture)
    if bar is None:
        bar = ref16
    with torch.device("meta"):
        net = VideoUNet(**O.TINY.as_reference_kwargs())
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net = net.to_empty(device=gpu)
    net.load_state_dict(weights.synth_state_dict_heavy(shapes, g["salt"], g["nu"], g["geglu_gain"]))
    net.eval()
    x, ts, ctx, y, ioi = _unet_inputs(O.TINY, g["T"], g["h"], g["w"], g["input_seed"])
    net.engine.taps = {}
    out = net(x.to(gpu), ts.to(gpu), context=ctx.to(gpu), y=y.to(gpu), num_video_frames=g["T"],
              image_only_indicator=ioi.to(gpu))
    torch.cuda.synchronize()
    taps, net.engine.taps = net.engine.taps, None
    assert torch.isfinite(out).all(), "non-finite output under stress weights"
    errs = {}
    for k, v in taps.items():
        assert torch.isfinite(v).all(), k
        f = v.reshape(-1).cpu()
        idx = torch.linspace(0, f.numel() - 1, min(4096, f.numel())).long()
        errs[k] = rel_l2(f[idx], g["tap_samples"][k])
    worst = max(errs, key=errs.get)
    e = rel_l2(out, g["out"])
    print(f"{fixture} (GEGLU hidden peaks at {g['geglu_hidden_absmax']:.0f}): output rel-L2 {e:.3e}, "
          f"worst block {worst} {errs[worst]:.3e}; the reference's own fp16 autocast on this fixture: {ref16:.3e}")
    assert e < ref16, "further from the fp32 reference than the reference's own fp16-autocast forward"
    assert set(taps) == set(g["tap_samples"])
    assert errs[worst] < bar and e < bar, f"rel-L2 {e:.3e}, block {worst} {errs[worst]:.3e}"
    del net
    torch.cuda.empty_cache()


@pytest.mark.parametrize("T,h,w,seed", [(14, 16, 16, 21), (2, 8, 24, 22), (1, 8, 8, 23), (16, 8, 8, 24)])
def test_unet_forward_vs_oracle_shapes(gpu, tiny, T, h, w, seed):
    """T = 14 (GCD), ragged aspect, single frame, maximum T of the temporal kernel."""
    net, sd = tiny
    x, ts, ctx, y, ioi = _unet_inputs(O.TINY, T, h, w, seed)
    with torch.no_grad():
        ref = O.unet_forward(sd, O.TINY, x, ts, ctx, y, T, ioi)
    out = net(x.to(gpu), ts.to(gpu), context=ctx.to(gpu), y=y.to(gpu), num_video_frames=T,
              image_only_indicator=ioi.to(gpu))
    e = rel_l2(out, ref)
    assert e < TOL_FWD, f"T={T} {h}x{w}: rel-L2 {e:.3e}"


def test_unet_image_only_indicator_and_repeatability(gpu, tiny):
    net, sd = tiny
    T, h, w = 4, 8, 8
    x, ts, ctx, y, ioi = _unet_inputs(O.TINY, T, h, w, 31)
    ioi[0, 1] = 1.0
    ioi[1, 3] = 1.0
    with torch.no_grad():
        ref = O.unet_forward(sd, O.TINY, x, ts, ctx, y, T, ioi)
    args = (x.to(gpu), ts.to(gpu))
    kw = dict(context=ctx.to(gpu), y=y.to(gpu), num_video_frames=T, image_only_indicator=ioi.to(gpu))
    out1 = net(*args, **kw)
    out2 = net(*args, **kw)
    assert rel_l2(out1, ref) < TOL_FWD
    assert torch.equal(out1, out2), "forward is not bit-reproducible run to run"


@pytest.mark.parametrize("force_tiles", [False, True])
def test_unet_walk_directions_are_bit_identical(gpu, tiny, monkeypatch, force_tiles):
    """The zig-zag schedule (engine._ZIGZAG: reversed tile walks of the GEMMs, walk orders of LayerNorm / GroupNorm
    apply) is scheduling only: every mode returns the bits of mode 0 — with the automatic kernel choice and with the
    256 x 320 tile kernels (the ones that honour gcd_gemm_desc.sched) forced on every GEMM."""
    from gcd_amd import engine, ops
    net, sd = tiny
    T, h, w = 14, 16, 16
    x, ts, ctx, y, ioi = _unet_inputs(O.TINY, T, h, w, 41)
    args = (x.to(gpu), ts.to(gpu))
    kw = dict(context=ctx.to(gpu), y=y.to(gpu), num_video_frames=T, image_only_indicator=ioi.to(gpu))
    if force_tiles:
        ops.tune_set(ops.TUNE_GEMM_IMPL, 2)
    try:
        outs = []
        for mode in range(5):
            monkeypatch.setattr(engine, "_ZIGZAG", mode)
            outs.append(net(*args, **kw).clone())
        torch.cuda.synchronize()
    finally:
        ops.tune_set(ops.TUNE_GEMM_IMPL, 0)
    assert torch.isfinite(outs[0]).all()
    for mode in range(1, 5):
        assert torch.equal(outs[mode], outs[0]), f"GCD_ZIGZAG={mode} changed the result"


def test_cross_attention_cache_survives_address_reuse(gpu, tiny):
    """The collapsed cross-attention vectors are cached per context TENSOR OBJECT.  A new clip's
    context that the allocator places at the freed address of the previous one (same shape, same
    version counter) must not be served the previous clip's vectors."""
    net, sd = tiny
    T, h, w = 4, 8, 8
    x, ts, ctx_a, y, ioi = _unet_inputs(O.TINY, T, h, w, 33)
    ctx_b = torch.randn(ctx_a.shape, generator=torch.Generator().manual_seed(34)) * 2.0
    kw = dict(y=y.to(gpu), num_video_frames=T, image_only_indicator=ioi.to(gpu))
    xg, tg = x.to(gpu), ts.to(gpu)
    ca = ctx_a.to(gpu)
    ptr = ca.data_ptr()
    out_a = net(xg, tg, context=ca, **kw)
    out_a2 = net(xg, tg, context=ca, **kw)                 # same object: cache hit, same result
    assert torch.equal(out_a, out_a2)
    del ca
    cb = ctx_b.to(gpu)                                      # usually lands on the freed block
    reused = cb.data_ptr() == ptr
    out_b = net(xg, tg, context=cb, **kw)
    with torch.no_grad():
        ref_b = O.unet_forward(sd, O.TINY, x, ts, ctx_b, y, T, ioi)
    print(f"address reused: {reused}; rel-L2 vs oracle {rel_l2(out_b, ref_b):.3e}")
    assert rel_l2(out_b, ref_b) < TOL_FWD and rel_l2(out_b, out_a) > 1e-2
    cb.mul_(0.5)                                            # in-place edit: version bump -> miss
    out_c = net(xg, tg, context=cb, **kw)
    with torch.no_grad():
        ref_c = O.unet_forward(sd, O.TINY, x, ts, ctx_b * 0.5, y, T, ioi)
    assert rel_l2(out_c, ref_c) < TOL_FWD


def test_unet_rejects_bad_inputs(gpu, tiny):
    net, _ = tiny
    x, ts, ctx, y, ioi = _unet_inputs(O.TINY, 2, 8, 8, 41)
    with pytest.raises(Exception):     # CPU tensors: no CPU path
        net(x, ts, context=ctx, y=y, num_video_frames=2, image_only_indicator=ioi)
    with pytest.raises(NotImplementedError):   # multi-token context is outside the SVD family
        net(x.to(gpu), ts.to(gpu), context=ctx.repeat(1, 2, 1).to(gpu), y=y.to(gpu),
            num_video_frames=2, image_only_indicator=ioi.to(gpu))
    with pytest.raises(AssertionError):        # y width must be adm + aux (video_model.py:494)
        net(x.to(gpu), ts.to(gpu), context=ctx.to(gpu), y=y[:, :-1].to(gpu), num_video_frames=2,
            image_only_indicator=ioi.to(gpu))
    with pytest.raises(ValueError):            # latent size must survive 3 downsamples
        net(x[..., :6].to(gpu), ts.to(gpu), context=ctx.to(gpu), y=y.to(gpu), num_video_frames=2,
            image_only_indicator=ioi.to(gpu))


def test_state_dict_roundtrip_and_repack(gpu, tiny):
    """load_state_dict with reference key names re-packs the fp16 operands."""
    net, sd = tiny
    x, ts, ctx, y, ioi = _unet_inputs(O.TINY, 2, 8, 8, 51)
    kw = dict(context=ctx.to(gpu), y=y.to(gpu), num_video_frames=2, image_only_indicator=ioi.to(gpu))
    out_a = net(x.to(gpu), ts.to(gpu), **kw)
    g = torch.load(GOLD / "unet_tiny.pt")
    sd2 = weights.synth_state_dict(g["state_dict_shapes"], salt=5)
    net.load_state_dict(sd2)
    with torch.no_grad():
        ref = O.unet_forward(sd2, O.TINY, x, ts, ctx, y, 2, ioi)
    out_b = net(x.to(gpu), ts.to(gpu), **kw)
    assert rel_l2(out_b, ref) < TOL_FWD and rel_l2(out_b, out_a) > 0.1
    net.load_state_dict(sd)            # restore for the other tests
    assert set(net.state_dict().keys()) == set(g["state_dict_shapes"].keys())


def _sampler(T, steps, device):
    from gcd_amd.sampling import EulerEDMSampler
    return EulerEDMSampler(
        discretization_config={"target": "gcd_amd.discretizer.EDMDiscretization",
                               "params": {"sigma_max": 700.0}},
        num_steps=steps,
        guider_config={"target": "gcd_amd.guiders.LinearPredictionGuider",
                       "params": {"num_frames": T, "max_scale": 1.5, "min_scale": 1.0}},
        device=device)


def _stack(net, T, gpu, clips=1):
    from gcd_amd.denoiser import Denoiser
    from gcd_amd.sampling import FusedDenoiser
    from gcd_amd.wrappers import OpenAIWrapper
    den = Denoiser({"target": "gcd_amd.denoiser_scaling.VScalingWithEDMcNoise"})
    model = OpenAIWrapper(net)
    extra = {"num_video_frames": T, "image_only_indicator": torch.zeros(2 * clips, T, device=gpu)}
    return den, model, extra, FusedDenoiser(den, model, **extra)


def test_sampler_vs_reference_golden(gpu, tiny):
    """5 EulerEDM steps through the plugin stack: generic closure path, fused eager, fused graph."""
    net, sd = tiny
    g = torch.load(GOLD / "sampler_tiny.pt")
    T, steps = g["T"], g["steps"]
    noise, c, uc = weights.synth_inputs(1, T, g["h"], g["w"], O.TINY.context_dim,
                                        O.TINY.adm_in_channels + O.TINY.aux_emb_dim, g["input_seed"])
    cg = {k: v.to(gpu) for k, v in c.items()}
    ucg = {k: v.to(gpu) for k, v in uc.items()}
    den, model, extra, fused = _stack(net, T, gpu)
    sampler = _sampler(T, steps, "cuda")

    def closure(inp, sigma, cc):           # what DiffusionEngine.sample_video builds
        return den(model, inp, sigma, cc, **extra)

    class Opaque:                          # a callable the sampler cannot see into: generic path
        def __call__(self, inp, sigma, cc):
            return den(model, inp, sigma, cc, **extra)

    out_generic = sampler(Opaque(), noise.clone().to(gpu), cond=cg, uc=ucg)
    assert sampler.last_path == "generic"
    out_closure = sampler(closure, noise.clone().to(gpu), cond=cg, uc=ucg)
    assert sampler.last_path == "fused", "the sample_video-style closure must reach the fused loop"
    sampler.use_graph = False
    out_fused = sampler(fused, noise.clone().to(gpu), cond=cg, uc=ucg)
    assert sampler.last_path == "fused"
    sampler.use_graph = True
    out_graph = sampler(fused, noise.clone().to(gpu), cond=cg, uc=ucg)
    torch.cuda.synchronize()
    # 5 steps on 4 frames of 8x8 latents: each step weighs far more than in the 25-step GCD loop
    # (test_sampler_25_steps_T14_vs_oracle holds the 1e-3 contract), so allow 1.5e-3 here
    for name, o in [("generic", out_generic), ("fused", out_fused), ("graph", out_graph)]:
        e = rel_l2(o, g["final"])
        print(f"sampler {name}: rel-L2 vs reference golden {e:.3e}")
        assert e < 1.5 * TOL_LOOP, f"{name}: {e:.3e}"
    assert torch.equal(out_fused, out_graph), "hipGraph replay differs from eager launches"
    assert torch.equal(out_closure, out_graph), "closure-recovered fused path differs from FusedDenoiser"
    # the two paths differ by ~1 ulp in c_in / c_noise; fp16 operand quantisation decorrelates the
    # rounding noise within a few layers, so they agree to the noise level, not to the ulp
    assert rel_l2(out_fused, out_generic) < 1.5 * TOL_LOOP


def test_sampler_25_steps_T14_vs_oracle(gpu, tiny):
    """The GCD configuration of the loop (25 steps, 14 frames, CFG 1.0 -> 1.5) at 16x16 latents."""
    net, sd = tiny
    T, steps, h, w = 14, 25, 16, 16
    noise, c, uc = weights.synth_inputs(1, T, h, w, O.TINY.context_dim,
                                        O.TINY.adm_in_channels + O.TINY.aux_emb_dim, 61)
    trace = []
    with torch.no_grad():
        ref = O.sample_loop(sd, O.TINY, noise, c, uc, T, steps, trace=trace)
    den, model, extra, fused = _stack(net, T, gpu)
    sampler = _sampler(T, steps, "cuda")
    out = sampler(fused, noise.clone().to(gpu), cond={k: v.to(gpu) for k, v in c.items()},
                  uc={k: v.to(gpu) for k, v in uc.items()})
    e = rel_l2(out, ref)
    print(f"25-step loop rel-L2 {e:.3e}")
    assert sampler.last_path == "fused" and e < TOL_LOOP, f"25-step loop: rel-L2 {e:.3e}"


def test_unet_full_width_kubric_and_pardom(gpu):
    """The real 1.5 B-parameter topology (320 base channels) at 14 x 16 x 16 latents, Kubric (camera
    pose via aux_label_emb) and ParDom (no aux) variants, against the oracle on host cores."""
    for cfg, salt in ((O.KUBRIC, 2), (O.PARDOM, 3)):
        net, sd = _build(cfg, gpu, salt)
        T, h, w = 14, 16, 16
        x, ts, ctx, y, ioi = _unet_inputs(cfg, T, h, w, 71)
        with torch.no_grad():
            ref = O.unet_forward(sd, cfg, x, ts, ctx, y, T, ioi)
        out = net(x.to(gpu), ts.to(gpu), context=ctx.to(gpu), y=y.to(gpu), num_video_frames=T,
                  image_only_indicator=ioi.to(gpu))
        e = rel_l2(out, ref)
        print(f"full width aux={cfg.aux_emb_dim}: rel-L2 {e:.3e}, ws {net.engine.ws.nbytes() / 2**20:.0f} MiB")
        assert e < TOL_FWD, f"full-width UNet (aux={cfg.aux_emb_dim}): rel-L2 {e:.3e}"
        del net, sd
        torch.cuda.empty_cache()


def test_sampler_25_steps_full_width_vs_oracle(gpu):
    """The contract at the real width: the 1.5 B-parameter Kubric VideoUNet, 25 EulerEDM steps with
    CFG on a 14-frame clip (16x16 latents so that the fp32 CPU oracle finishes in ~2 minutes),
    final latents within 1e-3 rel-L2 of the oracle."""
    net, sd = _build(O.KUBRIC, gpu, salt=2)
    T, steps, h, w = 14, 25, 16, 16
    noise, c, uc = weights.synth_inputs(1, T, h, w, O.KUBRIC.context_dim,
                                        O.KUBRIC.adm_in_channels + O.KUBRIC.aux_emb_dim, 91)
    torch.set_num_threads(min(32, torch.get_num_threads()))
    with torch.no_grad():
        ref = O.sample_loop(sd, O.KUBRIC, noise, c, uc, T, steps)
    den, model, extra, fused = _stack(net, T, gpu)
    sampler = _sampler(T, steps, "cuda")
    out = sampler(fused, noise.clone().to(gpu), cond={k: v.to(gpu) for k, v in c.items()},
                  uc={k: v.to(gpu) for k, v in uc.items()})
    e = rel_l2(out, ref)
    print(f"full-width 25-step loop rel-L2 {e:.3e}")
    assert sampler.last_path == "fused" and e < TOL_LOOP, f"full-width 25-step loop: rel-L2 {e:.3e}"


# ------------------------------------------------------------------------------------------------
# the metric's own shapes (BASELINE.json cfg0 / cfg1 / cfg3) against goldens made by the reference
# modules in the build container (oracle/make_golden_fullres.py, oracle/make_golden_cfg3.py)
# ------------------------------------------------------------------------------------------------
def _sample64(t, n=4096):
    f = t.reshape(-1)
    idx = torch.linspace(0, f.numel() - 1, min(n, f.numel()), dtype=torch.float64).long()
    return f[idx.to(f.device)].cpu()


@pytest.fixture(scope="module")
def kubric_full(gpu):
    net, sd = _build(O.KUBRIC, gpu, salt=2)
    yield net
    del net
    torch.cuda.empty_cache()


def test_unet_forward_72x128_full_width_vs_reference_golden(gpu, kubric_full):
    """cfg1's shape: the 1.53 B-parameter Kubric VideoUNet on N = 28 frames of 72 x 128 latents
    (S = 9216 attention, 1008-tile persistent GEMMs, the 4.5 GiB slab pool) against strided samples
    of the reference modules' own forward (185 s on the CPU), output and every block."""
    net = kubric_full
    g = torch.load(GOLD / "unet_kubric_72x128.pt")
    T, h, w = g["T"], g["h"], g["w"]
    x, ts, ctx, y, ioi = _unet_inputs(O.KUBRIC, T, h, w, g["input_seed"])
    net.engine.taps = {}
    out = net(x.to(gpu), ts.to(gpu), context=ctx.to(gpu), y=y.to(gpu), num_video_frames=T,
              image_only_indicator=ioi.to(gpu))
    torch.cuda.synchronize()
    taps, net.engine.taps = net.engine.taps, None
    assert tuple(out.shape) == tuple(g["out_shape"]) and set(taps) == set(g["tap_samples"])
    errs = {}
    for k, v in taps.items():
        assert tuple(v.shape) == tuple(g["tap_shapes"][k]), k
        errs[k] = rel_l2(_sample64(v), g["tap_samples"][k])
        nrm = float(v.double().norm())
        assert abs(nrm / g["tap_norms"][k] - 1.0) < 2e-3, f"{k}: norm {nrm} vs {g['tap_norms'][k]}"
    taps.clear()
    worst = max(errs, key=errs.get)
    print("72x128 per-block rel-L2:", {k: f"{e:.2e}" for k, e in errs.items()})
    assert errs[worst] < TOL_FWD, f"block {worst}: rel-L2 {errs[worst]:.3e}"
    e = rel_l2(_sample64(out, 65536), g["out_samples"])
    nrm = float(out.double().norm())
    print(f"72x128 full-width forward: rel-L2 {e:.3e} on 65536 samples, norm {nrm:.4f} vs {g['out_norm']:.4f}")
    assert e < TOL_FWD, f"UNet forward at 28x72x128 vs reference golden: rel-L2 {e:.3e}"
    assert abs(nrm / g["out_norm"] - 1.0) < 2e-3


def test_sampler_step_32x32_cfg0_vs_reference_golden(gpu, kubric_full):
    """BASELINE.json cfg0: one EulerEDM sampler_step of the full-width network on a 14 x 32 x 32 x 4
    latent, at the first step's noise level and a mid-schedule one, generic and fused paths, against
    the reference plugin stack's own result."""
    net = kubric_full
    g = torch.load(GOLD / "step_kubric_32x32.pt")
    T, h, w = g["T"], g["h"], g["w"]
    noise, c, uc = weights.synth_inputs(1, T, h, w, O.KUBRIC.context_dim,
                                        O.KUBRIC.adm_in_channels + O.KUBRIC.aux_emb_dim, g["input_seed"])
    cg = {k: v.to(gpu) for k, v in c.items()}
    ucg = {k: v.to(gpu) for k, v in uc.items()}
    den, model, extra, fused = _stack(net, T, gpu)
    sampler = _sampler(T, 25, "cuda")
    from gcd_amd.sampling import FusedEulerLoop
    for st in g["steps"]:
        sig, nxt = st["sigma"], st["next_sigma"]
        x = (noise * (1.0 + sig ** 2) ** 0.5).to(gpu)
        s_in = x.new_ones([x.shape[0]])
        out_gen = sampler.sampler_step(s_in * sig, s_in * nxt, fused, x, cg, ucg)
        loop = FusedEulerLoop(sampler, fused, noise.clone().to(gpu), cg, ucg)
        with loop:
            loop.x.copy_(x)
            loop.sig.copy_(torch.tensor([sig, nxt], device=gpu))
            loop.launch_step()
        loop.close()
        # x_next = x + (s'/s - 1) (x - D): remove the part carried by x itself so the figure measures D
        carried = (x * (nxt / sig)).cpu()
        ref_d = st["x_next"] - carried
        for name, o in (("generic", out_gen), ("fused", loop.x)):
            e_x = rel_l2(o, st["x_next"])
            e_d = rel_l2(o.cpu() - carried, ref_d)
            print(f"cfg0 step sigma {sig}->{nxt} [{name}]: rel-L2 x_next {e_x:.3e}, denoised part {e_d:.3e}")
            assert e_x < TOL_LOOP, f"{name} sigma {sig}: x_next rel-L2 {e_x:.3e}"
            # D = CFG mix of two forwards (x_u + s (x_c - x_u), s up to 1.5): ~1.3-1.6x one forward's error
            assert e_d < 2 * TOL_FWD, f"{name} sigma {sig}: denoised-part rel-L2 {e_d:.3e}"


def test_sampler_50_steps_pardom_cfg3_vs_reference_golden(gpu):
    """BASELINE.json cfg3: the ParDom network (no aux_label_emb, y 768 wide), the full 50-step
    EulerEDM loop with CFG on 14 frames, against the reference plugin stack's own trajectory."""
    g = torch.load(GOLD / "sampler_pardom_50.pt")
    net, sd = _build(O.PARDOM, gpu, salt=g["salt"])
    T, steps, h, w = g["T"], g["steps"], g["h"], g["w"]
    noise, c, uc = weights.synth_inputs(1, T, h, w, O.PARDOM.context_dim,
                                        O.PARDOM.adm_in_channels + O.PARDOM.aux_emb_dim, g["input_seed"])
    den, model, extra, fused = _stack(net, T, gpu)
    sampler = _sampler(T, steps, "cuda")
    from gcd_amd.sampling import FusedEulerLoop
    loop = FusedEulerLoop(sampler, fused, noise.clone().to(gpu),
                          {k: v.to(gpu) for k, v in c.items()}, {k: v.to(gpu) for k, v in uc.items()})
    assert loop.num_steps == 50
    errs = {}
    with loop:
        for i in range(loop.num_steps):
            loop.step(i)
            if i + 1 in g["trace"]:
                loop.side.synchronize()
                errs[i + 1] = rel_l2(loop.x, g["trace"][i + 1])
    loop.close()
    e = rel_l2(loop.x, g["final"])
    print("cfg3 trajectory rel-L2:", {k: f"{v:.2e}" for k, v in errs.items()}, f"final {e:.3e}")
    assert max(errs.values()) < TOL_LOOP and e < TOL_LOOP, f"50-step ParDom loop: rel-L2 {e:.3e}"
    del net
    torch.cuda.empty_cache()


def _loop_vs_reference_golden(gpu, fname):
    """Run the fused EulerEDM + CFG loop on the inputs of a oracle/make_golden_loop72.py fixture and compare x after
    the kept steps (65 536 strided samples each) and the full final latents.  Returns (errors per step, final error,
    final latents, golden)."""
    from oracle.make_golden_fullres import sample
    from gcd_amd.sampling import FusedEulerLoop
    path = GOLD / fname
    if not path.exists():
        pytest.skip(f"tests/golden/{fname} has not been generated (python -m oracle.make_golden_loop72)")
    g = torch.load(path)
    cfg = getattr(O, g["config"])
    net, sd = _build(cfg, gpu, salt=g["salt"])
    del sd
    T, steps, h, w, first = g["T"], g["steps"], g["h"], g["w"], g["first_step"]
    clips = g.get("clips", 1)     # num_samples: several clips in ONE sampler call (scripts/test.py:326)
    noise, c, uc = weights.synth_inputs(clips, T, h, w, cfg.context_dim, cfg.adm_in_channels + cfg.aux_emb_dim,
                                        g["input_seed"])
    den, model, extra, fused = _stack(net, T, gpu, clips)
    sampler = _sampler(T, steps, "cuda")
    loop = FusedEulerLoop(sampler, fused, noise.clone().to(gpu),
                          {k: v.to(gpu) for k, v in c.items()}, {k: v.to(gpu) for k, v in uc.items()})
    assert loop.num_steps == steps
    assert torch.allclose(loop.sigmas.cpu(), g["sigmas"], rtol=1e-6, atol=0)
    if first:    # the fixture's seeded mid-trajectory state: x = n * sqrt(1 + sigma_first^2)
        loop.x.copy_((noise * float((1.0 + g["sigmas"][first] ** 2) ** 0.5)).to(gpu))
    errs = {}
    with loop:
        for i in range(first, steps):
            loop.step(i)
            if i + 1 in g["trace"]:
                loop.side.synchronize()
                errs[i + 1] = rel_l2(sample(loop.x.cpu(), 65536), g["trace"][i + 1]["samples"])
                nr = float(loop.x.double().norm()) / g["trace"][i + 1]["norm"]
                assert abs(nr - 1.0) < 1e-3, f"step {i + 1}: norm ratio {nr}"
    loop.close()
    e = rel_l2(loop.x, g["final"])
    z = loop.x.clone()
    del net, loop
    torch.cuda.empty_cache()
    return errs, e, z, g


def test_sampler_25_steps_72x128_cfg1_vs_reference_golden(gpu):
    """BASELINE.json cfg1 AT THE METRIC'S OWN RESOLUTION: the full 25-step EulerEDM + CFG loop of the full-width
    Kubric network on a 14 x 72 x 128 latent clip against the unmodified reference plugin stack's own fp32
    trajectory (oracle/make_golden_loop72.py cfg1; ~2 h of CPU time once): every sampled step and the final
    latents within the loop contract of 1e-3 rel-L2, then frames decoded from both by the HIP VideoDecoder at
    576 x 1024 compared by PSNR."""
    errs, e, z, g = _loop_vs_reference_golden(gpu, "loop_kubric_72x128.pt")
    print("cfg1 72x128 trajectory rel-L2:", {k: f"{v:.2e}" for k, v in errs.items()}, f"final {e:.3e}")
    assert max(errs.values()) < TOL_LOOP and e < TOL_LOOP, f"25-step loop at 72x128: rel-L2 {e:.3e}"
    # decoded frames at 576 x 1024 through the HIP first-stage decoder (full 128-channel VideoDecoder, procedural
    # weights) against (a) the frames the UNMODIFIED reference VideoDecoder made from the reference loop's own final
    # latents (oracle/make_golden_decoder72.py: the reference stack end to end, loop + decode) and (b) the HIP
    # decoder on the reference's latents (what the latent error alone is in pixels)
    import math
    from gcd_amd.first_stage import decode_first_stage
    from gcd_amd.temporal_ae import VideoDecoder
    from oracle import vae_decoder_ref as D
    from oracle.make_golden_fullres import sample
    with torch.device("meta"):
        dec = VideoDecoder(**D.KUBRIC.as_reference_kwargs())
    sdd = weights.synth_state_dict({k: tuple(v.shape) for k, v in dec.state_dict().items()}, salt=1)
    dec = dec.to_empty(device=gpu)
    dec.load_state_dict(sdd)
    dec.eval()
    frames = decode_first_stage(dec, z, 0.18215, en_and_decode_n_samples_a_time=14).cpu()
    assert frames.shape == (14, 3, 576, 1024)
    gd_path = GOLD / "decoder_kubric_72x128.pt"
    if gd_path.exists():
        gd = torch.load(gd_path)
        got = sample(frames, gd["out_samples"].numel())
        mse = float(((got.double() - gd["out_samples"].double()) ** 2).mean())
        psnr_ref = 10.0 * math.log10(4.0 / max(mse, 1e-30))
        e_px = rel_l2(got, gd['out_samples'])
        print(f"576x1024 frames, HIP loop + HIP decoder vs REFERENCE loop + REFERENCE decoder: rel-L2 "
              f"{e_px:.3e}, PSNR {psnr_ref:.1f} dB on the [-1, 1] range")
        # What is claimed: the 1e-3 rel-L2 contract is held on the LATENTS the loop returns (asserted
        # above); decoded PIXELS are held to "PSNR-equivalent" — the VAE decoder amplifies the 6.7e-4 latent error
        # ~1.65x, measured 1.07e-3 rel-L2 / 70.4 dB (procedural weights) — with these bars:
        assert psnr_ref >= TOL_PSNR_DB, f"decoded frames: PSNR {psnr_ref:.1f} dB"
        assert e_px < TOL_PIXELS, f"decoded frames: rel-L2 {e_px:.3e}"
    frames_ref = decode_first_stage(dec, g["final"].to(gpu), 0.18215, en_and_decode_n_samples_a_time=14).cpu()
    mse = float(((frames.double() - frames_ref.double()) ** 2).mean())
    psnr = 10.0 * math.log10(4.0 / max(mse, 1e-30))
    print(f"576x1024 frames, latent error alone (HIP decoder on both): rel-L2 {rel_l2(frames, frames_ref):.3e}, "
          f"PSNR {psnr:.1f} dB")
    assert psnr >= TOL_PSNR_DB and rel_l2(frames, frames_ref) < TOL_PIXELS
    del dec
    torch.cuda.empty_cache()


def test_sampler_25_steps_two_clips_40x64_cfg1_vs_reference_golden(gpu):
    """num_samples = 2 (scripts/test.py:326): TWO clips in one sampler call (28 frames, 56 under CFG), the full 25-step
    loop of the full-width Kubric network at 40 x 64 latents against the UNMODIFIED reference plugin stack's own
    trajectory (oracle/make_golden_loop72.py cfg1b2mid) under the 1e-3 loop contract."""
    errs, e, z, g = _loop_vs_reference_golden(gpu, "loop_kubric_b2_40x64.pt")
    print("cfg1 B=2 40x64 trajectory rel-L2:", {k: f"{v:.2e}" for k, v in errs.items()}, f"final {e:.3e}")
    assert z.shape[0] == 28 and max(errs.values()) < TOL_LOOP and e < TOL_LOOP, f"B=2 25-step loop: rel-L2 {e:.3e}"


def test_sampler_25_steps_two_clips_72x128_cfg1_vs_reference_golden(gpu):
    """The same at the metric's own resolution (cfg1b2; skips until that ~4 h fixture has been generated)."""
    errs, e, z, g = _loop_vs_reference_golden(gpu, "loop_kubric_b2_72x128.pt")
    print("cfg1 B=2 72x128 trajectory rel-L2:", {k: f"{v:.2e}" for k, v in errs.items()}, f"final {e:.3e}")
    assert z.shape[0] == 28 and max(errs.values()) < TOL_LOOP and e < TOL_LOOP, f"B=2 25-step loop: rel-L2 {e:.3e}"


def test_sampler_50_steps_40x64_pardom_cfg3_vs_reference_golden(gpu):
    """BASELINE.json cfg3: the ParDom network's full 50-step loop at 14 x 40 x 64 against the reference stack."""
    errs, e, z, g = _loop_vs_reference_golden(gpu, "loop_pardom_40x64.pt")
    print("cfg3 40x64 trajectory rel-L2:", {k: f"{v:.2e}" for k, v in errs.items()}, f"final {e:.3e}")
    assert max(errs.values()) < TOL_LOOP and e < TOL_LOOP, f"50-step ParDom loop at 40x64: rel-L2 {e:.3e}"


def test_sampler_50_steps_72x128_pardom_cfg3_vs_reference_golden(gpu):
    """BASELINE.json cfg3 IN FULL at the metric's own resolution: the ParDom network's whole 50-step EulerEDM + CFG loop
    on a 14 x 72 x 128 latent clip against the unmodified reference stack (oracle/make_golden_loop72.py cfg3; ~3 h of
    CPU time once)."""
    errs, e, z, g = _loop_vs_reference_golden(gpu, "loop_pardom_72x128.pt")
    print("cfg3 72x128 trajectory rel-L2:", {k: f"{v:.2e}" for k, v in errs.items()}, f"final {e:.3e}")
    assert max(errs.values()) < TOL_LOOP and e < TOL_LOOP, f"50-step ParDom loop at 72x128: rel-L2 {e:.3e}"


def test_sampler_last_15_of_50_steps_72x128_pardom_cfg3_vs_reference_golden(gpu):
    """cfg3 at 14 x 72 x 128: the last 15 of the 50 steps (sigma_35 = 1.17 ... 0), where the network term carries the
    result, from the fixture's seeded mid-trajectory state, against the reference stack."""
    errs, e, z, g = _loop_vs_reference_golden(gpu, "loop_pardom_72x128_tail.pt")
    print("cfg3 72x128 tail rel-L2:", {k: f"{v:.2e}" for k, v in errs.items()}, f"final {e:.3e}")
    assert max(errs.values()) < TOL_LOOP and e < TOL_LOOP, f"ParDom 72x128 tail: rel-L2 {e:.3e}"


def test_two_clips_batched_with_image_only_indicator(gpu, tiny):
    """num_samples / batched clips: B = 2 clips in one call (56 frames under CFG: per-clip time_stack
    GroupNorm, per-clip first-frame temporal context, > 32 rows through the small-M kernel), with a
    non-zero image_only_indicator (4, 14) — UNet forward and the fused loop vs the oracle: 5 steps (short loop, relaxed
    bar) and the full 25 steps under the 1e-3 contract."""
    net, sd = tiny
    T, h, w, B = 14, 8, 8, 2
    cfg = O.TINY
    noise, c, uc = weights.synth_inputs(B, T, h, w, cfg.context_dim, cfg.adm_in_channels + cfg.aux_emb_dim, 77)
    ioi = torch.zeros(2 * B, T)
    ioi[0, 3] = ioi[1, 0] = ioi[2, 13] = ioi[3, 5] = ioi[3, 6] = 1.0
    x = torch.cat([torch.cat([noise, uc["concat"]], 1), torch.cat([noise, c["concat"]], 1)])
    ts = torch.linspace(-1.2, 1.4, 2 * B * T)
    ctx = torch.cat([uc["crossattn"], c["crossattn"]])
    y = torch.cat([uc["vector"], c["vector"]])
    with torch.no_grad():
        ref = O.unet_forward(sd, cfg, x, ts, ctx, y, T, ioi)
    out = net(x.to(gpu), ts.to(gpu), context=ctx.to(gpu), y=y.to(gpu), num_video_frames=T,
              image_only_indicator=ioi.to(gpu))
    e = rel_l2(out, ref)
    assert out.shape[0] == 56 and e < TOL_FWD, f"B=2 forward: rel-L2 {e:.3e}"
    # clips are independent: clip 1 of the batch == the same clip run alone (same ioi rows)
    sel = torch.cat([torch.arange(T, 2 * T), torch.arange(3 * T, 4 * T)])
    alone = net(x[sel].to(gpu), ts[sel].to(gpu), context=ctx[sel].to(gpu), y=y[sel].to(gpu),
                num_video_frames=T, image_only_indicator=ioi[[1, 3]].to(gpu))
    assert rel_l2(out[sel.to(gpu)], alone) < 2e-4
    steps = 5
    with torch.no_grad():
        ref_loop = O.sample_loop(sd, cfg, noise, c, uc, T, steps, ioi2=ioi)
    from gcd_amd.denoiser import Denoiser
    from gcd_amd.sampling import FusedDenoiser
    from gcd_amd.wrappers import OpenAIWrapper
    fd = FusedDenoiser(Denoiser({"target": "gcd_amd.denoiser_scaling.VScalingWithEDMcNoise"}),
                       OpenAIWrapper(net), num_video_frames=T, image_only_indicator=ioi.to(gpu))
    sampler = _sampler(T, steps, "cuda")
    got = sampler(fd, noise.clone().to(gpu), cond={k: v.to(gpu) for k, v in c.items()},
                  uc={k: v.to(gpu) for k, v in uc.items()})
    e = rel_l2(got, ref_loop)
    print(f"B=2 fused 5-step loop rel-L2 {e:.3e}")
    assert sampler.last_path == "fused" and got.shape[0] == B * T and e < 1.5 * TOL_LOOP
    with torch.no_grad():
        ref25 = O.sample_loop(sd, cfg, noise, c, uc, T, 25, ioi2=ioi)
    sampler25 = _sampler(T, 25, "cuda")
    got25 = sampler25(fd, noise.clone().to(gpu), cond={k: v.to(gpu) for k, v in c.items()},
                      uc={k: v.to(gpu) for k, v in uc.items()})
    e25 = rel_l2(got25, ref25)
    print(f"B=2 fused 25-step loop rel-L2 {e25:.3e}")
    assert sampler25.last_path == "fused" and e25 < TOL_LOOP, f"B=2 25-step loop: rel-L2 {e25:.3e}"
