"""GPU: clips of 17..64 frames through every layer — the long-clip temporal-attention kernels against fp64 torch, the
VideoUNet forward, the fused sampling loop (eager step, hipGraph capture and replays), sample-then-decode and the
fine-tune step (both engines) against the CPU oracle at T = 25 and beyond; T = 65 is refused."""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from oracle import svd_unet_ref as O, vae_decoder_ref as D, weights

pytestmark = pytest.mark.gpu
TOL_F16 = 6e-4      # the temporal-attention bar of test_kernels_gpu.py
TOL_FWD = 2e-3
TOL_LOOP = 1e-3
TOL_NET = 5e-3      # test_unet_training_step_vs_oracle's bar


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ref_attention(qkv, clips, T, HW, heads):
    C = heads * 64
    q, k, v = [t.reshape(clips, T, HW, heads, 64).permute(0, 2, 3, 1, 4) for t in qkv.split(C, dim=1)]
    ref = F.scaled_dot_product_attention(q.double(), k.double(), v.double())   # b s h t d
    return ref.permute(0, 3, 1, 2, 4).reshape(clips * T * HW, C).float()


def _long_fwd(qkv16, out16, clips, T, HW, heads):
    from gcd_amd import _lib, ops
    _lib.check(_lib.load().gcd_attn_temporal_long_f16(qkv16.data_ptr(), ops._ld(qkv16), out16.data_ptr(),
                                                      ops._ld(out16), clips, T, HW, heads, ops._stream()),
               "gcd_attn_temporal_long_f16")


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("clips,T,HW,heads", [(2, 17, 10, 3), (1, 25, 33, 1), (2, 32, 7, 5), (1, 48, 5, 2),
                                              (2, 63, 3, 2), (2, 64, 9, 5), (2, 25, 1500, 5)])
def test_long_temporal_attention_vs_fp64(gpu, clips, T, HW, heads):
    """ops.attn_temporal at T > 16 (the long entry); the last shape has more problems than resident waves."""
    from gcd_amd import ops
    g = _gen(31)
    C = heads * 64
    M = clips * T * HW
    qkv = (torch.randn(M, 3 * C, generator=g) * 1.5).half()
    ref = _ref_attention(qkv.float(), clips, T, HW, heads)
    out = torch.full((M, C), float("nan"), dtype=torch.float16, device=gpu)
    ops.attn_temporal(qkv.to(gpu), out, clips, T, HW, heads)
    torch.cuda.synchronize()
    e = rel_l2(out.float(), ref)
    assert e < TOL_F16, f"T={T}: rel-L2 {e:.3e}"


def test_long_temporal_attention_strided(gpu):
    """q|k|v a column view of a wider tensor, output rows wider than C (ldo > C): the columns around stay untouched."""
    from gcd_amd import ops
    clips, T, HW, heads = 2, 41, 6, 3
    C = heads * 64
    M = clips * T * HW
    g = _gen(32)
    wide = (torch.randn(M, 3 * C + 72, generator=g)).half().to(gpu)
    qkv = wide[:, 40:40 + 3 * C]
    ref = _ref_attention(qkv.float().cpu(), clips, T, HW, heads)
    outw = torch.full((M, C + 24), 7.0, dtype=torch.float16, device=gpu)
    out = outw[:, 8:8 + C]
    ops.attn_temporal(qkv, out, clips, T, HW, heads)
    torch.cuda.synchronize()
    e = rel_l2(out.float(), ref)
    assert e < TOL_F16, f"strided: rel-L2 {e:.3e}"
    assert bool((outw[:, :8] == 7.0).all()) and bool((outw[:, 8 + C:] == 7.0).all())


@pytest.mark.parametrize("T", [1, 14, 16])
def test_long_entry_matches_short_entry(gpu, T):
    """Within the old kernel's range the new entry computes what gcd_attn_temporal_f16 computes."""
    from gcd_amd import ops
    clips, HW, heads = 2, 37, 3
    C = heads * 64
    M = clips * T * HW
    qkv = (torch.randn(M, 3 * C, generator=_gen(33)) * 1.5).half().to(gpu)
    a = torch.empty(M, C, dtype=torch.float16, device=gpu)
    b = torch.empty(M, C, dtype=torch.float16, device=gpu)
    ops.attn_temporal(qkv, a, clips, T, HW, heads)
    _long_fwd(qkv, b, clips, T, HW, heads)
    torch.cuda.synchronize()
    ref = _ref_attention(qkv.float().cpu(), clips, T, HW, heads)
    assert rel_l2(b.float(), a.float()) < TOL_F16
    assert rel_l2(b.float(), ref) < TOL_F16


@pytest.mark.parametrize("clips,T,HW,heads", [(2, 17, 5, 3), (1, 25, 9, 2), (2, 32, 4, 5), (1, 64, 6, 2)])
def test_long_temporal_attention_backward(gpu, clips, T, HW, heads):
    """TemporalAttention.backward at T > 16 (gcd_attn_temporal_long_bwd) vs fp64 autograd on the fp16-rounded q|k|v."""
    from gcd_amd import autograd_ops as A
    g = _gen(34)
    C = heads * 64
    M = clips * T * HW
    qkv = torch.randn(M, 3 * C, generator=g).half().float()
    dO = torch.randn(M, C, generator=g)
    qr = qkv.double().requires_grad_(True)
    q, k, v = (t.reshape(clips, T, HW, heads, 64).permute(0, 2, 3, 1, 4) for t in qr.chunk(3, dim=-1))
    F.scaled_dot_product_attention(q, k, v).permute(0, 3, 1, 2, 4).reshape(M, C).backward(dO.double())
    qg = qkv.clone().to(gpu).requires_grad_(True)
    y = A.temporal_attention(qg, clips, T, HW, heads)
    y.backward(dO.to(gpu))
    torch.cuda.synchronize()
    e = rel_l2(qg.grad, qr.grad)
    assert e < 1e-3, f"T={T}: dqkv rel-L2 {e:.3e}"
    for i, name in enumerate("qkv"):
        ei = rel_l2(qg.grad[:, i * C:(i + 1) * C], qr.grad[:, i * C:(i + 1) * C])
        assert ei < 1e-3, f"T={T}: d{name} rel-L2 {ei:.3e}"


# ------------------------------------------------------------------------------------------------ the network
def _build(cfg, gpu, salt=0):
    from gcd_amd.video_model import VideoUNet
    with torch.device("meta"):
        net = VideoUNet(**cfg.as_reference_kwargs())
    sd = weights.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, salt)
    net = net.to_empty(device=gpu)
    net.load_state_dict(sd)
    return net.eval(), sd


def _unet_inputs(cfg, T, h, w, seed, clips=1):
    noise, c, uc = weights.synth_inputs(clips, T, h, w, cfg.context_dim, cfg.adm_in_channels + cfg.aux_emb_dim, seed)
    x = torch.cat([torch.cat([noise, uc["concat"]], 1), torch.cat([noise, c["concat"]], 1)])
    ts = torch.linspace(-1.5, 1.63, 2 * clips * T)
    return (x, ts, torch.cat([uc["crossattn"], c["crossattn"]]), torch.cat([uc["vector"], c["vector"]]),
            torch.zeros(2 * clips, T))


@pytest.fixture(scope="module")
def tiny(gpu):
    return _build(O.TINY, gpu)


@pytest.mark.parametrize("T,clips", [(17, 1), (25, 1), (40, 1), (25, 2)])
def test_unet_forward_long_clips_vs_oracle(gpu, tiny, T, clips):
    net, sd = tiny
    x, ts, ctx, y, ioi = _unet_inputs(O.TINY, T, 8, 8, 40 + T + clips, clips)
    if clips == 2:
        ioi[1, 3] = ioi[2, 20] = 1.0
    with torch.no_grad():
        ref = O.unet_forward(sd, O.TINY, x, ts, ctx, y, T, ioi)
    out = net(x.to(gpu), ts.to(gpu), context=ctx.to(gpu), y=y.to(gpu), num_video_frames=T,
              image_only_indicator=ioi.to(gpu))
    e = rel_l2(out, ref)
    assert out.shape[0] == 2 * clips * T and e < TOL_FWD, f"T={T} clips={clips}: rel-L2 {e:.3e}"


def test_unet_rejects_65_frames(gpu, tiny):
    from gcd_amd import _lib
    net, _ = tiny
    T = 65
    x, ts, ctx, y, ioi = _unet_inputs(O.TINY, T, 8, 8, 3)
    with pytest.raises(_lib.GcdError, match="T=65"):
        net(x.to(gpu), ts.to(gpu), context=ctx.to(gpu), y=y.to(gpu), num_video_frames=T,
            image_only_indicator=ioi.to(gpu))
    torch.cuda.synchronize()


def test_unet_full_width_kubric_25_frames(gpu):
    """The 1.5 B-parameter Kubric topology at 25 x 16 x 16 latents against the oracle on host cores."""
    net, sd = _build(O.KUBRIC, gpu, salt=2)
    T = 25
    x, ts, ctx, y, ioi = _unet_inputs(O.KUBRIC, T, 16, 16, 72)
    torch.set_num_threads(min(32, torch.get_num_threads()))
    with torch.no_grad():
        ref = O.unet_forward(sd, O.KUBRIC, x, ts, ctx, y, T, ioi)
    out = net(x.to(gpu), ts.to(gpu), context=ctx.to(gpu), y=y.to(gpu), num_video_frames=T,
              image_only_indicator=ioi.to(gpu))
    e = rel_l2(out, ref)
    del net, sd
    torch.cuda.empty_cache()
    assert e < TOL_FWD, f"full width T=25: rel-L2 {e:.3e}"


def _sampler(T, steps):
    from gcd_amd.sampling import EulerEDMSampler
    return EulerEDMSampler(
        discretization_config={"target": "gcd_amd.discretizer.EDMDiscretization", "params": {"sigma_max": 700.0}},
        num_steps=steps,
        guider_config={"target": "gcd_amd.guiders.LinearPredictionGuider",
                       "params": {"num_frames": T, "max_scale": 1.5, "min_scale": 1.0}},
        device="cuda")


def _fused(net, T, gpu):
    from gcd_amd.denoiser import Denoiser
    from gcd_amd.sampling import FusedDenoiser
    from gcd_amd.wrappers import OpenAIWrapper
    return FusedDenoiser(Denoiser({"target": "gcd_amd.denoiser_scaling.VScalingWithEDMcNoise"}), OpenAIWrapper(net),
                         num_video_frames=T, image_only_indicator=torch.zeros(2, T, device=gpu))


def test_sampler_25_steps_25_frames_vs_oracle(gpu, tiny):
    """The fused 25-step loop on a 25-frame clip at 16 x 16: eager first step, hipGraph capture, replays."""
    net, sd = tiny
    T, steps = 25, 25
    noise, c, uc = weights.synth_inputs(1, T, 16, 16, O.TINY.context_dim,
                                        O.TINY.adm_in_channels + O.TINY.aux_emb_dim, 62)
    with torch.no_grad():
        ref = O.sample_loop(sd, O.TINY, noise, c, uc, T, steps)
    sampler = _sampler(T, steps)
    out = sampler(_fused(net, T, gpu), noise.clone().to(gpu), cond={k: v.to(gpu) for k, v in c.items()},
                  uc={k: v.to(gpu) for k, v in uc.items()})
    e = rel_l2(out, ref)
    print(f"T=25 25-step loop rel-L2 {e:.3e}")
    assert sampler.last_path == "fused" and e < TOL_LOOP, f"T=25 loop: rel-L2 {e:.3e} ({sampler.last_path})"


def _psnr(a, b):
    mse = float(((a.double().cpu() - b.double().cpu()) ** 2).mean())
    return 10.0 * math.log10(4.0 / max(mse, 1e-30))


def test_sample_then_decode_25_frames_in_chunks(gpu, tiny):
    """25 frames sampled, then decoded 14 + 11 at a time (en_and_decode_n_samples_a_time = 14)."""
    from gcd_amd.first_stage import decode_first_stage
    from gcd_amd.temporal_ae import VideoDecoder
    net, sd_u = tiny
    with torch.device("meta"):
        dec = VideoDecoder(**D.TINY.as_reference_kwargs())
    sd_d = weights.synth_state_dict({k: tuple(v.shape) for k, v in dec.state_dict().items()}, salt=1)
    dec = dec.to_empty(device=gpu)
    dec.load_state_dict(sd_d)
    dec.eval()
    T, steps, h, w = 25, 25, 8, 8
    noise, c, uc = weights.synth_inputs(1, T, h, w, O.TINY.context_dim,
                                        O.TINY.adm_in_channels + O.TINY.aux_emb_dim, 83)
    with torch.no_grad():
        z_ref = O.sample_loop(sd_u, O.TINY, noise, c, uc, T, steps)
        frames_ref = D.decode_first_stage(sd_d, D.TINY, z_ref, 0.18215, n_samples=14)
    sampler = _sampler(T, steps)
    z = sampler(_fused(net, T, gpu), noise.clone().to(gpu), cond={k: v.to(gpu) for k, v in c.items()},
                uc={k: v.to(gpu) for k, v in uc.items()})
    frames = decode_first_stage(dec, z, 0.18215, en_and_decode_n_samples_a_time=14)
    torch.cuda.synchronize()
    assert frames.shape == frames_ref.shape == (T, 3, 8 * h, 8 * w)
    ez, psnr = rel_l2(z, z_ref), _psnr(frames, frames_ref)
    print(f"T=25: latents rel-L2 {ez:.3e}, PSNR {psnr:.1f} dB")
    assert sampler.last_path == "fused" and ez < TOL_LOOP
    assert psnr >= 55.0


# ------------------------------------------------------------------------------------------------ fine-tune step
@pytest.fixture
def train_engine(request):
    from gcd_amd import training as TR
    old = TR.TRAIN_ENGINE
    TR.set_train_engine(request.param)
    yield request.param
    TR.set_train_engine(old)


@pytest.mark.parametrize("train_engine", ["planned", "autograd"], indirect=True)
def test_training_step_25_frames_vs_oracle(gpu, train_engine):
    """The fine-tune step at T = 25 (O.TINY, step 0): loss, every parameter gradient and the Adam update vs autograd over
    the CPU oracle, at test_unet_training_step_vs_oracle's bars."""
    from gcd_amd import training as TR
    from gcd_amd.video_model import VideoUNet
    from oracle import loss_ref as LR
    with torch.device("meta"):
        net = VideoUNet(**O.TINY.as_reference_kwargs())
    sd = weights.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 3)
    net = net.to_empty(device=gpu)
    net.load_state_dict(sd)
    net.train()
    T, H, W, B = 25, 16, 16, 1
    BT = B * T
    cfg = O.TINY
    g = _gen(12)
    x0 = torch.randn(BT, 4, H, W, generator=g)
    noise = torch.randn(BT, 4, H, W, generator=g)
    cond = {"crossattn": torch.randn(BT, 1, cfg.context_dim, generator=g),
            "concat": torch.randn(BT, 4, H, W, generator=g) * 0.8,
            "vector": torch.randn(BT, cfg.adm_in_channels + cfg.aux_emb_dim, generator=g).clamp(-1, 1)}
    sig = LR.harmonize(LR.edm_sigmas(torch.randn(BT, generator=g), 1.0, 1.6), T)
    ioi = torch.zeros(B, T)
    loss_scale = 256.0
    step = 0
    sdr = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    noised = x0 + noise * sig[:, None, None, None]
    out_r = O.denoise(sdr, cfg, noised, sig, cond, T, ioi)
    loss_r = LR.get_loss(out_r, x0, LR.edm_weighting(sig, 1.0)[:, None, None, None], step, "l2", 0.1, 5000).mean()
    loss_r.backward()
    den = TR.TrainDenoiser({"target": "gcd_amd.denoiser_scaling.VScalingWithEDMcNoise"})
    loss_fn = TR.StandardDiffusionLoss(
        sigma_sampler_config={"target": "gcd_amd.training.EDMSampling", "params": {"p_mean": 1.0, "p_std": 1.6}},
        loss_weighting_config={"target": "gcd_amd.training.EDMWeighting", "params": {"sigma_data": 1.0}},
        focus_top=0.1, focus_steps=5000, batch2model_keys=["image_only_indicator", "num_video_frames"])
    cg = {k: v.to(gpu) for k, v in cond.items()}
    sg = sig.to(gpu)
    out = den(net, noised.to(gpu), sg, cg, num_video_frames=T, image_only_indicator=ioi.to(gpu))
    w = loss_fn.loss_weighting(sg)[:, None, None, None]
    loss = loss_fn.get_loss(out, x0.to(gpu), w, {"global_step": step}).mean()
    (loss * loss_scale).backward()
    torch.cuda.synchronize()
    assert abs(float(loss) / float(loss_r) - 1.0) < 2e-3
    assert rel_l2(out, out_r) < 2e-3
    num = den_ = 0.0
    worst = ("", 0.0)
    for name, prm in net.named_parameters():
        ref = sdr[name].grad
        if ref is None or float(ref.abs().max()) == 0.0:
            assert prm.grad is None or float(prm.grad.abs().max()) == 0.0, name
            continue
        got = prm.grad.double().cpu() / loss_scale
        num += float((got - ref.double()).pow(2).sum())
        den_ += float(ref.double().pow(2).sum())
        if ref.numel() >= 64:      # (a scalar blend logit's gradient is one long cancelling sum: the global norm has it)
            e = rel_l2(got, ref)
            if e > worst[1]:
                worst = (name, e)
    total = math.sqrt(num / den_)
    print(f"{train_engine} T=25: gradients global rel-L2 {total:.3e}, worst {worst[0]} {worst[1]:.3e}")
    assert total < TOL_NET and worst[1] < 4 * TOL_NET, (total, worst)
    lr = 1e-3
    ref_params = [torch.nn.Parameter(sd[n].clone()) for n, _ in net.named_parameters()]
    for rp, (n, _) in zip(ref_params, net.named_parameters()):
        rp.grad = sdr[n].grad.clone() if sdr[n].grad is not None else torch.zeros_like(rp)
    torch.optim.Adam(ref_params, lr=lr).step()
    opt = TR.AdamHIP(net.parameters(), lr=lr)
    opt.step(grad_scale=1.0 / loss_scale)
    torch.cuda.synchronize()
    moved = 0.0
    for rp, (n, prm) in zip(ref_params, net.named_parameters()):
        if prm.grad is None:
            continue
        du, dr = prm.detach().cpu() - sd[n], rp.detach() - sd[n]
        big = sdr[n].grad.abs() > 0.05 * sdr[n].grad.abs().max()
        if big.any():
            assert rel_l2(du[big], dr[big]) < 2e-2, n
            moved += float(dr[big].abs().sum())
    assert moved > 0
