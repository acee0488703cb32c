"""GPU: the standalone DiffusionEngine end to end — built from the reference's `sgm.*` target strings through
gcd_amd.config.translate_targets, tiny networks (64-wide UNet, E.TINY / D.TINY first stage, a 160-wide CLIP tower), 64 x 64
frames, weights from a synthetic checkpoint loaded by `ckpt_path`.

"The rule": two results that should be the same computation are compared against the run-to-run spread of that
computation.  The hand-wired (or first) run is made twice under one seed; if its two runs are bit-equal the other result
must be bit-equal to it, otherwise it must lie within twice their rel-L2 spread (printed)."""
import json
import math
import os

import pytest
import torch
import yaml

import engine_util as U
from conftest import rel_l2
from oracle import svd_unet_ref as O, vae_decoder_ref as D, vae_encoder_ref as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    return U.write_checkpoint(tmp_path_factory.mktemp("engine") / "tiny.safetensors", salt=0)


def _engine(gpu, ckpt, T=4, steps=5, **kw):
    return U.build(U.tiny_sgm_config(T=T, steps=steps, **kw), ckpt_path=ckpt).to(gpu).eval()


def _by_the_rule(other, a, b, what):
    if torch.equal(a, b):
        print(f"{what}: the two reference runs are bit-equal")
        assert torch.equal(other, a), f"{what}: rel-L2 {rel_l2(other, a):.3e} from a bit-reproducible reference"
    else:
        spread = rel_l2(b, a)
        e = rel_l2(other, a)
        print(f"{what}: run-to-run spread {spread:.3e}, distance {e:.3e}")
        assert e <= 2.0 * spread, (what, e, spread)


class _HandWired:
    """The stages wired by hand, each instantiated from its own sub-config and loaded from its own part of the weights:
    what tests/test_e2e_gpu.py and the training tests do, without the engine."""

    def __init__(self, gpu, T, steps, ucg_rate=0.0, n_a_time=None):
        from gcd_amd import config as C
        from gcd_amd.training import TrainDenoiser
        from gcd_amd.util import get_obj_from_str, instantiate_from_config
        p = C.translate_targets(U.tiny_sgm_config(T=T, steps=steps, ucg_rate=ucg_rate))["params"]
        sd = U.synth_engine_state_dict(0)
        for emb in p["conditioner_config"]["params"]["emb_models"]:       # what the engine propagates (diffusion.py:97-105)
            if "en_and_decode_n_samples_a_time" in emb["params"]:
                emb["params"]["en_and_decode_n_samples_a_time"] = n_a_time
        self.unet = instantiate_from_config(p["network_config"])
        self.unet.load_state_dict(U.sub_state_dict(sd, "model.diffusion_model."))
        self.model = get_obj_from_str("gcd_amd.wrappers.OpenAIWrapper")(self.unet).to(gpu)
        self.conditioner = instantiate_from_config(p["conditioner_config"])
        self.conditioner.load_state_dict(U.sub_state_dict(sd, "conditioner."))
        self.conditioner.to(gpu)
        fs = p["first_stage_config"]["params"]
        self.encoder = instantiate_from_config(fs["encoder_config"])
        self.encoder.load_state_dict(U.sub_state_dict(sd, "first_stage_model.encoder."))
        self.encoder.to(gpu).eval().requires_grad_(False)
        self.decoder = instantiate_from_config(fs["decoder_config"])
        self.decoder.load_state_dict(U.sub_state_dict(sd, "first_stage_model.decoder."))
        self.decoder.to(gpu).eval().requires_grad_(False)
        self.regularizer = instantiate_from_config(fs["regularizer_config"])
        self.denoiser = instantiate_from_config(p["denoiser_config"])
        self.train_denoiser = TrainDenoiser(p["denoiser_config"]["params"]["scaling_config"], input_grads=True)
        self.sampler = instantiate_from_config(p["sampler_config"])
        self.loss_fn = instantiate_from_config(p["loss_fn_config"])
        self.T = T

    @torch.no_grad()
    def sample_video(self, batch):
        from gcd_amd.first_stage import decode_first_stage
        from gcd_amd.sampling import FusedDenoiser
        c, uc = self.conditioner.get_unconditional_conditioning(
            batch, batch_uc=batch, force_uc_zero_embeddings=["cond_frames", "cond_frames_without_noise"])
        fd = FusedDenoiser(self.denoiser, self.model, num_video_frames=batch["num_video_frames"],
                           image_only_indicator=batch["image_only_indicator"].repeat_interleave(2, dim=0))
        n, _, Hp, Wp = batch["cond_frames"].shape
        noise = torch.randn((n, 4, Hp // 8, Wp // 8), device=batch["cond_frames"].device)
        z = self.sampler(fd, noise, cond=c, uc=uc)
        x = decode_first_stage(self.decoder, z, U.SCALE_FACTOR, en_and_decode_n_samples_a_time=None)
        return z, torch.clamp((x + 1.0) / 2.0, 0.0, 1.0)

    def train_step(self, batch, lr):
        """encoder -> regularizer sample -> StandardDiffusionLoss over TrainDenoiser -> backward -> AdamHIP.step."""
        from gcd_amd.training import AdamHIP
        params = list(self.model.parameters()) + list(self.conditioner.embedders[5].parameters())
        opt = AdamHIP(params, lr=lr)
        with torch.no_grad():
            z = U.SCALE_FACTOR * self.regularizer.sample(self.encoder(batch["jpg"]))
        batch["global_step"] = 0
        loss = self.loss_fn(self.model, self.train_denoiser, self.conditioner, z, batch).mean()
        loss.backward()
        opt.step()
        return loss.detach()


class _Spy:
    """Counts the calls of the operator-level training engine while active."""

    def __enter__(self):
        from gcd_amd import training as TR
        self.TR, self.real, self.calls = TR, TR.unet_forward_train, 0

        def spy(*a, **kw):
            self.calls += 1
            return self.real(*a, **kw)
        TR.unet_forward_train = spy
        return self

    def __exit__(self, *exc):
        self.TR.unet_forward_train = self.real


@pytest.fixture
def deterministic():
    from gcd_amd import training as TR
    old = TR.is_deterministic()
    TR.set_deterministic(True)
    yield
    TR.set_deterministic(old)


# ------------------------------------------------------------------------------------------------------------------ 1
def test_sample_video_against_the_cpu_oracles_of_every_stage(gpu, ckpt):
    from gcd_amd import clip_vision as cv
    T, steps = 14, 25
    eng = _engine(gpu, ckpt, T=T, steps=steps, n_a_time=T)
    sd = U.synth_engine_state_dict(0)
    batch_cpu = U.tiny_batch(T, clips=1)
    batch = {k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in batch_cpu.items()}
    torch.manual_seed(4321)
    noise = torch.randn((T, 4, 8, 8), device=gpu).cpu()
    torch.manual_seed(4321)
    out = eng.sample_video(batch)
    torch.cuda.synchronize()
    assert eng.sampler.last_path == "fused", "the engine did not reach the fused loop"
    c_dev, uc_dev = eng.conditioner.get_unconditional_conditioning(
        batch, batch_uc=batch, force_uc_zero_embeddings=["cond_frames", "cond_frames_without_noise"])
    # ---- oracle of every stage ----
    tower = cv.FrozenOpenCLIPImageEmbedder(vision_cfg=dict(U.CLIP_TINY))
    tower.model.visual.load_state_dict(U.sub_state_dict(sd, "conditioner.embedders.0.open_clip.model.visual."))
    sd_c = U.sub_state_dict(sd, "conditioner.")
    with torch.no_grad():
        token = tower(batch_cpu["cond_frames_without_noise"]).reshape(T, 1, -1)
        concat = E.encode_mode(U.sub_state_dict(sd_c, "embedders.3.encoder.encoder."), E.TINY, batch_cpu["cond_frames"],
                               sd_c["embedders.3.encoder.quant_conv.weight"],
                               sd_c["embedders.3.encoder.quant_conv.bias"])   # (the configs give this embedder no scale_factor)
        vec = torch.cat([O.concat_timestep_embed(batch_cpu["fps_id"], 32),
                         O.concat_timestep_embed(batch_cpu["motion_bucket_id"], 32),
                         O.concat_timestep_embed(batch_cpu["cond_aug"], 32),
                         O.spherical_embed(batch_cpu["scaled_relative_angles"], sd_c["embedders.5.proj.weight"],
                                           sd_c["embedders.5.proj.bias"])], 1)
        embedded = [("cond_frames_without_noise", token), ("v", vec), ("cond_frames", concat)]
        c = O.general_conditioner(embedded)
        uc = O.general_conditioner(embedded, force_zero=("cond_frames", "cond_frames_without_noise"))
        z_ref = O.sample_loop(U.sub_state_dict(sd, "model.diffusion_model."), U.UCFG, noise, c, uc, T, steps)
        x_ref = D.decode_first_stage(U.sub_state_dict(sd, "first_stage_model.decoder."), D.TINY, z_ref, U.SCALE_FACTOR,
                                     n_samples=T)
        vid_ref = torch.clamp((x_ref + 1.0) / 2.0, 0.0, 1.0)
    e_cat, e_vec = rel_l2(c_dev["concat"], c["concat"]), rel_l2(c_dev["vector"], c["vector"])
    e_tok = rel_l2(c_dev["crossattn"], c["crossattn"])
    ez = rel_l2(out["sampled_z"], z_ref)
    mse = float(((out["sampled_video"].double().cpu() - vid_ref.double()) ** 2).mean())
    psnr = 10.0 * math.log10(1.0 / max(mse, 1e-30))                  # [0, 1] range
    print(f"engine sample_video: concat {e_cat:.2e}, vector {e_vec:.2e}, crossattn {e_tok:.2e}, latents {ez:.3e}, "
          f"video PSNR {psnr:.1f} dB")
    assert out["sampled_video"].shape == (T, 3, 64, 64) and out["sampled_z"].shape == (T, 4, 8, 8)
    assert torch.equal(out["gt_video"], torch.clamp((batch["jpg"] + 1.0) / 2.0, 0.0, 1.0))
    assert e_cat < 2e-3 and e_vec < 2e-5
    # the tower against its fp32 restatement on the CPU: the bar tests/test_clip_vision_gpu.py holds this tower (the same
    # widths and weight seed) to, twice the drift of the fp32 tower under fp16 autocast recorded in its golden
    import clip_util
    rec = clip_util.load_golden()["tower"]["w160_s17"]
    assert rec["cfg"] == U.CLIP_TINY and rec["weight_seed"] == U.CLIP_SEED
    assert e_tok < 2.0 * rec["drift_fp16"], (e_tok, rec["drift_fp16"])
    assert float(uc_dev["concat"].abs().max()) == 0.0 and float(uc_dev["crossattn"].abs().max()) == 0.0
    assert ez < 2e-3 and psnr >= 55.0


# ------------------------------------------------------------------------------------------------------------------ 2
def test_sample_video_equals_the_stages_wired_by_hand(gpu, ckpt):
    T, steps = 4, 5
    eng = _engine(gpu, ckpt, T=T, steps=steps)
    hand = _HandWired(gpu, T, steps)
    batch = U.tiny_batch(T, clips=1, device=gpu)
    runs = []
    for _ in range(2):
        torch.manual_seed(99)
        runs.append(hand.sample_video(batch))
    torch.manual_seed(99)
    out = eng.sample_video(batch)
    torch.cuda.synchronize()
    assert eng.sampler.last_path == "fused" and hand.sampler.last_path == "fused"
    _by_the_rule(out["sampled_z"], runs[0][0], runs[1][0], "sample_video latents, engine vs hand-wired")
    _by_the_rule(out["sampled_video"], runs[0][1], runs[1][1], "sample_video frames, engine vs hand-wired")


# ------------------------------------------------------------------------------------------------------------------ 3
def test_fit_step_is_bit_equal_to_the_hand_wired_step(gpu, ckpt, deterministic):
    T, clips, lr = 4, 2, 2e-5
    eng = _engine(gpu, ckpt, T=T, ucg_rate=0.1).train()
    assert eng.learning_rate == lr
    hand = _HandWired(gpu, T, 5, ucg_rate=0.1)
    hand.model.train()
    hand.conditioner.train()
    torch.manual_seed(2024)
    loss_hand = hand.train_step(U.tiny_batch(T, clips=clips, device=gpu), lr)
    torch.manual_seed(2024)
    with _Spy() as spy:
        loss = eng.fit_step(U.tiny_batch(T, clips=clips, device=gpu))
    torch.cuda.synchronize()
    assert spy.calls == 0 and "_gcd_train_plan" in eng.model.diffusion_model.__dict__, "the step left the planned engine"
    assert eng.global_step == 1
    print(f"fit_step: loss {float(loss):.6f}, hand-wired {float(loss_hand):.6f}")
    assert torch.equal(loss, loss_hand)
    pairs = list(zip(eng.model.named_parameters(), hand.model.parameters())) + \
        list(zip(eng.conditioner.embedders[5].named_parameters(), hand.conditioner.embedders[5].parameters()))
    reached = 0
    for (name, p), q in pairs:
        assert (p.grad is None) == (q.grad is None), name
        if p.grad is not None:
            reached += 1
            assert torch.equal(p.grad, q.grad), f"gradient of {name}: {rel_l2(p.grad, q.grad):.2e}"
        assert torch.equal(p, q), f"updated {name}: {rel_l2(p, q):.2e}"
    assert reached > 100
    spherical = eng.conditioner.embedders[5].proj
    assert spherical.weight.grad is not None and float(spherical.weight.grad.abs().max()) > 0
    before = U.synth_engine_state_dict(0)
    assert not torch.equal(spherical.weight.cpu(), before["conditioner.embedders.5.proj.weight"])
    # nothing outside the optimizer's list moved
    now = eng.state_dict()
    assert all(torch.equal(now[k].cpu(), before[k]) for k in before
               if not k.startswith(("model.", "conditioner.embedders.5.")))


# ------------------------------------------------------------------------------------------------------------------ 4
def test_ema_rides_in_the_optimizer_swaps_and_survives_a_checkpoint(gpu, ckpt, tmp_path):
    T = 4
    eng = _engine(gpu, ckpt, T=T, use_ema=True, ema_decay_rate=0.999).train()
    names = [n for n, p in eng.model.named_parameters() if p.requires_grad]
    p0 = {n: p.detach().clone() for n, p in eng.model.named_parameters()}
    shadow = lambda n: eng.model_ema._buffers[eng.model_ema.m_name2s_name[n]]      # noqa: E731
    assert all(torch.equal(shadow(n), p0[n]) for n in names) and int(eng.model_ema.num_updates) == 0
    torch.manual_seed(7)
    eng.fit_step(U.tiny_batch(T, clips=1, device=gpu))
    torch.cuda.synchronize()
    assert eng._ema_in_optimizer and eng.optimizers().ema is eng.model_ema
    assert int(eng.model_ema.num_updates) == 1, "the shadows were updated twice (optimizer and on_train_batch_end)"
    # LitEma's rule for update 1: decay = min(0.999, (1 + 1) / (10 + 1)); shadow -= (1 - decay) (shadow - p_new)
    decay = min(0.999, 2.0 / 11.0)
    p1 = dict(eng.model.named_parameters())
    moved = 0
    for n in names:
        want = p0[n].double() - (1.0 - decay) * (p0[n].double() - p1[n].detach().double())
        err = float((shadow(n).double() - want).abs().max())
        assert err <= 4.0 * 2.0 ** -24 * max(float(p0[n].abs().max()), 1e-3), (n, err)      # a few fp32 ulps
        moved += int(not torch.equal(p1[n], p0[n]))
    assert moved > 100
    # ema_scope: the shadows inside, the training weights back afterwards, bit for bit
    train = {n: p.detach().clone() for n, p in eng.model.named_parameters()}
    with eng.ema_scope():
        assert all(torch.equal(p, shadow(n)) for n, p in eng.model.named_parameters() if n in names)
    assert all(torch.equal(p, train[n]) for n, p in eng.model.named_parameters())
    # the checkpoint carries model_ema.*, and a fresh engine told so loads it late
    path = str(tmp_path / "ema.ckpt")
    eng.save_checkpoint(path)
    fresh = U.build(U.tiny_sgm_config(T=T, use_ema=True, ema_decay_rate=0.999, ckpt_has_ema=True), ckpt_path=path).to(gpu)
    a, b = eng.state_dict(), fresh.state_dict()
    ema_keys = [k for k in a if k.startswith("model_ema.")]
    assert len(ema_keys) == len(names) + 2 and list(a) == list(b)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert fresh.global_step == 0


# ------------------------------------------------------------------------------------------------------------------ 5
def test_time_lora_step_changes_adapters_only_and_saves_peft_names(gpu, ckpt, tmp_path):
    T = 4
    eng = _engine(gpu, ckpt, T=T, ft_strategy="time_lora").train()
    lora, unet = eng.lora, eng.model.diffusion_model
    adapted = {n + ".weight" for n in lora.names}
    w0 = [w.clone() for w in lora.w0()]
    a0, b0 = [a.detach().clone() for a in lora.lora_A], [b.detach().clone() for b in lora.lora_B]
    plain0 = {n: p.detach().clone() for n, p in unet.named_parameters()}
    assert all(torch.equal(plain0[n + ".weight"], w) for n, w in zip(lora.names, w0))          # B = 0: merged = W0
    eng.learning_rate = 1e-3
    torch.manual_seed(11)
    eng.fit_step(U.tiny_batch(T, clips=1, device=gpu))
    torch.cuda.synchronize()
    assert sum(int(not torch.equal(b, old)) for b, old in zip(lora.lora_B, b0)) > len(b0) // 2, "the adapters did not move"
    assert all(torch.equal(a, old) for a, old in zip(lora.lora_A, a0))       # dA = s B^T dW = 0 while B = 0
    assert all(torch.equal(w, old) for w, old in zip(lora.w0(), w0))
    for n, p in unet.named_parameters():
        if n not in adapted:
            assert torch.equal(p, plain0[n]), f"{n} is not adapted and moved"
    for n, m, w, a, b in zip(lora.names, lora.weights(), w0, lora.lora_A, lora.lora_B):
        want = w.double() + lora.scale * (b.detach().double() @ a.detach().double())
        err = float((m.detach().double() - want).abs().max())
        assert err <= 2.0 * 2.0 ** -24 * float(want.abs().max()), (n, err)      # W = W0 + s B A to fp32 rounding
    path = str(tmp_path / "lora.ckpt")
    eng.save_checkpoint(path)
    saved = torch.load(path, map_location="cpu", weights_only=True)["state_dict"]
    n0 = "model.diffusion_model." + lora.names[0]
    assert torch.equal(saved[n0 + ".base_layer.weight"], w0[0].cpu()) and n0 + ".weight" not in saved
    assert torch.equal(saved[n0 + ".lora_B.default.weight"], lora.lora_B[0].detach().cpu())
    assert sum(1 for k in saved if k.endswith(".lora_A.default.weight")) == len(lora.names)
    assert not any(k.startswith("lora.") for k in saved)
    # the reference loads a checkpoint of a peft network late (after the adapters exist)
    fresh = U.build(U.tiny_sgm_config(T=T, ft_strategy="time_lora", ckpt_has_ema=True), ckpt_path=ckpt).to(gpu)
    missing, unexpected = fresh.init_from_ckpt(path)
    assert not missing and not unexpected
    a, b = eng.state_dict(), fresh.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    for m, f in zip(lora.weights(), fresh.lora.weights()):
        assert float((m.detach() - f.detach()).abs().max()) <= 2.0 * 2.0 ** -24 * float(m.detach().abs().max())


# ------------------------------------------------------------------------------------------------------------------ 6
def test_validation_step_scores_the_first_clip(gpu, ckpt):
    from gcd_amd.validation import validation_metrics
    T = 4
    eng = _engine(gpu, ckpt, T=T)
    batch = U.tiny_batch(T, clips=2, device=gpu)
    direct = []
    for _ in range(2):
        torch.manual_seed(5)
        vd = eng.sample_video(dict(batch), limit_batch=1)
        direct.append((vd, validation_metrics(vd["gt_video"].contiguous(), vd["sampled_video"].contiguous(), eng.lpips)))
    vd = direct[0][0]
    assert vd["sampled_video"].shape == (T, 3, 64, 64) and vd["sampled_z"].shape == (T, 4, 8, 8)
    assert torch.equal(vd["gt_video"], torch.clamp((batch["jpg"][:T] + 1.0) / 2.0, 0.0, 1.0))
    assert torch.equal(vd["cond_video"], torch.clamp((batch["cond_frames"][:T] + 1.0) / 2.0, 0.0, 1.0))
    torch.manual_seed(5)
    got = eng.validation_step(dict(batch), 0)
    assert set(got) == {"lpips", "psnr", "ssim"} and eng.validation_step_outputs == [got]
    print(f"validation_step: {got}; direct {direct[0][1]} / {direct[1][1]}")
    for k in got:
        a, b = direct[0][1][k], direct[1][1][k]
        assert math.isfinite(got[k])
        if torch.equal(direct[0][0]["sampled_video"], direct[1][0]["sampled_video"]):
            assert got[k] == a == b, k
        else:
            assert abs(got[k] - a) <= 2.0 * abs(b - a), k
    assert eng.on_validation_epoch_end() == dict(got, step=0) and eng.validation_step_outputs == []


# ------------------------------------------------------------------------------------------------------------------ 7
def test_checkpoint_round_trip_after_a_step(gpu, ckpt, tmp_path):
    T = 4
    eng = _engine(gpu, ckpt, T=T).train()
    torch.manual_seed(21)
    eng.fit_step(U.tiny_batch(T, clips=1, device=gpu))
    eng.eval()
    path = str(tmp_path / "step1.ckpt")
    eng.save_checkpoint(path)
    assert torch.load(path, map_location="cpu", weights_only=True)["global_step"] == 1
    fresh = _engine(gpu, path, T=T)
    a, b = eng.state_dict(), fresh.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["model.diffusion_model.out.2.weight"].cpu(),
                           U.synth_engine_state_dict(0)["model.diffusion_model.out.2.weight"])
    batch = U.tiny_batch(T, clips=1, device=gpu)
    runs = []
    for _ in range(2):
        torch.manual_seed(31)
        runs.append(eng.sample_video(batch)["sampled_video"])
    torch.manual_seed(31)
    out = fresh.sample_video(batch)["sampled_video"]
    _by_the_rule(out, runs[0], runs[1], "sample_video after the round trip")


# ------------------------------------------------------------------------------------------------------------------ 8
def test_encode_first_stage_draws_its_noise_per_chunk(gpu, ckpt):
    eng = _engine(gpu, ckpt, T=4, n_a_time=2)
    x = U.tiny_batch(4, clips=1)["jpg"]
    torch.manual_seed(17)
    z = eng.encode_first_stage(x.to(gpu))
    torch.cuda.synchronize()
    torch.manual_seed(17)
    noise = torch.cat([torch.randn(2, 4, 8, 8), torch.randn(2, 4, 8, 8)], 0)           # two chunks, in chunk order
    with torch.no_grad():
        moments = E.encoder_forward(U.sub_state_dict(U.synth_engine_state_dict(0), "first_stage_model.encoder."), E.TINY, x)
    mean, logvar = torch.chunk(moments, 2, dim=1)
    want = U.SCALE_FACTOR * (mean + torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0)) * noise)
    e = rel_l2(z, want)
    print(f"encode_first_stage, 2 frames at a time: rel-L2 {e:.3e} of scale (mean + std noise)")
    assert z.shape == (4, 4, 8, 8) and e < 2e-3                     # tests/test_encoder_gpu.py's TOL


# ------------------------------------------------------------------------------------------------------------------ 9
def test_run_inference_from_a_folder_of_frames(gpu, ckpt, tmp_path):
    import numpy as np
    from PIL import Image
    from gcd_amd import inference as I
    T = 4
    cfg_path = tmp_path / "infer_tiny.yaml"
    cfg = U.tiny_sgm_config(T=14, steps=25)                          # the call's own arguments win
    for k in ("loss_fn_config", "optimizer_config"):
        del cfg["params"][k]
    with open(cfg_path, "w") as f:
        yaml.safe_dump({"model": json.loads(json.dumps(cfg))}, f)          # (tuples to lists)
    frames_dir = tmp_path / "clip_rgb"
    frames_dir.mkdir()
    g = np.random.RandomState(3)
    for i in range(T):
        Image.fromarray(g.randint(0, 256, size=(64, 96, 3), dtype=np.uint8)).save(frames_dir / f"{i:04d}.png")
    model = I.load_model_bundle(str(gpu), cfg_path, ckpt, False, num_steps=5, num_frames=T)
    assert not model.training and model.device == gpu and model.sampler.num_steps == 5
    kw = dict(num_samples=1, num_frames=T, num_steps=5, frame_stride=1, frame_width=64, frame_height=64,
              controls=I.CameraControls(move_time=3))
    runs = []
    for r in range(3):
        torch.manual_seed(8)
        runs.append(I.run_inference(model, frames_dir, tmp_path / f"out{r}", **kw))
    out = runs[0]
    assert model.sampler.last_path == "fused"
    assert len(out["samples"]) == 1 and out["samples"][0].shape == (T, 3, 64, 64) and out["input_rgb"].shape == (T, 3, 64, 64)
    assert out["samples"][0].dtype == np.float32 and 0.0 <= out["samples"][0].min() and out["samples"][0].max() <= 1.0
    pred, inp = out["written"]
    assert [os.path.basename(p) for p in pred["frames"]] == [f"{i:04d}.png" for i in range(T)]
    assert all(os.path.isfile(p) for p in pred["frames"] + inp["frames"])
    assert pred["video"] == str(tmp_path / "out0" / "clip_rgb_pred_s0.mp4") and os.path.getsize(pred["video"]) > 0
    assert os.path.isfile(inp["video"])
    with Image.open(pred["frames"][0]) as im:
        assert im.size == (64, 64)
    a, b, c = (torch.from_numpy(r["samples"][0]) for r in runs)
    _by_the_rule(c, a, b, "run_inference under one seed")


# ----------------------------------------------------------------------------------------------------------------- 10
def test_time_lora_checkpoint_loaded_on_the_cpu_is_merged_on_the_gpu(gpu, ckpt, tmp_path):
    """The path of INTEGRATION.md: build on the CPU with `ckpt_path` (adapters with B != 0: no kernel can merge there),
    then `.to(gpu)`.  The live weights must hold W0 + s B A, not W0."""
    T = 4
    src = U.build(U.tiny_sgm_config(T=T, ft_strategy="time_lora"), ckpt_path=ckpt)
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    g = torch.Generator().manual_seed(23)
    for k in sd:
        if k.endswith(".lora_B.default.weight"):
            sd[k] = 0.05 * torch.randn(sd[k].shape, generator=g)
    path = str(tmp_path / "trained_lora.ckpt")
    torch.save({"state_dict": sd, "global_step": 3}, path)
    eng = U.build(U.tiny_sgm_config(T=T, ft_strategy="time_lora", ckpt_has_ema=True), ckpt_path=path)
    assert eng._lora_unmerged() and torch.equal(eng.lora.weights()[0], eng.lora.w0()[0])      # on the CPU: W0, and known
    eng = eng.to(gpu).eval()
    torch.cuda.synchronize()
    assert not eng._lora_unmerged()
    lora = eng.lora
    for n, m, w, a, b in zip(lora.names, lora.weights(), lora.w0(), lora.lora_A, lora.lora_B):
        pre = "model.diffusion_model." + n
        assert torch.equal(w.cpu(), sd[pre + ".base_layer.weight"]) and torch.equal(b.detach().cpu(), sd[pre + ".lora_B.default.weight"])
        want = w.double() + lora.scale * (b.detach().double() @ a.detach().double())
        err = float((m.detach().double() - want).abs().max())
        assert err <= 2.0 * 2.0 ** -24 * float(want.abs().max()), (n, err)
        assert float((m.detach() - w).abs().max()) > 0, f"{n} still holds W0"
    # and the network that samples is the merged one: the same engine with the adapters zeroed gives other latents
    batch = U.tiny_batch(T, clips=1, device=gpu)
    torch.manual_seed(41)
    z = eng.sample_video(batch)["sampled_z"]
    base = _engine(gpu, ckpt, T=T)
    torch.manual_seed(41)
    z0 = base.sample_video(batch)["sampled_z"]
    print(f"time_lora loaded on the CPU: latents differ from the base network's by rel-L2 {rel_l2(z, z0):.3e}")
    assert rel_l2(z, z0) > 1e-3
