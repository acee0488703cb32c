"""CPU: the standalone DiffusionEngine — GCD's own configs translated to gcd_amd classes (gcd_amd/config.py), the engine's
assembly, key contract and checkpoints (gcd_amd/diffusion.py, gcd_amd/autoencoder.py) and the host pieces of the
inference script (gcd_amd/inference.py).  Where the reference tree is present, the chunking of the first stage and the
checkpoint format are checked against the reference's own unmodified methods, called unbound."""
import types

import numpy as np
import pytest
import torch
import yaml

import engine_util as U


def _walk_targets(node, found):
    if isinstance(node, dict):
        for k, v in node.items():
            if k in ("target", "network_wrapper") and isinstance(v, str):
                found.add(v)
            else:
                _walk_targets(v, found)
    elif isinstance(node, list):
        for v in node:
            _walk_targets(v, found)
    return found


def _fixture(name):
    with open(U.CONFIGS / f"{name}.yaml") as f:
        return yaml.safe_load(f)


# ---------------------------------------------------------------------------------------------------------------- config
def test_every_target_of_the_six_configs_translates_to_an_importable_class():
    from gcd_amd import config as C
    from gcd_amd.util import get_obj_from_str
    listed = set((U.CONFIGS / "targets.txt").read_text().split())
    assert len(listed) == 23
    source = set()
    for name in U.CONFIG_NAMES:
        doc = _fixture(name)
        assert set(doc) == {"model"}, "the fixtures hold the model section only"
        source |= _walk_targets(doc["model"], set())
        translated = C.load_config(U.CONFIGS / f"{name}.yaml")
        for t in _walk_targets(translated, set()):
            assert t.startswith(("gcd_amd.", "torch.")), t
            assert isinstance(get_obj_from_str(t), type), t
    assert source == listed
    assert listed <= set(C.TARGETS)
    assert C.TARGETS["sgm.models.diffusion.DiffusionEngine"] == "gcd_amd.diffusion.DiffusionEngine"
    assert C.TARGETS["sgm.modules.encoders.modules.FrozenOpenCLIPImageEmbedder"].startswith("gcd_amd.clip_vision.")
    for t in ("loss.StandardDiffusionLoss", "loss_weighting.EDMWeighting", "sigma_sampling.EDMSampling"):
        assert C.TARGETS["sgm.modules.diffusionmodules." + t].startswith("gcd_amd.training.")
    for t in C.TARGETS.values():               # the ones beside the configs' resolve too
        assert isinstance(get_obj_from_str(t), type), t


def test_translate_targets_copies_passes_torch_and_names_unknown_targets():
    from gcd_amd import config as C
    from gcd_amd._lib import GcdError
    cfg = {"target": "sgm.modules.GeneralConditioner", "network_wrapper": "sgm.modules.diffusionmodules.wrappers.OpenAIWrapper",
           "params": {"emb_models": [{"target": "torch.nn.Identity", "params": {"a": [1, 2]}},
                                     {"target": "gcd_amd.conditioning.IdentityEncoder"}]}}
    out = C.translate_targets(cfg)
    assert out["target"] == "gcd_amd.conditioning.GeneralConditioner"
    assert out["network_wrapper"] == "gcd_amd.wrappers.OpenAIWrapper"
    assert [e["target"] for e in out["params"]["emb_models"]] == ["torch.nn.Identity", "gcd_amd.conditioning.IdentityEncoder"]
    out["params"]["emb_models"][0]["params"]["a"].append(3)
    assert cfg["params"]["emb_models"][0]["params"]["a"] == [1, 2] and cfg["target"].startswith("sgm.")
    with pytest.raises(GcdError, match="sgm.modules.encoders.modules.FrozenT5Embedder"):
        C.translate_targets({"x": [{"target": "sgm.modules.encoders.modules.FrozenT5Embedder"}]})
    with pytest.raises(GcdError, match="main.ImageLogger"):
        C.translate_targets({"target": "main.ImageLogger"})


# ------------------------------------------------------------------------------------------------------ the full section
@pytest.fixture(scope="module")
def full_engine():
    """train_kubric_max90's model section, unmodified but for the checkpoint path and the CLIP tower's init_device, on the
    meta device."""
    from gcd_amd import config as C
    cfg = C.load_config(U.CONFIGS / "train_kubric_max90.yaml")
    cfg["params"]["ckpt_path"] = None
    cfg["params"]["conditioner_config"]["params"]["emb_models"][0]["params"]["open_clip_embedding_config"]["params"][
        "init_device"] = "meta"
    with torch.device("meta"):
        return C.instantiate_model(cfg)


def test_full_kubric_section_builds_with_the_checkpoint_key_contract(full_engine):
    from gcd_amd.diffusion import DiffusionEngine
    eng = full_engine
    assert type(eng) is DiffusionEngine and eng.learning_rate == 2e-5 and eng.global_step == 0
    keys = list(eng.state_dict())
    parts = {"model.diffusion_model.": eng.model.diffusion_model, "conditioner.": eng.conditioner,
             "first_stage_model.encoder.": eng.first_stage_model.encoder,
             "first_stage_model.decoder.": eng.first_stage_model.decoder, "lpips.": eng.lpips}
    union = [p + k for p, m in parts.items() for k in m.state_dict()]
    assert sorted(keys) == sorted(union) and len(set(keys)) == len(keys)
    count = lambda p: sum(1 for k in keys if k.startswith(p))      # noqa: E731
    assert count("model.diffusion_model.") == 1432
    assert count("first_stage_model.encoder.") == 106 and count("first_stage_model.decoder.") == 266
    assert count("conditioner.embedders.") == 504 and count("lpips.") == len(eng.lpips.state_dict()) > 0
    assert any(k.startswith("conditioner.embedders.0.open_clip.model.visual.") for k in keys)
    assert "conditioner.embedders.5.proj.weight" in keys and "conditioner.embedders.3.encoder.quant_conv.weight" in keys
    assert not any(k.startswith(("model_ema.", "lora.", "denoiser.", "train_denoiser.", "loss_fn.")) for k in keys)
    # frozen first stage, pinned to eval
    assert all(not p.requires_grad for p in eng.first_stage_model.parameters())
    eng.train()
    assert not eng.first_stage_model.training and eng.model.training
    eng.eval()
    # diffusion.py:97-105: the engine's two settings overwrite the embedder's own
    assert eng.conditioner.embedders[3].en_and_decode_n_samples_a_time == 2 == eng.en_and_decode_n_samples_a_time
    assert eng.conditioner.embedders[3].disable_encoder_autocast is True
    # the loss gets the training denoiser, with input gradients: SphericalEmbedder is trainable
    from gcd_amd.training import StandardDiffusionLoss, TrainDenoiser
    assert isinstance(eng.loss_fn, StandardDiffusionLoss) and isinstance(eng.train_denoiser, TrainDenoiser)
    assert eng.train_denoiser.input_grads is True and type(eng.train_denoiser.scaling) is type(eng.denoiser.scaling)


def test_optimizer_gets_the_model_then_the_trainable_embedder(full_engine):
    from gcd_amd.training import AdamHIP
    eng = full_engine
    want = list(eng.model.parameters()) + list(eng.conditioner.embedders[5].parameters())
    got = eng.optimizer_parameters()
    assert len(got) == len(want) == len(list(eng.model.parameters())) + 2 and all(a is b for a, b in zip(got, want))
    opt = eng.configure_optimizers()
    assert isinstance(opt, AdamHIP) and opt.lr == 2e-5 and not opt.decoupled_weight_decay and opt.ema is None
    assert len(opt.params) == len(want) and all(a is b for a, b in zip(opt.params, want))
    assert opt.params[-1] is eng.conditioner.embedders[5].proj.bias


def test_adamw_maps_to_decoupled_decay_and_other_optimizers_are_taken_as_given():
    with torch.device("meta"):
        eng = U.build(U.tiny_sgm_config(init_device="meta", optimizer_config={"target": "torch.optim.SGD",
                                                                               "params": {"momentum": 0.5}}))
    eng.learning_rate = 1e-3
    opt = eng.configure_optimizers()
    assert isinstance(opt, torch.optim.SGD) and opt.param_groups[0]["momentum"] == 0.5 and opt.param_groups[0]["lr"] == 1e-3
    eng.optimizer_config = {"target": "torch.optim.AdamW"}
    assert eng.instantiate_optimizer_from_config([torch.nn.Parameter(torch.zeros(2, device="meta"))], 1e-3,
                                                 eng.optimizer_config).weight_decay == 1e-2


def test_scheduler_config_and_unknown_strategy_raise():
    cfg = U.tiny_sgm_config(init_device="meta")
    with torch.device("meta"):
        with pytest.raises(NotImplementedError):
            U.build(cfg, scheduler_config={"target": "torch.nn.Identity"})
        with pytest.raises(NotImplementedError):
            U.build(cfg, ft_strategy="space")


def test_ft_strategies_on_the_tiny_network():
    from gcd_amd.lora import DUMMY_PARAM, TimeLora
    cfg = U.tiny_sgm_config(init_device="meta")
    with torch.device("meta"):
        every, time, dummy, lora = (U.build(cfg, ft_strategy=s) for s in ("everything", "time", "dummy", "time_lora"))
    assert every.lora is None and all(p.requires_grad for p in every.model.parameters())
    flags = {n: p.requires_grad for n, p in time.model.diffusion_model.named_parameters()}
    assert flags == {n: "time" in n for n in flags} and any(flags.values()) and not all(flags.values())
    flags = {n for n, p in dummy.model.diffusion_model.named_parameters() if p.requires_grad}
    assert flags == {DUMMY_PARAM}
    assert isinstance(lora.lora, TimeLora) and lora.lora.unet is lora.model.diffusion_model
    adapted = {id(w) for w in lora.lora.weights()}
    assert all(p.requires_grad == (id(p) in adapted) for p in lora.model.parameters())        # frozen but for the merge
    got = lora.optimizer_parameters()
    want = list(lora.lora.parameters()) + list(lora.conditioner.embedders[5].parameters())
    assert len(got) == len(want) and all(a is b for a, b in zip(got, want))
    # the state dict carries the reference's peft names, once
    keys = set(lora.state_dict())
    name = lora.lora.names[0]
    assert {f"model.diffusion_model.{name}.base_layer.weight", f"model.diffusion_model.{name}.lora_A.default.weight",
            f"model.diffusion_model.{name}.lora_B.default.weight"} <= keys
    assert f"model.diffusion_model.{name}.weight" not in keys and not any(k.startswith("lora.") for k in keys)
    assert len(keys) == len(every.state_dict()) + 2 * len(lora.lora.names)


def test_time_lora_adapters_loaded_without_a_gpu_are_known_unmerged_and_refuse_use(tmp_path):
    from gcd_amd._lib import GcdError
    src = U.build(U.tiny_sgm_config(ft_strategy="time_lora"))
    assert not src._lora_unmerged()                       # B = 0: the weights hold W0, which is the merge
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    for k in sd:
        if k.endswith(".lora_B.default.weight"):
            sd[k] = torch.ones_like(sd[k])
    path = str(tmp_path / "lora.ckpt")
    torch.save({"state_dict": sd, "global_step": 0}, path)
    eng = U.build(U.tiny_sgm_config(ft_strategy="time_lora", ckpt_has_ema=True), ckpt_path=path)
    assert eng._lora_unmerged() and bool(eng.lora.lora_B[0].detach().eq(1).all())
    eng = eng.to("cpu")                                   # no GPU reached: still unmerged, nothing raised
    assert eng._lora_unmerged()
    batch = U.tiny_batch(4)
    for use in (lambda: eng.sample_video(batch), lambda: eng.training_step(batch),
                lambda: eng.sample({}, batch_size=4, shape=(4, 8, 8))):
        with pytest.raises(GcdError, match="not merged"):
            use()


# -------------------------------------------------------------------------------------------- against the reference's own
class _RecordingFirstStage:
    """encode / decode that record what they were handed and return something that depends on it."""

    def __init__(self, decoder):
        self.decoder = decoder
        self.calls = []

    def encode(self, x):
        self.calls.append(("encode", x.clone(), {}))
        return x[:, :2] * 3.0 + 1.0

    def decode(self, z, **kwargs):
        self.calls.append(("decode", z.clone(), dict(kwargs)))
        return z.repeat(1, 2, 1, 1) - 0.5


def _same_calls(a, b):
    assert len(a) == len(b) > 0
    for (na, ta, ka), (nb, tb, kb) in zip(a, b):
        assert na == nb and ka == kb and ta.shape == tb.shape and torch.equal(ta, tb)


@pytest.mark.parametrize("n_a_time,frames", [(None, 4), (2, 4), (3, 7), (14, 14), (5, 3)])
@pytest.mark.parametrize("video", [True, False], ids=["video_decoder", "image_decoder"])
def test_first_stage_chunking_makes_the_references_calls(n_a_time, frames, video):
    from oracle import ref_shim
    if not ref_shim.available():
        pytest.skip("reference tree not mounted (GPU box)")
    from gcd_amd.diffusion import DiffusionEngine
    from gcd_amd.temporal_ae import VideoDecoder
    ref = ref_shim.reference_diffusion_module()
    dec_ref = ref.VideoDecoder.__new__(ref.VideoDecoder) if video else object()
    dec_own = VideoDecoder.__new__(VideoDecoder) if video else object()
    g = torch.Generator().manual_seed(frames)
    x, z = torch.randn(frames, 3, 4, 4, generator=g), torch.randn(frames, 4, 2, 2, generator=g)
    outs = []
    for cls, dec in ((ref.DiffusionEngine, dec_ref), (DiffusionEngine, dec_own)):
        stub = types.SimpleNamespace(first_stage_model=_RecordingFirstStage(dec), scale_factor=0.18215,
                                     en_and_decode_n_samples_a_time=n_a_time, disable_first_stage_autocast=True)
        outs.append((cls.encode_first_stage(stub, x), cls.decode_first_stage(stub, z), stub.first_stage_model.calls))
    (ze_r, xd_r, calls_r), (ze, xd, calls) = outs
    _same_calls(calls, calls_r)
    assert torch.equal(ze, ze_r) and torch.equal(xd, xd_r)
    dec_calls = [c for c in calls if c[0] == "decode"]
    n = frames if n_a_time is None else n_a_time
    assert [c[1].shape[0] for c in dec_calls] == [min(n, frames - i) for i in range(0, frames, n)]
    assert all(c[2] == ({"timesteps": c[1].shape[0]} if video else {}) for c in dec_calls)
    # scale_factor: the decoder sees z / s, the encoder's output is multiplied afterwards
    assert torch.equal(torch.cat([c[1] for c in dec_calls]), 1.0 / 0.18215 * z)
    assert torch.equal(torch.cat([c[1] for c in calls if c[0] == "encode"]), x)
    assert torch.equal(ze, 0.18215 * (x[:, :2] * 3.0 + 1.0))


def _cpu_engine(**kw):
    return U.build(U.tiny_sgm_config(), **kw)


def test_reference_init_from_ckpt_reads_what_save_checkpoint_writes(tmp_path):
    from oracle import ref_shim
    if not ref_shim.available():
        pytest.skip("reference tree not mounted (GPU box)")
    from safetensors.torch import save_file
    ref = ref_shim.reference_diffusion_module()
    torch.manual_seed(3)
    src = _cpu_engine(use_ema=True)
    src.global_step = 7
    ck = str(tmp_path / "step7.ckpt")
    src.save_checkpoint(ck)
    blob = torch.load(ck, map_location="cpu", weights_only=True)
    assert set(blob) == {"state_dict", "global_step"} and blob["global_step"] == 7
    assert any(k.startswith("model_ema.") for k in blob["state_dict"])
    st = str(tmp_path / "step7.safetensors")
    save_file({k: v.contiguous() for k, v in blob["state_dict"].items()}, st)
    for path in (ck, st):
        torch.manual_seed(4)
        dst = _cpu_engine(use_ema=True)
        seen = {}
        real = dst.load_state_dict

        def spy(sd, strict=True):
            res = real(sd, strict=strict)
            seen.update(missing=list(res.missing_keys), unexpected=list(res.unexpected_keys), strict=strict)
            return res
        dst.load_state_dict = spy
        ref.DiffusionEngine.init_from_ckpt(dst, path)           # the reference's unmodified method, unbound
        assert seen == {"missing": [], "unexpected": [], "strict": False}
        a, b = src.state_dict(), dst.state_dict()
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    # and this engine's own reader, with the ablation filter: the U-Net (and its EMA) stay as initialised
    torch.manual_seed(5)
    abl = _cpu_engine(use_ema=True, ablate_unet_scratch=True)
    before = {k: v.clone() for k, v in abl.state_dict().items()}
    missing, unexpected = abl.init_from_ckpt(ck)
    assert not unexpected and missing and all("diffusion" in k.lower() for k in missing)
    after, a = abl.state_dict(), src.state_dict()
    assert all(torch.equal(after[k], before[k] if "diffusion" in k.lower() else a[k]) for k in after)


def test_ckpt_path_loads_early_without_ema_and_late_with_it(tmp_path):
    torch.manual_seed(6)
    src = _cpu_engine(use_ema=True)
    with torch.no_grad():
        for b in src.model_ema.buffers():
            if b.dtype == torch.float32 and b.dim() > 0:
                b.add_(1.0)
    ck = str(tmp_path / "ema.ckpt")
    src.save_checkpoint(ck)
    a = src.state_dict()
    late = _cpu_engine(use_ema=True, ckpt_has_ema=True, ckpt_path=ck)
    b = late.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    # early: the shadows are made from the loaded weights, the checkpoint's model_ema.* never arrive; lpips.* do
    early = _cpu_engine(use_ema=True, ckpt_has_ema=False, ckpt_path=ck)
    c = early.state_dict()
    assert all(torch.equal(a[k], c[k]) for k in a if not k.startswith("model_ema."))
    name = next(n for n, _ in early.model.named_parameters())
    assert torch.equal(c["model_ema." + name.replace(".", "")], c["model." + name])


# ----------------------------------------------------------------------------------------------------------- regularizer
def test_diagonal_gaussian_regularizer_draws_the_references_noise():
    from gcd_amd.autoencoder import DiagonalGaussianRegularizer
    g = torch.Generator().manual_seed(1)
    z = torch.randn(3, 8, 4, 4, generator=g)
    reg = DiagonalGaussianRegularizer()
    mean, logvar = z[:, :4], z[:, 4:]
    torch.manual_seed(77)
    want = mean + torch.exp(0.5 * logvar) * torch.randn(mean.shape)
    torch.manual_seed(77)
    got = reg.sample(z)
    assert torch.equal(got, want)
    torch.manual_seed(77)
    out, log = reg(z)
    assert torch.equal(out, want) and set(log) == {"kl_loss"}
    kl = 0.5 * torch.sum(mean ** 2 + torch.exp(logvar) - 1.0 - logvar, dim=[1, 2, 3])
    assert torch.allclose(log["kl_loss"], kl.sum() / 3)
    assert torch.equal(reg.mode(z), mean)
    out, _ = DiagonalGaussianRegularizer(sample=False)(z)
    assert torch.equal(out, mean)
    # the clamp of logvar to [-30, 20]
    big = torch.cat([torch.zeros(1, 4, 2, 2), torch.full((1, 4, 2, 2), 1e3)], 1)
    small = torch.cat([torch.zeros(1, 4, 2, 2), torch.full((1, 4, 2, 2), -1e3)], 1)
    torch.manual_seed(5)
    eps = torch.randn(1, 4, 2, 2)
    torch.manual_seed(5)
    assert torch.equal(reg.sample(big), torch.exp(torch.tensor(10.0)) * eps)
    torch.manual_seed(5)
    assert torch.equal(reg.sample(small), torch.exp(torch.tensor(-15.0)) * eps)
    assert torch.isfinite(reg(big)[1]["kl_loss"])


def test_autoencoding_engine_names_and_ignored_keywords():
    from gcd_amd import config as C
    from gcd_amd.util import instantiate_from_config
    cfg = C.translate_targets(U.tiny_sgm_config()["params"]["first_stage_config"])
    cfg["params"].update(optimizer_config={"target": "torch.optim.Adam"}, lr_g_factor=2.0, disc_start_iter=5,
                         ckpt_engine=None, monitor="val/rec_loss", input_key="jpg")
    with torch.device("meta"):
        ae = instantiate_from_config(cfg)
    keys = list(ae.state_dict())
    assert keys and all(k.startswith(("encoder.", "decoder.")) for k in keys)
    assert len([k for k in keys if k.startswith("encoder.")]) == 106


# ------------------------------------------------------------------------------------------------------------- inference
def test_construct_batch_keys_shapes_motion_value_and_last_frame_repeat():
    from gcd_amd import inference as I
    Tc, Hp, Wp = 14, 8, 16
    g = torch.Generator().manual_seed(2)
    rgb = torch.rand(Tc, 3, Hp, Wp, generator=g).numpy()
    torch.manual_seed(9)
    b = I.construct_batch(rgb, 30.0, 15.0, 1.0, 4, 12, 127, 0.02, False, None, "cpu")
    assert set(b) == {"motion_bucket_id", "fps_id", "cond_aug", "cond_frames_without_noise", "cond_frames", "jpg",
                      "image_only_indicator", "num_video_frames", "scaled_relative_angles"}
    assert b["num_video_frames"] == Tc
    for k, shape, dt in [("motion_bucket_id", (Tc,), torch.int32), ("fps_id", (Tc,), torch.int32),
                         ("cond_aug", (Tc,), torch.float32), ("cond_frames", (Tc, 3, Hp, Wp), torch.float32),
                         ("cond_frames_without_noise", (Tc, 3, Hp, Wp), torch.float32),
                         ("jpg", (Tc, 3, Hp, Wp), torch.float32), ("image_only_indicator", (1, Tc), torch.float32),
                         ("scaled_relative_angles", (Tc, 3), torch.float32)]:
        assert tuple(b[k].shape) == shape and b[k].dtype == dt, k
    # by hand: |(30, 15)| / |(90, 30)| = 33.541 / 94.868 = 0.35355; 0 + 255 * 0.35355 = 90.16 -> 90
    assert b["motion_bucket_id"].tolist() == [90] * Tc and I.motion_value(30.0, 15.0, I.CameraControls()) == 90
    assert b["fps_id"].tolist() == [12] * Tc and float(b["jpg"].abs().max()) == 0.0
    # 4 of 14 frames given: frames 4 .. 13 repeat frame 3
    clean = b["cond_frames_without_noise"]
    want = torch.from_numpy(rgb) * 2.0 - 1.0
    assert torch.equal(clean[:4], want[:4]) and all(torch.equal(clean[t], want[3]) for t in range(4, Tc))
    torch.manual_seed(9)
    assert torch.equal(b["cond_frames"], clean + torch.randn_like(clean) * 0.02)
    # the trajectory: linear over move_time 13 frames, radians
    assert torch.allclose(b["scaled_relative_angles"][1], torch.tensor([30.0 / 13 * np.pi / 180, 15.0 / 13 * np.pi / 180,
                                                                          1.0 / 13]), atol=1e-6)
    # a custom bucket is kept when forced, or when the model was not trained with synchronised values
    assert I.construct_batch(rgb, 30.0, 15.0, 1.0, Tc, 12, 33, 0.02, True, None, "cpu")["motion_bucket_id"].tolist() == [33] * Tc
    fixed = I.CameraControls(motion_bucket_range=[127, 127])
    from gcd_amd._lib import GcdError
    with pytest.raises(GcdError, match="move_time"):
        I.construct_batch(rgb[:6], 30.0, 15.0, 1.0, 6, 12, 33, 0.02, False, None, "cpu")
    assert I.construct_batch(rgb, 30.0, 15.0, 1.0, Tc, 12, 33, 0.02, False, fixed, "cpu")["motion_bucket_id"].tolist() == [33] * Tc


def test_process_image_crop_boxes_and_bilinear_resize():
    from gcd_amd import inference as I
    # 5:3 input (W 500, H 300) to 384 x 256 (aspect 1.5): 1.667 > 1.502 -> crop the width to int(300 * 1.5) = 450,
    # x1 = (500 - 450) // 2 = 25
    assert I.center_crop_box(300, 500, 384 / 256) == (0, 300, 25, 475)
    # 1:2 input (W 100, H 200): 0.5 < 1.498 -> crop the height to int(100 / 1.5) = 66, y1 = (200 - 66) // 2 = 67
    assert I.center_crop_box(200, 100, 384 / 256) == (67, 133, 0, 100)
    assert I.center_crop_box(256, 384, 1.5) is None and I.center_crop_box(1000, 1501, 1.5) is None
    g = np.random.RandomState(0)
    img = g.randint(0, 256, size=(200, 100, 4), dtype=np.uint8)          # RGBA: the fourth channel is dropped
    assert np.array_equal(I.center_crop_numpy(img, 1.5), img[67:133])
    out = I.process_image(img, True, 384, 256)
    assert out.shape == (3, 256, 384) and out.dtype == np.float32 and -1.0 <= out.min() and out.max() <= 1.0
    # no resize needed: exactly rgb / 255 * 2 - 1 of the crop, channels first
    same = I.process_image(img, True, 100, 66)
    assert np.array_equal(same, np.transpose((img[67:133, :, :3] / 255.0).astype(np.float32) * 2.0 - 1.0, (2, 0, 1)))
    # half-pixel-centre bilinear without antialias: 2 -> 4 samples of a ramp are 0, .25, .75, 1 of the step (edges clamp)
    ramp = np.tile(np.array([[0.0], [1.0]], dtype=np.float32)[None], (1, 1, 3)).reshape(1, 2, 3)
    up = I.resize_bilinear(ramp, 4, 1)
    assert np.allclose(up[0, :, 0], [0.0, 0.25, 0.75, 1.0])
    # and 4 -> 2 takes the mean of the two nearest samples, not of an antialias window
    down = I.resize_bilinear(np.array([0.0, 1.0, 5.0, 2.0], dtype=np.float32).reshape(1, 4, 1), 2, 1)
    assert np.allclose(down[0, :, 0], [0.5, 3.5])


def test_loaders_read_files_and_folders_and_refuse_video(tmp_path):
    from PIL import Image
    from gcd_amd import inference as I
    from gcd_amd._lib import GcdError
    g = np.random.RandomState(1)
    frames = [g.randint(0, 256, size=(64, 96, 3), dtype=np.uint8) for _ in range(3)]
    d = tmp_path / "clip"
    d.mkdir()
    for i, f in enumerate(frames):
        Image.fromarray(f).save(d / f"{i:04d}.png")
    (d / "notes.txt").write_text("not a frame")
    clip = I.load_image_or_video(d, [0, 1, 2, 3], True, 96, 64)
    assert clip.shape == (4, 3, 64, 96)
    want = [np.transpose((f / 255.0).astype(np.float32) * 2.0 - 1.0, (2, 0, 1)) for f in frames]
    assert all(np.array_equal(clip[i], want[min(i, 2)]) for i in range(4)) and I.frames_in(d, [0, 1, 2, 3]) == 3
    still = I.load_image_or_video(d / "0001.png", [0, 2, 4], True, 96, 64)
    assert still.shape == (3, 3, 64, 96) and all(np.array_equal(still[i], want[1]) for i in range(3))
    with pytest.raises(GcdError, match="video files are not read"):
        I.load_image_or_video(tmp_path / "clip.mp4", [0], True, 96, 64)


def test_limit_batch_true_counts_as_one_clip_and_frames_in_counts_files_only(tmp_path):
    """`limit_batch=True` limits to one clip, as in the reference (diffusion.py:510: True is an int >= 1); a sub-folder
    with an image's extension is no frame."""
    from PIL import Image
    from gcd_amd import inference as I
    from gcd_amd.diffusion import DiffusionEngine
    seen = {}

    class Stop(Exception):
        pass

    class Cond:
        def get_unconditional_conditioning(self, batch, **kw):
            seen.update(batch)
            raise Stop

    stub = types.SimpleNamespace(_ensure_merged=lambda: None, conditioner=Cond())
    batch = U.tiny_batch(4, clips=2)
    with pytest.raises(Stop):
        DiffusionEngine.sample_video.__wrapped__(stub, batch, limit_batch=True)
    assert seen["jpg"].shape[0] == 4 and seen["idx"].shape[0] == 1 and seen["image_only_indicator"].shape == (1, 4)
    d = tmp_path / "clip"
    (d / "x.png").mkdir(parents=True)
    for i in range(2):
        Image.fromarray(np.zeros((8, 8, 3), dtype=np.uint8)).save(d / f"{i:04d}.png")
    assert I.image_files_in(d) == ["0000.png", "0001.png"] and I.frames_in(d, [0, 1, 2]) == 2
    assert I.load_image_or_video(d, [0, 1, 2], False, 8, 8).shape == (3, 3, 8, 8)


def test_cli_arguments():
    from gcd_amd import infer
    a = infer.parse_args(["--input", "a", "b", "--output", "o", "--config", "c.yaml", "--checkpoint", "m.ckpt", "--steps", "5",
                          "--frames", "4", "--samples", "1", "--delta_azimuth", "10", "--frame_width", "64",
                          "--frame_height", "64"])
    assert (a.input, a.num_steps, a.num_frames, a.num_samples, a.delta_azimuth) == (["a", "b"], 5, 4, 1, 10.0)
    assert (a.guider_max_scale, a.guider_min_scale, a.motion_id, a.cond_aug, a.decoding_t) == (1.5, 1.0, 127, 0.02, 14)
    assert (a.delta_elevation, a.delta_radius, a.frame_start, a.frame_stride, a.center_crop) == (15.0, 0.0, 0, 2, 1)
