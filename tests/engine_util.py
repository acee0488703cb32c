"""Shared by tests/test_engine_host.py and tests/test_engine_gpu.py (a helper module like clip_util.py, not a conftest): the
tiny `model:` section written with the reference's `sgm.*` target strings, and a synthetic checkpoint for it."""
from __future__ import annotations

from pathlib import Path

import torch

from oracle import svd_unet_ref as O, vae_decoder_ref as D, vae_encoder_ref as E, weights

CONFIGS = Path(__file__).resolve().parent / "golden" / "configs"
CONFIG_NAMES = ("infer_kubric", "infer_pardom", "train_kubric_max90", "train_kubric_max180", "train_pardom_rgb",
                "train_pardom_semantic")
UCFG = O.UNetConfig(model_channels=64, context_dim=64, adm_in_channels=96, aux_emb_dim=32)
CLIP_TINY = dict(width=160, layers=2, heads=2, mlp_width=640, patch_size=14, image_size=56, embed_dim=64)
CLIP_SEED = 101
SCALE_FACTOR = 0.18215
_DM = "sgm.modules.diffusionmodules."
_EM = "sgm.modules.encoders.modules."


def tiny_sgm_config(T=4, steps=5, max_scale=1.5, ucg_rate=0.0, n_a_time=None, init_device=None, **engine_kw) -> dict:
    """train_kubric_max90's `model:` section at test size: the same sockets, embedders and order, `sgm.*` targets."""
    enc_dd = dict(E.TINY.as_reference_kwargs(), attn_type="vanilla-xformers")
    clip_params = dict(freeze=True, vision_cfg=dict(CLIP_TINY))
    if init_device is not None:
        clip_params["init_device"] = init_device
    params = dict(
        scale_factor=SCALE_FACTOR, disable_first_stage_autocast=True, disable_loss_fn_autocast=True,
        en_and_decode_n_samples_a_time=n_a_time,
        optimizer_config={"target": "torch.optim.Adam"},
        denoiser_config={"target": _DM + "denoiser.Denoiser", "params": {
            "scaling_config": {"target": _DM + "denoiser_scaling.VScalingWithEDMcNoise"}}},
        network_config={"target": _DM + "video_model.VideoUNet", "params": UCFG.as_reference_kwargs()},
        conditioner_config={"target": "sgm.modules.GeneralConditioner", "params": {"emb_models": [
            dict(input_key="cond_frames_without_noise", is_trainable=False, ucg_rate=ucg_rate,
                 target=_EM + "FrozenOpenCLIPImagePredictionEmbedder", params=dict(
                     n_cond_frames=1, n_copies=1, open_clip_embedding_config={
                         "target": _EM + "FrozenOpenCLIPImageEmbedder", "params": clip_params})),
            dict(input_key="fps_id", is_trainable=False, target=_EM + "ConcatTimestepEmbedderND", params=dict(outdim=32)),
            dict(input_key="motion_bucket_id", is_trainable=True, target=_EM + "ConcatTimestepEmbedderND",
                 params=dict(outdim=32)),
            dict(input_key="cond_frames", is_trainable=False, ucg_rate=ucg_rate,
                 target=_EM + "VideoPredictionEmbedderWithEncoder", params=dict(
                     disable_encoder_autocast=True, en_and_decode_n_samples_a_time=2, n_cond_frames=1, n_copies=1,
                     is_ae=True, encoder_config={"target": "sgm.models.autoencoder.AutoencoderKLModeOnly", "params": {
                         "embed_dim": 4, "monitor": "val/rec_loss", "ddconfig": enc_dd,
                         "lossconfig": {"target": "torch.nn.Identity"}}})),
            dict(input_key="cond_aug", is_trainable=False, target=_EM + "ConcatTimestepEmbedderND", params=dict(outdim=32)),
            dict(input_key="scaled_relative_angles", is_trainable=True, target=_EM + "SphericalEmbedder",
                 params=dict(embed_dim=32, zero_init=False))]}},
        sampler_config={"target": _DM + "sampling.EulerEDMSampler", "params": {
            "num_steps": steps,
            "discretization_config": {"target": _DM + "discretizer.EDMDiscretization", "params": {"sigma_max": 700.0}},
            "guider_config": {"target": _DM + "guiders.LinearPredictionGuider",
                              "params": {"num_frames": T, "max_scale": max_scale, "min_scale": 1.0}}}},
        loss_fn_config={"target": _DM + "loss.StandardDiffusionLoss", "params": {
            "harmonize_sigmas": True, "focus_top": 0.1, "focus_steps": 5000,
            "batch2model_keys": ["image_only_indicator", "num_video_frames"],
            "loss_weighting_config": {"target": _DM + "loss_weighting.EDMWeighting", "params": {"sigma_data": 1.0}},
            "sigma_sampler_config": {"target": _DM + "sigma_sampling.EDMSampling",
                                     "params": {"p_mean": 1.0, "p_std": 1.6}}}},
        first_stage_config={"target": "sgm.models.autoencoder.AutoencodingEngine", "params": {
            "loss_config": {"target": "torch.nn.Identity"},
            "regularizer_config": {"target": "sgm.modules.autoencoding.regularizers.DiagonalGaussianRegularizer"},
            "encoder_config": {"target": _DM + "model.Encoder", "params": E.TINY.as_reference_kwargs()},
            "decoder_config": {"target": "sgm.modules.autoencoding.temporal_ae.VideoDecoder",
                               "params": D.TINY.as_reference_kwargs()}}})
    params.update(engine_kw)
    return {"base_learning_rate": 2e-5, "target": "sgm.models.diffusion.DiffusionEngine", "params": params}


def build(cfg: dict, **overrides):
    """The engine of an `sgm.*`-named section, through translate_targets."""
    from gcd_amd import config as C
    return C.instantiate_model(C.translate_targets(cfg), **overrides)


_SD = {}


def synth_engine_state_dict(salt: int = 0) -> dict:
    """Seeded weights under the engine's own keys (fp32, CPU; made once per salt and never written to): every stage from
    oracle.weights, the CLIP tower from its own seeded generator; LPIPS's fixed input scaling is left as constructed."""
    if salt not in _SD:
        from gcd_amd import clip_vision as cv
        with torch.device("meta"):
            eng = build(tiny_sgm_config(init_device="meta"))
        shapes = {k: tuple(v.shape) for k, v in eng.state_dict().items() if not k.startswith("lpips.scaling_layer.")}
        sd = weights.synth_state_dict(shapes, salt)
        clip_prefix = "conditioner.embedders.0.open_clip.model.visual."
        for k, v in cv.seeded_state_dict(CLIP_TINY, CLIP_SEED + salt).items():
            assert tuple(sd[clip_prefix + k].shape) == tuple(v.shape), k
            sd[clip_prefix + k] = v
        _SD[salt] = {k: v.contiguous() for k, v in sd.items()}
    return _SD[salt]


def write_checkpoint(path, salt: int = 0) -> str:
    """`synth_engine_state_dict(salt)` as a .safetensors or a .ckpt ({"state_dict", "global_step"}) file."""
    sd = synth_engine_state_dict(salt)
    path = str(path)
    if path.endswith(".safetensors"):
        from safetensors.torch import save_file
        save_file({k: v.clone() for k, v in sd.items()}, path)
    else:
        torch.save({"state_dict": sd, "global_step": 0}, path)
    return path


def sub_state_dict(sd: dict, prefix: str) -> dict:
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def tiny_batch(T: int, clips: int = 1, Hp: int = 64, Wp: int = 64, seed: int = 55, device="cpu") -> dict:
    """A training / sampling batch in the data modules' format: (clips T) leading rows, `idx` per clip."""
    from gcd_amd.camera import scaled_relative_angles
    g = torch.Generator().manual_seed(seed)
    n = clips * T
    frames = torch.rand(n, 3, Hp, Wp, generator=g) * 2.0 - 1.0
    target = torch.rand(n, 3, Hp, Wp, generator=g) * 2.0 - 1.0
    batch = {"jpg": target, "cond_frames_without_noise": frames,
             "cond_frames": frames + 0.02 * torch.randn(n, 3, Hp, Wp, generator=g),
             "fps_id": torch.full((n,), 12.0), "motion_bucket_id": torch.full((n,), 127.0),
             "cond_aug": torch.full((n,), 0.02),
             "scaled_relative_angles": torch.cat([scaled_relative_angles(30.0 + 10.0 * c, 15.0, 1.0, num_frames=T, move_time=min(13, T - 1))
                                                  for c in range(clips)], 0),
             "image_only_indicator": torch.zeros(clips, T), "idx": torch.arange(clips)}
    batch = {k: v.to(device) for k, v in batch.items()}
    batch["num_video_frames"] = T
    return batch
