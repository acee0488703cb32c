"""GCD's own YAML configs without the reference's package: every `target:` string of the reference's `model:` sections
(gcd-model/configs/*.yaml) mapped to the class of `gcd_amd` that fills the same socket.

    cfg = load_config("configs/train_kubric_max90.yaml")        # the translated `model:` section
    engine = gcd_amd.util.instantiate_from_config(cfg)           # a gcd_amd.diffusion.DiffusionEngine

`TARGETS` holds the 23 strings the six configs use (tests/golden/configs/targets.txt) and the classes the project offers
beside them (the other samplers and guiders, CameraEmbedder, IdentityEncoder, the wrappers).  `torch.*` and `gcd_amd.*`
targets pass through; any other string raises `GcdError`: a socket is never filled by guessing.
"""
from __future__ import annotations

import copy
from typing import Any, Dict

from ._lib import GcdError

_DM = "sgm.modules.diffusionmodules."
_EM = "sgm.modules.encoders.modules."

TARGETS: Dict[str, str] = {
    # ---- the 23 of the reference's configs
    "sgm.models.diffusion.DiffusionEngine": "gcd_amd.diffusion.DiffusionEngine",
    "sgm.models.autoencoder.AutoencodingEngine": "gcd_amd.autoencoder.AutoencodingEngine",
    "sgm.models.autoencoder.AutoencoderKLModeOnly": "gcd_amd.ae_encoder.AutoencoderKLModeOnly",
    "sgm.modules.autoencoding.regularizers.DiagonalGaussianRegularizer": "gcd_amd.autoencoder.DiagonalGaussianRegularizer",
    "sgm.modules.autoencoding.temporal_ae.VideoDecoder": "gcd_amd.temporal_ae.VideoDecoder",
    "sgm.modules.GeneralConditioner": "gcd_amd.conditioning.GeneralConditioner",
    _DM + "denoiser.Denoiser": "gcd_amd.denoiser.Denoiser",
    _DM + "denoiser_scaling.VScalingWithEDMcNoise": "gcd_amd.denoiser_scaling.VScalingWithEDMcNoise",
    _DM + "discretizer.EDMDiscretization": "gcd_amd.discretizer.EDMDiscretization",
    _DM + "guiders.LinearPredictionGuider": "gcd_amd.guiders.LinearPredictionGuider",
    _DM + "loss.StandardDiffusionLoss": "gcd_amd.training.StandardDiffusionLoss",
    _DM + "loss_weighting.EDMWeighting": "gcd_amd.training.EDMWeighting",
    _DM + "sigma_sampling.EDMSampling": "gcd_amd.training.EDMSampling",
    _DM + "model.Encoder": "gcd_amd.ae_encoder.Encoder",
    _DM + "sampling.EulerEDMSampler": "gcd_amd.sampling.EulerEDMSampler",
    _DM + "video_model.VideoUNet": "gcd_amd.video_model.VideoUNet",
    _EM + "ConcatTimestepEmbedderND": "gcd_amd.conditioning.ConcatTimestepEmbedderND",
    _EM + "FrozenOpenCLIPImageEmbedder": "gcd_amd.clip_vision.FrozenOpenCLIPImageEmbedder",
    _EM + "FrozenOpenCLIPImagePredictionEmbedder": "gcd_amd.conditioning.FrozenOpenCLIPImagePredictionEmbedder",
    _EM + "SphericalEmbedder": "gcd_amd.conditioning.SphericalEmbedder",
    _EM + "VideoPredictionEmbedderWithEncoder": "gcd_amd.conditioning.VideoPredictionEmbedderWithEncoder",
    "torch.nn.Identity": "torch.nn.Identity",
    "torch.optim.Adam": "torch.optim.Adam",
    # ---- what the project offers beside them
    "sgm.modules.encoders.modules.GeneralConditioner": "gcd_amd.conditioning.GeneralConditioner",
    _EM + "CameraEmbedder": "gcd_amd.conditioning.CameraEmbedder",
    _EM + "IdentityEncoder": "gcd_amd.conditioning.IdentityEncoder",
    _DM + "sampling.HeunEDMSampler": "gcd_amd.sampling.HeunEDMSampler",
    _DM + "sampling.EulerAncestralSampler": "gcd_amd.sampling.EulerAncestralSampler",
    _DM + "sampling.DPMPP2SAncestralSampler": "gcd_amd.sampling.DPMPP2SAncestralSampler",
    _DM + "sampling.DPMPP2MSampler": "gcd_amd.sampling.DPMPP2MSampler",
    _DM + "guiders.VanillaCFG": "gcd_amd.guiders.VanillaCFG",
    _DM + "guiders.IdentityGuider": "gcd_amd.guiders.IdentityGuider",
    _DM + "wrappers.OpenAIWrapper": "gcd_amd.wrappers.OpenAIWrapper",
    _DM + "wrappers.IdentityWrapper": "gcd_amd.wrappers.IdentityWrapper",
    "sgm.modules.ema.LitEma": "gcd_amd.ema.LitEma",
    "sgm.modules.autoencoding.lpips.loss.lpips.LPIPS": "gcd_amd.lpips.LPIPS",
    "torch.optim.AdamW": "torch.optim.AdamW",
}

_TARGET_KEYS = ("target", "network_wrapper")


def translate_target(target: str) -> str:
    """One `target:` string -> the string to instantiate here."""
    if target in TARGETS:
        return TARGETS[target]
    if target.startswith(("torch.", "gcd_amd.")):
        return target
    raise GcdError(f"config target {target!r} has no counterpart in gcd_amd (known: gcd_amd.config.TARGETS)")


def translate_targets(cfg: Any) -> Any:
    """A deep copy of a plain dict / list config with every `target:` value and the `network_wrapper` string rewritten
    by `TARGETS`.  `torch.*` and `gcd_amd.*` targets stay; any other unknown target raises GcdError naming it."""
    if isinstance(cfg, dict):
        out = {}
        for k, v in cfg.items():
            if k in _TARGET_KEYS and isinstance(v, str):
                out[k] = translate_target(v)
            else:
                out[k] = translate_targets(v)
        return out
    if isinstance(cfg, (list, tuple)):
        return [translate_targets(v) for v in cfg]
    return copy.deepcopy(cfg)


def load_config(path) -> Dict[str, Any]:
    """The translated `model:` section ({'target', 'params', ...}) of a GCD YAML file.  The `data:` and `lightning:`
    sections (datasets, the Lightning trainer and its callbacks) are not read."""
    import yaml
    with open(path) as f:
        doc = yaml.safe_load(f)
    if not isinstance(doc, dict) or not isinstance(doc.get("model"), dict):
        raise GcdError(f"{path}: no `model:` section")
    return translate_targets(doc["model"])


def instantiate_model(cfg: Dict[str, Any], **overrides):
    """The model of a translated `model:` section: `instantiate_from_config` with `overrides` written over `params`
    (ckpt_path, use_ema, ...), and `learning_rate` set from `base_learning_rate` when the section has one (the
    reference's main.py does that on the instantiated model)."""
    from .util import instantiate_from_config
    cfg = dict(cfg, params=dict(cfg.get("params", {}), **overrides))
    model = instantiate_from_config(cfg)
    if cfg.get("base_learning_rate") is not None:
        model.learning_rate = float(cfg["base_learning_rate"])
    return model
