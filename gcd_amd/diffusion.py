"""`DiffusionEngine`: the object that owns the stages.  A restatement of the reference's
`sgm.models.diffusion.DiffusionEngine` (diffusion.py:40-577, a `pl.LightningModule`) as a plain `nn.Module` over the HIP
classes of this package: same constructor keywords, same attribute names — so `state_dict()` carries a GCD checkpoint's
prefixes (`model.diffusion_model.`, `conditioner.embedders.N.`, `first_stage_model.encoder.` / `.decoder.`, `model_ema.`,
`lpips.`) — and the same methods.  What Lightning did around `training_step` is `fit_step`.

    cfg = gcd_amd.config.load_config("configs/train_kubric_max90.yaml")
    engine = gcd_amd.config.instantiate_model(cfg).to("cuda")
    loss = engine.fit_step(batch)                   # zero_grad, training_step, backward, optimizer, EMA, global_step
    video = engine.sample_video(batch)              # conditioner -> fused sampling loop -> VideoDecoder
    engine.save_checkpoint("last.ckpt")             # {"state_dict", "global_step"}: the reference reads it

Differences from the reference, all of them:
  * no autocast and no logger: `disable_first_stage_autocast`, `disable_loss_fn_autocast`, `log_keys`, `no_cond_log` are
    accepted and have no effect (the first is still propagated into the embedder configs, diffusion.py:97-105);
  * `scheduler_config` other than None raises NotImplementedError (no GCD config sets it);
  * the loss receives a `TrainDenoiser` (`self.train_denoiser`, the same `scaling_config`) where the reference hands the
    sampling `Denoiser` to both: the fine-tune step runs on the planned training engine, with input gradients whenever a
    trainable embedder has parameters;
  * `ft_strategy="time_lora"` is `gcd_amd.lora.TimeLora` (kept as `self.lora`), not peft: the network keeps its plain
    names and holds the merged weights; checkpoints are written and read under the reference's peft names.  The merge
    is a kernel: adapters loaded while the engine is on the CPU are merged when it reaches a GPU (`.to("cuda")`), and
    sampling or training on an unmerged network raises instead of running on W0;
  * `sample_video` hands the sampler a `FusedDenoiser` instead of a closure, and accepts the `force_uc=` /
    `keep_intermediate=` keywords the reference's `validation_step` passes (its own `sample_video` raises on them).
"""
from __future__ import annotations

import copy
import math
import os
from contextlib import contextmanager
from typing import Any, Dict, List, Optional, Tuple, Union

import torch
import torch.nn as nn

from ._lib import GcdError
from .conditioning import _disabled_train
from .ema import LitEma
from .lora import TimeLora, apply_ft_strategy
from .lpips import LPIPS
from .sampling import FusedDenoiser
from .temporal_ae import VideoDecoder
from .training import AdamHIP, TrainDenoiser
from .util import default, get_obj_from_str, instantiate_from_config
from .wrappers import OPENAIUNETWRAPPER

UNCONDITIONAL_CONFIG = {"target": "gcd_amd.conditioning.GeneralConditioner", "params": {"emb_models": []}}
UNET_PREFIX = "model.diffusion_model."


def _get(node, key, fallback=None):
    """A key of a config node that is a dict or an attribute container (OmegaConf-style)."""
    if isinstance(node, dict):
        return node.get(key, fallback)
    return getattr(node, key, fallback)


class DiffusionEngine(nn.Module):
    learning_rate: Optional[float] = None      # set by the caller (main.py:914-929 does so from `base_learning_rate`)

    def __init__(self, network_config, denoiser_config, first_stage_config, conditioner_config=None, sampler_config=None,
                 optimizer_config=None, scheduler_config=None, loss_fn_config=None, network_wrapper: Optional[str] = None,
                 ckpt_path: Optional[str] = None, ckpt_has_ema: bool = False, use_ema: bool = False,
                 ema_decay_rate: float = 0.9999, ablate_unet_scratch: bool = False, scale_factor: float = 1.0,
                 disable_first_stage_autocast=False, disable_loss_fn_autocast=False, input_key: str = "jpg",
                 log_keys: Union[List, None] = None, no_cond_log: bool = False, compile_model: bool = False,
                 en_and_decode_n_samples_a_time: Optional[int] = None, ft_strategy: str = "everything"):
        super().__init__()
        if scheduler_config is not None:
            raise NotImplementedError("gcd_amd DiffusionEngine: scheduler_config (learning-rate schedulers are not provided; "
                                      "no GCD config sets one)")
        self.input_key = input_key
        self.log_keys = log_keys
        self.ablate_unet_scratch = ablate_unet_scratch
        self.optimizer_config = default(optimizer_config, {"target": "torch.optim.AdamW"})
        model = instantiate_from_config(network_config)
        self.model = get_obj_from_str(default(network_wrapper, OPENAIUNETWRAPPER))(model, compile_model=compile_model)
        self.denoiser = instantiate_from_config(denoiser_config)
        self.sampler = instantiate_from_config(sampler_config) if sampler_config is not None else None

        # diffusion.py:97-105: these two cannot be overridden per embedder on a command line, so the engine's win
        conditioner_config = copy.deepcopy(default(conditioner_config, UNCONDITIONAL_CONFIG))
        for embedder in _get(_get(conditioner_config, "params", {}), "emb_models", []):
            params = _get(embedder, "params", None)
            if isinstance(params, dict) and "disable_encoder_autocast" in params and \
                    "en_and_decode_n_samples_a_time" in params:
                params["disable_encoder_autocast"] = disable_first_stage_autocast
                params["en_and_decode_n_samples_a_time"] = en_and_decode_n_samples_a_time
        self.disable_first_stage_autocast = disable_first_stage_autocast
        self.disable_loss_fn_autocast = disable_loss_fn_autocast

        self.conditioner = instantiate_from_config(conditioner_config)
        self.scheduler_config = scheduler_config
        self._init_first_stage(first_stage_config)

        self.loss_fn = instantiate_from_config(loss_fn_config) if loss_fn_config is not None else None
        # beside the sampling Denoiser: the training-mode denoiser the loss receives.  A trainable embedder with parameters
        # (the Kubric configs' SphericalEmbedder) gets its gradient from the planned pass's input gradients
        trainable = any(e.is_trainable and any(True for _ in e.parameters()) for e in self.conditioner.embedders)
        self.train_denoiser = TrainDenoiser(_get(_get(denoiser_config, "params", {}), "scaling_config"),
                                            input_grads=True if trainable else None)

        self.lora: Optional[TimeLora] = None        # a registered sub-module once set: `.to(device)` moves the adapters
        self.global_step = 0
        self._pending_lpips = None
        self._optimizer = None
        self._ema_in_optimizer = False

        # NOTE (reference): checkpoint loading is BEFORE the EMA setup if the EMA is not stored inside
        if ckpt_path is not None and not ckpt_has_ema:
            self.init_from_ckpt(ckpt_path)

        lora = apply_ft_strategy(self.model.diffusion_model, ft_strategy)      # diffusion.py:127-170
        if lora is not None:
            self.lora = lora
        self.ft_strategy = ft_strategy

        self.use_ema = use_ema
        if self.use_ema:
            # under time_lora the trainable tensors are the adapters (peft leaves those trainable in the reference too)
            self.model_ema = LitEma(self.lora if self.lora is not None else self.model, decay=ema_decay_rate)

        self.scale_factor = scale_factor
        self.no_cond_log = no_cond_log

        if ckpt_path is not None and ckpt_has_ema:
            self.init_from_ckpt(ckpt_path)

        self.en_and_decode_n_samples_a_time = en_and_decode_n_samples_a_time
        self.lpips = LPIPS().eval()
        if self._pending_lpips:                      # see init_from_ckpt
            self.lpips.load_state_dict(self._pending_lpips, strict=False)        # as the engine's own keys: not strict
        self._pending_lpips = None
        self.validation_step_outputs = []

    # ------------------------------------------------------------------------------------------------------ construction
    def _init_first_stage(self, config):                                  # diffusion.py:221-226
        model = instantiate_from_config(config).eval()
        model.train = _disabled_train.__get__(model)
        for param in model.parameters():
            param.requires_grad = False
        self.first_stage_model = model

    @property
    def device(self) -> torch.device:
        return next(self.model.parameters()).device

    def _lora_unmerged(self) -> bool:
        """Under time_lora: the live weights do not hold W0 + s B A of the current adapters (a checkpoint was loaded
        where no GPU could run the merge)."""
        return self.lora is not None and self.lora._merged != self.lora._versions()

    def _apply(self, fn, *args, **kwargs):
        """`.to()` / `.cuda()`: adapters that were loaded on the CPU are merged the moment the network reaches a GPU."""
        out = super()._apply(fn, *args, **kwargs)
        if self._lora_unmerged() and self.device.type == "cuda":
            self.lora.merge()
        return out

    def _ensure_merged(self) -> None:
        """Before any use of the network: never run on W0 while the adapters hold something else."""
        if self._lora_unmerged():
            if self.device.type != "cuda":
                raise GcdError("DiffusionEngine: the time_lora adapters were loaded without a GPU and are not merged into "
                               "the weights; move the engine to the GPU (`.to('cuda')`) before using it")
            self.lora.merge()

    # ------------------------------------------------------------------------------------------------------- checkpoints
    def _unet_reference_keys(self, sd: Dict[str, torch.Tensor]):
        """Under time_lora: split a checkpoint's `model.diffusion_model.*` part off and express it in TimeLora's reference
        names (`<layer>.base_layer.*`, `<layer>.lora_A|B.default.weight`); a plain-named tensor of an adapted layer is that
        layer's base weight.  Returns (rest of sd, complete reference dict, missing, unexpected)."""
        adapted = set(self.lora.names)
        cur = self.lora.reference_state_dict()
        rest, given = {}, {}
        for k, v in sd.items():
            if not k.startswith(UNET_PREFIX):
                rest[k] = v
                continue
            name = k[len(UNET_PREFIX):]
            layer, _, leaf = name.rpartition(".")
            given[f"{layer}.base_layer.{leaf}" if layer in adapted else name] = v
        unexpected = [UNET_PREFIX + k for k in given if k not in cur]
        missing = [UNET_PREFIX + k for k in cur if k not in given]
        full = {k: given.get(k, cur[k]) for k in cur}
        return rest, (full if given else None), missing, unexpected

    def init_from_ckpt(self, path: str) -> Tuple[List[str], List[str]]:
        """diffusion.py:191-219.  Returns (missing, unexpected) keys.

        One addition: the reference builds its LPIPS (from a weights file of its own) after both loading sites, so a
        checkpoint's `lpips.*` tensors never reach it.  No such file ships here: when this runs before `self.lpips`
        exists, the checkpoint's `lpips.*` tensors are set aside and loaded once the constructor has built it."""
        assert os.path.exists(path) and os.path.isfile(path), path
        if path.endswith("ckpt"):
            sd = torch.load(path, map_location="cpu", weights_only=False)["state_dict"]
        elif path.endswith("safetensors"):
            from safetensors.torch import load_file as load_safetensors
            sd = load_safetensors(path)
        else:
            raise NotImplementedError(path)
        if self.ablate_unet_scratch:
            # the (frozen) VAE and every embedder from the checkpoint, the U-Net left as initialised
            sd = {k: v for k, v in sd.items() if "diffusion" not in k.lower()}
        if "lpips" not in self._modules:
            self._pending_lpips = {k[len("lpips."):]: v for k, v in sd.items() if k.startswith("lpips.")}
            sd = {k: v for k, v in sd.items() if not k.startswith("lpips.")}
        missing, unexpected = self.load_state_dict(sd, strict=False)
        print(f"Restored from {path} with {len(missing)} missing and {len(unexpected)} unexpected keys")
        if missing:
            print(f"Missing keys: {len(missing)}; first 10: {missing[0:10]}")
        if unexpected:
            print(f"Unexpected keys: {len(unexpected)}; first 5: {unexpected[0:5]}")
        return missing, unexpected

    def state_dict(self, *args, **kwargs):
        """nn.Module.state_dict.  Under time_lora the `model.diffusion_model.*` part carries the reference's peft names
        (`TimeLora.reference_state_dict`: `<layer>.base_layer.*` = W0, `<layer>.lora_A|B.default.weight`) in place of
        the merged weights, and the adapters are not listed a second time under `lora.`."""
        sd = super().state_dict(*args, **kwargs)
        if self.lora is None:
            return sd
        prefix = kwargs.get("prefix", "")
        for k in [k for k in sd if k.startswith((prefix + UNET_PREFIX, prefix + "lora."))]:
            del sd[k]
        for k, v in self.lora.reference_state_dict().items():
            sd[prefix + UNET_PREFIX + k] = v
        return sd

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """nn.Module.load_state_dict; under time_lora the `model.diffusion_model.*` part goes through
        `TimeLora.load_reference_state_dict` (W0, the adapters, then the merge), whichever of the two namings it has."""
        if self.lora is None:
            return super().load_state_dict(state_dict, strict=strict, assign=assign)
        rest, full, missing_u, unexpected_u = self._unet_reference_keys(dict(state_dict))
        res = super().load_state_dict(rest, strict=False, assign=assign)
        missing = [k for k in res.missing_keys if not k.startswith((UNET_PREFIX, "lora."))] + missing_u
        unexpected = list(res.unexpected_keys) + unexpected_u
        if full is not None:
            self.lora.load_reference_state_dict(full, merge=self.device.type == "cuda")
        if strict and (missing or unexpected):
            raise RuntimeError(f"DiffusionEngine.load_state_dict: missing {missing[:4]}, unexpected {unexpected[:4]}")
        res.missing_keys[:] = missing
        res.unexpected_keys[:] = unexpected
        return res

    def checkpoint_state_dict(self) -> Dict[str, torch.Tensor]:
        """`state_dict()` as a checkpoint holds it: copies on the CPU."""
        return {k: v.detach().cpu().clone() for k, v in self.state_dict().items()}

    def save_checkpoint(self, path: str) -> None:
        """{"state_dict", "global_step"} by torch.save: what the reference's `init_from_ckpt` (and this one) reads."""
        torch.save({"state_dict": self.checkpoint_state_dict(), "global_step": int(self.global_step)}, path)

    # ------------------------------------------------------------------------------------------------------- first stage
    def get_input(self, batch):
        return batch[self.input_key]

    @torch.no_grad()
    def decode_first_stage(self, z):                                       # diffusion.py:233-251
        z = 1.0 / self.scale_factor * z
        n_samples = default(self.en_and_decode_n_samples_a_time, z.shape[0])
        n_rounds = math.ceil(z.shape[0] / n_samples)
        all_out = []
        for n in range(n_rounds):
            if isinstance(self.first_stage_model.decoder, VideoDecoder):
                kwargs = {"timesteps": len(z[n * n_samples: (n + 1) * n_samples])}
            else:
                kwargs = {}
            out = self.first_stage_model.decode(z[n * n_samples: (n + 1) * n_samples], **kwargs)
            all_out.append(out)
        return torch.cat(all_out, dim=0)

    @torch.no_grad()
    def encode_first_stage(self, x):                                       # diffusion.py:253-266
        n_samples = default(self.en_and_decode_n_samples_a_time, x.shape[0])
        n_rounds = math.ceil(x.shape[0] / n_samples)
        all_out = []
        for n in range(n_rounds):
            out = self.first_stage_model.encode(x[n * n_samples: (n + 1) * n_samples])
            all_out.append(out)
        z = torch.cat(all_out, dim=0)
        z = self.scale_factor * z
        return z

    # ---------------------------------------------------------------------------------------------------------- training
    def forward(self, x, batch):                                           # diffusion.py:268-277
        loss = self.loss_fn(self.model, self.train_denoiser, self.conditioner, x, batch)
        loss_mean = loss.mean()
        return loss_mean, {"loss": loss_mean}

    def shared_step(self, batch: Dict) -> Any:                             # diffusion.py:279-289
        x = self.get_input(batch)
        x = self.encode_first_stage(x)
        batch["global_step"] = self.global_step
        loss, loss_dict = self(x, batch)
        return loss, loss_dict

    def training_step(self, batch, batch_idx=0):                           # diffusion.py:291-315, nothing logged
        self._ensure_merged()
        loss, _ = self.shared_step(batch)
        return loss

    def on_train_start(self, *args, **kwargs):
        if self.sampler is None or self.loss_fn is None:
            raise ValueError("Sampler and loss function need to be set for training.")

    def on_train_batch_end(self, *args, **kwargs):                         # diffusion.py:383-385
        if self.use_ema and not self._ema_in_optimizer:
            self.model_ema(self.lora if self.lora is not None else self.model)

    def optimizer_parameters(self) -> List[nn.Parameter]:
        """diffusion.py:412-418: the wrapped model's parameters, then every trainable embedder's.  Under time_lora the
        model's part is the adapters (the merged weights are written by `TimeLora.merge`, never by the optimizer)."""
        params = list(self.lora.parameters()) if self.lora is not None else list(self.model.parameters())
        for embedder in self.conditioner.embedders:
            if embedder.is_trainable:
                params = params + list(embedder.parameters())
        return params

    def instantiate_optimizer_from_config(self, params, lr, cfg):
        """diffusion.py:407-410, with torch.optim.Adam -> AdamHIP and torch.optim.AdamW -> AdamHIP(decoupled weight decay);
        the EMA, when kept, rides in the optimizer's update pass.  Any other target is instantiated as given."""
        target, kw = cfg["target"], dict(cfg.get("params", dict()))
        if target in ("torch.optim.Adam", "torch.optim.AdamW"):
            if target.endswith("AdamW"):
                kw["decoupled_weight_decay"] = True
                kw.setdefault("weight_decay", 1e-2)                          # torch.optim.AdamW's default
            if self.use_ema:
                kw["ema"] = self.model_ema
            self._ema_in_optimizer = self.use_ema
            return AdamHIP(params, lr=lr, **kw)
        self._ema_in_optimizer = False
        return get_obj_from_str(target)(params, lr=lr, **kw)

    def configure_optimizers(self):                                        # diffusion.py:412-431
        if self.learning_rate is None:
            raise GcdError("DiffusionEngine.configure_optimizers: set engine.learning_rate first (the configs' "
                           "base_learning_rate; gcd_amd.config.instantiate_model does)")
        opt = self.instantiate_optimizer_from_config(self.optimizer_parameters(), self.learning_rate,
                                                     self.optimizer_config)
        self._optimizer = opt
        return opt

    def optimizers(self):
        return self._optimizer if self._optimizer is not None else self.configure_optimizers()

    def fit_step(self, batch: Dict) -> torch.Tensor:
        """What Lightning's fit loop does around `training_step` for one batch.  Returns the detached loss."""
        opt = self.optimizers()
        opt.zero_grad()
        if self.lora is not None:
            self.lora.zero_grad()
        loss = self.training_step(batch, self.global_step)
        scaled = opt.scale(loss) if getattr(opt, "loss_scale", None) is not None else loss
        scaled.backward()
        if self.lora is not None:
            self.lora.step(opt)
        else:
            opt.step()
        self.on_train_batch_end()
        self.global_step += 1
        return loss.detach()

    # --------------------------------------------------------------------------------------------------------------- EMA
    @contextmanager
    def ema_scope(self, context=None):                                     # diffusion.py:387-405
        target = self.lora if self.lora is not None else self.model
        if self.use_ema:
            self.model_ema.store(target.parameters())
            self.model_ema.copy_to(target)
            if self.lora is not None:
                self.lora.merge()
            if context is not None:
                print(f"{context}: Switched to EMA weights")
        elif context is not None:
            print(f"{context}: EMA is disabled; using training weights as is")
        try:
            yield None
        finally:
            if self.use_ema:
                self.model_ema.restore(target.parameters())
                if self.lora is not None:
                    self.lora.merge()
                if context is not None:
                    print(f"{context}: Restored training weights")

    # ---------------------------------------------------------------------------------------------------------- sampling
    @torch.no_grad()
    def sample(self, cond: Dict, uc: Union[Dict, None] = None, batch_size: int = 16,
               shape: Union[None, Tuple, List] = None, **kwargs):          # diffusion.py:433-448
        self._ensure_merged()
        randn = torch.randn(batch_size, *shape).to(self.device)
        return self.sampler(FusedDenoiser(self.denoiser, self.model, **kwargs), randn, cond, uc=uc)

    @torch.no_grad()
    def sample_video(self, batch, enter_ema=False, limit_batch=False, **ignored):
        """diffusion.py:504-577.  `**ignored`: the reference's `validation_step` passes `force_uc=` and
        `keep_intermediate=`, which its own `sample_video` does not accept (the reference raises there); here they are
        accepted and have no effect."""
        if enter_ema:
            with self.ema_scope("Sampling"):
                return self.sample_video(batch, enter_ema=False, limit_batch=limit_batch)

        self._ensure_merged()
        if isinstance(limit_batch, int) and limit_batch >= 1:      # (True counts as 1, as in the reference)
            # only the first K (usually 1) examples of the batch
            B, T = batch["idx"].shape[0], batch["num_video_frames"]
            batch_old = batch
            batch = dict()
            batch.update({k: v[0:T * limit_batch] for k, v in batch_old.items()
                          if torch.is_tensor(v) and v.shape[0] >= B * T})
            batch.update({k: v[0:limit_batch] for k, v in batch_old.items()
                          if torch.is_tensor(v) and v.shape[0] < B * T})
            batch.update({k: v for k, v in batch_old.items() if not torch.is_tensor(v)})

        c, uc = self.conditioner.get_unconditional_conditioning(
            batch, batch_uc=batch, force_uc_zero_embeddings=["cond_frames", "cond_frames_without_noise"])

        additional_model_inputs = {}
        additional_model_inputs["num_video_frames"] = batch["num_video_frames"]
        additional_model_inputs["image_only_indicator"] = batch["image_only_indicator"].repeat_interleave(2, dim=0)
        # the reference's closure `denoiser(input, sigma, c)` (:531-532) with its captured objects visible to the sampler
        denoiser = FusedDenoiser(self.denoiser, self.model, **additional_model_inputs)

        BT, Cp, Hp, Wp = batch["cond_frames"].shape
        assert Cp == 3
        latent_shape = (BT, 4, Hp // 8, Wp // 8)
        latent_noise = torch.randn(latent_shape, device=batch["cond_frames"].device)
        samples_z = self.sampler(denoiser, latent_noise, cond=c, uc=uc).detach()
        samples_x = self.decode_first_stage(samples_z).detach()
        sampled_video = torch.clamp((samples_x + 1.0) / 2.0, min=0.0, max=1.0)
        gt_video = torch.clamp((batch["jpg"] + 1.0) / 2.0, min=0.0, max=1.0) if "jpg" in batch else None
        cond_video = torch.clamp((batch["cond_frames"] + 1.0) / 2.0, min=0.0, max=1.0)

        extra_info = {k: v.detach().cpu() for k, v in batch.items() if torch.is_tensor(v) and v.shape.numel() <= 256}
        extra_info.update({k: v for k, v in batch.items() if not torch.is_tensor(v)})
        video_dict = {"cond_video": cond_video, "sampled_z": samples_z, "sampled_video": sampled_video,
                      "extra": extra_info}
        if gt_video is not None:
            video_dict["gt_video"] = gt_video
        return video_dict

    # -------------------------------------------------------------------------------------------------------- validation
    def validation_step(self, batch, batch_idx=0) -> Dict[str, float]:
        """diffusion.py:317-364 with the metrics on the device (gcd_amd.validation): the first clip of the batch, sampled
        under the EMA weights when they are kept, against `batch['jpg']`."""
        from .validation import validation_metrics
        with self.ema_scope("Validation"):
            with torch.no_grad():
                video_dict = self.sample_video(batch, enter_ema=False, limit_batch=1, force_uc=False,
                                               keep_intermediate=False)
                metrics_dict = validation_metrics(video_dict["gt_video"].contiguous(),
                                                  video_dict["sampled_video"].contiguous(), self.lpips)
        self.validation_step_outputs.append(metrics_dict)
        return metrics_dict

    def on_validation_epoch_end(self) -> Dict[str, float]:                 # diffusion.py:366-377
        outs = self.validation_step_outputs
        if not outs:
            return {"step": self.global_step}
        metrics_dict = {k: float(sum(out[k] for out in outs) / len(outs)) for k in outs[0]}
        metrics_dict["step"] = self.global_step
        self.validation_step_outputs.clear()
        return metrics_dict
