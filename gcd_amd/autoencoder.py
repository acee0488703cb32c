"""The first stage as the reference's configs name it: `sgm.models.autoencoder.AutoencodingEngine` (autoencoder.py:121-241)
over the HIP `Encoder` and `VideoDecoder`, with `DiagonalGaussianRegularizer` (regularizers/__init__.py:13-31) between them.

Only what `DiffusionEngine` reaches is here: `encode`, `decode`, the parameter names `encoder.*` / `decoder.*` of the
checkpoints.  The autoencoder's own training (discriminator losses, its optimizers, `ckpt_engine`) is accepted in the
constructor and ignored: no GCD config reaches it, the first stage is frozen.

The encoder and decoder run on libgcd_amd kernels; the regularizer is elementwise torch on their output, as in the
reference.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple, Union

import torch
import torch.nn as nn

from .util import instantiate_from_config


class DiagonalGaussianRegularizer(nn.Module):
    """regularizers/__init__.py:13-31 with the `DiagonalGaussianDistribution` it builds (distributions.py:24-72) folded
    in: `forward(moments) -> (z, {"kl_loss"})`, z the sample (`sample=True`, the default) or the mode.

    The reference keeps the flag as the attribute `sample`; here that name is the method, the flag is `do_sample`."""

    def __init__(self, sample: bool = True):
        super().__init__()
        self.do_sample = bool(sample)

    def get_trainable_parameters(self):
        yield from ()

    @staticmethod
    def moments(z: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(mean, logvar clamped to [-30, 20]) of the moments tensor (distributions.py:27-28)."""
        mean, logvar = torch.chunk(z, 2, dim=1)
        return mean, torch.clamp(logvar, -30.0, 20.0)

    def mode(self, z: torch.Tensor) -> torch.Tensor:
        return self.moments(z)[0]

    def sample(self, z: torch.Tensor) -> torch.Tensor:
        """distributions.py:37-41, exactly: the noise is drawn by `torch.randn(mean.shape)` — the default (CPU) generator —
        and then moved to the moments' device, so one `torch.manual_seed` gives the reference's latents."""
        mean, logvar = self.moments(z)
        std = torch.exp(0.5 * logvar)
        return mean + std * torch.randn(mean.shape).to(device=z.device)

    @staticmethod
    def kl(mean: torch.Tensor, logvar: torch.Tensor) -> torch.Tensor:
        """distributions.py:47-51 against the standard normal, per sample."""
        return 0.5 * torch.sum(torch.pow(mean, 2) + torch.exp(logvar) - 1.0 - logvar, dim=[1, 2, 3])

    def forward(self, z: torch.Tensor) -> Tuple[torch.Tensor, dict]:
        mean, logvar = self.moments(z)
        out = self.sample(z) if self.do_sample else mean
        kl_loss = self.kl(mean, logvar)
        return out, {"kl_loss": torch.sum(kl_loss) / kl_loss.shape[0]}


class AutoencodingEngine(nn.Module):
    """autoencoder.py:121-241, the inference side.  `loss_config` is instantiated (the configs give torch.nn.Identity) so
    that the attribute exists; every other keyword of the reference's constructor (autoencoder.py:128-147 and the
    AbstractAutoencoder keywords behind its **kwargs) is accepted and has no effect."""

    def __init__(self, *args, encoder_config: Dict, decoder_config: Dict, loss_config: Dict, regularizer_config: Dict,
                 optimizer_config: Optional[Dict] = None, lr_g_factor: float = 1.0, trainable_ae_params=None,
                 ae_optimizer_args=None, trainable_disc_params=None, disc_optimizer_args=None, disc_start_iter: int = 0,
                 diff_boost_factor: float = 3.0, ckpt_engine=None, ckpt_path: Optional[str] = None,
                 additional_decode_keys=None, **kwargs):
        super().__init__()
        self.encoder: nn.Module = instantiate_from_config(encoder_config)
        self.decoder: nn.Module = instantiate_from_config(decoder_config)
        self.loss: nn.Module = instantiate_from_config(loss_config)
        self.regularization: nn.Module = instantiate_from_config(regularizer_config)
        self.additional_decode_keys = set(additional_decode_keys or [])

    def encode(self, x: torch.Tensor, return_reg_log: bool = False,
               unregularized: bool = False) -> Union[torch.Tensor, Tuple[torch.Tensor, dict]]:
        z = self.encoder(x)
        if unregularized:
            return z, dict()
        z, reg_log = self.regularization(z)
        if return_reg_log:
            return z, reg_log
        return z

    def decode(self, z: torch.Tensor, **kwargs) -> torch.Tensor:
        return self.decoder(z, **kwargs)

    def forward(self, x: torch.Tensor, **additional_decode_kwargs):
        z, reg_log = self.encode(x, return_reg_log=True)
        return z, self.decode(z, **additional_decode_kwargs), reg_log
