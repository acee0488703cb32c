"""The tail of the reference's `DiffusionEngine.validation_step` (diffusion.py:317-364) on the device: per-frame LPIPS,
PSNR and SSIM of a sampled clip against its ground truth, and their three means.

The reference moves every frame to the host for skimage's PSNR / SSIM and calls LPIPS frame by frame.  Here the frames
stay where they are: `gcd_amd.lpips.LPIPS` takes all frames as one batch (its `value_range="unit"` does the reference's
`frames * 2 - 1` inside the packing kernel), `gcd_amd.metrics_device.frame_metrics` computes
`peak_signal_noise_ratio(data_range=1)` and `structural_similarity(channel_axis=0, data_range=1)` per frame (its first
two values with one sample), the three means are taken in float64 on the device, and one transfer brings them back.
"""
from __future__ import annotations

from typing import Dict

import torch

from . import metrics_device
from ._lib import GcdError
from .lpips import LPIPS


def validation_metrics(gt_video: torch.Tensor, sampled_video: torch.Tensor, lpips: LPIPS) -> Dict[str, float]:
    """gt_video, sampled_video: contiguous fp32 frames [B T, 3, H, W] in [0, 1] on the GPU (the reference's
    `video_dict["gt_video"]` / `["sampled_video"]`).  Returns {'lpips', 'psnr', 'ssim'}: Python floats, the means over
    the frames, as `validation_step` appends them to `validation_step_outputs`."""
    if not isinstance(lpips, LPIPS):
        raise GcdError(f"validation_metrics: lpips must be a gcd_amd.lpips.LPIPS, got {type(lpips).__name__}")
    d = lpips(gt_video, sampled_video, value_range="unit")                       # checks the operands: [F, 1, 1, 1]
    fm = metrics_device.frame_metrics(sampled_video.unsqueeze(0), gt_video)      # [1, F, 6] float64
    means = torch.stack((d.double().mean(), fm[0, :, 0].mean(), fm[0, :, 1].mean())).cpu()      # the one synchronising copy
    return {"lpips": float(means[0]), "psnr": float(means[1]), "ssim": float(means[2])}
