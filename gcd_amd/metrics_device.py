"""The evaluation metrics of `gcd_amd.metrics` computed on the device (libgcd_amd_metrics.so, include/gcd_amd_metrics.h).

`gcd_amd.metrics.calculate_metrics` is numpy / scipy on the host, like the reference: the decoded frames have to leave
the GPU first.  Here the decoder's output and the ground truth stay where they are; `frame_metrics` and `diversity` launch
two small kernels each and `calculate_metrics` brings back S x T x 6 + T x 3 doubles (and the uncertainty map, when asked
for) to build the dictionary of the host function, key for key.  The kernels work in fp64 on the fp32 frames, so their
values are the float64 evaluation of the inputs; the host function on float32 arrays differs from that by its own
float32 rounding (a few 1e-7).

Like gcd_amd.ops: the kernels launch on the current device's current stream and there is no CPU fallback — operands that
are not contiguous float32 GPU tensors raise GcdError.  `gcd_amd/metrics.py` is the oracle of this module.
"""
from __future__ import annotations

import warnings
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from .ops import _need_gpu, _stream

FRAME_NAMES = ("psnr", "ssim", "psnr_vis", "ssim_vis", "psnr_occ", "ssim_occ")     # the 6 values per (sample, frame)


def _operands(who: str, pred, gt, reproject):
    """Shape / dtype / layout checks shared by the entries; returns (S, T, H, W)."""
    ts = [t for t in (pred, gt, reproject) if t is not None]
    if not all(torch.is_tensor(t) for t in ts):
        raise _lib.GcdError(f"{who}: operands must be torch tensors on the GPU; there is no CPU fallback")
    _need_gpu(*ts)
    if any(t.dtype != torch.float32 for t in ts):
        raise _lib.GcdError(f"{who}: operands must be float32 (got {[str(t.dtype) for t in ts]})")
    if not all(t.is_contiguous() for t in ts):
        raise _lib.GcdError(f"{who}: operands must be contiguous")
    if pred.dim() != 5 or pred.shape[2] != 3:
        raise _lib.GcdError(f"{who}: pred must be [S, T, 3, H, W], got {tuple(pred.shape)}")
    S, T, _, H, W = pred.shape
    for name, t in (("gt", gt), ("reproject", reproject)):
        if t is not None and tuple(t.shape) != (T, 3, H, W):
            raise _lib.GcdError(f"{who}: {name} {tuple(t.shape)} does not fit pred {tuple(pred.shape)}: expected {(T, 3, H, W)}")
    return S, T, H, W


def _scratch(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=device)


def frame_metrics(pred: torch.Tensor, gt: torch.Tensor, reproject: Optional[torch.Tensor] = None,
                  signed: bool = False) -> torch.Tensor:
    """pred [S, T, 3, H, W], gt / reproject [T, 3, H, W] -> [S, T, 6] float64 on the device, in FRAME_NAMES order.
    `signed`: pred is the decoder's raw output in [-1, 1] (mapped with clamp((x + 1) / 2, 0, 1) on load).  Without
    `reproject` the four masked values are stored as 0 and mean nothing."""
    S, T, H, W = _operands("frame_metrics", pred, gt, reproject)
    lib = _lib.load_metrics()
    need = lib.gcd_metrics_frames_scratch_bytes(S, T, H, W)
    scratch = _scratch(need, pred.device)
    out = torch.empty(S, T, _lib.METRICS_FRAME_VALUES, dtype=torch.float64, device=pred.device)
    _lib.check_metrics(lib.gcd_metrics_frames_f32(
        pred.data_ptr(), gt.data_ptr(), 0 if reproject is None else reproject.data_ptr(), S, T, H, W,
        _lib.METRICS_SIGNED if signed else 0, scratch.data_ptr(), scratch.numel() * 8, out.data_ptr(), _stream()),
        "gcd_metrics_frames_f32")
    return out


def diversity(pred: torch.Tensor, reproject: Optional[torch.Tensor] = None,
              signed: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """pred [S, T, 3, H, W] -> (uncertainty [T, H, W] float32, per_frame [T, 3] float64), both on the device: the
    per-pixel standard deviation over the samples averaged over channels, and its per-frame mean over all, visible and
    occluded pixels (the last two 0 without `reproject`, NaN for an empty mask)."""
    S, T, H, W = _operands("diversity", pred, None, reproject)
    lib = _lib.load_metrics()
    need = lib.gcd_metrics_diversity_scratch_bytes(S, T, H, W)
    scratch = _scratch(need, pred.device)
    unc = torch.empty(T, H, W, dtype=torch.float32, device=pred.device)
    out = torch.empty(T, _lib.METRICS_DIVERSITY_VALUES, dtype=torch.float64, device=pred.device)
    _lib.check_metrics(lib.gcd_metrics_diversity_f32(
        pred.data_ptr(), 0 if reproject is None else reproject.data_ptr(), S, T, H, W,
        _lib.METRICS_SIGNED if signed else 0, unc.data_ptr(), scratch.data_ptr(), scratch.numel() * 8, out.data_ptr(),
        _stream()), "gcd_metrics_diversity_f32")
    return unc, out


def calculate_metrics(gt_rgb: torch.Tensor, reproject_rgb: Optional[torch.Tensor],
                      pred_samples: Union[torch.Tensor, Sequence[Dict[str, torch.Tensor]]], signed: bool = False,
                      return_uncertainty: bool = True) -> Tuple[Dict[str, np.ndarray], Optional[np.ndarray]]:
    """`gcd_amd.metrics.calculate_metrics` with device tensors: the same keys, shapes and dtypes.  pred_samples: a
    stacked [S, T, 3, H, W] tensor, or the reference's list of dicts with 'sampled_rgb' [T, 3, H, W] (stacked here, one
    device copy).  The uncertainty map comes back as a numpy array, or None when `return_uncertainty` is False."""
    if torch.is_tensor(pred_samples):
        pred = pred_samples
    elif len(pred_samples) == 0:
        pred = None
    else:
        frames = [p["sampled_rgb"] for p in pred_samples]
        if not all(torch.is_tensor(f) for f in frames):
            raise _lib.GcdError("calculate_metrics: 'sampled_rgb' must be torch tensors on the GPU; there is no CPU fallback")
        _need_gpu(*frames)
        pred = torch.stack(frames, dim=0)
    if pred is None or pred.shape[0] == 0:          # nothing to launch: the host function's answer for no samples
        from . import metrics as host
        md, unc = host.calculate_metrics(gt_rgb.cpu().numpy(), None if reproject_rgb is None else reproject_rgb.cpu().numpy(), [])
        return md, (unc if return_uncertainty else None)
    S, T, H, W = _operands("calculate_metrics", pred, gt_rgb, reproject_rgb)
    have_mask = reproject_rgb is not None
    fm = frame_metrics(pred, gt_rgb, reproject_rgb, signed)
    unc_dev, dv = diversity(pred, reproject_rgb, signed)
    flat = torch.cat((fm.reshape(-1), dv.reshape(-1))).cpu().numpy()          # the one synchronising copy
    fm_h = flat[:S * T * len(FRAME_NAMES)].reshape(S, T, len(FRAME_NAMES))
    dv_h = flat[S * T * len(FRAME_NAMES):].reshape(T, 3)
    md: Dict[str, np.ndarray] = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)              # nanmean of all-nan rows
        for i, n in enumerate(FRAME_NAMES if have_mask else FRAME_NAMES[:2]):
            arr = np.ascontiguousarray(fm_h[:, :, i])
            md["frame_" + n] = arr
            md["mean_" + n] = np.nanmean(arr, axis=1)
        # the host function's diversity values have the dtype of its float32 map
        md["frame_diversity"] = dv_h[:, 0].astype(np.float32)
        md["mean_diversity"] = np.nanmean(md["frame_diversity"])
        if have_mask:
            for col, tag in ((1, "vis"), (2, "occ")):
                fd = dv_h[:, col]
                # ... and float64 as soon as one frame's mask is empty (numpy's promotion of its python-float nan)
                fd = fd.copy() if np.isnan(fd).any() else fd.astype(np.float32)
                md["frame_diversity_" + tag] = fd
                md["mean_diversity_" + tag] = np.nanmean(fd)
    return md, (unc_dev.cpu().numpy() if return_uncertainty else None)
