"""The fine-tune loss on the device (libgcd_amd_loss.so, include/gcd_amd_loss.h): what
`training.StandardDiffusionLoss.get_loss` runs under the `hip` loss engine (training.set_loss_engine / GCD_TRAIN_LOSS=hip).

  class_weight_map(gt_rgb, latent_hw, classes)   the ParallelDomain class weight map: one launch, one read of the frames
  focal_loss(model_output, target, w, keep, ...)  the per-frame loss (BT,): one launch forward, one backward

`focal_loss` is differentiable in `model_output` only.  The forward leaves (tau, quota) per frame — the keep-th largest
per-element loss and how many elements equal to it are selected; the backward selects, among the elements equal to tau,
the lowest flat indices (this project's tie rule: torch.topk has none).  HIP only: CPU operands raise GcdError.  `keep` is
a launch argument that changes with the global step, so the loss stays outside any captured graph."""
from __future__ import annotations

import functools
from typing import Optional, Sequence

import torch

from . import _lib_loss, ops
from ._lib import GcdError

_TYPES = {"l2": _lib_loss.LOSS_L2, "l1": _lib_loss.LOSS_L1}


def class_table(classes: Sequence) -> torch.Tensor:
    """[((r, g, b) in 0..255, weight), ...] -> the fp32 [ncls, 4] host table (r, g, b, weight - 1) of gcd_loss_class_map,
    colours as `rgb / 127.5 - 1` in fp32 (what the torch path computes).  Built once per class list; read-only."""
    return _class_table(tuple((tuple(rgb), float(weight)) for rgb, weight in classes))


@functools.lru_cache(maxsize=16)
def _class_table(classes: tuple) -> torch.Tensor:
    if not 1 <= len(classes) <= _lib_loss.LOSS_MAX_CLASSES:
        raise GcdError(f"class_weight_map: {len(classes)} classes (1 .. {_lib_loss.LOSS_MAX_CLASSES})")
    tab = torch.empty(len(classes), 4, dtype=torch.float32)
    for k, (rgb, weight) in enumerate(classes):
        tab[k, :3] = torch.tensor(rgb, dtype=torch.float32) / 127.5 - 1.0
        tab[k, 3] = weight - 1.0
    return tab


def class_weight_map(gt_rgb: torch.Tensor, latent_hw, classes, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gt_rgb fp32 [BT, 3, Hp, Wp] in [-1, 1] -> [BT, 1, Hl, Wl]: per latent pixel, the sum over the classes of
    (weight - 1) x the fraction of the pixels of its F.interpolate(mode="area") bin whose colour matches the class.
    `classes`: [((r, g, b), weight), ...] or a table made by `class_table`."""
    ops._need_gpu(gt_rgb, out)
    tab = classes if torch.is_tensor(classes) else class_table(classes)
    if tab.is_cuda or tab.dtype != torch.float32 or tab.dim() != 2 or tab.shape[1] != 4 or not tab.is_contiguous():
        raise GcdError("class_weight_map: the class table is a contiguous fp32 [ncls, 4] tensor in host memory")
    if gt_rgb.dim() != 4 or gt_rgb.shape[1] != 3 or gt_rgb.dtype != torch.float32 or not gt_rgb.is_contiguous():
        raise GcdError(f"class_weight_map: gt_rgb must be contiguous fp32 [BT, 3, Hp, Wp], got {tuple(gt_rgb.shape)} {gt_rgb.dtype}")
    BT, _, Hp, Wp = gt_rgb.shape
    Hl, Wl = int(latent_hw[0]), int(latent_hw[1])
    if out is None:
        out = torch.empty(BT, 1, Hl, Wl, dtype=torch.float32, device=gt_rgb.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == BT * Hl * Wl
    _lib_loss.check(_lib_loss.load().gcd_loss_class_map(gt_rgb.data_ptr(), BT, Hp, Wp, tab.data_ptr(), tab.shape[0],
                                                        out.data_ptr(), Hl, Wl, ops._stream()), "gcd_loss_class_map")
    return out


def focal_fwd(out: torch.Tensor, tgt: torch.Tensor, w: torch.Tensor, wmap: Optional[torch.Tensor], keep: int, loss_type: str,
              loss: torch.Tensor, state: torch.Tensor) -> torch.Tensor:
    """gcd_loss_focal_fwd on prepared operands (contiguous fp32; state int32 [BT, 2])."""
    BT, n, HW = _focal_shapes(out, tgt, w, wmap)
    assert loss.dtype == torch.float32 and loss.is_contiguous() and loss.numel() == BT
    assert state.dtype == torch.int32 and state.is_contiguous() and state.numel() == 2 * BT
    ops._need_gpu(out, tgt, w, wmap, loss, state)
    _lib_loss.check(_lib_loss.load().gcd_loss_focal_fwd(out.data_ptr(), tgt.data_ptr(), w.data_ptr(), ops._p(wmap), BT, n, HW,
                                                        _TYPES[loss_type], int(keep), loss.data_ptr(), state.data_ptr(),
                                                        ops._stream()), "gcd_loss_focal_fwd")
    return loss


def focal_bwd(out: torch.Tensor, tgt: torch.Tensor, w: torch.Tensor, wmap: Optional[torch.Tensor], g: torch.Tensor,
              state: torch.Tensor, keep: int, loss_type: str, dout: torch.Tensor) -> torch.Tensor:
    """gcd_loss_focal_bwd on prepared operands: dout = d (sum_f g[f] loss[f]) / d out."""
    BT, n, HW = _focal_shapes(out, tgt, w, wmap)
    assert g.dtype == torch.float32 and g.is_contiguous() and g.numel() == BT
    assert state.dtype == torch.int32 and state.is_contiguous() and state.numel() == 2 * BT
    assert dout.dtype == torch.float32 and dout.is_contiguous() and dout.shape == out.shape
    ops._need_gpu(out, tgt, w, wmap, g, state, dout)
    _lib_loss.check(_lib_loss.load().gcd_loss_focal_bwd(out.data_ptr(), tgt.data_ptr(), w.data_ptr(), ops._p(wmap), g.data_ptr(),
                                                        state.data_ptr(), BT, n, HW, _TYPES[loss_type], int(keep),
                                                        dout.data_ptr(), ops._stream()), "gcd_loss_focal_bwd")
    return dout


def _focal_shapes(out, tgt, w, wmap):
    if out.dim() != 4 or out.shape != tgt.shape:
        raise GcdError(f"focal_loss: model_output {tuple(out.shape)} and target {tuple(tgt.shape)} must be the same [BT, C, H, W]")
    for name, t in (("model_output", out), ("target", tgt), ("w", w), ("wmap", wmap)):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise GcdError(f"focal_loss: {name} must be contiguous fp32")
    BT, C_, H, W = out.shape
    if w.numel() != BT:
        raise GcdError(f"focal_loss: w has {w.numel()} elements for {BT} frames")
    if wmap is not None and tuple(wmap.shape) != (BT, 1, H, W):
        raise GcdError(f"focal_loss: wmap {tuple(wmap.shape)} must be {(BT, 1, H, W)}")
    return BT, C_ * H * W, H * W


class _FocalLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out, tgt, w, wmap, keep, loss_type):
        BT = out.shape[0]
        loss = torch.empty(BT, dtype=torch.float32, device=out.device)
        state = torch.empty(BT, 2, dtype=torch.int32, device=out.device)
        focal_fwd(out, tgt, w, wmap, keep, loss_type, loss, state)
        ctx.save_for_backward(out, tgt, w, state) if wmap is None else ctx.save_for_backward(out, tgt, w, state, wmap)
        ctx.keep, ctx.loss_type = keep, loss_type
        return loss

    @staticmethod
    def backward(ctx, g):
        out, tgt, w, state, *rest = ctx.saved_tensors
        dout = torch.empty_like(out)
        focal_bwd(out, tgt, w, rest[0] if rest else None, g.to(torch.float32).contiguous(), state, ctx.keep, ctx.loss_type,
                  dout)
        return dout, None, None, None, None, None


def focal_loss(model_output: torch.Tensor, target: torch.Tensor, w: torch.Tensor, keep: int, loss_type: str = "l2",
               wmap: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The per-frame training loss (BT,) of loss.py:163-273 with the focal selection made by `keep`:

        raw = diff^2 | |diff|;  all = raw (1 + 0.5 wmap);  loss = (0.9 top_mean + 0.1 mean(all) + 0.5 mean(raw wmap)) w

    top_mean: the mean of the `keep` largest values of `all` (keep = int(n * cur_top), computed by the caller as the
    reference does; keep = 0: no focal selection, loss = (mean(all) + 0.5 mean(raw wmap)) w).  model_output, target:
    [BT, C, H, W]; w: BT values (any shape); wmap: [BT, 1, H, W] or None.  Differentiable in model_output only; target,
    w and wmap enter detached.  A model_output that is not contiguous fp32 is made so through ordinary torch ops, so
    autograd carries the cast."""
    if loss_type not in _TYPES:
        raise GcdError(f"focal_loss: loss_type must be 'l2' or 'l1', got {loss_type!r}")
    tensors = [t for t in (model_output, target, w, wmap) if t is not None]
    if not all(torch.is_tensor(t) for t in tensors):
        raise GcdError("focal_loss: operands must be tensors")
    ops._need_gpu(*tensors)
    if model_output.dim() != 4:
        raise GcdError(f"focal_loss: model_output must be [BT, C, H, W], got {tuple(model_output.shape)}")
    n = model_output[0].numel()
    keep = int(keep)
    if not 0 <= keep <= n:
        raise GcdError(f"focal_loss: keep={keep} outside [0, n={n}]")
    if n > _lib_loss.LOSS_MAX_N or model_output.shape[0] > _lib_loss.LOSS_MAX_BT:
        raise GcdError(f"focal_loss: {model_output.shape[0]} frames of {n} elements (at most {_lib_loss.LOSS_MAX_BT} of "
                       f"{_lib_loss.LOSS_MAX_N})")
    out = model_output.to(torch.float32).contiguous()

    def plain(t):
        return None if t is None else t.detach().to(torch.float32).contiguous()
    return _FocalLoss.apply(out, plain(target), plain(w).reshape(-1), plain(wmap), keep, loss_type)
