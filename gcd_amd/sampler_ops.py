"""torch-tensor wrapper of libgcd_amd_sampler.so (include/gcd_amd_sampler.h): the sampler-stage kernel.

Like gcd_amd.ops: the kernel launches on the current device's current stream, allocates nothing and has no CPU fallback.
"""
from __future__ import annotations

import torch

from . import _lib
from .ops import _need_gpu, _stream


def sampler_stage(cur, net, scale, coef, T: int, h0=None, h1=None, noise=None):
    """One row of a stage table (gcd_amd.sampler_stages) applied in place to `cur`.

    cur: [nx, C, H, W] fp32, the state the network was evaluated on; net: [2*nx, C, H, W] fp32 in [uc | c] order;
    scale: [T] per-frame guidance scale; coef: 12 floats on the device (see the header); h0 / h1 / noise: fp32 tensors
    shaped like `cur`, or None when no row the caller uses gives them a non-zero coefficient."""
    opt = [t for t in (h0, h1, noise) if t is not None]
    _need_gpu(cur, net, scale, coef, *opt)
    nx, chw = cur.shape[0], cur[0].numel()
    if not (cur.is_contiguous() and net.is_contiguous() and scale.is_contiguous() and coef.is_contiguous()):
        raise _lib.GcdError("sampler_stage: operands must be contiguous")
    if any(t.dtype != torch.float32 for t in (cur, net, scale, coef, *opt)):
        raise _lib.GcdError("sampler_stage: operands must be float32")
    if net.shape[0] != 2 * nx or net[0].numel() != chw or scale.numel() < T or coef.numel() < _lib.SAMPLER_ROW:
        raise _lib.GcdError(f"sampler_stage: net {tuple(net.shape)} / scale {tuple(scale.shape)} / coef "
                            f"{tuple(coef.shape)} do not fit cur {tuple(cur.shape)}, T={T}")
    for t in opt:
        if not t.is_contiguous() or t.shape[0] != nx or t[0].numel() != chw:
            raise _lib.GcdError(f"sampler_stage: h0 / h1 / noise must be contiguous and shaped like cur {tuple(cur.shape)}")
    ptr = lambda t: 0 if t is None else t.data_ptr()      # noqa: E731
    _lib.check_sampler(_lib.load_sampler().gcd_sampler_stage_f32(
        cur.data_ptr(), net.data_ptr(), scale.data_ptr(), coef.data_ptr(), ptr(h0), ptr(h1), ptr(noise), nx, T, chw,
        _stream()), "gcd_sampler_stage_f32")
    return cur
