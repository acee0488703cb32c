"""LPIPS, the perceptual metric of the reference's validation step (`self.lpips = LPIPS().eval()`, diffusion.py:187,342): a
drop-in for `sgm.modules.autoencoding.lpips.loss.lpips.LPIPS` in eval mode that needs neither torchvision nor a
download.  Same 33 `state_dict` names (`scaling_layer.shift|scale`, `net.slice{1..5}.{i}.weight|bias` under torchvision's
VGG-16 `features` indices, `lin{0..4}.model.1.weight`), same `forward(input, target) -> [N, 1, 1, 1]`.

The constructor reads no file and reaches no network: the parameters start from torch's default initialisation and come
from `load_state_dict` (a lin-only LPIPS checkpoint loads with strict=False, as in the reference) and
`load_torchvision_vgg16` (a torchvision `vgg16().state_dict()` or its `features.*` part).  Everything is frozen.

The forward is HIP only (there is no CPU path): gcd_lpips_pack_f16 (ScalingLayer + token-major fp16 packing),
13 x gcd_gemm_f16 (GCD_GEMM_CONV3X3, fp16 output, bias) each followed by gcd_lpips_relu_pool_f16, and one
gcd_lpips_distance per tap (libgcd_amd_lpips.so).  Input and target go through the tower as ONE batch of 2 n images, so
a pair of identical images meets identical arithmetic and scores exactly 0.  Storage points in fp16: the scaled input,
the convolution weights, every convolution output (ReLU and max-pool are exact on fp16).  Accumulation is fp32 in the
convolutions and the distance, fp64 in the final sums.  Forward only, on the caller's current stream, no host
synchronisation, workspace from torch allocations.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Optional

import torch
import torch.nn as nn

from . import _lib_lpips, ops, packing
from ._lib import GEMM_CONV3X3, OUT_F16, GcdError
from .engine import CIN_PAD

VGG16_CHNS = (64, 128, 256, 512, 512)
# torchvision vgg16().features indices of the convolutions of each slice (a ReLU follows each; a 2x2 max-pool sits at
# 4, 9, 16, 23, before slices 2-5); the taps are the post-ReLU outputs 3, 8, 15, 22, 29
SLICE_CONVS = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
MIN_SIZE = 16                  # four floor-mode 2x2 pools must leave a pixel
# Largest single activation of a chunk of pairs.  Bounds the workspace (a chunk holds about three such tensors at its
# peak) and keeps every operand of gcd_gemm_f16 far below 2^31 bytes: its M is an int32 count of tokens, and its tile
# kernels address through 32-bit byte offsets.
MAX_ACTIVATION_BYTES = 1 << 30
GEMM_OPERAND_LIMIT = (1 << 31) - 1
_RANGES = {"signed": (1.0, 0.0), "unit": (2.0, -1.0)}      # (a, b) of x * a + b: the tower takes [-1, 1]


class ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor(SHIFT)[None, :, None, None])
        self.register_buffer("scale", torch.tensor(SCALE)[None, :, None, None])


class NetLinLayer(nn.Module):
    """The reference's 1x1 `lin` layer (parameter holder): `model` = [Dropout,] Conv2d(C, 1, 1, bias=False)."""

    def __init__(self, chn_in: int, chn_out: int = 1, use_dropout: bool = False):
        super().__init__()
        layers = [nn.Dropout()] if use_dropout else []
        layers += [nn.Conv2d(chn_in, chn_out, 1, stride=1, padding=0, bias=False)]
        self.model = nn.Sequential(*layers)


class _VGG16Slices(nn.Module):
    """`features[0:30]` of VGG-16 cut into the reference's five slices, children named by torchvision's indices."""

    def __init__(self, chns):
        super().__init__()
        self.N_slices = 5
        cin, idx = 3, 0
        for k, (convs, cout) in enumerate(zip(SLICE_CONVS, chns)):
            seq = nn.Sequential()
            if k > 0:
                seq.add_module(str(idx), nn.MaxPool2d(kernel_size=2, stride=2))
                idx += 1
            for i in convs:
                assert i == idx
                seq.add_module(str(idx), nn.Conv2d(cin, cout, kernel_size=3, padding=1))
                seq.add_module(str(idx + 1), nn.ReLU(inplace=True))
                cin, idx = cout, idx + 2
            setattr(self, f"slice{k + 1}", seq)


class LPIPS(nn.Module):
    def __init__(self, use_dropout: bool = True, chns=VGG16_CHNS):
        super().__init__()
        chns = tuple(int(c) for c in chns)
        if len(chns) != 5 or any(c <= 0 or c % _lib_lpips.LPIPS_C_MULTIPLE or c > _lib_lpips.LPIPS_MAX_C for c in chns):
            raise GcdError(f"LPIPS: chns must be five widths, multiples of {_lib_lpips.LPIPS_C_MULTIPLE} up to "
                           f"{_lib_lpips.LPIPS_MAX_C}, got {chns}")
        self.scaling_layer = ScalingLayer()
        self.chns = list(chns)
        self.net = _VGG16Slices(chns)
        for k, c in enumerate(chns):
            setattr(self, f"lin{k}", NetLinLayer(c, use_dropout=use_dropout))
        for p in self.parameters():
            p.requires_grad = False
        self.eval()
        self._packs = None
        self._packs_key = None

    # -- loading ----------------------------------------------------------------------------------------------------
    def load_torchvision_vgg16(self, state_dict) -> None:
        """Take the 13 convolutions from a torchvision `vgg16().state_dict()` (`features.{i}.weight|bias`; the classifier's
        entries are ignored).  Every convolution must be there."""
        own = OrderedDict()
        for k, convs in enumerate(SLICE_CONVS):
            for i in convs:
                for leaf in ("weight", "bias"):
                    src = f"features.{i}.{leaf}"
                    if src not in state_dict:
                        raise GcdError(f"load_torchvision_vgg16: {src} is missing")
                    own[f"net.slice{k + 1}.{i}.{leaf}"] = state_dict[src]
        missing, unexpected = self.load_state_dict(own, strict=False)
        assert not unexpected, unexpected

    def _lin_weight(self, k: int) -> torch.Tensor:
        return getattr(self, f"lin{k}").model[-1].weight

    def _convs(self, k: int):
        seq = getattr(self.net, f"slice{k + 1}")
        return [getattr(seq, str(i)) for i in SLICE_CONVS[k]]

    # -- the HIP path -----------------------------------------------------------------------------------------------
    def _packed(self, device) -> dict:
        """Operand forms of the weights, built at the first forward and rebuilt when a parameter's version (or storage)
        moves."""
        tensors = list(self.parameters()) + list(self.buffers())
        key = (str(device),) + tuple((t.data_ptr(), t._version) for t in tensors)
        if self._packs is not None and self._packs_key == key:
            return self._packs
        f32 = lambda t: t.detach().to(device=device, dtype=torch.float32).contiguous()
        slices = []
        for k in range(5):
            layers = []
            for conv in self._convs(k):
                first = conv.in_channels == 3
                w = packing.pack_conv3x3(f32(conv.weight), cin_pad=CIN_PAD if first else 0)
                layers.append((w, f32(conv.bias), CIN_PAD if first else conv.in_channels, conv.out_channels))
            slices.append(layers)
        packs = dict(slices=slices, lin=[f32(self._lin_weight(k)).reshape(-1) for k in range(5)],
                     shift=f32(self.scaling_layer.shift).reshape(-1), scale=f32(self.scaling_layer.scale).reshape(-1))
        self._packs, self._packs_key = packs, key
        return packs

    def _image_bytes(self, H: int, W: int) -> int:
        """fp16 bytes of the largest activation of one image."""
        best = H * W * CIN_PAD * 2
        for k, c in enumerate(self.chns):
            best = max(best, (H >> k) * (W >> k) * c * 2)
        return best

    def pairs_per_chunk(self, H: int, W: int, pairs_at_a_time: Optional[int] = None) -> int:
        """How many (input, target) pairs go through the tower at once: the most whose largest activation (2 n images)
        stays within MAX_ACTIVATION_BYTES, or the caller's number if no operand of gcd_gemm_f16 then reaches 2^31 bytes."""
        per_pair = 2 * self._image_bytes(H, W)
        if per_pair > GEMM_OPERAND_LIMIT:
            raise GcdError(f"LPIPS: one pair of {H}x{W} images makes an activation of {per_pair} bytes, past the "
                           f"{GEMM_OPERAND_LIMIT} of one gcd_gemm_f16 operand; tile the images")
        if pairs_at_a_time is None:
            return max(1, MAX_ACTIVATION_BYTES // per_pair)
        if pairs_at_a_time < 1 or pairs_at_a_time * per_pair > GEMM_OPERAND_LIMIT:
            raise GcdError(f"LPIPS: pairs_at_a_time={pairs_at_a_time} at {H}x{W} makes an activation of "
                           f"{pairs_at_a_time * per_pair} bytes; at most {GEMM_OPERAND_LIMIT // per_pair} pairs fit one "
                           "gcd_gemm_f16 operand")
        return int(pairs_at_a_time)

    def _check(self, input, target, value_range):
        if value_range not in _RANGES:
            raise GcdError(f"LPIPS: value_range must be one of {sorted(_RANGES)}, got {value_range!r}")
        if not (torch.is_tensor(input) and torch.is_tensor(target)):
            raise GcdError("LPIPS: operands must be torch tensors on the GPU; there is no CPU fallback")
        ops._need_gpu(input, target)
        if input.dtype != torch.float32 or target.dtype != torch.float32:
            raise GcdError(f"LPIPS: operands must be float32 (got {input.dtype}, {target.dtype})")
        if input.shape != target.shape or input.dim() != 4 or input.shape[1] != 3 or input.shape[0] < 1:
            raise GcdError(f"LPIPS: operands must be two [N, 3, H, W] tensors of one shape, got {tuple(input.shape)} and "
                           f"{tuple(target.shape)}")
        if not (input.is_contiguous() and target.is_contiguous()):
            raise GcdError("LPIPS: operands must be contiguous")
        if min(input.shape[2:]) < MIN_SIZE:
            raise GcdError(f"LPIPS: images must be at least {MIN_SIZE}x{MIN_SIZE} (four 2x2 pools must leave a pixel), got "
                           f"{input.shape[2]}x{input.shape[3]}")
        if self._lin_weight(0).device != input.device:
            raise GcdError(f"LPIPS: parameters on {self._lin_weight(0).device}, operands on {input.device}: move the module "
                           "to the GPU (`.to('cuda')`); there is no CPU execution path")

    @torch.no_grad()
    def forward(self, input: torch.Tensor, target: torch.Tensor, value_range: str = "signed",
                pairs_at_a_time: Optional[int] = None) -> torch.Tensor:
        """input, target: contiguous fp32 [N, 3, H, W] on the GPU, in [-1, 1] ("signed", the reference's convention) or
        in [0, 1] ("unit": `x * 2 - 1` happens inside the packing kernel).  Returns fp32 [N, 1, 1, 1]."""
        self._check(input, target, value_range)
        N, _, H, W = input.shape
        chunk = self.pairs_per_chunk(H, W, pairs_at_a_time)
        with torch.cuda.device(input.device):
            pk = self._packed(input.device)
            out = torch.empty(N, device=input.device, dtype=torch.float32)
            for i0 in range(0, N, chunk):
                i1 = min(N, i0 + chunk)
                self._forward_chunk(pk, input[i0:i1], target[i0:i1], _RANGES[value_range], out[i0:i1])
        return out.view(N, 1, 1, 1)

    def _forward_chunk(self, pk, x0, x1, ab, out) -> None:
        n, _, H, W = x0.shape
        dev = x0.device
        empty = lambda rows, cols: torch.empty(rows, cols, device=dev, dtype=torch.float16)
        h = empty(2 * n * H * W, CIN_PAD)
        pack(x0, h[:n * H * W], ab, pk["shift"], pk["scale"])
        pack(x1, h[n * H * W:], ab, pk["shift"], pk["scale"])
        tap_means = torch.empty(5, n, device=dev, dtype=torch.float64)
        for k, layers in enumerate(pk["slices"]):
            M = 2 * n * H * W
            pooled = None
            for j, (w, b, cin, cout) in enumerate(layers):
                raw = empty(M, cout)
                ops.gemm(h, w, raw, M=M, mode=GEMM_CONV3X3, out_kind=OUT_F16, bias=b,
                         conv=dict(Cin=cin, Hi=H, Wi=W, Ho=H, Wo=W, stride=1, upsample=0),
                         alg_flops_scale=3 / CIN_PAD if (k, j) == (0, 0) else 1.0)
                if j == len(layers) - 1 and k < 4:
                    pooled = empty(2 * n * (H // 2) * (W // 2), cout)
                relu_pool(raw, raw, pooled, 2 * n, H, W)          # in place; the tap also leaves its pooled form
                h = raw
            distance(h[:M // 2], h[M // 2:], pk["lin"][k], n, H * W, tap_means, k, 5, out if k == 4 else None)
            if k < 4:
                h, H, W = pooled, H // 2, W // 2


# ------------------------------------------------------------------------------------------------------- kernel wrappers
def pack(x: torch.Tensor, out16: torch.Tensor, ab, shift: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """gcd_lpips_pack_f16: fp32 [n, 3, H, W] -> fp16 [n H W, cpad] = ((x a + b) - shift) / scale, zero pad channels."""
    ops._need_gpu(x, out16, shift, scale)
    n, c, H, W = x.shape
    assert c == _lib_lpips.LPIPS_IMAGE_CHANNELS and x.dtype == torch.float32 and x.is_contiguous()
    assert out16.dtype == torch.float16 and out16.is_contiguous() and out16.shape[0] == n * H * W
    assert shift.dtype == scale.dtype == torch.float32 and shift.numel() == scale.numel() == c
    _lib_lpips.check(_lib_lpips.load().gcd_lpips_pack_f16(x.data_ptr(), n, H, W, float(ab[0]), float(ab[1]), shift.data_ptr(),
                                                          scale.data_ptr(), out16.data_ptr(), out16.shape[1], ops._stream()),
                     "gcd_lpips_pack_f16")
    return out16


def relu_pool(src: torch.Tensor, full: Optional[torch.Tensor], pooled: Optional[torch.Tensor], n: int, H: int, W: int):
    """gcd_lpips_relu_pool_f16: src fp16 [n H W, C] -> full [n H W, C] = relu(src) (may be src) and / or pooled
    [n (H // 2) (W // 2), C] = its 2x2 floor max-pool."""
    ops._need_gpu(src, full, pooled)
    C_ = src.shape[1]
    assert src.dtype == torch.float16 and src.is_contiguous() and src.shape[0] == n * H * W
    assert full is None or (full.dtype == torch.float16 and full.is_contiguous() and full.shape == src.shape)
    assert pooled is None or (pooled.dtype == torch.float16 and pooled.is_contiguous()
                              and tuple(pooled.shape) == (n * (H // 2) * (W // 2), C_))
    _lib_lpips.check(_lib_lpips.load().gcd_lpips_relu_pool_f16(src.data_ptr(), ops._p(full), ops._p(pooled), n, H, W, C_,
                                                               ops._stream()), "gcd_lpips_relu_pool_f16")


def distance_blocks(HW: int, C_: int) -> int:
    """Workgroups (= partial sums) per image: one per group of pixels a workgroup takes at a time, at most the limit."""
    lanes = 4
    while lanes * 8 < C_:
        lanes *= 2
    per_step = (64 // lanes) * 4
    return max(1, min(_lib_lpips.LPIPS_MAX_BLOCKS, -(-HW // per_step)))


def distance(f0: torch.Tensor, f1: torch.Tensor, w: torch.Tensor, n: int, HW: int, tap_means: torch.Tensor, tap: int,
             taps: int, out: Optional[torch.Tensor] = None, blocks: Optional[int] = None,
             partials: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gcd_lpips_distance: f0, f1 fp16 [n HW, C], w fp32 [C] -> tap_means[tap] (fp64 [taps, n]) = the mean over the
    pixels of sum_c (f0 / (|f0| + 1e-10) - f1 / (|f1| + 1e-10))^2 w; with `out` (fp32 [n]) also the sum over the taps."""
    ops._need_gpu(f0, f1, w, tap_means, out, partials)
    C_ = f0.shape[1]
    assert f0.dtype == f1.dtype == torch.float16 and f0.is_contiguous() and f1.is_contiguous()
    assert tuple(f0.shape) == tuple(f1.shape) == (n * HW, C_) and w.dtype == torch.float32 and w.numel() == C_
    assert tap_means.dtype == torch.float64 and tap_means.is_contiguous() and tuple(tap_means.shape) == (taps, n)
    assert out is None or (out.dtype == torch.float32 and out.is_contiguous() and out.numel() == n)
    if blocks is None:
        blocks = distance_blocks(HW, C_)
    if partials is None:
        partials = torch.empty(n, blocks, device=f0.device, dtype=torch.float32)
    assert partials.dtype == torch.float32 and partials.is_contiguous() and partials.numel() == n * blocks
    _lib_lpips.check(_lib_lpips.load().gcd_lpips_distance(f0.data_ptr(), f1.data_ptr(), w.data_ptr(), n, HW, C_,
                                                          partials.data_ptr(), blocks, tap_means.data_ptr(), tap, taps,
                                                          ops._p(out), ops._stream()), "gcd_lpips_distance")
    return tap_means
