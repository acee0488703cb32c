"""The CLIP ViT-H/14 image tower behind `cond["crossattn"]`: a drop-in for
`sgm.modules.encoders.modules.FrozenOpenCLIPImageEmbedder` (reference encoders/modules.py:653-815) that needs neither
open_clip nor kornia.  `VisionTransformer` carries the parameter names of open_clip 2.23.0's class, so the tensors under
`conditioner.embedders.0.open_clip.model.visual.*` of a GCD checkpoint load unchanged.

On the GPU the forward is HIP only: gcd_clip_preprocess (kornia's antialiased bicubic resize + CLIP normalisation, straight
into conv1's patch matrix), gcd_clip_tokens_ln_pre, gcd_clip_attn_f16 (head dim 80) and gcd_clip_bias_gelu_f16 of
libgcd_amd_clip.so, and gcd_gemm_f16 / gcd_layernorm_f16 of libgcd_amd.so for the six GEMMs and two LayerNorms of a block.
Forward only, on the caller's current stream, no host synchronisation, workspace from torch allocations.  CPU tensors run a
plain-torch fp32 restatement of the same arithmetic (`forward_torch`, `preprocess_reference`): the CPU plumbing path and
the host oracle of the tests.
"""
from __future__ import annotations

import math
import os
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib_clip, ops
from ._lib import OUT_F16, GcdError
from .conditioning import AbstractEmbModel

HEAD_DIM = _lib_clip.CLIP_HEAD_DIM
# softmax scale of the 80-wide heads in exp2 units, folded into the q rows of the packed in_proj (fp32, before the cast)
ATTN_Q_SCALE_LOG2 = 1.4426950408889634 / math.sqrt(HEAD_DIM)
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)

# open_clip model_configs/<arch>.json, the vision half
ARCHS = {
    "ViT-H-14": dict(width=1280, layers=32, heads=16, mlp_width=5120, patch_size=14, image_size=224, embed_dim=1024),
}
LN_EPS = 1e-5


# ------------------------------------------------------------------------------------------------------- preprocessing
def blur_taps(extent: int, size: int):
    """(k, sigma) of kornia 0.7.0's antialias Gaussian along one axis resized from `extent` to `size`."""
    sigma = max((extent / size - 1.0) / 2.0, 0.001)
    k = int(max(2.0 * 2 * sigma, 3))
    return k + 1 if k % 2 == 0 else k, sigma


def _gaussian(k: int, sigma: float, dtype, device) -> torch.Tensor:
    t = torch.arange(k, dtype=dtype, device=device) - k // 2
    g = torch.exp(-t * t / (2.0 * sigma * sigma))
    return g / g.sum()


def preprocess_reference(x: torch.Tensor, size: int, antialias: bool, mean: torch.Tensor, std: torch.Tensor) -> torch.Tensor:
    """kornia 0.7.0 `geometry.resize(x, (size, size), "bicubic", align_corners=True, antialias)`, `(x + 1) / 2` and
    `enhance.normalize(x, mean, std)` restated in torch, in x's dtype (float32 or float64): reflect padding, two grouped
    1-D Gaussian convolutions (only when antialias and max(H / size, W / size) > 1), F.interpolate."""
    n, c, H, W = x.shape
    if antialias and max(H / size, W / size) > 1:
        (ky, sy), (kx, sx) = blur_taps(H, size), blur_taps(W, size)
        gy, gx = _gaussian(ky, sy, x.dtype, x.device), _gaussian(kx, sx, x.dtype, x.device)
        x = F.pad(x, (kx // 2, kx // 2, ky // 2, ky // 2), mode="reflect")
        x = F.conv2d(x, gx.view(1, 1, 1, kx).expand(c, 1, 1, kx), groups=c)
        x = F.conv2d(x, gy.view(1, 1, ky, 1).expand(c, 1, ky, 1), groups=c)
    x = F.interpolate(x, size=(size, size), mode="bicubic", align_corners=True)
    x = (x + 1.0) / 2.0
    return (x - mean.to(x.dtype).view(1, -1, 1, 1)) / std.to(x.dtype).view(1, -1, 1, 1)


# --------------------------------------------------------------------------------------------------------------- tower
class _Attention(nn.Module):
    """Parameter names of nn.MultiheadAttention (what open_clip's ResidualAttentionBlock.attn is)."""

    def __init__(self, width: int):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * width, width))
        self.in_proj_bias = nn.Parameter(torch.empty(3 * width))
        self.out_proj = nn.Linear(width, width)


class _Block(nn.Module):
    def __init__(self, width: int, mlp_width: int):
        super().__init__()
        self.ln_1 = nn.LayerNorm(width, eps=LN_EPS)
        self.attn = _Attention(width)
        self.ln_2 = nn.LayerNorm(width, eps=LN_EPS)
        self.mlp = nn.Sequential(OrderedDict([("c_fc", nn.Linear(width, mlp_width)), ("gelu", nn.GELU()),
                                              ("c_proj", nn.Linear(mlp_width, width))]))


class _Transformer(nn.Module):
    def __init__(self, width: int, layers: int, mlp_width: int):
        super().__init__()
        self.resblocks = nn.ModuleList([_Block(width, mlp_width) for _ in range(layers)])


class VisionTransformer(nn.Module):
    """open_clip 2.23.0 `VisionTransformer` (class-token pooling, no patch dropout): same parameter names and shapes.

    `forward(image)` takes normalised [n, 3, S, S] images on the CPU (the fp32 restatement, `forward_torch`); on the GPU
    the tower starts from the patch matrix gcd_clip_preprocess writes (`forward_patches`), which is how
    FrozenOpenCLIPImageEmbedder drives it."""

    def __init__(self, width: int, layers: int, heads: int, mlp_width: int, patch_size: int, image_size: int,
                 embed_dim: int):
        super().__init__()
        assert image_size % patch_size == 0 and width % heads == 0
        self.width, self.layers, self.heads, self.mlp_width = width, layers, heads, mlp_width
        self.patch_size, self.image_size, self.embed_dim = patch_size, image_size, embed_dim
        self.grid = image_size // patch_size
        self.output_tokens = False
        scale = width ** -0.5
        self.class_embedding = nn.Parameter(scale * torch.randn(width))
        self.positional_embedding = nn.Parameter(scale * torch.randn(self.grid ** 2 + 1, width))
        self.proj = nn.Parameter(scale * torch.randn(width, embed_dim))
        self.conv1 = nn.Conv2d(3, width, kernel_size=patch_size, stride=patch_size, bias=False)
        self.ln_pre = nn.LayerNorm(width, eps=LN_EPS)
        self.transformer = _Transformer(width, layers, mlp_width)
        self.ln_post = nn.LayerNorm(width, eps=LN_EPS)
        for blk in self.transformer.resblocks:
            nn.init.normal_(blk.attn.in_proj_weight, std=scale)
            nn.init.zeros_(blk.attn.in_proj_bias)
        self._packs = None
        self._packs_key = None

    @property
    def kp(self) -> int:
        """Columns of the patch matrix: 3 P P rounded up to gcd_gemm_f16's K % 32 == 0."""
        return (3 * self.patch_size ** 2 + 31) // 32 * 32

    # -- the restatement ------------------------------------------------------------------------------------------
    def forward_torch(self, image: torch.Tensor) -> torch.Tensor:
        """open_clip's forward in plain torch, in the parameters' dtype (autocast applies as to any torch code)."""
        n, W, hd = image.shape[0], self.width, self.width // self.heads
        x = self.conv1(image).reshape(n, W, -1).permute(0, 2, 1)
        cls = self.class_embedding.to(x.dtype).expand(n, 1, W)
        x = torch.cat([cls, x], dim=1) + self.positional_embedding.to(x.dtype)
        x = self.ln_pre(x)
        S = x.shape[1]
        for blk in self.transformer.resblocks:
            qkv = F.linear(blk.ln_1(x), blk.attn.in_proj_weight, blk.attn.in_proj_bias)
            q, k, v = (t.reshape(n, S, self.heads, hd).transpose(1, 2) for t in qkv.chunk(3, dim=-1))
            p = torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(hd), dim=-1)
            x = x + blk.attn.out_proj((p.to(v.dtype) @ v).transpose(1, 2).reshape(n, S, W))
            x = x + blk.mlp(blk.ln_2(x))
        return self.ln_post(x[:, 0]) @ self.proj.to(x.dtype)

    def forward(self, image: torch.Tensor) -> torch.Tensor:
        if image.is_cuda:
            raise GcdError("VisionTransformer.forward takes normalised images on the CPU only; on the GPU the tower runs "
                           "from gcd_clip_preprocess's patch matrix (FrozenOpenCLIPImageEmbedder, forward_patches)")
        return self.forward_torch(image)

    # -- the HIP path ---------------------------------------------------------------------------------------------
    def _packed(self, device) -> dict:
        """fp16 operand forms of the weights, built at the first GPU forward and rebuilt when a parameter's version (or
        storage) moves."""
        params = list(self.parameters())
        key = (str(device),) + tuple((p.data_ptr(), p._version) for p in params)
        if self._packs is not None and self._packs_key == key:
            return self._packs
        W, K = self.width, 3 * self.patch_size ** 2
        f32 = lambda t: t.detach().to(device=device, dtype=torch.float32).contiguous()
        conv = torch.zeros(W, self.kp, device=device, dtype=torch.float32)
        conv[:, :K] = f32(self.conv1.weight).reshape(W, K)
        packs = dict(conv1=conv.half(), cls=f32(self.class_embedding), pos=f32(self.positional_embedding),
                     ln_pre=(f32(self.ln_pre.weight), f32(self.ln_pre.bias)),
                     ln_post=(f32(self.ln_post.weight), f32(self.ln_post.bias)),
                     proj=f32(self.proj).t().contiguous().half(), blocks=[])
        for blk in self.transformer.resblocks:
            w_in, b_in = f32(blk.attn.in_proj_weight).clone(), f32(blk.attn.in_proj_bias).clone()
            w_in[:W] *= ATTN_Q_SCALE_LOG2
            b_in[:W] *= ATTN_Q_SCALE_LOG2
            packs["blocks"].append(dict(
                ln_1=(f32(blk.ln_1.weight), f32(blk.ln_1.bias)), ln_2=(f32(blk.ln_2.weight), f32(blk.ln_2.bias)),
                w_in=w_in.half(), b_in=b_in, w_out=f32(blk.attn.out_proj.weight).half(), b_out=f32(blk.attn.out_proj.bias),
                w_fc=f32(blk.mlp.c_fc.weight).half(), b_fc=f32(blk.mlp.c_fc.bias),
                w_proj=f32(blk.mlp.c_proj.weight).half(), b_proj=f32(blk.mlp.c_proj.bias)))
        self._packs, self._packs_key = packs, key
        return packs

    def _check_gpu(self) -> None:
        if self.width != self.heads * HEAD_DIM:
            raise GcdError(f"gcd_clip_attn_f16 is built for head dim {HEAD_DIM}: width {self.width} over {self.heads} heads "
                           f"gives {self.width // self.heads}")
        grads = [n for n, p in self.named_parameters() if p.requires_grad]
        if grads and torch.is_grad_enabled():
            raise GcdError(f"the HIP image tower is forward-only, but {grads[0]} (and {len(grads) - 1} more) require grad: "
                           "freeze the embedder (is_trainable: False) or run it under torch.no_grad()")

    def forward_patches(self, patches16: torch.Tensor, n: int) -> torch.Tensor:
        """patches16: fp16 [n G G, kp] from gcd_clip_preprocess -> fp32 [n, embed_dim]."""
        self._check_gpu()
        ops._need_gpu(patches16)
        dev, W, G2 = patches16.device, self.width, self.grid ** 2
        S, M = G2 + 1, n * (G2 + 1)
        pk = self._packed(dev)
        lib, stream = _lib_clip.load(), ops._stream()
        empty = lambda *shape, dtype=torch.float16: torch.empty(*shape, device=dev, dtype=dtype)
        pe = empty(n * G2, W, dtype=torch.float32)
        ops.gemm(patches16, pk["conv1"], pe, M=n * G2)
        x = empty(M, W, dtype=torch.float32)                       # the residual stream
        _lib_clip.check(lib.gcd_clip_tokens_ln_pre(pe.data_ptr(), W, pk["cls"].data_ptr(), pk["pos"].data_ptr(),
                                                   pk["ln_pre"][0].data_ptr(), pk["ln_pre"][1].data_ptr(), LN_EPS,
                                                   x.data_ptr(), W, n, G2, W, stream), "gcd_clip_tokens_ln_pre")
        h16, qkv, a16 = empty(M, W), empty(M, 3 * W), empty(M, W)
        hid32, hid16 = empty(M, self.mlp_width, dtype=torch.float32), empty(M, self.mlp_width)
        for b in pk["blocks"]:
            ops.layernorm(x, *b["ln_1"], h16, eps=LN_EPS)
            ops.gemm(h16, b["w_in"], qkv, M=M, out_kind=OUT_F16, bias=b["b_in"])
            attention(qkv, a16, n, S, self.heads, q_prescaled=True)
            ops.gemm(a16, b["w_out"], x, M=M, bias=b["b_out"], r1=x)
            ops.layernorm(x, *b["ln_2"], h16, eps=LN_EPS)
            ops.gemm(h16, b["w_fc"], hid32, M=M)
            bias_gelu(hid32, b["b_fc"], hid16)
            ops.gemm(hid16, b["w_proj"], x, M=M, bias=b["b_proj"], r1=x)
        c16 = empty(n, W)
        ops.layernorm(x.view(n, S * W)[:, :W], *pk["ln_post"], c16, eps=LN_EPS)      # the class rows, through the stride
        out = empty(n, self.embed_dim, dtype=torch.float32)
        ops.gemm(c16, pk["proj"], out, M=n)
        return out


def seeded_state_dict(vision_cfg: dict, seed: int) -> "OrderedDict[str, torch.Tensor]":
    """Seeded random weights of a tower (no checkpoint ships with the project): one torch.Generator walks the state dict in
    order; matrices N(0, 1 / fan_in), biases and embeddings 0.3 N(0, 1), norm gains 1 +- 0.1 (uniform), norm shifts
    0.1 N(0, 1).  fp32, on the CPU.  tests/golden/clip_vision_tiny.pt stores seeds and per-tensor checksums, not weights."""
    with torch.device("meta"):
        shapes = {k: tuple(v.shape) for k, v in VisionTransformer(**vision_cfg).state_dict().items()}
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    for name, shape in shapes.items():
        leaf = name.rsplit(".", 2)[-2] if "." in name else name
        if leaf.startswith("ln_"):
            t = 1.0 + 0.1 * (2.0 * torch.rand(shape, generator=g) - 1.0) if name.endswith("weight") \
                else 0.1 * torch.randn(shape, generator=g)
        elif len(shape) >= 2 and name != "positional_embedding":
            fan_in = shape[0] if name == "proj" else math.prod(shape[1:])
            t = torch.randn(shape, generator=g) / math.sqrt(fan_in)
        else:
            t = 0.3 * torch.randn(shape, generator=g)
        sd[name] = t
    return sd


# ------------------------------------------------------------------------------------------------- kernel wrappers
def preprocess(image: torch.Tensor, size: int, patch: int, antialias: bool, mean: torch.Tensor, std: torch.Tensor,
               kp: int, want_image: bool = False):
    """gcd_clip_preprocess: fp32 [n, 3, H, W] (any strides) -> (fp16 patch matrix [n G G, kp], fp32 [n, 3, size, size] or None)."""
    ops._need_gpu(image, mean, std)
    if image.dim() != 4 or image.shape[1] != 3 or image.dtype != torch.float32:
        raise GcdError(f"gcd_clip_preprocess takes fp32 [n, 3, H, W] images, got {image.dtype} {tuple(image.shape)}")
    n, _, H, W = image.shape
    G = size // patch
    patches = torch.empty(n * G * G, kp, device=image.device, dtype=torch.float16)
    img = torch.empty(n, 3, size, size, device=image.device, dtype=torch.float32) if want_image else None
    sn, sc, sh, sw = image.stride()
    _lib_clip.check(_lib_clip.load().gcd_clip_preprocess(
        image.data_ptr(), sn, sc, sh, sw, n, H, W, size, patch, int(bool(antialias)), mean.data_ptr(), std.data_ptr(),
        patches.data_ptr(), kp, ops._p(img), ops._stream()), "gcd_clip_preprocess")
    return patches, img


def attention(qkv16: torch.Tensor, out16: torch.Tensor, n: int, S: int, heads: int, q_prescaled: bool = False):
    """gcd_clip_attn_f16: qkv16 fp16 [n S, 3 heads 80] -> out16 fp16 [n S, heads 80]."""
    ops._need_gpu(qkv16, out16)
    assert qkv16.dtype == out16.dtype == torch.float16
    _lib_clip.check(_lib_clip.load().gcd_clip_attn_f16(qkv16.data_ptr(), ops._ld(qkv16), out16.data_ptr(), ops._ld(out16),
                                                       n, S, heads, int(q_prescaled), ops._stream()), "gcd_clip_attn_f16")
    return out16


def bias_gelu(h32: torch.Tensor, bias: torch.Tensor, out16: torch.Tensor):
    """gcd_clip_bias_gelu_f16: out16 = gelu(h32 + bias), exact erf."""
    ops._need_gpu(h32, bias, out16)
    assert h32.dtype == bias.dtype == torch.float32 and out16.dtype == torch.float16 and h32.shape == out16.shape
    M, N = h32.shape
    _lib_clip.check(_lib_clip.load().gcd_clip_bias_gelu_f16(h32.data_ptr(), ops._ld(h32), bias.data_ptr(), out16.data_ptr(),
                                                            ops._ld(out16), M, N, ops._stream()), "gcd_clip_bias_gelu_f16")
    return out16


def tokens_ln_pre(patch32: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                  tok32: torch.Tensor, n: int, eps: float = LN_EPS):
    """gcd_clip_tokens_ln_pre: patch32 fp32 [n G2, C] -> tok32 fp32 [n (G2 + 1), C]."""
    ops._need_gpu(patch32, cls, pos, gamma, beta, tok32)
    C_ = patch32.shape[1]
    G2 = patch32.shape[0] // n
    assert pos.is_contiguous() and tuple(pos.shape) == (G2 + 1, C_) and tok32.shape == (n * (G2 + 1), C_)
    _lib_clip.check(_lib_clip.load().gcd_clip_tokens_ln_pre(patch32.data_ptr(), ops._ld(patch32), cls.data_ptr(), pos.data_ptr(),
                                                            gamma.data_ptr(), beta.data_ptr(), eps, tok32.data_ptr(),
                                                            ops._ld(tok32), n, G2, C_, ops._stream()), "gcd_clip_tokens_ln_pre")
    return tok32


# ------------------------------------------------------------------------------------------------------------ embedder
class _OpenCLIPModel(nn.Module):
    """What is left of open_clip's CLIP model in the reference embedder: `.visual` (the text side is never used)."""

    def __init__(self, visual: VisionTransformer):
        super().__init__()
        self.visual = visual


# text-side entries of a full open_clip state dict, relative to `model.`
_TEXT_KEYS = ("logit_scale", "positional_embedding", "text_projection")
_TEXT_PREFIXES = ("token_embedding.", "ln_final.")


def _read_open_clip_file(path: str) -> dict:
    """The `visual.*` tensors of a local open_clip checkpoint (.pt: torch.load; .safetensors)."""
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        sd = load_file(path)
    else:
        sd = torch.load(path, map_location="cpu", weights_only=True)
    return {k[len("visual."):]: v for k, v in sd.items() if k.startswith("visual.")}


class FrozenOpenCLIPImageEmbedder(AbstractEmbModel):
    """Drop-in for the reference class (encoders/modules.py:653-815): same constructor keywords, same call, same
    `model.visual.*` parameter names.  `version` never downloads: an existing local open_clip file is loaded, any other
    value (the reference's "laion2b_s32b_b79k") leaves the parameters to `load_state_dict`.  `vision_cfg` (not a
    reference keyword) overrides the arch table, for test-sized towers."""

    def __init__(self, arch="ViT-H-14", version="laion2b_s32b_b79k", device="cuda", max_length=77, freeze=True,
                 antialias=True, ucg_rate=0.0, unsqueeze_dim=False, repeat_to_max_len=False, num_image_crops=0,
                 output_tokens=False, init_device=None, vision_cfg=None):
        super().__init__()
        if num_image_crops > 0:
            raise GcdError("FrozenOpenCLIPImageEmbedder: num_image_crops > 0 is not supported (no GCD config uses it)")
        if output_tokens:
            raise GcdError("FrozenOpenCLIPImageEmbedder: output_tokens=True is not supported (no GCD config uses it)")
        if vision_cfg is None:
            if arch not in ARCHS:
                raise GcdError(f"FrozenOpenCLIPImageEmbedder: unknown arch {arch!r} (known: {sorted(ARCHS)}); pass vision_cfg")
            vision_cfg = ARCHS[arch]
        with torch.device(init_device if init_device is not None else "cpu"):
            self.model = _OpenCLIPModel(VisionTransformer(**vision_cfg))
        if isinstance(version, (str, os.PathLike)) and os.path.isfile(version):
            self.model.visual.load_state_dict(_read_open_clip_file(os.fspath(version)), strict=True)
        self.max_crops = num_image_crops
        self.pad_to_max_len = False
        self.repeat_to_max_len = repeat_to_max_len
        self.device = device
        self.max_length = max_length
        if freeze:
            self.freeze()
        self.antialias = antialias
        self.register_buffer("mean", torch.tensor(CLIP_MEAN), persistent=False)
        self.register_buffer("std", torch.tensor(CLIP_STD), persistent=False)
        self.ucg_rate = ucg_rate
        self.unsqueeze_dim = unsqueeze_dim
        self.stored_batch = None
        self.output_tokens = output_tokens
        self._register_load_state_dict_pre_hook(self._drop_text_keys)

    @staticmethod
    def _drop_text_keys(state_dict, prefix, *args):
        """The reference loads a full open_clip state dict with strict=False; dropping its text side makes strict=True work."""
        base = prefix + "model."
        for k in list(state_dict):
            if k.startswith(base):
                rest = k[len(base):]
                if rest in _TEXT_KEYS or rest.startswith(_TEXT_PREFIXES):
                    del state_dict[k]

    def freeze(self):
        self.model = self.model.eval()
        for param in self.parameters():
            param.requires_grad = False

    def preprocess(self, x: torch.Tensor) -> torch.Tensor:
        """The normalised [n, 3, S, S] image (CPU: the torch restatement; GPU: gcd_clip_preprocess's fp32 output)."""
        v = self.model.visual
        if x.is_cuda:
            return preprocess(x.float(), v.image_size, v.patch_size, self.antialias, self.mean, self.std, v.kp,
                              want_image=True)[1]
        return preprocess_reference(x.float(), v.image_size, self.antialias, self.mean, self.std)

    def encode_with_vision_transformer(self, img: torch.Tensor) -> torch.Tensor:
        v = self.model.visual
        if img.dim() != 4:
            raise GcdError(f"FrozenOpenCLIPImageEmbedder takes [n, 3, H, W] images, got {tuple(img.shape)}")
        if img.is_cuda:
            with torch.cuda.device(img.device):
                patches, _ = preprocess(img.float(), v.image_size, v.patch_size, self.antialias, self.mean, self.std, v.kp)
                return v.forward_patches(patches, img.shape[0])
        with torch.autocast("cpu", enabled=False):
            return v.forward_torch(self.preprocess(img))

    def forward(self, image, no_dropout=False):
        z = self.encode_with_vision_transformer(image).to(image.dtype)
        if self.ucg_rate > 0.0 and not no_dropout:
            z = torch.bernoulli((1.0 - self.ucg_rate) * torch.ones(z.shape[0], device=z.device))[:, None] * z
        if self.unsqueeze_dim:
            z = z[:, None, :]
        if self.repeat_to_max_len:
            z_ = z[:, None, :] if z.dim() == 2 else z
            return z_.repeat(1, self.max_length, 1), z                   # "b 1 d -> b n d"
        return z

    def encode(self, text):
        return self(text)
