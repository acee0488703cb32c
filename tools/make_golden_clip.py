#!/usr/bin/env python3
"""tests/golden/clip_vision_tiny.pt: the pins of the CLIP image tower (gcd_amd/clip_vision.py).  Data only.

The reference's `FrozenOpenCLIPImageEmbedder` cannot be executed here: it needs open_clip_torch (the ViT) and kornia (the
resize), and neither is installed.  So the two halves are pinned as follows.

Tower.  `transformers.CLIPVisionModelWithProjection(CLIPVisionConfig(...))` builds the same architecture from a config
alone and is an independent implementation.  The seeded weights of `clip_vision.seeded_state_dict` (open_clip names) are
mapped to its names (`to_hf`), and its output on the normalised images is recorded in float32, in float64 (the error
of the float32 run is the bar of the host test), and under CPU float16 / bfloat16 autocast (the fp16 drift is what the
GPU test's bar is made of).  The file stores seeds and per-tensor checksums, not weights.

Preprocess.  kornia 0.7.0's `geometry.resize(..., "bicubic", align_corners=True, antialias)` is restated from its published
source, not executed: sigma = max((factor - 1) / 2, 0.001), k = int(max(4 sigma, 3)) made odd, normalised Gaussian taps,
reflect padding, separable; then torch's bicubic (A = -0.75, clamped indices).  This file builds that operator as two dense
float64 matrices per axis from the formulae (numpy, no torch operator involved) and requires `clip_vision.
preprocess_reference` — F.pad / grouped conv2d / F.interpolate — to agree with it in float64 to 1e-12; it then records
the float64 result and the largest gap of the same chain run in float32.

Usage: python tools/make_golden_clip.py
"""
from __future__ import annotations

import math
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
from clip_util import seeded_image  # noqa: E402  (tests/clip_util.py: the tests regenerate the same images)
from gcd_amd import clip_vision as cv  # noqa: E402

OUT = ROOT / "tests" / "golden" / "clip_vision_tiny.pt"

TINY = dict(width=160, layers=2, heads=2, mlp_width=640, patch_size=14, image_size=56, embed_dim=64)
TOWER_CASES = {
    # name: (vision_cfg, weight seed, image seed, n)
    "w160_s17": (TINY, 101, 201, 3),
    "w160_s257": (dict(TINY, layers=1, image_size=224), 102, 202, 2),
    "w1280_s257": (dict(cv.ARCHS["ViT-H-14"], layers=2), 103, 203, 2),
}
PRE_CASES = {
    # name: (n, H, W, size, image seed)
    "56x56": (1, 56, 56, 56, 301),
    "96x160": (1, 96, 160, 56, 302),
    "72x200": (1, 72, 200, 56, 303),
    "40x200": (1, 40, 200, 56, 304),
    "576x1024": (1, 576, 1024, 224, 305),
}
PRE_SAMPLES = 4096        # positions of the 576x1024 case recorded in full precision (the whole image passes the size limit)


def checksums(sd) -> dict:
    return {k: (float(v.double().sum()), float(v.double().abs().sum())) for k, v in sd.items()}


def rel_l2(a, b) -> float:
    return float((a.double() - b.double()).norm() / b.double().norm())


# ------------------------------------------------------------------------------------------------------------- tower
def to_hf(sd: dict, cfg: dict) -> dict:
    """open_clip VisionTransformer names -> transformers CLIPVisionModelWithProjection names."""
    W = cfg["width"]
    out = {"vision_model.embeddings.class_embedding": sd["class_embedding"],
           "vision_model.embeddings.position_embedding.weight": sd["positional_embedding"],
           "vision_model.embeddings.patch_embedding.weight": sd["conv1.weight"],
           "vision_model.pre_layrnorm.weight": sd["ln_pre.weight"], "vision_model.pre_layrnorm.bias": sd["ln_pre.bias"],
           "vision_model.post_layernorm.weight": sd["ln_post.weight"], "vision_model.post_layernorm.bias": sd["ln_post.bias"],
           "visual_projection.weight": sd["proj"].t().contiguous()}
    for i in range(cfg["layers"]):
        s, d = f"transformer.resblocks.{i}.", f"vision_model.encoder.layers.{i}."
        for j, n in enumerate(("q_proj", "k_proj", "v_proj")):
            out[d + f"self_attn.{n}.weight"] = sd[s + "attn.in_proj_weight"][j * W:(j + 1) * W]
            out[d + f"self_attn.{n}.bias"] = sd[s + "attn.in_proj_bias"][j * W:(j + 1) * W]
        for a, b in (("attn.out_proj", "self_attn.out_proj"), ("ln_1", "layer_norm1"), ("ln_2", "layer_norm2"),
                     ("mlp.c_fc", "mlp.fc1"), ("mlp.c_proj", "mlp.fc2")):
            out[d + b + ".weight"], out[d + b + ".bias"] = sd[s + a + ".weight"], sd[s + a + ".bias"]
    return out


def hf_tower(cfg: dict, sd: dict):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    hf_cfg = CLIPVisionConfig(hidden_size=cfg["width"], intermediate_size=cfg["mlp_width"], num_hidden_layers=cfg["layers"],
                              num_attention_heads=cfg["heads"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
                              projection_dim=cfg["embed_dim"], hidden_act="gelu", layer_norm_eps=cv.LN_EPS,
                              attention_dropout=0.0, attn_implementation="sdpa")
    m = CLIPVisionModelWithProjection(hf_cfg).eval()
    missing, unexpected = m.load_state_dict(to_hf(sd, cfg), strict=False)
    assert not unexpected and all("position_ids" in k for k in missing), (missing, unexpected)
    return m


def tower_case(cfg, wseed, iseed, n) -> dict:
    sd = cv.seeded_state_dict(cfg, wseed)
    raw = seeded_image(n, cfg["image_size"], cfg["image_size"], iseed)
    mean, std = torch.tensor(cv.CLIP_MEAN), torch.tensor(cv.CLIP_STD)
    img = cv.preprocess_reference(raw.double(), cfg["image_size"], True, mean, std)      # identity resize: normalisation only
    hf = hf_tower(cfg, sd)
    with torch.no_grad():
        out32 = hf(pixel_values=img.float()).image_embeds
        out64 = hf.double()(pixel_values=img).image_embeds
        hf.float()
        with torch.autocast("cpu", dtype=torch.float16):
            out16 = hf(pixel_values=img.float()).image_embeds.float()
        with torch.autocast("cpu", dtype=torch.bfloat16):
            outbf = hf(pixel_values=img.float()).image_embeds.float()
        # the module's own restatement, in float64, against the independent implementation
        vt = cv.VisionTransformer(**cfg).double()
        vt.load_state_dict({k: v.double() for k, v in sd.items()})
        own64 = vt.forward_torch(img)
    rec = dict(cfg=dict(cfg), weight_seed=wseed, image_seed=iseed, n=n, checksums=checksums(sd),
               image_checksum=(float(raw.double().sum()), float(raw.double().abs().sum())),
               out32=out32.clone(), out64=out64.clone(), out_fp16_autocast=out16.clone(), out_bf16_autocast=outbf.clone(),
               err32=rel_l2(out32, out64), drift_fp16=rel_l2(out16, out32), drift_bf16=rel_l2(outbf, out32),
               restatement_vs_hf_fp64=rel_l2(own64, out64))
    assert rec["restatement_vs_hf_fp64"] < 1e-12, rec["restatement_vs_hf_fp64"]
    return rec


# -------------------------------------------------------------------------------------------------------- preprocess
def axis_matrix(extent: int, size: int, blur: bool) -> np.ndarray:
    """[size, extent] float64: bicubic (A = -0.75, align_corners, clamped taps) after the reflect-padded Gaussian."""
    A = -0.75
    R = np.zeros((size, extent))
    scale = (extent - 1) / (size - 1) if size > 1 else 0.0
    for o in range(size):
        src = scale * o
        i0 = math.floor(src)
        t = src - i0
        w = [((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A, ((A + 2) * t - (A + 3)) * t * t + 1,
             ((A + 2) * (1 - t) - (A + 3)) * (1 - t) ** 2 + 1, ((A * (2 - t) - 5 * A) * (2 - t) + 8 * A) * (2 - t) - 4 * A]
        for j in range(4):
            R[o, min(max(i0 - 1 + j, 0), extent - 1)] += w[j]
    if not blur:
        return R
    sigma = max((extent / size - 1.0) / 2.0, 0.001)
    k = int(max(2.0 * 2 * sigma, 3))
    k += 1 - k % 2
    taps = np.exp(-((np.arange(k) - k // 2) ** 2) / (2.0 * sigma * sigma))
    taps /= taps.sum()
    B = np.zeros((extent, extent))
    for y in range(extent):
        for a in range(k):
            i = abs(y + a - k // 2)
            B[y, 2 * (extent - 1) - i if i > extent - 1 else i] += taps[a]
    return R @ B


def preprocess_case(n, H, W, size, seed) -> dict:
    raw = seeded_image(n, H, W, seed)
    mean, std = torch.tensor(cv.CLIP_MEAN), torch.tensor(cv.CLIP_STD)
    blur = max(H / size, W / size) > 1
    Ry, Rx = axis_matrix(H, size, blur), axis_matrix(W, size, blur)
    dense = np.einsum("oh,nchw,pw->ncop", Ry, raw.double().numpy(), Rx)
    dense = ((dense + 1.0) / 2.0 - mean.double().numpy().reshape(1, 3, 1, 1)) / std.double().numpy().reshape(1, 3, 1, 1)
    dense = torch.from_numpy(dense)
    chain64 = cv.preprocess_reference(raw.double(), size, True, mean, std)
    chain32 = cv.preprocess_reference(raw, size, True, mean, std)
    agree = float((chain64 - dense).abs().max())
    assert agree < 1e-12, f"torch chain vs dense matrices in float64: {agree:.3e}"
    rec = dict(n=n, H=H, W=W, size=size, image_seed=seed, k=(cv.blur_taps(H, size)[0], cv.blur_taps(W, size)[0]) if blur else (1, 1),
               image_checksum=(float(raw.double().sum()), float(raw.double().abs().sum())),
               gap32=float((chain32.double() - dense).abs().max()), chain_vs_dense_fp64=agree,
               range=(float(dense.min()), float(dense.max())),
               out64_checksum=(float(dense.sum()), float(dense.abs().sum())))
    if dense.numel() * 8 <= 160 * 1024:
        rec["out64"], rec["out32"] = dense.clone(), chain32.clone()
    else:
        idx = torch.randperm(dense.numel(), generator=torch.Generator().manual_seed(seed))[:PRE_SAMPLES].clone()
        rec["sample_index"], rec["out64_samples"] = idx, dense.reshape(-1)[idx].clone()
        rec["out32_samples"] = chain32.reshape(-1)[idx].clone()
    return rec


def main():
    golden = dict(about="CLIP image tower pins: see tools/make_golden_clip.py", torch=str(torch.__version__),
                  tower={k: tower_case(*v) for k, v in TOWER_CASES.items()},
                  preprocess={k: preprocess_case(*v) for k, v in PRE_CASES.items()})
    for k, r in golden["tower"].items():
        print(f"tower {k}: err32 {r['err32']:.3e}  fp16 drift {r['drift_fp16']:.3e}  bf16 drift {r['drift_bf16']:.3e}  "
              f"restatement vs HF (fp64) {r['restatement_vs_hf_fp64']:.3e}")
    for k, r in golden["preprocess"].items():
        print(f"preprocess {k}: k {r['k']}  fp32-chain gap {r['gap32']:.3e}  range [{r['range'][0]:.2f}, {r['range'][1]:.2f}]")
    OUT.parent.mkdir(parents=True, exist_ok=True)
    torch.save(golden, OUT)
    print(f"{OUT}: {OUT.stat().st_size} bytes")


if __name__ == "__main__":
    main()
