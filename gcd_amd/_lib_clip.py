"""ctypes binding of libgcd_amd_clip.so (include/gcd_amd_clip.h; gcd_amd/csrc/clip_vision.hip): the kernels of the CLIP ViT
image tower.  A library beside gcd_amd/_lib.py (gcd_amd.csrc.build.LIBRARIES): the same `Binding` record, made by the same
`_bind`, so loading and error reporting behave as for every other library — a missing shared object or a non-zero status
raises GcdError, nothing falls back."""
from __future__ import annotations

import ctypes as C

from ._lib import _PKG, _bind

CLIP_LIB_PATH = _PKG / "libgcd_amd_clip.so"
CLIP_ABI_VERSION = 1
CLIP_ATTN_MAX_S = 288          # keys of one (image, head) that gcd_clip_attn_f16 keeps in LDS
CLIP_HEAD_DIM = 80
CLIP_MAX_BLUR = 63
CLIP_MAX_WIDTH = 8192
CLIP_MAX_MODEL_WIDTH = 4096

_vp, _i, _i64, _f = C.c_void_p, C.c_int, C.c_int64, C.c_float

CLIP_SIGNATURES = {
    "gcd_clip_abi_version": (_i, []),
    "gcd_clip_last_error": (C.c_char_p, []),
    "gcd_clip_preprocess": (_i, [_vp, _i64, _i64, _i64, _i64, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    "gcd_clip_tokens_ln_pre": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _f, _vp, _i64, _i, _i, _i, _vp]),
    "gcd_clip_attn_f16": (_i, [_vp, _i64, _vp, _i64, _i, _i, _i, _i, _vp]),
    "gcd_clip_bias_gelu_f16": (_i, [_vp, _i64, _vp, _vp, _i64, _i64, _i, _vp]),
}

BINDING = _bind("gcd_amd_clip", CLIP_LIB_PATH, CLIP_ABI_VERSION, "gcd_clip_abi_version", "gcd_clip_last_error",
                CLIP_SIGNATURES)
load, check = BINDING.load, BINDING.check
