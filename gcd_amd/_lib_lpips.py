"""ctypes binding of libgcd_amd_lpips.so (include/gcd_amd_lpips.h; gcd_amd/csrc/lpips.hip): the kernels of the LPIPS metric.
A library beside gcd_amd/_lib.py (gcd_amd.csrc.build.LIBRARIES), like gcd_amd/_lib_clip.py: the same `Binding` record,
made by the same `_bind`, so loading and error reporting behave as for every other library — a missing shared object or
a non-zero status raises GcdError, nothing falls back."""
from __future__ import annotations

import ctypes as C

from ._lib import _PKG, _bind

LPIPS_LIB_PATH = _PKG / "libgcd_amd_lpips.so"
LPIPS_ABI_VERSION = 1
LPIPS_MAX_C = 512              # widest feature row of gcd_lpips_distance
LPIPS_C_MULTIPLE = 32
LPIPS_MAX_BLOCKS = 1024        # partial sums (workgroups) per image of gcd_lpips_distance
LPIPS_MAX_TAPS = 16
LPIPS_MAX_IMAGES = 65535
LPIPS_IMAGE_CHANNELS = 3

_vp, _i, _i64, _f = C.c_void_p, C.c_int, C.c_int64, C.c_float

LPIPS_SIGNATURES = {
    "gcd_lpips_abi_version": (_i, []),
    "gcd_lpips_last_error": (C.c_char_p, []),
    "gcd_lpips_pack_f16": (_i, [_vp, _i, _i, _i, _f, _f, _vp, _vp, _vp, _i, _vp]),
    "gcd_lpips_relu_pool_f16": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "gcd_lpips_distance": (_i, [_vp, _vp, _vp, _i, _i64, _i, _vp, _i, _vp, _i, _i, _vp, _vp]),
}

BINDING = _bind("gcd_amd_lpips", LPIPS_LIB_PATH, LPIPS_ABI_VERSION, "gcd_lpips_abi_version", "gcd_lpips_last_error",
                LPIPS_SIGNATURES)
load, check = BINDING.load, BINDING.check
