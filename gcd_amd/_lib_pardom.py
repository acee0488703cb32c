"""ctypes binding of libgcd_amd_pardom.so (include/gcd_amd_pardom.h; gcd_amd/csrc/pardom.hip): the colours of a
ParallelDomain point cloud.  A library beside gcd_amd/_lib.py (gcd_amd.csrc.build.LIBRARIES), like gcd_amd/_lib_lora.py: the
same `Binding` record, made by the same `_bind`, so loading and error reporting behave as for every other library — a
missing shared object or a non-zero status raises GcdError, nothing falls back."""
from __future__ import annotations

import ctypes as C

from ._lib import _PKG, _bind

PARDOM_LIB_PATH = _PKG / "libgcd_amd_pardom.so"
PARDOM_ABI_VERSION = 1
PARDOM_PALETTE_ROWS = 256      # rows of a palette: one per value of a uint8 class id
PARDOM_MAX_LD = 16777216       # largest row stride, in elements
PARDOM_RGB = 0                 # mode: the stored colour
PARDOM_BLEND = 1               # (1 - alpha) colour + alpha class colour
PARDOM_PALETTE = 2             # the class colour

_vp, _i, _i64, _d = C.c_void_p, C.c_int, C.c_int64, C.c_double

PARDOM_SIGNATURES = {
    "gcd_pardom_abi_version": (_i, []),
    "gcd_pardom_last_error": (C.c_char_p, []),
    "gcd_pardom_colours": (_i, [_vp, _i64, _vp, _i64, _i64, _vp, _i, _d, _i, _vp, _i64, _vp, _vp]),
}

BINDING = _bind("gcd_amd_pardom", PARDOM_LIB_PATH, PARDOM_ABI_VERSION, "gcd_pardom_abi_version", "gcd_pardom_last_error",
                PARDOM_SIGNATURES)
load, check = BINDING.load, BINDING.check
