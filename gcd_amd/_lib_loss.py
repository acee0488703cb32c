"""ctypes binding of libgcd_amd_loss.so (include/gcd_amd_loss.h; gcd_amd/csrc/loss.hip): the fine-tune loss on the device.
A library beside gcd_amd/_lib.py (gcd_amd.csrc.build.LIBRARIES), like gcd_amd/_lib_lpips.py: the same `Binding` record, made
by the same `_bind`, so loading and error reporting behave as for every other library — a missing shared object or a
non-zero status raises GcdError, nothing falls back."""
from __future__ import annotations

import ctypes as C

from ._lib import _PKG, _bind

LOSS_LIB_PATH = _PKG / "libgcd_amd_loss.so"
LOSS_ABI_VERSION = 1
LOSS_MAX_CLASSES = 16          # rows of a class table of gcd_loss_class_map
LOSS_MAX_BT = 65535            # frames per call
LOSS_MAX_N = 16777216          # elements per frame of the focal loss
LOSS_MAX_MAP_W = 512           # widest weight map
LOSS_L2 = 0
LOSS_L1 = 1

_vp, _i = C.c_void_p, C.c_int

LOSS_SIGNATURES = {
    "gcd_loss_abi_version": (_i, []),
    "gcd_loss_last_error": (C.c_char_p, []),
    "gcd_loss_class_map": (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _i, _i, _vp]),
    "gcd_loss_focal_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "gcd_loss_focal_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
}

BINDING = _bind("gcd_amd_loss", LOSS_LIB_PATH, LOSS_ABI_VERSION, "gcd_loss_abi_version", "gcd_loss_last_error",
                LOSS_SIGNATURES)
load, check = BINDING.load, BINDING.check
