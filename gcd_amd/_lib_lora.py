"""ctypes binding of libgcd_amd_lora.so (include/gcd_amd_lora.h; gcd_amd/csrc/lora.hip): LoRA by merged weights.
A library beside gcd_amd/_lib.py (gcd_amd.csrc.build.LIBRARIES), like gcd_amd/_lib_loss.py: the same `Binding` record, made
by the same `_bind`, so loading and error reporting behave as for every other library — a missing shared object or a
non-zero status raises GcdError, nothing falls back."""
from __future__ import annotations

import ctypes as C

from ._lib import _PKG, _bind

LORA_LIB_PATH = _PKG / "libgcd_amd_lora.so"
LORA_ABI_VERSION = 1
LORA_MAX_RANK = 64             # largest r
LORA_MAX_ENTRIES = 65535       # entries of one table
LORA_MAX_DIM = 1048576         # largest N and K
LORA_MERGE_TILE = 64           # gcd_lora_merge: one workgroup per tile of this side
LORA_PROJECT_TILE = 256        # gcd_lora_project: one workgroup per region of this side

_vp, _i, _i64 = C.c_void_p, C.c_int, C.c_int64


class LoraEntry(C.Structure):
    """gcd_lora_entry (include/gcd_amd_lora.h): one adapted layer of a grouped launch."""
    _fields_ = [("W0", _vp), ("W", _vp), ("A", _vp), ("B", _vp), ("dW", _vp), ("dA", _vp), ("dB", _vp),
                ("scratch0", _i64), ("N", C.c_int32), ("K", C.c_int32), ("r", C.c_int32), ("scale", C.c_float),
                ("merge_tile0", C.c_int32), ("project_tile0", C.c_int32)]


LORA_SIGNATURES = {
    "gcd_lora_abi_version": (_i, []),
    "gcd_lora_last_error": (C.c_char_p, []),
    "gcd_lora_merge": (_i, [_vp, _i, _i, _vp]),
    "gcd_lora_project_scratch_floats": (_i64, [_i, _i, _i]),
    "gcd_lora_project": (_i, [_vp, _i, _i, _i, _vp, _i64, _vp]),
}

BINDING = _bind("gcd_amd_lora", LORA_LIB_PATH, LORA_ABI_VERSION, "gcd_lora_abi_version", "gcd_lora_last_error",
                LORA_SIGNATURES)
load, check = BINDING.load, BINDING.check


def _tiles(N: int, K: int, tile: int) -> int:
    return ((N + tile - 1) // tile) * ((K + tile - 1) // tile)


def fill_table(entries) -> tuple:
    """Set the running sums of a list of LoraEntry (merge_tile0, project_tile0, scratch0) from their N, K, r and return
    (merge tiles, project tiles, scratch floats) of the whole table."""
    lib = load()
    mt = pt = sf = 0
    for e in entries:
        need = lib.gcd_lora_project_scratch_floats(e.N, e.K, e.r)
        if need < 0:
            check(2, "gcd_lora_project_scratch_floats")
        e.merge_tile0, e.project_tile0, e.scratch0 = mt, pt, sf
        mt += _tiles(e.N, e.K, LORA_MERGE_TILE)
        pt += _tiles(e.N, e.K, LORA_PROJECT_TILE)
        sf += need
    return mt, pt, sf
