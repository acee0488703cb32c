"""CPU: the deterministic reduction mode of the fine-tune step — the C-ABI surface of include/gcd_amd_train_det.h (symbols,
scratch sizes, argument validation: observable without a GPU), the switch and its public spellings, and the rule that the
new source holds no read-modify-write reduction."""
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
_DECL = r"^\s*(?:int|int64_t|const char\*)\s+(gcd_\w+)\s*\("


def _cdiv(a, b):
    return -(-a // b)


def test_det_header_signatures_and_abi_version():
    from gcd_amd import _lib
    header = (ROOT / "include" / "gcd_amd_train_det.h").read_text()
    declared = set(re.findall(_DECL, header, flags=re.M))
    assert declared == set(_lib.TRAIN_DET_SIGNATURES), (declared ^ set(_lib.TRAIN_DET_SIGNATURES))
    assert len(declared) == 10
    # exported, bound, apart from every other table, ABI version 3: tests/test_libraries_host.py
    from gcd_amd.csrc import build
    train = build.LIBRARIES["gcd_amd_train"]
    assert "train_det.hip" in train.sources and "train_det.hip" not in build.SOURCES
    assert ROOT / "include" / "gcd_amd_train_det.h" in train.headers


# (M, C, rows_per_block): cfg4's level-0 token count; per-frame blocks; M not a multiple of any row chunk
_SHAPES = [(43008, 320, 43008), (43008, 320, 1536), (28 * 97, 1280, 97)]


def test_scratch_floats_formulas():
    from gcd_amd import _lib
    lib = _lib.load_train()
    for M, C, rows in _SHAPES:
        nblk = M // rows
        # 1. row-block sums: clamp(rows / 256, 1, 64) slots per (block, column)
        assert lib.gcd_rowblock_sum_det_scratch_floats(M, C, rows) == nblk * min(max(rows // 256, 1), 64) * C
        # 2. LayerNorm backward: one slot of 2 C per workgroup of four rows-in-flight waves, at most 768
        assert lib.gcd_layernorm_bwd_det_scratch_floats(M, C) == min(_cdiv(M, 4), 768) * 2 * C
        # 3. cast + column sums: ~2048 workgroups over the launch, >= 32 rows per chunk
        colb = _cdiv(C, 64)
        chunks = min(max(_cdiv(2048, nblk * colb), 1), _cdiv(rows, 32))
        chunks = _cdiv(rows, _cdiv(rows, chunks))
        assert lib.gcd_cast_colsum_det_scratch_floats(M, C, rows) == nblk * chunks * C
        # 4. blend backward: one float per (frame, chunk); chunks = min(ceil(rows C / 1024), cap)
        cap = 1 if nblk >= 512 else _cdiv(4096, nblk)
        assert lib.gcd_blend_bwd_det_scratch_floats(M, C, rows) == nblk * min(_cdiv(rows * (C // 4), 256), cap)
    # the sizes DESIGN.md quotes for cfg4's level 0 (M = 43 008 tokens, C = 320)
    assert lib.gcd_layernorm_bwd_det_scratch_floats(43008, 320) * 4 == 768 * 2 * 320 * 4 < 2 << 20
    assert lib.gcd_cast_colsum_det_scratch_floats(43008, 320, 43008) * 4 < 1 << 20
    assert lib.gcd_rowblock_sum_det_scratch_floats(43008, 320, 43008) * 4 < 1 << 20
    # 5. few-row dgrad: a [32][256] tile per (problem, k chunk)
    for blocks in (1, 7, 440):
        assert lib.gcd_smallm_dgrad_det_scratch_floats(blocks) == blocks * 32 * 256
    # shapes the entries refuse have no scratch size
    assert lib.gcd_rowblock_sum_det_scratch_floats(100, 64, 33) == 0
    assert lib.gcd_cast_colsum_det_scratch_floats(0, 64, 1) == 0
    assert lib.gcd_smallm_dgrad_det_scratch_floats(0) == 0


def test_entries_refuse_small_scratch_and_misaligned_strides_without_a_gpu():
    """Argument validation happens before any launch.  Pointers are fake (16 = aligned, non-null): nothing is launched."""
    from gcd_amd import _lib
    lib = _lib.load_train()
    P, BIG = 16, 1 << 40
    M, C, rows = 1000, 64, 100

    def refused(rc, *words):
        assert rc != 0
        msg = lib.gcd_train_last_error()
        for w in words:
            assert w in msg, (w, msg)

    need = lib.gcd_rowblock_sum_det_scratch_floats(M, C, rows)
    refused(lib.gcd_rowblock_sum_det_f32(P, 64, M, C, rows, P, P, need - 1, None), b"scratch", b"gcd_rowblock_sum_det_scratch_floats")
    refused(lib.gcd_rowblock_sum_det_f32(P, 66, M, C, rows, P, P, BIG, None), b"multiples of 4")
    need = lib.gcd_layernorm_bwd_det_scratch_floats(M, C)
    refused(lib.gcd_layernorm_bwd_det(P, 64, P, 64, M, C, P, 1e-5, P, 64, P, P, None, 0, P, need - 1, None),
            b"scratch", b"gcd_layernorm_bwd_det_scratch_floats")
    refused(lib.gcd_layernorm_bwd_det(P, 64, P, 66, M, C, P, 1e-5, P, 64, P, P, None, 0, P, BIG, None), b"multiples of 4")
    need = lib.gcd_cast_colsum_det_scratch_floats(M, C, rows)
    refused(lib.gcd_cast_colsum_det_f32(P, 64, P, 64, M, C, rows, P, 0, None, P, need - 1, None),
            b"scratch", b"gcd_cast_colsum_det_scratch_floats")
    refused(lib.gcd_cast_colsum_det_f32(P, 64, P, 68, M, C, rows, P, 0, None, P, BIG, None), b"ldy of 8")
    need = lib.gcd_blend_bwd_det_scratch_floats(M, C, rows)
    refused(lib.gcd_blend_bwd_det_f32(P, 64, P, 64, P, 64, P, M, C, rows, P, 64, 0, P, 64, P, P, need - 1, None),
            b"scratch", b"gcd_blend_bwd_det_scratch_floats")
    refused(lib.gcd_blend_bwd_det_f32(P, 66, P, 64, P, 64, P, M, C, rows, P, 64, 0, P, 64, P, P, BIG, None), b"multiples of 4")
    # the few-row dgrad's strides live in its device table: what the host can refuse is the scratch and an empty table
    refused(lib.gcd_smallm_dgrad_det(P, 3, 7, P, 7 * 32 * 256 - 1, None), b"scratch", b"gcd_smallm_dgrad_det_scratch_floats")
    refused(lib.gcd_smallm_dgrad_det(P, 0, 7, P, BIG, None), b"empty table")
    # a misaligned scratch pointer is refused too
    refused(lib.gcd_rowblock_sum_det_f32(P, 64, M, C, rows, P, 20, BIG, None), b"16-byte aligned")


def test_switch_environment_default_and_denoiser_argument():
    from gcd_amd import autograd_ops as A, training as TR
    old = A.DETERMINISTIC
    try:
        assert TR.set_deterministic is A.set_deterministic
        A.set_deterministic(True)
        assert A.DETERMINISTIC is True and TR.is_deterministic()
        A.set_deterministic(False)
        assert A.DETERMINISTIC is False and not TR.is_deterministic()
        with pytest.raises(ValueError):
            A.set_deterministic("yes")
        # the environment default, read at import: "1" = on, anything else (and unset) = off — in fresh interpreters
        for value, want in (("1", True), ("0", False), (None, False)):
            env = {k: v for k, v in os.environ.items() if k != "GCD_TRAIN_DETERMINISTIC"}
            if value is not None:
                env["GCD_TRAIN_DETERMINISTIC"] = value
            out = subprocess.check_output(
                [sys.executable, "-c", "from gcd_amd import training as TR; print(TR.is_deterministic())"],
                cwd=str(ROOT), env=env).decode().strip().splitlines()[-1]
            assert out == str(want), (value, out)
    finally:
        A.set_deterministic(old)
    cfg = {"target": "gcd_amd.denoiser_scaling.VScalingWithEDMcNoise"}
    assert TR.TrainDenoiser(cfg).deterministic is None                # follows the process default, like engine=
    assert TR.TrainDenoiser(cfg, deterministic=True).deterministic is True
    assert TR.TrainDenoiser(cfg, deterministic=False).deterministic is False
    for bad in (1, 0, "on", "planned"):
        with pytest.raises(ValueError):
            TR.TrainDenoiser(cfg, deterministic=bad)


def test_new_source_holds_no_read_modify_write_reduction():
    """train_det.hip is two-pass only: the word does not even appear in a comment."""
    src = (ROOT / "gcd_amd" / "csrc" / "train_det.hip").read_text()
    assert "atomic" not in src.lower()
    assert "ordered fold" in src and "fold_slots" in src
