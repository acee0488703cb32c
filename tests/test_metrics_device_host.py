"""CPU: the C ABI of libgcd_amd_metrics.so (include/gcd_amd_metrics.h) — header, binding table and exported symbols are
one set and the library builds from a tree that holds no build product (tests/test_libraries_host.py); the header's
constants are the binding's; arguments are validated before any launch; the Python surface refuses what is not a GPU tensor."""
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
DECL = r"^\s*(?:int|int64_t|const char\*)\s+(gcd_\w+)\s*\("


def test_metrics_header_binding_table_and_exports_are_one_set():
    from gcd_amd import _lib
    from gcd_amd.csrc import build as b
    header = (ROOT / "include" / "gcd_amd_metrics.h").read_text()
    declared = set(re.findall(DECL, header, flags=re.M))      # == table == exports: tests/test_libraries_host.py
    assert {"gcd_metrics_abi_version", "gcd_metrics_last_error", "gcd_metrics_frames_f32", "gcd_metrics_frames_scratch_bytes",
            "gcd_metrics_diversity_f32"} <= declared
    assert int(re.search(r"#define GCD_METRICS_SIGNED (\d+)", header).group(1)) == _lib.METRICS_SIGNED
    assert int(re.search(r"#define GCD_METRICS_FRAME_VALUES (\d+)", header).group(1)) == _lib.METRICS_FRAME_VALUES == 6
    assert int(re.search(r"#define GCD_METRICS_DIVERSITY_VALUES (\d+)", header).group(1)) == _lib.METRICS_DIVERSITY_VALUES == 3
    # a library of its own (its symbols, sources and headers are apart from the others': tests/test_libraries_host.py)
    assert "gcd_metrics" not in (ROOT / "include" / "gcd_amd.h").read_text()
    assert b.LIBRARIES["gcd_amd_metrics"].sources == ["metrics.hip"] and "metrics.hip" not in b.SOURCES


def test_metrics_entries_validate_their_arguments_before_any_launch():
    from gcd_amd import _lib
    lib = _lib.load_metrics()
    P = 4096                                   # a stand-in for a device pointer: never dereferenced, nothing is launched
    S, T, H, W = 2, 3, 9, 13
    need = lib.gcd_metrics_frames_scratch_bytes(S, T, H, W)
    need_d = lib.gcd_metrics_diversity_scratch_bytes(S, T, H, W)
    assert need > 0 and need % 8 == 0 and need_d > 0 and need_d % 8 == 0
    assert lib.gcd_metrics_frames_scratch_bytes(S, T, 6, W) == 0 and b"7 x 7" in lib.gcd_metrics_last_error()

    def frames(pred=P, gt=P, rep=P, S=S, T=T, H=H, W=W, flags=0, scratch=P, nbytes=need, out=P):
        return lib.gcd_metrics_frames_f32(pred, gt, rep, S, T, H, W, flags, scratch, nbytes, out, None)

    def div(pred=P, rep=P, S=S, T=T, H=H, W=W, flags=0, unc=P, scratch=P, nbytes=need_d, out=P):
        return lib.gcd_metrics_diversity_f32(pred, rep, S, T, H, W, flags, unc, scratch, nbytes, out, None)

    for kw, msg in [(dict(H=6), b"7 x 7"), (dict(W=6), b"7 x 7"), (dict(H=0), b"7 x 7"), (dict(W=-5), b"7 x 7"),
                    (dict(S=0), b"empty problem"), (dict(S=-1), b"empty problem"), (dict(T=0), b"empty problem"),
                    (dict(pred=None), b"null pointer"), (dict(gt=None), b"null pointer"), (dict(out=None), b"null pointer"),
                    (dict(nbytes=need - 8), b"scratch too small"), (dict(scratch=None), b"scratch too small"),
                    (dict(scratch=P + 4), b"8-byte aligned"), (dict(flags=2), b"unknown flags"),
                    (dict(S=1 << 20, T=1 << 20, H=1 << 20, W=1 << 20), b"overflows")]:
        assert frames(**kw) != 0, kw
        assert msg in lib.gcd_metrics_last_error(), (kw, lib.gcd_metrics_last_error())
    for kw, msg in [(dict(H=6), b"7 x 7"), (dict(W=3), b"7 x 7"), (dict(S=0), b"empty problem"), (dict(T=0), b"empty problem"),
                    (dict(pred=None), b"null pointer"), (dict(unc=None), b"null pointer"), (dict(out=None), b"null pointer"),
                    (dict(nbytes=need_d - 8), b"scratch too small"), (dict(scratch=None), b"scratch too small"),
                    (dict(flags=4), b"unknown flags")]:
        assert div(**kw) != 0, kw
        assert msg in lib.gcd_metrics_last_error(), (kw, lib.gcd_metrics_last_error())
    # the scratch sizes are what the header's scheme says: ten doubles per 16 x 32 tile, four per block of 1024 pixels
    assert need == S * T * 1 * 1 * 10 * 8 and need_d == T * 1 * 4 * 8
    assert lib.gcd_metrics_frames_scratch_bytes(1, 1, 17, 33) == 2 * 2 * 10 * 8
    assert lib.gcd_metrics_diversity_scratch_bytes(1, 1, 576, 1024) == 576 * 4 * 8


def test_metrics_device_refuses_what_is_not_a_gpu_tensor():
    from gcd_amd import _lib, metrics_device as md
    pred, gt = torch.zeros(1, 1, 3, 9, 9), torch.zeros(1, 3, 9, 9)
    with pytest.raises(_lib.GcdError, match="no CPU"):
        md.frame_metrics(pred, gt)
    with pytest.raises(_lib.GcdError, match="no CPU"):
        md.diversity(pred)
    with pytest.raises(_lib.GcdError, match="no CPU"):
        md.calculate_metrics(gt, None, [{"sampled_rgb": pred[0]}])
    with pytest.raises(_lib.GcdError, match="no CPU"):
        md.calculate_metrics(gt, None, [{"sampled_rgb": pred[0].numpy()}])
