"""CPU: the C ABI of libgcd_amd_metrics.so (include/gcd_amd_metrics.h) — header, binding table and exported symbols are
one set; the library builds from a tree that holds no build product, through build(); arguments are validated before
any launch; the Python surface refuses what is not a GPU tensor."""
import importlib.util
import re
import shutil
import struct
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
DECL = r"^\s*(?:int|int64_t|const char\*)\s+(gcd_\w+)\s*\("


def _dynamic_exports(path: Path):
    """Names of the defined global functions in the .dynsym of an ELF64 little-endian shared object."""
    d = path.read_bytes()
    assert d[:6] == b"\x7fELF\x02\x01", "an ELF64 little-endian file"
    shoff, = struct.unpack_from("<Q", d, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", d, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", d, shoff + i * shentsize) for i in range(shnum)]
    names = set()
    for (_, sh_type, _, _, off, size, link, _, _, entsize) in sections:
        if sh_type != 11:                      # SHT_DYNSYM
            continue
        stroff = sections[link][4]
        for j in range(size // entsize):
            st_name, st_info, _, st_shndx, _, _ = struct.unpack_from("<IBBHQQ", d, off + j * entsize)
            if st_shndx != 0 and (st_info & 0xF) == 2 and (st_info >> 4) == 1:      # defined, FUNC, GLOBAL
                names.add(d[stroff + st_name:d.index(b"\0", stroff + st_name)].decode())
    return names


def test_metrics_header_binding_table_and_exports_are_one_set():
    from gcd_amd import _lib
    from gcd_amd.csrc import build as b
    b.build(verbose=False)                     # a no-op when the libraries are current
    header = (ROOT / "include" / "gcd_amd_metrics.h").read_text()
    declared = set(re.findall(DECL, header, flags=re.M))
    assert declared == set(_lib.METRICS_SIGNATURES), declared ^ set(_lib.METRICS_SIGNATURES)
    exported = {n for n in _dynamic_exports(_lib.METRICS_LIB_PATH) if n.startswith("gcd_")}
    assert exported == declared, exported ^ declared
    assert {"gcd_metrics_abi_version", "gcd_metrics_last_error", "gcd_metrics_frames_f32", "gcd_metrics_frames_scratch_bytes",
            "gcd_metrics_diversity_f32"} <= declared
    lib = _lib.load_metrics()
    assert lib.gcd_metrics_abi_version() == _lib.METRICS_ABI_VERSION == 1
    assert int(re.search(r"#define GCD_AMD_METRICS_ABI_VERSION (\d+)", header).group(1)) == 1
    assert int(re.search(r"#define GCD_METRICS_SIGNED (\d+)", header).group(1)) == _lib.METRICS_SIGNED
    assert int(re.search(r"#define GCD_METRICS_FRAME_VALUES (\d+)", header).group(1)) == _lib.METRICS_FRAME_VALUES == 6
    assert int(re.search(r"#define GCD_METRICS_DIVERSITY_VALUES (\d+)", header).group(1)) == _lib.METRICS_DIVERSITY_VALUES == 3
    # a library of its own: the main header, its table, its ABI version and the step's source digest do not know it
    main_header = (ROOT / "include" / "gcd_amd.h").read_text()
    assert "gcd_metrics" not in main_header and not (declared & set(_lib.SIGNATURES)) and _lib.ABI_VERSION == 9
    assert set(re.findall(DECL, main_header, flags=re.M)) == set(_lib.SIGNATURES)
    assert not (set(b.METRICS_SOURCES) & set(b.SOURCES + b.TRAIN_SOURCES + b.SAMPLER_SOURCES))
    assert not (set(b.METRICS_HEADERS) & set(b.HEADERS + b.TRAIN_HEADERS + b.SAMPLER_HEADERS))


def test_metrics_library_builds_from_a_clean_tree_through_build(tmp_path):
    """A copy of the build script, the source and the header, and nothing built: build() makes the library even when
    the main library is current (it returns early then), and a second call compiles nothing."""
    (tmp_path / "gcd_amd" / "csrc").mkdir(parents=True)
    (tmp_path / "include").mkdir()
    for rel in ("gcd_amd/csrc/build.py", "gcd_amd/csrc/metrics.hip", "include/gcd_amd_metrics.h"):
        shutil.copy(ROOT / rel, tmp_path / rel)
    spec = importlib.util.spec_from_file_location("clean_tree_build", tmp_path / "gcd_amd" / "csrc" / "build.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert m.LIB_METRICS == tmp_path / "gcd_amd" / "libgcd_amd_metrics.so" and not m.LIB_METRICS.exists()
    # the other libraries are none of this test's business: stand-ins, and a main library that counts as current
    called = []
    m.build_train = lambda **k: called.append("train")
    m.build_sampler = lambda **k: called.append("sampler")
    m._digest = lambda: "current"
    m.LIB.write_bytes(b"")
    m.STAMP.write_text("current")
    assert m.build(verbose=False) == m.LIB and called == ["train", "sampler"]
    assert m.LIB_METRICS.exists() and m.STAMP_METRICS.exists()
    exported = {n for n in _dynamic_exports(m.LIB_METRICS) if n.startswith("gcd_")}
    assert "gcd_metrics_frames_f32" in exported and "gcd_metrics_diversity_f32" in exported
    before = m.LIB_METRICS.stat().st_mtime_ns
    m.build(verbose=False)
    assert m.LIB_METRICS.stat().st_mtime_ns == before
    assert ".libgcd_amd_metrics.stamp" in (ROOT / ".gitignore").read_text().split()


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
