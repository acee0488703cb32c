"""CPU: the add-on library libgcd_amd_clip.so (gcd_amd.csrc.build.ADDONS, gcd_amd/_lib_clip.py) held to the rules
tests/test_libraries_host.py states for every entry of LIBRARIES: its public header, its binding table and the symbols
the shared object exports are one set; header, binding and library agree on the ABI version; it shares no source, header
or symbol with any other library; it has no ctypes.Structure (so there is no layout to check against gcc); and it builds
from a tree that holds no build product, through build(), while every other library is current."""
import ctypes
import importlib.util
import re
import shutil

from gcd_amd import _lib, _lib_clip
from gcd_amd.csrc import build as b
from test_libraries_host import DECL, ROOT, _dynamic_exports, _public_headers

NAME = "gcd_amd_clip"


def test_addon_table_and_binding_name_the_same_library():
    assert list(b.ADDONS) == [NAME] and NAME not in b.LIBRARIES and NAME not in _lib.BINDINGS
    lib, rec = b.ADDONS[NAME], _lib_clip.BINDING
    assert isinstance(lib, b.Library) and isinstance(rec, _lib.Binding) and rec.name == NAME
    assert lib.so == rec.path == ROOT / "gcd_amd" / f"lib{NAME}.so" and lib.stamp == ROOT / "gcd_amd" / f".lib{NAME}.stamp"
    assert (_lib_clip.load, _lib_clip.check) == (rec.load, rec.check)
    assert lib.stamp.name in (ROOT / ".gitignore").read_text().split()


def test_header_binding_table_and_exports_are_one_set():
    b.build(verbose=False)
    lib, rec = b.ADDONS[NAME], _lib_clip.BINDING
    headers = _public_headers(lib)
    assert len(headers) == len(rec.tables) == 1
    declared = set(re.findall(DECL, headers[0].read_text(), flags=re.M))
    assert declared == set(rec.tables[0]), declared ^ set(rec.tables[0])
    assert {rec.version_entry, rec.error_entry} <= declared
    exported = {n for n in _dynamic_exports(lib.so) if n.startswith("gcd_")}
    assert exported == declared, exported ^ declared
    assert len(declared) == 6


def test_header_binding_and_library_agree_on_the_abi_version():
    b.build(verbose=False)
    lib, rec = b.ADDONS[NAME], _lib_clip.BINDING
    text = _public_headers(lib)[0].read_text()
    assert [int(v) for v in re.findall(r"^#define GCD_AMD_\w*ABI_VERSION (\d+)", text, flags=re.M)] == [1]
    assert rec.abi_version == _lib_clip.CLIP_ABI_VERSION == 1
    assert getattr(rec.load(), rec.version_entry)() == 1
    # the limits the binding mirrors
    for define, value in (("GCD_CLIP_ATTN_MAX_S", _lib_clip.CLIP_ATTN_MAX_S), ("GCD_CLIP_HEAD_DIM", _lib_clip.CLIP_HEAD_DIM),
                          ("GCD_CLIP_MAX_BLUR", _lib_clip.CLIP_MAX_BLUR), ("GCD_CLIP_MAX_WIDTH", _lib_clip.CLIP_MAX_WIDTH),
                          ("GCD_CLIP_MAX_MODEL_WIDTH", _lib_clip.CLIP_MAX_MODEL_WIDTH)):
        assert re.findall(rf"^#define {define} (\d+)", text, flags=re.M) == [str(value)], define


def test_addon_shares_no_symbol_source_or_header_and_has_no_structure():
    lib, rec = b.ADDONS[NAME], _lib_clip.BINDING
    for other in _lib.BINDINGS.values():
        for t in other.tables:
            assert not set(t) & set(rec.tables[0]), (other.name, set(t) & set(rec.tables[0]))
    for other in b.LIBRARIES.values():
        assert not set(lib.sources) & set(other.sources) and not set(lib.headers) & set(other.headers), other.name
    assert all((b.CSRC / s).is_file() for s in lib.sources) and all(h.is_file() for h in lib.headers)
    # the source includes its own public header and nothing else of the project
    for s in lib.sources:
        includes = re.findall(r'^#include "([^"]+)"', (b.CSRC / s).read_text(), flags=re.M)
        assert includes == ["../../include/gcd_amd_clip.h"], includes
    assert not [n for n, v in vars(_lib_clip).items()
                if isinstance(v, type) and issubclass(v, ctypes.Structure) and v.__module__ == _lib_clip.__name__]
    assert "struct" not in re.sub(r"/\*.*?\*/", "", _public_headers(lib)[0].read_text(), flags=re.S)
    # the step's source digest does not know the add-on
    assert not set(lib.sources) & set(b.SOURCES) and not set(lib.headers) & set(b.HEADERS)


def test_addon_builds_from_a_clean_tree_through_build(tmp_path):
    """A copy of the build script, the sources and the headers, and nothing built.  With every library of LIBRARIES
    current, build() compiles exactly the add-on and returns the main library's path; a second call compiles nothing."""
    shutil.copytree(ROOT / "gcd_amd" / "csrc", tmp_path / "gcd_amd" / "csrc", ignore=shutil.ignore_patterns("build", "__pycache__"))
    shutil.copytree(ROOT / "include", tmp_path / "include")
    spec = importlib.util.spec_from_file_location("clean_tree_build_clip", tmp_path / "gcd_amd" / "csrc" / "build.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    lib = m.ADDONS[NAME]
    assert lib.so == tmp_path / "gcd_amd" / f"lib{NAME}.so" and not lib.so.exists()
    for o in m.LIBRARIES.values():
        o.so.write_bytes(b"")
        o.stamp.write_text(m._digest(o))
    assert m.build(verbose=False) == m.LIB == tmp_path / "gcd_amd" / "libgcd_amd.so"
    assert all(o.so.stat().st_size == 0 for o in m.LIBRARIES.values())
    assert lib.stamp.read_text() == m._digest(lib)
    exported = {n for n in _dynamic_exports(lib.so) if n.startswith("gcd_")}
    assert exported == set(_lib_clip.CLIP_SIGNATURES), exported
    before = lib.so.stat().st_mtime_ns
    m.build(verbose=False)
    assert lib.so.stat().st_mtime_ns == before
