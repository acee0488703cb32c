"""CPU: what a HIP library of this project is, checked once for every entry of `gcd_amd.csrc.build.LIBRARIES` — its public
header(s), its binding table(s) (gcd_amd/_lib.py for the first five, gcd_amd/_lib_<x>.py for each later one) and the symbols
the shared object exports are one set; header, binding and library agree on the ABI version; no library knows another's
sources, headers or symbols; the binding mirrors every constant of a one-header library and nothing else; every
ctypes.Structure of a binding has the layout gcc gives the C struct; and each library beside the main one builds from a
tree that holds no build product, through build(), while every other library is current."""
import ctypes
import importlib
import importlib.util
import itertools
import re
import shutil
import struct
import subprocess
from pathlib import Path

import pytest

from gcd_amd import _lib
from gcd_amd.csrc import build as b

ROOT = Path(__file__).resolve().parent.parent
DECL = r"^\s*(?:int|int64_t|const char\*)\s+(gcd_\w+)\s*\("
NAMES = list(b.LIBRARIES)
ABI = {"gcd_amd": 9, "gcd_amd_train": 3, "gcd_amd_sampler": 1, "gcd_amd_metrics": 1, "gcd_amd_render": 1,
       "gcd_amd_clip": 1, "gcd_amd_lpips": 1, "gcd_amd_loss": 1, "gcd_amd_lora": 1, "gcd_amd_pardom": 1}
EXPORTS = {"gcd_amd": 69, "gcd_amd_train": 28, "gcd_amd_sampler": 3, "gcd_amd_metrics": 6, "gcd_amd_render": 6,
           "gcd_amd_clip": 6, "gcd_amd_lpips": 5, "gcd_amd_loss": 5, "gcd_amd_lora": 5, "gcd_amd_pardom": 3}
# every ctypes.Structure of a binding module: its C name and the header that defines it
STRUCTS = {"GemmDesc": ("gcd_gemm_desc", "gcd_amd.h"), "FfDesc": ("gcd_ff_desc", "gcd_amd.h"),
           "PackEntry": ("gcd_pack_entry", "gcd_amd_train.h"), "SmallmProblem": ("gcd_smallm_problem", "gcd_amd_train.h"),
           "OptimState": ("gcd_optim_state", "gcd_amd_train_optim.h"), "OptimTensor": ("gcd_optim_tensor", "gcd_amd_train_optim.h"),
           "OptimConfig": ("gcd_optim_config", "gcd_amd_train_optim.h"),
           "RenderSplatDesc": ("gcd_render_splat_desc", "gcd_amd_render.h"),
           "LoraEntry": ("gcd_lora_entry", "gcd_amd_lora.h")}


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


def _public_headers(lib):
    return [h for h in lib.headers if h.parent == b.INCLUDE]


def _module(name):
    """The module that binds library `name`: gcd_amd/_lib.py while it lists it, else gcd_amd/_lib_<x>.py for gcd_amd_<x>."""
    return _lib if name in _lib.BINDINGS else importlib.import_module("gcd_amd._lib_" + name[len("gcd_amd_"):])


def _binding(name):
    return _lib.BINDINGS[name] if name in _lib.BINDINGS else _module(name).BINDING


def _prefix(name):
    """What the binding module's constants of library `name` begin with: "" for the main one, else "TRAIN_", "CLIP_", ..."""
    return name[len("gcd_amd_"):].upper() + "_" if name != "gcd_amd" else ""


def _structures(name):
    """pyname -> C name of the structures STRUCTS registers for library `name` (by the header that defines them)."""
    headers = {h.name for h in _public_headers(b.LIBRARIES[name])}
    return {py: cname for py, (cname, header) in STRUCTS.items() if header in headers}


@pytest.fixture(scope="module")
def built():
    b.build(verbose=False)                     # a no-op when the libraries are current


def test_build_table_and_binding_records_name_the_same_libraries():
    assert NAMES == list(ABI) == list(EXPORTS) and len(NAMES) == 10
    assert NAMES[0] == "gcd_amd" and b.MAIN is b.LIBRARIES["gcd_amd"]
    assert (b.LIB, b.STAMP) == (b.MAIN.so, b.MAIN.stamp) and b.MAIN.sources is b.SOURCES and b.MAIN.headers is b.HEADERS
    # the convention _module() follows: the first five are gcd_amd/_lib.py's, each later one has gcd_amd/_lib_<x>.py
    assert list(_lib.BINDINGS) == NAMES[:5]
    assert sorted(p.stem for p in (ROOT / "gcd_amd").glob("_lib_*.py")) == sorted("_lib_" + n[len("gcd_amd_"):] for n in NAMES[5:])
    assert _lib.LIB_PATH == _lib.BINDINGS["gcd_amd"].path


@pytest.mark.parametrize("name", NAMES)
def test_library_and_its_binding_record_agree(name):
    lib, rec = b.LIBRARIES[name], _binding(name)
    assert isinstance(lib, b.Library) and isinstance(rec, _lib.Binding) and lib.name == rec.name == name
    assert lib.so == ROOT / "gcd_amd" / f"lib{name}.so" and lib.stamp == ROOT / "gcd_amd" / f".lib{name}.stamp"
    assert lib.stamp.name in (ROOT / ".gitignore").read_text().split()
    if name != "gcd_amd":                      # (GCD_AMD_LIB overrides the main library's path, and only that one)
        assert rec.path == lib.so
    suffix = name[len("gcd_amd"):] if name in _lib.BINDINGS else ""      # load_train, check_train, ... in _lib.py
    mod = _module(name)
    assert (getattr(mod, "load" + suffix), getattr(mod, "check" + suffix)) == (rec.load, rec.check)


@pytest.mark.parametrize("name", NAMES)
def test_header_binding_table_and_exports_are_one_set(built, name):
    lib, rec = b.LIBRARIES[name], _binding(name)
    headers = _public_headers(lib)
    assert len(headers) == len(rec.tables) >= 1
    for header, table in zip(headers, rec.tables):         # header by header: each table is exactly its header
        declared = set(re.findall(DECL, header.read_text(), flags=re.M))
        assert declared == set(table), (header.name, declared ^ set(table))
    bound = set().union(*rec.tables)
    assert {rec.version_entry, rec.error_entry} <= bound
    exported = {n for n in _dynamic_exports(lib.so) if n.startswith("gcd_")}
    assert exported == bound, exported ^ bound
    assert len(bound) == EXPORTS[name]
    if name == "gcd_amd_pardom":
        assert bound == {"gcd_pardom_abi_version", "gcd_pardom_last_error", "gcd_pardom_colours"}


@pytest.mark.parametrize("name", NAMES)
def test_header_binding_and_library_agree_on_the_abi_version(built, name):
    lib, rec = b.LIBRARIES[name], _binding(name)
    defines = [int(v) for h in _public_headers(lib) for v in re.findall(r"^#define GCD_AMD_\w*ABI_VERSION (\d+)", h.read_text(), flags=re.M)]
    assert defines == [ABI[name]]              # one header of the library defines it
    assert rec.abi_version == getattr(_module(name), _prefix(name) + "ABI_VERSION") == ABI[name]
    assert getattr(rec.load(), rec.version_entry)() == ABI[name]


def test_libraries_share_no_symbol_source_or_header():
    tables = [t for name in NAMES for t in _binding(name).tables]
    assert len(tables) == 12                   # 7 of gcd_amd/_lib.py and one of each later module
    for t, u in itertools.combinations(tables, 2):
        assert not set(t) & set(u), set(t) & set(u)
    for x, y in itertools.combinations(b.LIBRARIES.values(), 2):
        assert not set(x.sources) & set(y.sources) and not set(x.headers) & set(y.headers), (x.name, y.name)
    # the step's source digest knows the main library only
    for lib in list(b.LIBRARIES.values())[1:]:
        assert not set(lib.sources) & set(b.SOURCES) and not set(lib.headers) & set(b.HEADERS), lib.name
    for lib in b.LIBRARIES.values():
        assert all((b.CSRC / s).is_file() for s in lib.sources) and all(h.is_file() for h in lib.headers), lib.name


@pytest.mark.parametrize("name", NAMES[2:])
def test_sources_include_their_own_public_header_and_nothing_else_of_the_project(name):
    lib = b.LIBRARIES[name]
    header, = _public_headers(lib)
    for s in lib.sources:
        includes = re.findall(r'^#include "([^"]+)"', (b.CSRC / s).read_text(), flags=re.M)
        assert includes == ["../../include/" + header.name], (s, includes)


@pytest.mark.parametrize("name", NAMES[2:])
def test_binding_mirrors_every_constant_of_the_header_and_nothing_else(name):
    """Both ways, as a name-to-value map: the header's `#define GCD_<PFX>_<X> <int>` lines are the binding module's
    upper-case <PFX>_<X> names, beside the three every binding has (path, ABI version, signature table)."""
    header, = _public_headers(b.LIBRARIES[name])
    pfx = _prefix(name)
    text = header.read_text()
    defines = {k[len("GCD_"):]: int(v) for k, v in re.findall(rf"^#define (GCD_{pfx}\w+)\s+(-?\d+)\b", text, flags=re.M)}
    assert len(defines) == len(re.findall(rf"^#define GCD_{pfx}\w+", text, flags=re.M)) >= 1      # each one is an integer
    mirrored = {n: v for n, v in vars(_module(name)).items() if n.startswith(pfx) and n.isupper()
                and n not in (pfx + "LIB_PATH", pfx + "ABI_VERSION", pfx + "SIGNATURES")}
    assert mirrored == defines, set(mirrored.items()) ^ set(defines.items())


def test_every_structure_of_the_binding_is_registered():
    assert sorted(py for name in NAMES for py in _structures(name)) == sorted(STRUCTS)      # each in one library's header
    registered = {}                            # binding module -> the structures of the libraries it binds
    for name in NAMES:
        registered.setdefault(_module(name), set()).update(_structures(name))
    assert len(registered) == 6
    for mod, want in registered.items():
        defined = {n for n, v in vars(mod).items()
                   if isinstance(v, type) and issubclass(v, ctypes.Structure) and v.__module__ == mod.__name__}
        assert defined == want, (mod.__name__, defined ^ want)
    # and the other way: a public header has the structures registered for it, and without one it does not say `struct`
    for header in (h for name in NAMES for h in _public_headers(b.LIBRARIES[name])):
        text = re.sub(r"/\*.*?\*/", "", header.read_text(), flags=re.S)
        here = {cname for cname, h in STRUCTS.values() if h == header.name}
        assert set(re.findall(r"^\} (\w+);", text, flags=re.M)) == here, header.name
        assert ("struct" in text) == bool(here), header.name


@pytest.mark.parametrize("pyname", list(STRUCTS))
def test_struct_layout_matches_header(tmp_path, pyname):
    """The ctypes mirror has the C struct's field offsets and size (checked with gcc)."""
    assert shutil.which("gcc"), "gcc is a prerequisite of the suite"
    cname, header = STRUCTS[pyname]
    cls, = [getattr(_module(name), pyname) for name in NAMES if pyname in _structures(name)]
    fields = [f[0] for f in cls._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT / "include" / header}"', 'int main(void) {']
    src += [f'  printf("{n} %zu\\n", offsetof({cname}, {n}));' for n in fields]
    src += [f'  printf("sizeof %zu\\n", sizeof({cname}));', '  return 0;', '}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(c)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    for n in fields:
        assert int(out[n]) == getattr(cls, n).offset, n
    assert int(out["sizeof"]) == ctypes.sizeof(cls)


@pytest.mark.parametrize("name", NAMES[1:])
def test_library_builds_from_a_clean_tree_through_build(tmp_path, name):
    """A copy of the build script, the sources and the headers, and nothing built.  With every other library current,
    the main one included, build() compiles exactly the missing one and returns the main library's path; a second call
    compiles nothing; and no source of the library moves sources_digest()."""
    shutil.copytree(ROOT / "gcd_amd" / "csrc", tmp_path / "gcd_amd" / "csrc", ignore=shutil.ignore_patterns("build", "__pycache__"))
    shutil.copytree(ROOT / "include", tmp_path / "include")
    for f in ("engine.py", "ops.py", "sampling.py"):            # (the host side that sources_digest() reads)
        shutil.copy(ROOT / "gcd_amd" / f, tmp_path / "gcd_amd" / f)
    spec = importlib.util.spec_from_file_location("clean_tree_build_" + name, tmp_path / "gcd_amd" / "csrc" / "build.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert list(m.LIBRARIES) == NAMES
    lib = m.LIBRARIES[name]
    assert lib.so == tmp_path / "gcd_amd" / f"lib{name}.so" and not lib.so.exists()
    others = [o for o in m.LIBRARIES.values() if o is not lib]
    for o in others:
        o.so.write_bytes(b"")
        o.stamp.write_text(m._digest(o))
    digest = m.sources_digest()
    assert m.build(verbose=False) == m.LIB == tmp_path / "gcd_amd" / "libgcd_amd.so"
    assert all(o.so.stat().st_size == 0 for o in others)
    assert lib.stamp.read_text() == m._digest(lib)
    exported = {n for n in _dynamic_exports(lib.so) if n.startswith("gcd_")}
    assert exported == set().union(*_binding(name).tables), exported
    before = lib.so.stat().st_mtime_ns
    m.build(verbose=False)
    assert lib.so.stat().st_mtime_ns == before
    assert lib.stamp.name in (ROOT / ".gitignore").read_text().split()
    # the library is no part of what a sampler step launches: its sources move its own digest and not sources_digest()
    for s in lib.sources:
        was = m._digest(lib)
        (tmp_path / "gcd_amd" / "csrc" / s).write_text("// changed\n")
        assert m._digest(lib) != was and m._digest(lib) != lib.stamp.read_text() and m.sources_digest() == digest, s
