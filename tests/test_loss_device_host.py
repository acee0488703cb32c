"""CPU: the loss library (libgcd_amd_loss.so; gcd_amd.csrc.build.EXTRAS, gcd_amd/_lib_loss.py) and the loss engine switch
of gcd_amd/training.py.  The library is held to the rules tests/test_lpips_host.py states for an extension: header,
binding table and exports are one set, one ABI version, the limits mirrored, no shared source, header or symbol, no
ctypes.Structure, and a build from a clean tree through build().  The switch takes two names, defaults to torch, and under
`hip` operands that are not on a GPU raise GcdError."""
import ctypes
import importlib.util
import re
import shutil
from pathlib import Path

import pytest
import torch

from gcd_amd import _lib, _lib_clip, _lib_loss, _lib_lpips
from gcd_amd._lib import GcdError
from gcd_amd.csrc import build as b
from test_libraries_host import DECL, ROOT, _dynamic_exports, _public_headers

NAME = "gcd_amd_loss"
GOLD = Path(__file__).resolve().parent / "golden" / "loss_kat.pt"
CFG = dict(
    harmonize_sigmas=True, focus_top=0.1, focus_steps=5000,
    batch2model_keys=["image_only_indicator", "num_video_frames"],
    loss_weighting_config={"target": "gcd_amd.training.EDMWeighting", "params": {"sigma_data": 1.0}},
    sigma_sampler_config={"target": "gcd_amd.training.EDMSampling", "params": {"p_mean": 1.0, "p_std": 1.6}})


# ----------------------------------------------------------------------------------------------------------- the library
def test_extras_table_and_binding_name_the_same_library():
    assert list(b.EXTRAS) == [NAME] and NAME not in _lib.BINDINGS
    assert not any(NAME in table for table in (b.LIBRARIES, b.ADDONS, b.EXTENSIONS))
    lib, rec = b.EXTRAS[NAME], _lib_loss.BINDING
    assert isinstance(lib, b.Library) and isinstance(rec, _lib.Binding) and rec.name == NAME
    assert lib.so == rec.path == ROOT / "gcd_amd" / f"lib{NAME}.so" and lib.stamp == ROOT / "gcd_amd" / f".lib{NAME}.stamp"
    assert (_lib_loss.load, _lib_loss.check) == (rec.load, rec.check)
    assert lib.stamp.name in (ROOT / ".gitignore").read_text().split()


def test_header_binding_table_and_exports_are_one_set():
    b.build(verbose=False)
    lib, rec = b.EXTRAS[NAME], _lib_loss.BINDING
    headers = _public_headers(lib)
    assert len(headers) == len(rec.tables) == 1
    declared = set(re.findall(DECL, headers[0].read_text(), flags=re.M))
    assert declared == set(rec.tables[0]), declared ^ set(rec.tables[0])
    assert {rec.version_entry, rec.error_entry} <= declared
    exported = {n for n in _dynamic_exports(lib.so) if n.startswith("gcd_")}
    assert exported == declared, exported ^ declared
    assert len(declared) == 5


def test_header_binding_and_library_agree_on_the_abi_version_and_limits():
    b.build(verbose=False)
    lib, rec = b.EXTRAS[NAME], _lib_loss.BINDING
    text = _public_headers(lib)[0].read_text()
    assert [int(v) for v in re.findall(r"^#define GCD_AMD_\w*ABI_VERSION (\d+)", text, flags=re.M)] == [1]
    assert rec.abi_version == _lib_loss.LOSS_ABI_VERSION == 1
    assert getattr(rec.load(), rec.version_entry)() == 1
    mirrored = {"GCD_LOSS_MAX_CLASSES": _lib_loss.LOSS_MAX_CLASSES, "GCD_LOSS_MAX_BT": _lib_loss.LOSS_MAX_BT,
                "GCD_LOSS_MAX_N": _lib_loss.LOSS_MAX_N, "GCD_LOSS_MAX_MAP_W": _lib_loss.LOSS_MAX_MAP_W,
                "GCD_LOSS_L2": _lib_loss.LOSS_L2, "GCD_LOSS_L1": _lib_loss.LOSS_L1}
    defines = dict(re.findall(r"^#define (GCD_LOSS_\w+) (\d+)", text, flags=re.M))
    assert {k: int(v) for k, v in defines.items()} == mirrored          # every define of the header, and nothing else
    assert {n for n in vars(_lib_loss) if n.startswith("LOSS_") and n.isupper()} == \
        {k[4:] for k in mirrored} | {"LOSS_LIB_PATH", "LOSS_ABI_VERSION", "LOSS_SIGNATURES"}
    assert _lib_loss.LOSS_MAX_N >= 4 * 128 * 128 and _lib_loss.LOSS_MAX_CLASSES == 16     # full-resolution latents fit
    from gcd_amd import training as TR
    assert len(TR.PD_PERSON_RGB) + len(TR.PD_VEHICLE_RGB) <= _lib_loss.LOSS_MAX_CLASSES


def test_library_shares_no_symbol_source_or_header_and_has_no_structure():
    lib, rec = b.EXTRAS[NAME], _lib_loss.BINDING
    for other in (*_lib.BINDINGS.values(), _lib_clip.BINDING, _lib_lpips.BINDING):
        for t in other.tables:
            assert not set(t) & set(rec.tables[0]), (other.name, set(t) & set(rec.tables[0]))
    for other in (*b.LIBRARIES.values(), *b.ADDONS.values(), *b.EXTENSIONS.values()):
        assert not set(lib.sources) & set(other.sources) and not set(lib.headers) & set(other.headers), other.name
    assert all((b.CSRC / s).is_file() for s in lib.sources) and all(h.is_file() for h in lib.headers)
    for s in lib.sources:       # the source includes its own public header and nothing else of the project
        includes = re.findall(r'^#include "([^"]+)"', (b.CSRC / s).read_text(), flags=re.M)
        assert includes == ["../../include/gcd_amd_loss.h"], includes
    assert not [n for n, v in vars(_lib_loss).items()
                if isinstance(v, type) and issubclass(v, ctypes.Structure) and v.__module__ == _lib_loss.__name__]
    assert "struct" not in re.sub(r"/\*.*?\*/", "", _public_headers(lib)[0].read_text(), flags=re.S)
    assert not set(lib.sources) & set(b.SOURCES) and not set(lib.headers) & set(b.HEADERS)      # not in the step's digest


def test_library_builds_from_a_clean_tree_through_build(tmp_path):
    """A copy of the build script, the sources and the headers, and nothing built.  With every other library current,
    build() compiles exactly this one and returns the main library's path; a second call compiles nothing."""
    shutil.copytree(ROOT / "gcd_amd" / "csrc", tmp_path / "gcd_amd" / "csrc", ignore=shutil.ignore_patterns("build", "__pycache__"))
    shutil.copytree(ROOT / "include", tmp_path / "include")
    spec = importlib.util.spec_from_file_location("clean_tree_build_loss", tmp_path / "gcd_amd" / "csrc" / "build.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    lib = m.EXTRAS[NAME]
    assert lib.so == tmp_path / "gcd_amd" / f"lib{NAME}.so" and not lib.so.exists()
    others = (*m.LIBRARIES.values(), *m.ADDONS.values(), *m.EXTENSIONS.values())
    for o in others:
        o.so.write_bytes(b"")
        o.stamp.write_text(m._digest(o))
    for f in ("engine.py", "ops.py", "sampling.py"):            # (the host side that sources_digest() reads)
        shutil.copy(ROOT / "gcd_amd" / f, tmp_path / "gcd_amd" / f)
    digest = m.sources_digest()
    assert m.build(verbose=False) == m.LIB == tmp_path / "gcd_amd" / "libgcd_amd.so"
    assert all(o.so.stat().st_size == 0 for o in others)
    assert lib.stamp.read_text() == m._digest(lib)
    exported = {n for n in _dynamic_exports(lib.so) if n.startswith("gcd_")}
    assert exported == set(_lib_loss.LOSS_SIGNATURES), exported
    before = lib.so.stat().st_mtime_ns
    m.build(verbose=False)
    assert lib.so.stat().st_mtime_ns == before
    # the loss is no part of what a sampler step launches: its source does not move sources_digest()
    (tmp_path / "gcd_amd" / "csrc" / "loss.hip").write_text("// changed\n")
    assert m._digest(lib) != lib.stamp.read_text() and m.sources_digest() == digest


def test_bad_arguments_return_a_status_and_a_message():
    """Every argument is checked before anything is launched (no device is needed to be refused)."""
    b.build(verbose=False)
    lib = _lib_loss.load()
    one = ctypes.c_void_p(16)                   # never dereferenced: every call below fails its checks first
    tab = (ctypes.c_float * 4)()
    bad = [lambda: lib.gcd_loss_class_map(None, 1, 8, 8, tab, 1, one, 1, 1, None),
           lambda: lib.gcd_loss_class_map(one, 1, 8, 8, tab, _lib_loss.LOSS_MAX_CLASSES + 1, one, 1, 1, None),
           lambda: lib.gcd_loss_class_map(one, 1, 8, 8, tab, 1, one, 9, 1, None),           # a map taller than the frame
           lambda: lib.gcd_loss_class_map(one, 1, 8, 1024, tab, 1, one, 1, _lib_loss.LOSS_MAX_MAP_W + 1, None),
           lambda: lib.gcd_loss_class_map(one, _lib_loss.LOSS_MAX_BT + 1, 8, 8, tab, 1, one, 1, 1, None),
           lambda: lib.gcd_loss_focal_fwd(one, one, one, None, 1, 12, 6, 0, 13, one, one, None),            # keep > n
           lambda: lib.gcd_loss_focal_fwd(one, one, one, None, 1, 12, 5, 0, 1, one, one, None),             # HW does not divide n
           lambda: lib.gcd_loss_focal_fwd(one, one, one, None, 1, 12, 6, 2, 1, one, one, None),             # loss_type
           lambda: lib.gcd_loss_focal_fwd(one, one, one, None, 1, _lib_loss.LOSS_MAX_N + 1, 1, 0, 1, one, one, None),
           lambda: lib.gcd_loss_focal_fwd(one, one, one, None, 1, 12, 6, 0, 1, one, None, None),            # no state
           lambda: lib.gcd_loss_focal_bwd(one, one, one, None, one, one, 1, 12, 6, 0, -1, one, None),
           lambda: lib.gcd_loss_focal_bwd(one, one, one, None, one, one, 1, 12, 6, 0, 1, None, None),
           lambda: lib.gcd_loss_focal_bwd(one, one, one, None, one, one, 1, 12, 6, 0, 1, one, None)]        # dout aliases out
    for k, call in enumerate(bad):
        assert call() == 2, k
        assert lib.gcd_loss_last_error().decode().startswith("gcd_loss_"), k
        with pytest.raises(GcdError):
            _lib_loss.check(2, "gcd_loss")


# ------------------------------------------------------------------------------------------------------------ the switch
def test_loss_engine_switch_takes_two_names_and_defaults_to_torch():
    import os
    import subprocess
    import sys
    from gcd_amd import training as TR
    assert TR.LOSS_ENGINE == os.environ.get("GCD_TRAIN_LOSS", "torch")
    # the environment variable is read at import: one child process (the variable's value goes through set_loss_engine,
    # so a typo raises there as it does below)
    code = "from gcd_amd import training as TR; print(TR.LOSS_ENGINE)"
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, GCD_TRAIN_LOSS="hip"), capture_output=True,
                         text=True)
    assert run.stdout.strip() == "hip", run.stderr
    old = TR.LOSS_ENGINE
    try:
        for name in ("hip", "torch"):
            TR.set_loss_engine(name)
            assert TR.LOSS_ENGINE == name
        for bad in ("HIP", "triton", "", None):
            with pytest.raises(ValueError):
                TR.set_loss_engine(bad)
        assert TR.LOSS_ENGINE == "torch"
    finally:
        TR.set_loss_engine(old)


def test_hip_engine_refuses_cpu_operands_and_torch_engine_is_untouched():
    from gcd_amd import loss_device, training as TR
    g = torch.load(GOLD)
    w = g["weights"][:, None, None, None]
    case = next(c for c in g["cases"] if c["step"] > 0 and c["loss_type"] == "l2")
    loss = TR.StandardDiffusionLoss(**CFG)
    old = TR.LOSS_ENGINE
    try:
        TR.set_loss_engine("hip")
        with pytest.raises(GcdError):
            loss.get_loss(g["out"], g["tgt"], w, {"global_step": case["step"]})
        with pytest.raises(GcdError):          # also without a focal selection (step 0: cur_top = 1)
            loss.get_loss(g["out"], g["tgt"], w, {"global_step": 0})
        pd = TR.StandardDiffusionLoss(**dict(CFG, pd_person_weight=7.0))
        with pytest.raises(GcdError):
            pd.get_loss(g["out"], g["tgt"], w, {"global_step": 1, "jpg": torch.zeros(g["out"].shape[0], 3, 8, 8)})
        with pytest.raises(NotImplementedError):
            TR.StandardDiffusionLoss(**dict(CFG, loss_type="lpips"))
        TR.set_loss_engine("torch")
        got = loss.get_loss(g["out"], g["tgt"], w, {"global_step": case["step"]})
        assert torch.allclose(got, case["loss"], rtol=1e-6, atol=0)
    finally:
        TR.set_loss_engine(old)
    x = torch.zeros(2, 4, 3, 5)
    with pytest.raises(GcdError):
        loss_device.focal_loss(x, x, torch.ones(2), 1)
    with pytest.raises(GcdError):
        loss_device.class_weight_map(torch.zeros(2, 3, 8, 8), (1, 1), [((0, 0, 142), 3.0)])
    with pytest.raises(GcdError):
        loss_device.class_table([((0, 0, 0), 2.0)] * (_lib_loss.LOSS_MAX_CLASSES + 1))
    tab = loss_device.class_table([((0, 0, 142), 3.0), ((220, 20, 60), 7.0)])
    assert tab.dtype == torch.float32 and tab.shape == (2, 4) and tab[:, 3].tolist() == [2.0, 6.0]
    assert torch.equal(tab[0, :3], torch.tensor((0, 0, 142), dtype=torch.float32) / 127.5 - 1.0)


def test_class_list_is_the_reference_order():
    from gcd_amd import training as TR
    from oracle import loss_ref as R
    both = TR.StandardDiffusionLoss(**dict(CFG, pd_person_weight=7.0, pd_vehicle_weight=3.0))._pd_classes()
    assert [list(rgb) for rgb, _ in both] == R.PD_PERSON + R.PD_VEHICLE
    assert [wt for _, wt in both] == [7.0] * len(R.PD_PERSON) + [3.0] * len(R.PD_VEHICLE)
    assert TR.StandardDiffusionLoss(**CFG)._pd_classes() == []
    assert [list(rgb) for rgb, _ in TR.StandardDiffusionLoss(**dict(CFG, pd_vehicle_weight=3.0))._pd_classes()] == R.PD_VEHICLE
