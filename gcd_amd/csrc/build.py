"""Build the project's HIP libraries (C ABI, one shared object each) in-tree with hipcc for gfx950.

Usage: python -m gcd_amd.csrc.build [--force] [--save-temps]
The shared objects land next to the package (gcd_amd/libgcd_amd*.so), inside the source tree, and are git-ignored.
`LIBRARIES` is where a new library is added; the first five are bound by gcd_amd/_lib.py, each later one by a module of
its own beside it (gcd_amd/_lib_clip.py, gcd_amd/_lib_lpips.py, gcd_amd/_lib_loss.py, gcd_amd/_lib_lora.py,
gcd_amd/_lib_pardom.py).
"""
from __future__ import annotations

import hashlib
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from typing import NamedTuple

CSRC = Path(__file__).resolve().parent
PKG = CSRC.parent
ROOT = PKG.parent
INCLUDE = ROOT / "include"
SOURCES = ["runtime.hip", "gemm.hip", "gemm_pp.hip", "gemm_p8.hip", "conv_narrow.hip", "ff_fused.hip", "lnqkv.hip", "norm.hip", "attention.hip",
           "attn_temporal_long.hip", "attn_bwd.hip", "elementwise.hip", "backward.hip"]
# per-source extra flags.  ff_fused.hip: hipcc's SLP pass pairs the GELU polynomial's scalar FMAs into v_pk_fma_f32, which
# does not issue in the shadow of an MFMA (tools/issue_probe; the kernel places every one of them behind an MFMA by hand)
EXTRA_FLAGS = {"ff_fused.hip": ["-fno-slp-vectorize"]}
# records of experiments that lost their A/B: compiled into the ablation / A-B libraries only (tools/libgcd_amd_*.so)
ABLATION_ONLY_SOURCES = ["gemm_p8x.hip"]
HEADERS = [CSRC / "common.h", CSRC / "gemm_common.h", CSRC / "ff_fused_kernel.h", INCLUDE / "gcd_amd.h"]
ARCH = "gfx950"
FLAGS = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-Wall", "-Wno-unused-function",
         "-ffp-contract=fast"]
MAX_JOBS = 16      # compiler processes at a time


class Library(NamedTuple):
    """One shared object: gcd_amd/lib<name>.so, current while gcd_amd/.lib<name>.stamp holds its digest."""
    name: str
    sources: list      # file names under CSRC
    headers: list      # paths: every header whose change must rebuild the library
    extra_flags: dict  # source -> flags added to FLAGS for that source

    @property
    def so(self) -> Path:
        return PKG / f"lib{self.name}.so"

    @property
    def stamp(self) -> Path:
        return PKG / f".lib{self.name}.stamp"


# Only the first entry is part of `sources_digest()`: no source of the others can change a kernel that a sampler step
# launches (the Euler step that the traffic profile describes never launches the stage kernel either; the metrics and the
# renderer produce and judge the data of a step and launch nothing inside one, and so do the conditioner's image tower,
# LPIPS, the loss, the adapters and the ParallelDomain colours).
LIBRARIES = {lib.name: lib for lib in (
    Library("gcd_amd", SOURCES, HEADERS, EXTRA_FLAGS),
    # kernels of the fine-tune step only
    Library("gcd_amd_train", ["train_wgrad.hip", "train_ops.hip", "train_det.hip", "train_optim.hip"],
            [INCLUDE / "gcd_amd_train.h", INCLUDE / "gcd_amd_train_det.h", INCLUDE / "gcd_amd_train_optim.h",
             CSRC / "train_wgrad_kernel.h", CSRC / "train_common.h"], {}),
    # the stage kernel of the sampler family
    Library("gcd_amd_sampler", ["sampler_stage.hip"], [INCLUDE / "gcd_amd_sampler.h"], {}),
    # the evaluation metrics on the device
    Library("gcd_amd_metrics", ["metrics.hip"], [INCLUDE / "gcd_amd_metrics.h"], {}),
    # point clouds to (source, target) frames
    Library("gcd_amd_render", ["render.hip"], [INCLUDE / "gcd_amd_render.h"], {}),
    # the CLIP ViT image tower's own kernels (gcd_amd/_lib_clip.py, gcd_amd/clip_vision.py)
    Library("gcd_amd_clip", ["clip_vision.hip"], [INCLUDE / "gcd_amd_clip.h"], {}),
    # the LPIPS metric's own kernels (gcd_amd/_lib_lpips.py, gcd_amd/lpips.py)
    Library("gcd_amd_lpips", ["lpips.hip"], [INCLUDE / "gcd_amd_lpips.h"], {}),
    # the fine-tune loss on the device (gcd_amd/_lib_loss.py, gcd_amd/loss_device.py)
    Library("gcd_amd_loss", ["loss.hip"], [INCLUDE / "gcd_amd_loss.h"], {}),
    # LoRA by merged weights: the merge and the projection of dW (gcd_amd/_lib_lora.py, gcd_amd/lora.py)
    Library("gcd_amd_lora", ["lora.hip"], [INCLUDE / "gcd_amd_lora.h"], {}),
    # the colours of a ParallelDomain point cloud: class colours and the modal blend (gcd_amd/_lib_pardom.py, gcd_amd/geometry.py)
    Library("gcd_amd_pardom", ["pardom.hip"], [INCLUDE / "gcd_amd_pardom.h"], {}),
)}
MAIN = LIBRARIES["gcd_amd"]
LIB = MAIN.so
STAMP = MAIN.stamp


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and Path(cand).exists():
            return cand
    raise RuntimeError("hipcc not found (looked at $HIPCC, PATH and /opt/rocm/bin/hipcc)")


def _digest(lib: Library = MAIN) -> str:
    h = hashlib.sha256()
    for p in [CSRC / s for s in lib.sources] + lib.headers:
        h.update(p.read_bytes())
    h.update(" ".join(FLAGS).encode())
    h.update(repr(sorted(lib.extra_flags.items())).encode())
    return h.hexdigest()      # (ABLATION_ONLY_SOURCES are not in the product library)


def sources_digest() -> str:
    """Content hash of everything that decides which kernels a sampler step launches and how: the
    HIP sources + headers + flags and the host-side engine.  tools/pmc_traffic.py stamps a PMC
    profile with it and bench.py quotes `roofline.traffic` only while it matches."""
    h = hashlib.sha256(_digest().encode())
    for f in ("engine.py", "ops.py", "sampling.py"):
        h.update((PKG / f).read_bytes())
    return h.hexdigest()[:16]


def _compile_and_link(sources, out: Path, objdir: Path, extra_flags, defines=(), save_temps: bool = False,
                      verbose: bool = True) -> Path:
    """hipcc over `sources` (at most MAX_JOBS at a time) into `objdir`, then one link into `out`."""
    hipcc = _hipcc()
    objdir.mkdir(parents=True, exist_ok=True)

    def run(cmd, what, **kw):
        if verbose:
            print("[gcd_amd.build]", " ".join(cmd), flush=True)
        if subprocess.call(cmd, **kw) != 0:
            raise RuntimeError(f"hipcc failed on {what}")

    def compile_one(src):
        obj = objdir / (src + ".o")
        temps = ["-save-temps=obj"] if save_temps else []
        run([hipcc, *temps, *FLAGS, *extra_flags.get(src, []), *defines, "-c", str(CSRC / src), "-o", str(obj)], src,
            cwd=str(objdir))
        return str(obj)

    with ThreadPoolExecutor(max_workers=MAX_JOBS) as pool:
        objs = list(pool.map(compile_one, sources))
    run([hipcc, "-shared", "-fPIC", f"--offload-arch={ARCH}", *objs, "-o", str(out)], out.name)
    return out


def build_library(lib: Library, force: bool = False, save_temps: bool = False, verbose: bool = True) -> Path:
    """Bring one library up to date: a no-op while its stamp holds the digest of its sources, headers and flags."""
    digest = _digest(lib)
    if not force and lib.so.exists() and lib.stamp.exists() and lib.stamp.read_text().strip() == digest:
        return lib.so
    _compile_and_link(lib.sources, lib.so, CSRC / "build", lib.extra_flags, save_temps=save_temps, verbose=verbose)
    lib.stamp.write_text(digest)
    return lib.so


def build(force: bool = False, save_temps: bool = False, verbose: bool = True,
          ablation: bool = False) -> Path:
    """ablation=True builds tools/libgcd_amd_ablate.so instead: the same sources with
    -DGCD_ABLATION_BUILD, which adds the wrong-by-design kernel variants tools/gemm_bench times
    (GCD_TUNE_GEMM_IMPL >= 32).  The product library never contains them."""
    if ablation:
        return _build_ablation(verbose)
    for lib in LIBRARIES.values():
        build_library(lib, force=force, save_temps=save_temps, verbose=verbose)
    return LIB


def _build_ablation(verbose: bool, name: str = "ablate", defines=("-DGCD_ABLATION_BUILD",)) -> Path:
    """A second library beside the product one (tools/libgcd_amd_<name>.so) from the same sources with extra defines:
    the ablation build, and the A/B variants of tools/ab_sweep.sh (loaded through GCD_AMD_LIB, see _lib.py)."""
    if "-DGCD_ABLATION_BUILD" not in defines:
        defines = tuple(defines) + ("-DGCD_ABLATION_BUILD",)      # every A/B library carries the ablation-only variants
    return _compile_and_link(SOURCES + ABLATION_ONLY_SOURCES, ROOT / "tools" / f"libgcd_amd_{name}.so", CSRC / "build" / name,
                             EXTRA_FLAGS, defines=defines, verbose=verbose)


if __name__ == "__main__":
    if "--ablation" in sys.argv:
        print(build(ablation=True))
    elif "--epi-wt" in sys.argv:      # write-through epilogue stores (gemm_common.h, GCD_EPI_WT): A/B library
        mask = int(sys.argv[sys.argv.index("--epi-wt") + 1])
        print(_build_ablation(True, f"wt{mask}", (f"-DGCD_EPI_WT={mask}",)))
    elif "--epi-nt" in sys.argv:      # non-temporal epilogue stores / residual loads (GCD_EPI_NT): A/B library
        mask = int(sys.argv[sys.argv.index("--epi-nt") + 1])
        print(_build_ablation(True, f"nt{mask}", (f"-DGCD_EPI_NT={mask}",)))
    else:
        build(force="--force" in sys.argv, save_temps="--save-temps" in sys.argv)
        print(LIB)
