#!/usr/bin/env python3
"""tests/golden/lpips_tiny.pt: the pins of the LPIPS metric (gcd_amd/lpips.py).  Data only: seeds, per-tensor checksums,
shapes and outputs — no weights.

The reference's `forward`, `ScalingLayer`, `vgg16` slicing, `NetLinLayer`, `normalize_tensor` and `spatial_average`
(sgm/modules/autoencoding/lpips/loss/lpips.py) are executed unmodified on the CPU.  Its file is loaded on its own, under
its package name, with two stand-ins in sys.modules so that nothing is fetched and nothing else of the package runs:

  * `torchvision`: `models.vgg16(pretrained=...)` ignores `pretrained` and returns an object whose `.features` is a plain
    nn.Sequential in VGG-16's layout (features[0:31]) at the requested widths;
  * `sgm.modules.autoencoding.lpips.util`: a `get_ckpt_path` that raises (the real module holds the download).

`LPIPS()` / `__init__` / `from_pretrained` / `load_from_pretrained` are never called (`__init__` ends in the download): the
object is made with `LPIPS.__new__` + `nn.Module.__init__`, the attributes `__init__` would assign, and `.eval()`.

Per case: the reference's fp32 output `y32`, its fp64 output `y64` (the same module after `.double()`), and `y16emu`, the
fp64 forward with the HIP path's storage points rounded to fp16 — the scaled input (a forward hook on the ScalingLayer),
the convolution weights, and every post-ReLU and post-pool activation (forward hooks).  The GPU test's bar is made of
`y16emu` against `y64`.

Usage: python tools/make_golden_lpips.py        (needs the reference tree that oracle/ref_shim.py points at)
"""
from __future__ import annotations

import importlib.util
import sys
import types
from pathlib import Path

import torch
import torch.nn as nn

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import lpips_util as U  # noqa: E402  (tests/lpips_util.py: the tests regenerate the same weights and images)
from oracle.ref_shim import REF  # noqa: E402

OUT = ROOT / "tests" / "golden" / "lpips_tiny.pt"
PKG = "sgm.modules.autoencoding.lpips"
CASES = {
    # name: (widths, H, W, pairs, weight seed, image seed)
    "tiny_40x56": (U.TINY, 40, 56, 3, 401, 501),        # pools 20x28, 10x14, 5x7, 2x3: the floors 5 -> 2 and 7 -> 3
    "tiny_37x51": (U.TINY, 37, 51, 2, 402, 502),        # odd sizes at the first pool
    "full_64x96": (U.FULL, 64, 96, 2, 403, 503),        # every channel count the kernels must handle
}
_widths = [None]


def _features(chns) -> nn.Sequential:
    layers, cin = [], 3
    for k, (convs, c) in enumerate(zip(U.SLICE_CONVS, chns)):
        if k > 0:
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        for _ in convs:
            layers += [nn.Conv2d(cin, c, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = c
    layers.append(nn.MaxPool2d(kernel_size=2, stride=2))        # features[30]: never reached by the slices
    return nn.Sequential(*layers)


def load_reference():
    """The reference's lpips.py as a module, with the two stand-ins in place."""
    tv, models = types.ModuleType("torchvision"), types.ModuleType("torchvision.models")
    models.vgg16 = lambda pretrained=False, **kw: types.SimpleNamespace(features=_features(_widths[0]))
    tv.models = models
    sys.modules.update({"torchvision": tv, "torchvision.models": models})
    name = ""
    for part in (PKG + ".loss").split("."):                     # bare packages: no __init__ of the reference runs
        name = part if not name else name + "." + part
        pkg = types.ModuleType(name)
        pkg.__path__ = []
        sys.modules[name] = pkg
    util = types.ModuleType(PKG + ".util")

    def get_ckpt_path(*a, **k):
        raise RuntimeError("the golden generator never loads a checkpoint")
    util.get_ckpt_path = get_ckpt_path
    sys.modules[PKG + ".util"] = util
    path = REF / "sgm" / "modules" / "autoencoding" / "lpips" / "loss" / "lpips.py"
    spec = importlib.util.spec_from_file_location(PKG + ".loss.lpips", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def build(ref, chns, sd):
    _widths[0] = chns
    m = ref.LPIPS.__new__(ref.LPIPS)
    nn.Module.__init__(m)
    m.scaling_layer = ref.ScalingLayer()
    m.chns = list(chns)
    m.net = ref.vgg16(pretrained=False, requires_grad=False)
    for k, c in enumerate(chns):
        setattr(m, f"lin{k}", ref.NetLinLayer(c, use_dropout=True))
    m.load_state_dict(sd, strict=True)
    return m.eval()


def emulate_fp16_storage(m):
    """In place, on a float64 module: fp16 convolution weights, fp16 after the ScalingLayer, every ReLU and every pool."""
    r16 = lambda mod, inp, out: out.half().to(out.dtype)
    m.scaling_layer.register_forward_hook(r16)
    for mod in m.net.modules():
        if isinstance(mod, nn.Conv2d):
            mod.weight.data = mod.weight.data.half().double()
        elif isinstance(mod, (nn.ReLU, nn.MaxPool2d)):
            mod.register_forward_hook(r16)
    return m


def main():
    ref = load_reference()
    gold = dict(cases={})
    for name, (chns, H, W, n, wseed, iseed) in CASES.items():
        sd = U.seeded_state_dict(chns, wseed)
        x0, x1 = U.seeded_images(n, H, W, iseed)
        with torch.no_grad():
            m = build(ref, chns, sd)
            names = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
            y32 = m(x0, x1)
            y64 = m.double()(x0.double(), x1.double())
            y16 = emulate_fp16_storage(build(ref, chns, sd).double())(x0.double(), x1.double())
        mine = U.lpips_oracle(sd, x0, x1)
        rel = lambda a: ((a.double() - y64).abs().reshape(-1)[1:] / y64.abs().reshape(-1)[1:]).max().item()
        print(f"{name}: y64 {y64.reshape(-1).tolist()}")
        print(f"  identical pair: y32 {y32.reshape(-1)[0].item()!r} y64 {y64.reshape(-1)[0].item()!r} y16emu {y16.reshape(-1)[0].item()!r}")
        print(f"  y32 vs y64 {rel(y32):.3e}, y16emu vs y64 {rel(y16):.3e}, restatement vs y64 {(mine - y64).abs().max().item():.3e}")
        assert names == [(k, tuple(s)) for k, s in U.state_shapes(chns).items()]
        gold["cases"][name] = dict(
            chns=list(chns), H=H, W=W, n=n, weight_seed=wseed, image_seed=iseed,
            checksums={k: U.checksum(v) for k, v in sd.items()}, image_checksums=[U.checksum(x0), U.checksum(x1)],
            names=[k for k, _ in names], shapes=[list(s) for _, s in names],
            y32=y32.clone(), y64=y64.clone(), y16emu=y16.clone(), y32_gap=rel(y32))
    torch.save(gold, OUT)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
