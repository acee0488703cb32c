"""Shared by the LPIPS tests and tools/make_golden_lpips.py (a helper module like clip_util.py, not a conftest): a torch
restatement of the metric as the oracle (any dtype, CPU), the seeded weights and images, and the golden file.

The restatement is pinned to the executed reference by tests/golden/lpips_tiny.pt (test_lpips_host.py): it equals the
reference's float64 output to 1e-12.  `round16=True` rounds the HIP path's storage points to fp16 (the scaled input, the
convolution weights, every post-ReLU and post-pool activation) inside an otherwise float64 forward: what is left between
that and the GPU is the fp32 accumulation."""
from __future__ import annotations

import math
from collections import OrderedDict
from pathlib import Path

import torch
import torch.nn.functional as F

GOLDEN = Path(__file__).resolve().parent / "golden" / "lpips_tiny.pt"
SLICE_CONVS = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))      # torchvision vgg16().features indices
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
TINY = (32, 32, 64, 64, 64)
FULL = (64, 128, 256, 512, 512)
_CACHE = {}


def state_shapes(chns) -> "OrderedDict[str, tuple]":
    """The 33 names of the reference's state dict, in its order, with their shapes at the widths `chns`."""
    shapes = OrderedDict([("scaling_layer.shift", (1, 3, 1, 1)), ("scaling_layer.scale", (1, 3, 1, 1))])
    cin = 3
    for k, (convs, c) in enumerate(zip(SLICE_CONVS, chns)):
        for i in convs:
            shapes[f"net.slice{k + 1}.{i}.weight"] = (c, cin, 3, 3)
            shapes[f"net.slice{k + 1}.{i}.bias"] = (c,)
            cin = c
    for k, c in enumerate(chns):
        shapes[f"lin{k}.model.1.weight"] = (1, c, 1, 1)
    return shapes


def seeded_state_dict(chns, seed: int) -> "OrderedDict[str, torch.Tensor]":
    """Seeded weights (no checkpoint ships with the project): one torch.Generator walks the names in order.  Kaiming-normal
    convolutions (std sqrt(2 / fan_in): activations keep their scale through 13 ReLU layers), biases uniform in
    [-0.05, 0.05], lin weights uniform in [0, 2 / C] (the real ones are non-negative), the reference's shift / scale."""
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    for name, shape in state_shapes(chns).items():
        if name.startswith("scaling_layer."):
            t = torch.tensor(SHIFT if name.endswith("shift") else SCALE).view(shape)
        elif name.startswith("lin"):
            t = torch.rand(shape, generator=g) * (2.0 / shape[1])
        elif name.endswith("weight"):
            t = torch.randn(shape, generator=g) * math.sqrt(2.0 / (shape[1] * 9))
        else:
            t = (torch.rand(shape, generator=g) - 0.5) * 0.1
        sd[name] = t
    return sd


def seeded_images(n: int, H: int, W: int, seed: int):
    """(input, target): fp32 [n, 3, H, W] in [-1, 1].  The input is smooth low-resolution noise plus white noise, the
    target the input plus a perturbation.  Pair 0 is identical; the last pair has a constant left half in both images."""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(n, 3, max(H // 8, 2), max(W // 8, 2), generator=g) * 2 - 1
    smooth = F.interpolate(low, size=(H, W), mode="bilinear", align_corners=False)
    x0 = (0.7 * smooth + 0.3 * (torch.rand(n, 3, H, W, generator=g) * 2 - 1)).clamp(-1, 1).float()
    x1 = (x0 + 0.25 * torch.randn(n, 3, H, W, generator=g)).clamp(-1, 1).float()
    x1[0] = x0[0]
    x0[-1, :, :, :W // 2] = -1.0
    x1[-1, :, :, :W // 2] = -1.0
    return x0.contiguous(), x1.contiguous()


def checksum(t: torch.Tensor):
    return float(t.double().sum()), float(t.double().abs().sum())


def close(a, b, rel=1e-9) -> bool:
    return all(abs(x - y) <= rel * max(abs(y), 1.0) for x, y in zip(a, b))


def _r16(t: torch.Tensor) -> torch.Tensor:
    return t.half().to(t.dtype)


def features(sd, x: torch.Tensor, round16: bool = False):
    """The five taps of one batch of images in [-1, 1], in x's dtype."""
    dt = x.dtype
    if round16:     # the GPU evaluates the ScalingLayer in fp32 and rounds once to fp16
        h = ((x.float() - sd["scaling_layer.shift"].float()) / sd["scaling_layer.scale"].float()).half().to(dt)
    else:
        h = (x - sd["scaling_layer.shift"].to(dt)) / sd["scaling_layer.scale"].to(dt)
    taps = []
    for k, convs in enumerate(SLICE_CONVS):
        if k > 0:
            h = F.max_pool2d(h, kernel_size=2, stride=2)
        for i in convs:
            w = sd[f"net.slice{k + 1}.{i}.weight"].to(dt)
            h = F.relu(F.conv2d(h, _r16(w) if round16 else w, sd[f"net.slice{k + 1}.{i}.bias"].to(dt), padding=1))
            if round16:
                h = _r16(h)
        taps.append(h)
    return taps


def head(sd, taps0, taps1) -> torch.Tensor:
    """[n, 1, 1, 1]: sum over the taps of the spatial mean of the lin-weighted squared difference of the unit rows."""
    val = 0
    for k, (f0, f1) in enumerate(zip(taps0, taps1)):
        n0 = f0 / (torch.sqrt(torch.sum(f0 ** 2, dim=1, keepdim=True)) + 1e-10)
        n1 = f1 / (torch.sqrt(torch.sum(f1 ** 2, dim=1, keepdim=True)) + 1e-10)
        w = sd[f"lin{k}.model.1.weight"].to(f0.dtype)
        val = val + F.conv2d((n0 - n1) ** 2, w).mean([2, 3], keepdim=True)
    return val


def lpips_oracle(sd, x0: torch.Tensor, x1: torch.Tensor, dtype=torch.float64, round16: bool = False) -> torch.Tensor:
    """The metric of (input, target) in [-1, 1] on the CPU in `dtype`."""
    with torch.no_grad():
        return head(sd, features(sd, x0.to(dtype), round16), features(sd, x1.to(dtype), round16))


# gcd_lpips_distance against float64 on the same fp16 features, relative error of a tap mean: what fp32 accumulation
# leaves (sums of squares of C terms per row, the products, the sum over a workgroup's pixels).  Measured on the MI355X
# over the cases of test_lpips_gpu.py / test_memcontract_lpips_gpu.py: 2.7e-8 .. 1.03e-7 (the largest at C = 64, 203
# pixels, 3 workgroups per image), i.e. within two ulp of fp32; the bar is 4 x the largest.
DISTANCE_MEASURED = 1.03e-7
DISTANCE_BAR = 4.0 * DISTANCE_MEASURED


def seeded_features(n: int, HW: int, C: int, seed: int):
    """(f0, f1, w): post-ReLU-like fp16 features [n HW, C] (half of the entries zero) and non-negative lin weights [C]."""
    g = torch.Generator().manual_seed(seed)
    f0 = torch.relu(torch.randn(n * HW, C, generator=g)).half()
    f1 = torch.relu(f0.float() + 0.5 * torch.randn(n * HW, C, generator=g)).half()
    return f0, f1, (torch.rand(C, generator=g) * (2.0 / C)).float()


def distance_ref(f0: torch.Tensor, f1: torch.Tensor, w: torch.Tensor, n: int, HW: int) -> torch.Tensor:
    """float64 [n]: the mean over an image's pixels of sum_c (f0 / (|f0| + 1e-10) - f1 / (|f1| + 1e-10))^2 w."""
    a, b = f0.double().reshape(n, HW, -1), f1.double().reshape(n, HW, -1)
    na = a / (a.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    nb = b / (b.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    return ((na - nb).pow(2) * w.double()).sum(-1).mean(-1)


def load_golden() -> dict:
    if "gold" not in _CACHE:
        _CACHE["gold"] = torch.load(GOLDEN, map_location="cpu", weights_only=True)
    return _CACHE["gold"]


def golden_case(name: str):
    """(record, state dict, input, target) of a golden case: weights and images regenerated from the recorded seeds, once
    per process, and held to the recorded checksums (a torch whose generator drifted must not pass for a kernel error)."""
    if name not in _CACHE:
        rec = load_golden()["cases"][name]
        sd = seeded_state_dict(rec["chns"], rec["weight_seed"])
        assert list(sd) == list(rec["checksums"])
        for k, v in sd.items():
            assert close(checksum(v), rec["checksums"][k]), f"{name}: regenerated {k} does not match the recorded checksum"
        x0, x1 = seeded_images(rec["n"], rec["H"], rec["W"], rec["image_seed"])
        assert close(checksum(x0), rec["image_checksums"][0]) and close(checksum(x1), rec["image_checksums"][1]), \
            f"{name}: regenerated images do not match the recorded checksums"
        _CACHE[name] = (rec, sd, x0, x1)
    return _CACHE[name]


def case_bar(rec) -> float:
    """4 x the golden's recorded max |y16emu - y64| / |y64| over the case's non-identical pairs: the fp16 storage points of
    the HIP path, from the reference-side emulation; the factor covers fp32-versus-fp64 accumulation order."""
    y64, y16 = rec["y64"].double().reshape(-1), rec["y16emu"].double().reshape(-1)
    live = y64 != 0
    return 4.0 * float(((y16 - y64).abs()[live] / y64.abs()[live]).max())


def gpu_model(chns, sd, device):
    from gcd_amd.lpips import LPIPS
    m = LPIPS(chns=tuple(chns))
    m.load_state_dict(sd, strict=True)
    return m.to(device)
