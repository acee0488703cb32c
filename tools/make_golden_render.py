#!/usr/bin/env python3
"""tests/golden/render_tiny.pt: what the reference's renderer computes on tiny clouds (data only).

Stage 1: the *unmodified* `sgm/data/geometry.py` of the reference is imported at run time, with the modules it imports
and this machine lacks replaced by empty stand-ins, and `project_points_to_pixels` is run on the CPU per case.  The image
and the weights are recorded whole; uv and depth, for every case, at the first 64 points (where the special points sit) and at 448 more
drawn at random: the whole (N, 2) arrays of every case would pass the size limit of a committed file.

Stage 2: `blur_into_black` calls torchvision, which is not installed, so it cannot run unmodified.  This file carries a
torch restatement of torchvision's documented `gaussian_blur` (kernel from linspace / exp / normalise, the outer
product, reflect padding, a grouped convolution) and records the fill + resize + (* 2 - 1) chain twice: with the
reference's dtypes (the image blurred in float32, the mask in float64, promotion as torch does it) and in float64
throughout, and the largest gap between the two.  Stage 2 is therefore pinned to a restatement, not to executed
reference code.

The generator refuses to write a file when a fixture sits on an edge where a device that contracts multiply-adds could
legitimately land on the other side: uv + 0.5 within 1e-9 of an integer, a depth within 1e-9 of 0.1, a depth maximum
within 1e-9 of 64, a non-zero image value below 1e-40.

Usage: python tools/make_golden_render.py [--reference DIR]      (DIR: the reference's gcd-model directory)
"""
from __future__ import annotations

import argparse
import importlib
import importlib.util
import sys
import types
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "golden" / "render_tiny.pt"
STUBS = ("cv2", "lovely_tensors", "lovely_numpy", "mediapy", "pyquaternion", "torchvision", "torchvision.transforms")
FRAME_HW = (16, 24)
UVD_HEAD, UVD_RANDOM = 64, 448


def load_reference_geometry(ref_dir: Path):
    for name in STUBS:
        try:
            importlib.import_module(name)
        except Exception:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["lovely_tensors"].__dict__.setdefault("monkey_patch", lambda: None)
    sys.modules["lovely_numpy"].__dict__.setdefault("lo", None)
    sys.modules["pyquaternion"].__dict__.setdefault("Quaternion", None)
    if not hasattr(sys.modules["torchvision"], "transforms"):
        sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    opts = np.get_printoptions()
    spec = importlib.util.spec_from_file_location("reference_geometry", ref_dir / "sgm" / "data" / "geometry.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    np.set_printoptions(**opts)
    torch.set_printoptions(profile="default")
    return m


# ---- stage 2: the restatement ------------------------------------------------------------------------------------------

def gaussian_blur(img: torch.Tensor, k: int, sigma: float) -> torch.Tensor:
    """torchvision.transforms.functional.gaussian_blur on a (C, H, W) float tensor, in the tensor's dtype."""
    half = (k - 1) * 0.5
    x = torch.linspace(-half, half, steps=k, dtype=img.dtype)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    k1 = pdf / pdf.sum()
    k2 = torch.mm(k1[:, None], k1[None, :]).expand(img.shape[0], 1, k, k)
    padded = F.pad(img[None], [k // 2] * 4, mode="reflect")
    return F.conv2d(padded, k2, groups=img.shape[0])[0]


def fill_chain(img: torch.Tensor, k: int, sigma: float, frame_hw, all_f64: bool):
    """(H, W, 3) float32 -> (blurred (H, W, 3), frames (3, Hp, Wp) in [-1, 1]): blur_into_black, the resize and the map."""
    black = (img.sum(dim=-1) == 0.0)[None]
    chw = img.permute(2, 0, 1)
    if all_f64:
        chw = chw.double()
    borrow = (~black).type(torch.float64)
    blur_img = gaussian_blur(chw, k, sigma)
    blur_mask = gaussian_blur(borrow, k, sigma).clamp(min=1e-7)
    leak = blur_img / blur_mask
    filled = chw * (~black) + leak * black
    smooth = gaussian_blur(filled, 3, 0.6)
    frames = F.interpolate(smooth[None], frame_hw, mode="bilinear", align_corners=False)[0] * 2.0 - 1.0
    return smooth.permute(1, 2, 0).contiguous(), frames.contiguous()


# ---- stage 1: fixtures -------------------------------------------------------------------------------------------------

def intrinsics(H, W):
    return torch.tensor([[0.8 * W, 0.0, 0.5 * W - 0.3], [0.0, 0.8 * W, 0.5 * H + 0.2], [0.0, 0.0, 1.0]], dtype=torch.float32)


def scene_cloud(geo, g, n, H, W, RT, special=True, far=False, past_int32=False):
    """A cloud built in camera space and moved to the world: a dense part, a thin part that leaves isolated holes, a
    band more than 10 pixels wide that nothing reaches; every seventh point black; then the special points in front."""
    K = intrinsics(H, W).double().numpy()
    u = torch.rand(n, generator=g, dtype=torch.float64) * (W + 6) - 3
    v = torch.rand(n, generator=g, dtype=torch.float64) * (H + 4) - 2
    thin = torch.rand(n, generator=g) < 0.55
    v = torch.where((v < 0.4 * H) & thin, v + 0.45 * H, v)           # few points in the top rows: isolated holes
    band = (u > 0.30 * W) & (u < 0.30 * W + 13.5)
    u = torch.where(band, u + 14.0, u)                               # the band: a hole wider than 10 pixels
    u = torch.where(u.abs() < 0.02, u + 0.05, u)                     # no coordinate next to 0: the uv bar is relative
    v = torch.where(v.abs() < 0.02, v + 0.05, v)
    # depth layers half a unit apart with a little jitter: between two layers the weights differ by e^-64 (kept by
    # float32) or by e^-128 and less (an exact zero), never by the e^-92 .. e^-106 that would land among the denormals
    z = 1.5 + 0.5 * torch.randint(0, 14, (n,), generator=g).double() + 0.04 * torch.rand(n, generator=g, dtype=torch.float64)
    z[8] = 8.0
    if far:
        # depths of 64 .. 1600 for the sqrt branch: layers 4 apart in sqrt(depth) are e^-64 apart again once the point at
        # 1600 is clamped to 32 and sets the maximum
        z = (8.0 + 4.0 * torch.randint(0, 7, (n,), generator=g).double() + 0.05 * torch.rand(n, generator=g, dtype=torch.float64)) ** 2
        z[8] = 1600.0
    zs = 64.0 if far else 2.0
    x = (u - K[0, 2]) / K[0, 0] * z
    y = (v - K[1, 2]) / K[1, 1] * z
    cam = torch.stack([x, y, z], dim=1)
    if special:
        cam[0] = torch.tensor([0.2, 0.1, -3.0])                      # behind the camera
        cam[1] = torch.tensor([0.0, 0.0, 0.05])                      # in front of it, nearer than 0.1
        cam[2] = torch.tensor([40.0 * zs, 0.0, zs])                      # outside the image, right
        cam[3] = torch.tensor([0.0, -30.0 * zs, zs])                     # outside the image, above
    if past_int32:
        # only with an axis-aligned camera: behind a rotation, coordinates of 3e9 cancel down to a depth of 0.2 with an
        # absolute error of 3e9 * 2^-53, which no two orders of summation share to 1e-12 of the depth
        cam[4] = torch.tensor([3.0e9, 0.0, 0.2])                     # u past int32
        cam[5] = torch.tensor([0.0, -3.0e9, 0.2])                    # v past int32 (negative)
        cam[6] = torch.tensor([(-0.7 - K[0, 2]) / K[0, 0] * zs, 0.0, zs])      # u = -0.7: truncation puts it in column 0
    world = torch.from_numpy(geo.camera_to_world(cam.numpy(), RT.double().numpy()))
    rgb = torch.rand(n, 3, generator=g, dtype=torch.float64)
    rgb[::7] = 0.0
    return world, rgb


def occluder_cloud(background_depth: float, H, W):
    """Identity camera.  A black occluder at depth 2.0 over columns 8 .. 15, a coloured background over columns 16 .. 27, one
    far point at depth 8 that sets the normalisation.  Column 15 takes the background's 0.02 neighbour weight."""
    K = intrinsics(H, W).double()
    pts, cols = [], []
    for py in range(4, H - 4):
        for px in range(8, 28):
            d = 2.0 if px < 16 else background_depth
            pts.append([(px + 0.13 - K[0, 2]) / K[0, 0] * d, (py - 0.21 - K[1, 2]) / K[1, 1] * d, d])
            cols.append([0.0, 0.0, 0.0] if px < 16 else [0.9, 0.5, 0.25])
    pts.append([0.0, 0.0, 8.0])
    cols.append([0.3, 0.3, 0.3])
    return torch.tensor(pts, dtype=torch.float64), torch.tensor(cols, dtype=torch.float64)


def run_reference(geo, xyz, rgb, K, RT, H, W, radius):
    """As the dataset does it: xyz to float32, uint8 colours / 255.0 in float32, concatenated, float64."""
    x32 = xyz.type(torch.float32) if xyz.dtype == torch.float16 else xyz
    c = (rgb / 255.0).type(torch.float32) if rgb.dtype == torch.uint8 else rgb
    dt = torch.promote_types(x32.dtype, c.dtype)
    xyzrgb = torch.cat([x32.to(dt), c.to(dt)], dim=-1)
    return geo.project_points_to_pixels(xyzrgb, K, RT, H, W, spread_radius=radius)


def edge_checks(name, img, uv, depth, H, W):
    ok = torch.isfinite(uv).all(dim=1) & (uv.abs().max(dim=1).values < 1e6)
    t = uv[ok] + 0.5
    gap = (t - t.round()).abs().min().item() if t.numel() else 1.0
    assert gap > 1e-9, f"{name}: a uv + 0.5 within {gap:.1e} of an integer"
    assert ((depth - 0.1).abs() > 1e-9).all(), f"{name}: a depth within 1e-9 of 0.1"
    uvi = (uv + 0.5)
    mask = (uvi[:, 0] > -1) & (uvi[:, 0] < W) & (uvi[:, 1] > -1) & (uvi[:, 1] < H) & (depth[:, 0] > 0.1)
    if mask.any():
        assert abs(depth[mask].max().item() - 64.0) > 1e-9, f"{name}: the depth maximum within 1e-9 of 64"
    tiny = (img > 0) & (img < 1e-40)
    assert not tiny.any(), f"{name}: {int(tiny.sum())} non-zero image values below 1e-40"
    return int(mask.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None)
    args = ap.parse_args()
    if args.reference is None:
        sys.path.insert(0, str(ROOT))
        from oracle.ref_shim import REF
        args.reference = REF
    geo = load_reference_geometry(Path(args.reference))
    g = torch.Generator().manual_seed(20241)
    RT_a = torch.tensor(geo.extrinsics_from_look_at(np.array([0.4, -5.0, 1.1]), np.array([0.1, 0.0, 0.2])), dtype=torch.float32)
    # the second camera: rolled about the first one's optical axis and moved sideways, which keeps every depth (and with
    # it the depth layers of scene_cloud)
    roll = np.eye(4)
    roll[0:2, 0:2] = [[np.cos(0.35), -np.sin(0.35)], [np.sin(0.35), np.cos(0.35)]]
    roll[0:3, 3] = [0.3, -0.2, 0.0]
    RT_b = torch.tensor(RT_a.double().numpy() @ roll, dtype=torch.float32)
    eye = torch.eye(4, dtype=torch.float32)

    clouds, cases = {}, []

    def add(name, cloud, K, RT, H, W, radius, raises=False):
        xyz, rgb = clouds[cloud]
        n = xyz.shape[0]
        if raises:
            # the reference's .max() raises on an empty masked set: the expected image and weights are the documented ones;
            # uv and depth restate the function's first lines
            try:
                run_reference(geo, xyz, rgb, K, RT, H, W, radius)
                raise AssertionError(f"{name}: the reference was expected to raise")
            except RuntimeError:
                pass
            img, pw = torch.zeros(H, W, 3), -torch.ones(H, W, 1, dtype=torch.float64)
            cam = geo.world_to_camera(xyz.double(), RT.double())
            p = torch.mm(K.double(), cam.T).T
            uv, depth = p[:, 0:2] / p[:, 2:3], cam[:, 2:3]
            visible = 0
        else:
            img, pw, uv, depth = run_reference(geo, xyz, rgb, K, RT, H, W, radius)
            visible = edge_checks(name, img, uv, depth, H, W)
        gen = torch.Generator().manual_seed(len(cases))
        idx = torch.cat([torch.arange(min(UVD_HEAD, n)), UVD_HEAD + torch.randperm(max(n - UVD_HEAD, 0), generator=gen)[:UVD_RANDOM]])
        c = dict(name=name, cloud=cloud, K=K, RT=RT, H=H, W=W, radius=radius, raises=raises, visible=visible,
                 img=img.contiguous(), pixel_weights=pw.contiguous(), uvd_idx=idx, uv=uv[idx].contiguous(),
                 depth=depth[idx].contiguous())
        # the uv bar is relative to the coordinate itself: a sampled coordinate next to 0 would measure the absolute rounding
        # error of its image-sized terms (a few 1e-15) against nothing
        front = c["depth"][:, 0] > 0.1
        if front.any():
            small = c["uv"][front].abs().min().item()
            assert small >= 1e-2, f"{name}: a sampled uv of {small:.2e} in front of the camera; the relative bar needs |uv| >= 1e-2"
        cases.append(c)
        print(f"{name:14s} N={n:5d} visible={visible:5d} covered={int((pw > 0).sum()):4d}/{H * W} img max {img.max().item():.3f}")
        return c

    H, W = 24, 40
    K = intrinsics(H, W)
    xyz, rgb = scene_cloud(geo, g, 3000, H, W, RT_a)
    clouds["base_f32"] = (xyz.float(), rgb.float())
    r = {rad: add(f"base_r{rad}", "base_f32", K, RT_a, H, W, rad) for rad in (1, 2, 3)}
    add("base_r2_cam_b", "base_f32", K, RT_b, H, W, 2)
    covered = r[1]["pixel_weights"][..., 0] > 0
    assert covered.any() and (~covered).any(), "covered and uncovered pixels must both exist"
    pad = F.pad(covered[None, None].float(), [1, 1, 1, 1], value=1.0)[0, 0]
    isolated = (~covered) & (pad[:-2, 1:-1] > 0) & (pad[2:, 1:-1] > 0) & (pad[1:-1, :-2] > 0) & (pad[1:-1, 2:] > 0)
    run = max(len(s) for row in (~covered).int().tolist() for s in "".join(map(str, row)).split("0"))
    assert isolated.any() and run > 10, f"isolated holes: {int(isolated.sum())}, widest hole {run}"
    print(f"base_r1: {int(isolated.sum())} isolated holes, widest hole {run} pixels")

    xyz, rgb = scene_cloud(geo, g, 2000, H, W, RT_a, far=True)
    clouds["far_f32"] = (xyz.float(), (rgb * 255.0).round().to(torch.uint8))
    add("far", "far_f32", K, RT_a, H, W, 2)
    assert cases[-1]["depth"].max() > 1024.0

    shift = torch.eye(4, dtype=torch.float32)
    shift[0:3, 3] = torch.tensor([0.25, -0.5, -1.0])
    xyz, rgb = scene_cloud(geo, g, 600, H, W, shift, past_int32=True)
    clouds["past_int32"] = (xyz.float(), rgb.float())
    c = add("past_int32", "past_int32", K, shift, H, W, 2)
    assert c["uv"][4, 0] > 2.0 ** 31 and c["uv"][5, 1] < -2.0 ** 31 and (c["depth"][4:6] > 0.1).all()

    H2, W2 = 23, 37
    xyz, rgb = scene_cloud(geo, g, 2000, H2, W2, RT_b)
    clouds["ragged_f64"] = (xyz, rgb.float())           # float64 positions, float32 colours
    add("ragged_f64", "ragged_f64", intrinsics(H2, W2), RT_b, H2, W2, 2)

    xyz, rgb = scene_cloud(geo, g, 4000, H, W, RT_a, special=False)
    xyz16 = xyz.half()
    xyz16[0] = torch.tensor([0.4, -9.0, 1.1]).half()                 # behind the camera
    clouds["f16_u8"] = (xyz16, (rgb * 255.0).round().to(torch.uint8))
    add("f16_u8", "f16_u8", K, RT_a, H, W, 2)

    # 4 096 points into pixel (17, 9) at depths 2 .. 2.02, and a hundred others
    Kd = K.double()
    n1 = 4096
    du = torch.rand(n1, generator=g, dtype=torch.float64) * 0.8 - 0.4
    dv = torch.rand(n1, generator=g, dtype=torch.float64) * 0.8 - 0.4
    z = 2.0 + 0.02 * torch.rand(n1, generator=g, dtype=torch.float64)
    one = torch.stack([(17.0 + du - Kd[0, 2]) / Kd[0, 0] * z, (9.0 + dv - Kd[1, 2]) / Kd[1, 1] * z, z], dim=1)
    more, more_rgb = scene_cloud(geo, g, 104, H, W, eye, special=False)
    clouds["one_pixel"] = (torch.cat([one, more]).float(),
                           (torch.cat([torch.rand(n1, 3, generator=g, dtype=torch.float64), more_rgb]) * 255.0).round().to(torch.uint8))
    c = add("one_pixel", "one_pixel", K, eye, H, W, 1)

    clouds["empty"] = (torch.zeros(0, 3), torch.zeros(0, 3))
    add("n0", "empty", K, RT_a, H, W, 2, raises=True)
    behind = clouds["base_f32"][0][16:316].clone()         # past the special points
    behind = torch.from_numpy(geo.camera_to_world(
        (geo.world_to_camera(behind.double().numpy(), RT_a.double().numpy()) * np.array([1.0, 1.0, -1.0])), RT_a.double().numpy())).float()
    clouds["behind"] = (behind, clouds["base_f32"][1][16:316].clone())
    add("none_visible", "behind", K, RT_a, H, W, 2, raises=True)

    for tag, d in (("occluder_near", 2.5), ("occluder_far", 3.0)):
        clouds[tag] = occluder_cloud(d, H, W)
        c = add(tag, tag, K, eye, H, W, 2)
        col = c["img"][6:H - 6, 15, 0]
        print(f"{tag}: border column 15, red: min {col.min().item():.3e} max {col.max().item():.3e}")
        if d == 2.5:
            assert (col > 0).all() and (col < 1e-25).all(), "the border column must be tiny and not black"
        else:
            assert (col == 0).all(), "the border column must be exactly black"

    # ---- stage 2 -------------------------------------------------------------------------------------------------------
    fills = []
    by_name = {c["name"]: c for c in cases}
    for src in ("base_r1", "ragged_f64", "occluder_near"):
        img = by_name[src]["img"]
        assert ((img.sum(dim=-1) == 0).any() and (img.sum(dim=-1) != 0).any())
        # the two settings of the views and of the re-projection baseline; blur_into_black's own defaults once, unresized
        for k, sigma in ((21, 5.25), (3, 0.75)) + (((5, 1.5),) if src == "base_r1" else ()):
            b32, f32_ = fill_chain(img, k, sigma, FRAME_HW, all_f64=False)
            b64, f64_ = fill_chain(img, k, sigma, FRAME_HW, all_f64=True)
            gap_f, gap_b = (f32_.double() - f64_).abs().max().item(), (b32.double() - b64).abs().max().item()
            f = dict(src=src, k=k, sigma=sigma, frame_hw=FRAME_HW, gap_frames=gap_f, gap_blur=gap_b)
            f.update(dict(blur_ref=b32, blur_f64=b64) if k == 5 else dict(frames_ref=f32_, frames_f64=f64_))
            fills.append(f)
            print(f"fill {src:14s} k={k:2d}: dtype gap frames {gap_f:.3e} blur {gap_b:.3e} ({f32_.dtype})")

    torch.save(dict(clouds=clouds, cases=cases, fills=fills, frame_hw=FRAME_HW), OUT)
    print(f"{OUT.relative_to(ROOT)}: {OUT.stat().st_size} bytes")
    assert OUT.stat().st_size < 1024 * 1024


if __name__ == "__main__":
    main()
