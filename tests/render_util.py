"""Shared by the renderer's tests (a helper module like memcontract.py, not a conftest): the golden file of
tools/make_golden_render.py and the bars of DESIGN.md 12.2 for one splat."""
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "render_tiny.pt"


def load_golden():
    return torch.load(GOLDEN, map_location="cpu", weights_only=False)


def check_splat(name, got, c):
    """The bars of DESIGN.md §12.2 for one case of the golden file; returns the measured figures."""
    img, pw, uv, depth = got
    want, wpw = c["img"], c["pixel_weights"]
    assert torch.equal(img == 0, want == 0), f"{name}: {(int(((img == 0) != (want == 0)).sum()))} pixels are zero on one side only"
    ulp = int((img.view(torch.int32) - want.view(torch.int32)).abs().max()) if img.numel() else 0
    assert torch.equal(pw < 0, wpw < 0), f"{name}: the -1 marks of pixel_weights differ"
    rel = float(((pw - wpw).abs() / wpw.abs()).max()) if pw.numel() else 0.0
    fig = dict(ulp=ulp, weights=rel)
    print(f"[{name}] img: {ulp} ulp; pixel_weights: {rel:.2e} relative", end="")
    assert ulp <= 1, f"{name}: img differs by {ulp} fp32 ulp"
    assert rel <= 1e-9, f"{name}: pixel_weights differ by {rel:.3e} relative"
    i = c["uvd_idx"]                               # every case records its sample of uv and depth
    assert uv[i].shape == c["uv"].shape and depth[i].shape == c["depth"].shape
    if bool((c["depth"] > 0.1).any()):
        front = c["depth"][:, 0] > 0.1
        # relative to the coordinate itself (the generator refuses a sampled |uv| below 1e-2 in front of the camera)
        e_uv = float(((uv[i] - c["uv"])[front].abs() / c["uv"][front].abs()).max())
        e_d = float(((depth[i] - c["depth"])[front].abs() / c["depth"][front].abs()).max())
        fig.update(uv=e_uv, depth=e_d)
        print(f"; uv: {e_uv:.2e}; depth: {e_d:.2e}", end="")
        assert e_uv <= 1e-12 and e_d <= 1e-12, f"{name}: uv {e_uv:.3e} / depth {e_d:.3e} relative"
    print()
    return fig


def golden_cloud(gold, c):
    xyz, rgb = gold["clouds"][c["cloud"]]
    return xyz, rgb


def float_colour_cloud():
    """Float colours the stored uint8 clouds cannot hold, two points per pixel 20 apart in exponent: a near point with a
    tiny colour under a farther bright one (the near one must not set the channel's scale), a colour above 1 (only the
    final image is clamped), and a far point that sets the normalisation.  Identity camera, 8 x 12 image."""
    K = torch.tensor([[10.0, 0.0, 6.0], [0.0, 10.0, 4.0], [0.0, 0.0, 1.0]])
    dz = 20.0 * 8.0 / 1024.0

    def at(px, py, d):
        return [(px + 0.2 - 6.0) / 10.0 * d, (py - 0.1 - 4.0) / 10.0 * d, d]
    xyz = torch.tensor([at(3, 2, 2.0), at(3, 2, 2.0 + dz), at(7, 5, 3.0), at(7, 5, 3.0 + dz), at(9, 6, 8.0)], dtype=torch.float64)
    rgb = torch.tensor([[1e-10, 2.0, 0.5], [1.0, 1e-30, 0.25], [3.0, 0.0, 1e-5], [0.5, 0.75, 4.0], [0.3, 0.3, 0.3]], dtype=torch.float64)
    return xyz, rgb, K, torch.eye(4), 8, 12


def direct_splat(xyz, rgb, K, RT, H, W, radius):
    """The reference's arithmetic restated with float64 sums, for clouds whose weights a float64 sum can hold."""
    x, c, K, RT = xyz.double(), rgb.double(), K.double(), RT.double()
    cam = (x - RT[0:3, 3]) @ RT[0:3, 0:3]
    p = cam @ K.T
    t = p[:, 0:2] / p[:, 2:3] + 0.5
    m = (t[:, 0] > -1) & (t[:, 0] < W) & (t[:, 1] > -1) & (t[:, 1] < H) & (cam[:, 2] > 0.1)
    px, py, d, c = t[m, 0].long(), t[m, 1].long(), cam[m, 2], c[m]
    assert d.max() < 64.0
    w = torch.exp(-(d / d.max() * 2.0 - 1.0) * 512.0)
    acc = torch.zeros(H * W, 4, dtype=torch.float64)
    val = torch.cat([w[:, None], c * w[:, None]], dim=1)
    left, right = radius // 2, (radius + 1) // 2
    for dy in range(-left, right + 1):
        for dx in range(-left, right + 1):
            ok = (px + dx >= 0) & (px + dx < W) & (py + dy >= 0) & (py + dy < H)
            acc.index_add_(0, ((py + dy) * W + px + dx)[ok], val[ok] * (1.0 if dx == 0 and dy == 0 else 0.02))
    den = torch.where(acc[:, 0:1] > 0, acc[:, 0:1], torch.tensor(-1.0, dtype=torch.float64))
    return ((acc[:, 1:4] / den).clamp(0.0, 1.0) + 0.0).float().reshape(H, W, 3), den.reshape(H, W, 1)      # + 0.0: no -0


def check_float_colours(img, pw, radius):
    xyz, rgb, K, RT, H, W = float_colour_cloud()
    want, wpw = direct_splat(xyz, rgb, K, RT, H, W, radius)
    assert torch.equal(img == 0, want == 0) and torch.equal(pw < 0, wpw < 0)
    ulp = int((img.view(torch.int32) - want.view(torch.int32)).abs().max())
    rel = float(((pw - wpw).abs() / wpw.abs()).max())
    print(f"[float colours, radius {radius}] img: {ulp} ulp; pixel_weights: {rel:.2e} relative; pixel (3, 2): {img[2, 3].tolist()}")
    assert ulp <= 1 and rel <= 1e-9
    assert 0.0 < float(img[2, 3, 0]) < 1e-8 and float(img[2, 3, 1]) == 1.0 and float(img[5, 7, 0]) == 1.0
