"""CPU: the C ABI of libgcd_amd_render.so (include/gcd_amd_render.h) — header, binding table and exported symbols are one
set and the library builds from a tree that holds no build product (tests/test_libraries_host.py); every entry validates its arguments
before any launch; the scratch sizes are what the header says; the host module refuses what is not a GPU tensor; and the
accumulation scheme of the splat (four reference exponents per pixel, l for the denominator and l + ln c per channel, integer maxima, fixed-point integer sums), restated
here with integer tensors, reproduces the reference's images of tests/golden/render_tiny.pt at the bars of DESIGN.md §12.2.
The last one keeps the scheme itself pinned where no GPU is present."""
import ctypes as C
import math
import re
from pathlib import Path

import pytest
import torch

from render_util import GOLDEN, check_float_colours, check_splat, float_colour_cloud, golden_cloud, load_golden

ROOT = Path(__file__).resolve().parent.parent
DECL = r"^\s*(?:int|int64_t|const char\*)\s+(gcd_\w+)\s*\("


def test_render_header_binding_table_and_exports_are_one_set():
    from gcd_amd import _lib
    from gcd_amd.csrc import build as b
    header = (ROOT / "include" / "gcd_amd_render.h").read_text()
    declared = set(re.findall(DECL, header, flags=re.M))      # == table == exports: tests/test_libraries_host.py
    assert {"gcd_render_abi_version", "gcd_render_last_error", "gcd_render_scratch_bytes", "gcd_render_splat",
            "gcd_render_fill_resize_f32"} <= declared
    for name in ("F16", "F32", "F64", "U8", "MAX_CAMERAS", "CAM_DOUBLES", "MAX_KERNEL"):
        assert int(re.search(rf"#define GCD_RENDER_{name} (\d+)", header).group(1)) == getattr(_lib, "RENDER_" + name), name
    # the descriptor of the binding has the header's fields, in the header's order
    body = re.search(r"typedef struct gcd_render_splat_desc \{(.*?)\} gcd_render_splat_desc;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].replace(
        "void*", "").replace("double*", "").replace("float*", "").replace("int64_t*", "").split(",")]
    assert fields == [f[0] for f in _lib.RenderSplatDesc._fields_], fields
    # a library of its own (its symbols, sources and headers are apart from the others': tests/test_libraries_host.py)
    assert "gcd_render" not in (ROOT / "include" / "gcd_amd.h").read_text()
    assert b.LIBRARIES["gcd_amd_render"].sources == ["render.hip"] and "render.hip" not in b.SOURCES


def test_render_entries_validate_their_arguments_before_any_launch():
    from gcd_amd import _lib
    lib = _lib.load_render()
    P = 4096                                   # a stand-in for a device pointer: never dereferenced, nothing is launched
    nc, H, W, N = 2, 23, 37, 100
    need = lib.gcd_render_scratch_bytes(nc, H, W)
    need_f = lib.gcd_render_fill_scratch_bytes(H, W)
    # the header's formulas: per camera a 16-byte header and 64 bytes per pixel; three fp64 planes
    assert need == nc * (16 + H * W * 64) and need_f == 3 * H * W * 8
    assert lib.gcd_render_scratch_bytes(1, 384, 576) == 16 + 384 * 576 * 64
    assert lib.gcd_render_scratch_bytes(0, H, W) == 0 and b"cameras" in lib.gcd_render_last_error()
    assert lib.gcd_render_scratch_bytes(9, H, W) == 0 and lib.gcd_render_scratch_bytes(1, 0, W) == 0
    assert lib.gcd_render_fill_scratch_bytes(H, -1) == 0 and b"pixels a side" in lib.gcd_render_last_error()

    def splat(**kw):
        f = dict(xyz=P, rgb=P, xyz_ld=3, rgb_ld=3, N=N, xyz_dtype=_lib.RENDER_F16, rgb_dtype=_lib.RENDER_U8, cams=P, nc=nc, H=H, W=W,
                 spread_radius=2, img=P, img_cs=H * W * 3, img_ld=W * 3, weights=P, weights_cs=H * W, weights_ld=W, uv=None,
                 depth=None, status=P, scratch=P, scratch_bytes=need)
        f.update(kw)
        return lib.gcd_render_splat(C.byref(_lib.RenderSplatDesc(**f)), None)

    assert lib.gcd_render_splat(None, None) != 0 and b"null descriptor" in lib.gcd_render_last_error()
    for kw, msg in [(dict(xyz=None), b"null pointer"), (dict(rgb=None), b"null pointer"), (dict(cams=None), b"null pointer"),
                    (dict(img=None), b"null pointer"), (dict(weights=None), b"null pointer"), (dict(status=None), b"null pointer"),
                    (dict(xyz_dtype=_lib.RENDER_U8), b"bad dtype code"), (dict(xyz_dtype=7), b"bad dtype code"),
                    (dict(rgb_dtype=4), b"bad dtype code"), (dict(rgb_dtype=-1), b"bad dtype code"),
                    (dict(nc=0), b"cameras"), (dict(nc=9), b"cameras"), (dict(H=0), b"pixels a side"), (dict(W=40000), b"pixels a side"),
                    (dict(N=-1), b"2^31"), (dict(N=1 << 31), b"2^31"), (dict(xyz_ld=2), b"3 values"), (dict(rgb_ld=0), b"3 values"),
                    (dict(spread_radius=-1), b"spread_radius"), (dict(spread_radius=9), b"spread_radius"),
                    (dict(img_ld=W * 3 - 1), b"rows overlap"), (dict(weights_ld=W - 1), b"rows overlap"),
                    (dict(img_cs=H * W * 3 - 1), b"cameras overlap"), (dict(weights_cs=0), b"cameras overlap"),
                    (dict(scratch_bytes=need - 8), b"scratch too small"), (dict(scratch=None), b"scratch too small"),
                    (dict(scratch=P + 4), b"8-byte aligned")]:
        assert splat(**kw) != 0, kw
        assert msg in lib.gcd_render_last_error(), (kw, lib.gcd_render_last_error())

    def fill(img=P, img_ld=W * 3, H=H, W=W, k=21, sigma=5.25, out=P, cs=16 * 24, rs=24, xs=1, Hp=16, Wp=24, scale=2.0, offset=-1.0,
             scratch=P, nbytes=need_f):
        return lib.gcd_render_fill_resize_f32(img, img_ld, H, W, k, sigma, out, cs, rs, xs, Hp, Wp, scale, offset, scratch, nbytes,
                                              None)

    for kw, msg in [(dict(img=None), b"null pointer"), (dict(out=None), b"null pointer"),
                    (dict(H=10, nbytes=1 << 30), b"reflect padding"), (dict(W=10, img_ld=30, nbytes=1 << 30), b"reflect padding"),
                    (dict(k=3, H=1, nbytes=1 << 30), b"reflect padding"), (dict(k=1, W=1, img_ld=3, nbytes=1 << 30), b"reflect padding"),
                    (dict(k=4), b"kernel_size"), (dict(k=33), b"kernel_size"), (dict(k=0), b"kernel_size"), (dict(k=-3), b"kernel_size"),
                    (dict(sigma=0.0), b"sigma"), (dict(sigma=float("nan")), b"sigma"), (dict(sigma=float("inf")), b"sigma"),
                    (dict(Hp=0), b"pixels a side"), (dict(Wp=-2), b"pixels a side"), (dict(H=0), b"pixels a side"),
                    (dict(img_ld=W * 3 - 1), b"rows overlap"),
                    (dict(nbytes=need_f - 8), b"scratch too small"), (dict(scratch=None), b"scratch too small"),
                    (dict(scratch=P + 2), b"8-byte aligned")]:
        assert fill(**kw) != 0, kw
        assert msg in lib.gcd_render_last_error(), (kw, lib.gcd_render_last_error())


def test_geometry_refuses_what_is_not_a_gpu_tensor():
    from gcd_amd import _lib, geometry as G
    xyzrgb, K, RT = torch.rand(10, 6), torch.eye(3), torch.eye(4)
    with pytest.raises(_lib.GcdError, match="no CPU"):
        G.project_points_to_pixels(xyzrgb, K, RT, 8, 8)
    with pytest.raises(_lib.GcdError, match="no CPU"):
        G.project_points_to_pixels((xyzrgb[:, :3], xyzrgb[:, 3:]), K, RT, 8, 8)
    with pytest.raises(_lib.GcdError, match="no CPU"):
        G.project_points_to_pixels(xyzrgb.numpy(), K, RT, 8, 8)
    with pytest.raises(_lib.GcdError, match="no CPU"):
        G.blur_into_black(torch.rand(8, 8, 3))
    with pytest.raises(_lib.GcdError, match="no CPU"):
        G.render_views(xyzrgb[:, :3], xyzrgb[:, 3:], K, RT[None], (8, 8), (4, 4), 2, 3, 0.75)
    with pytest.raises(_lib.GcdError, match="no CPU"):
        G.synth_src_dst_rgb(dict(xyz=[xyzrgb[None, :, :3].half()], rgb=[torch.zeros(1, 10, 3, dtype=torch.uint8)]), RT[None], RT[None],
                            K[None], RT[None], model_frames=1, render_height=8, render_width=12, frame_height=4, frame_width=6,
                            spread_radius=2)


def test_camera_helpers():
    import numpy as np
    from gcd_amd import geometry as G
    c = G.cartesian_from_spherical(np.array([[90.0, 0.0, 2.0], [0.0, 90.0, 3.0]]), deg2rad=True)
    assert np.allclose(c, [[0.0, 2.0, 0.0], [0.0, 0.0, 3.0]], atol=1e-12)
    RT = G.extrinsics_from_look_at(np.array([0.0, -5.0, 1.0]), np.array([0.0, 0.0, 1.0]))
    R = RT[:3, :3]
    assert np.allclose(R.T @ R, np.eye(3), atol=1e-12) and np.isclose(np.linalg.det(R), 1.0)
    assert np.allclose(R[:, 2], [0.0, 1.0, 0.0]) and np.allclose(R[:, 1], [0.0, 0.0, -1.0]) and np.allclose(R[:, 0], [1.0, 0.0, 0.0])
    p = np.random.default_rng(0).normal(size=(5, 3))
    assert np.allclose(G.camera_to_world(G.world_to_camera(p, RT), RT), p, atol=1e-12)
    assert np.allclose(G.world_to_camera(np.array([0.0, 0.0, 1.0]), RT), [0.0, 0.0, 5.0])


# ---- the accumulation scheme, with integer tensors ---------------------------------------------------------------------------

def emulate_splat(xyz, rgb, K, RT, H, W, radius):
    """What render.hip computes, pass for pass, on the CPU: int64 index_add_ and amax do not depend on the order either."""
    x = (xyz.float() if xyz.dtype == torch.float16 else xyz).double()
    c = (rgb / 255.0).type(torch.float32).double() if rgb.dtype == torch.uint8 else rgb.double()
    K, RT = K.double(), RT.double()
    N = x.shape[0]
    cam = (x - RT[0:3, 3]) @ RT[0:3, 0:3]
    p = cam @ K.T
    uv, depth = p[:, 0:2] / p[:, 2:3], cam[:, 2]
    t = uv + 0.5
    mask = (t[:, 0] > -1) & (t[:, 0] < W) & (t[:, 1] > -1) & (t[:, 1] < H) & (depth > 0.1)
    img, pw = torch.zeros(H, W, 3), -torch.ones(H, W, 1, dtype=torch.float64)
    if not mask.any():
        return img, pw, uv, depth[:, None]
    px, py, d, c = t[mask, 0].long(), t[mask, 1].long(), depth[mask], c[mask]
    gmax, strength = d.max(), 512.0
    if gmax >= 64.0:
        strength, d, gmax = 256.0, d.sqrt().clamp(max=32.0), gmax.sqrt().clamp(max=32.0)
    l0 = -(d / gmax * 2.0 - 1.0) * strength
    left, right = radius // 2, (radius + 1) // 2
    idx, ls, cs = [], [], []
    for dy in range(-left, right + 1):
        for dx in range(-left, right + 1):
            ok = (px + dx >= 0) & (px + dx < W) & (py + dy >= 0) & (py + dy < H)
            idx.append(((py + dy) * W + px + dx)[ok])
            ls.append(l0[ok] if dx == 0 and dy == 0 else l0[ok] + math.log(0.02))
            cs.append(c[ok])
    idx, ls, cs = torch.cat(idx), torch.cat(ls), torch.cat(cs)
    fscale = 2.0 ** min(52, 63 - int(N).bit_length())
    ninf = torch.full((H * W,), -float("inf"), dtype=torch.float64)
    lmax = [ninf.clone().scatter_reduce(0, idx, ls, "amax")]
    sums = [torch.zeros(H * W, dtype=torch.int64).index_add_(0, idx, ((ls - lmax[0][idx]).exp().clamp(max=1.0) * fscale).floor().long())]
    for ch in range(3):
        sel = (cs[:, ch] > 0) & (cs[:, ch] < float("inf"))
        lc = ls[sel] + cs[sel, ch].log()                    # the channel's key: l + ln c
        lm = ninf.clone().scatter_reduce(0, idx[sel], lc, "amax")
        term = ((lc - lm[idx[sel]]).exp().clamp(max=1.0) * fscale).floor().long()
        lmax.append(lm)
        sums.append(torch.zeros(H * W, dtype=torch.int64).index_add_(0, idx[sel], term))
    hit = sums[0] > 0
    pw = torch.where(hit, sums[0].double() / fscale * lmax[0].exp(), torch.tensor(-1.0, dtype=torch.float64)).reshape(H, W, 1)
    chans = []
    for ch in range(3):
        ok = hit & (sums[1 + ch] > 0)
        v = sums[1 + ch].double() / sums[0].double().clamp(min=1.0) * (lmax[1 + ch] - lmax[0]).exp()
        chans.append(torch.where(ok, v, torch.zeros_like(v)).clamp(0.0, 1.0).float())
    return torch.stack(chans, dim=-1).reshape(H, W, 3), pw, uv, depth[:, None]


@pytest.fixture(scope="module")
def gold():
    return load_golden()


def test_golden_file_holds_the_fixtures_the_bars_are_stated_for(gold):
    names = [c["name"] for c in gold["cases"]]
    assert {"base_r1", "base_r2", "base_r3", "base_r2_cam_b", "past_int32", "far", "ragged_f64", "f16_u8", "one_pixel", "n0", "none_visible",
            "occluder_near", "occluder_far"} == set(names) and len(names) == 13
    by = {c["name"]: c for c in gold["cases"]}
    assert (by["ragged_f64"]["H"], by["ragged_f64"]["W"]) == (23, 37) and (by["base_r1"]["H"], by["base_r1"]["W"]) == (24, 40)
    assert gold["clouds"]["f16_u8"][0].dtype == torch.float16 and gold["clouds"]["f16_u8"][1].dtype == torch.uint8
    assert gold["clouds"]["ragged_f64"][0].dtype == torch.float64 and gold["clouds"]["base_f32"][0].dtype == torch.float32
    assert by["far"]["depth"].max() >= 64 and by["n0"]["raises"] and by["none_visible"]["raises"] and by["n0"]["visible"] == 0
    assert by["past_int32"]["uv"][4, 0] > 2.0 ** 31 and by["past_int32"]["uv"][5, 1] < -2.0 ** 31
    near, far = by["occluder_near"]["img"][6:18, 15, 0], by["occluder_far"]["img"][6:18, 15, 0]
    assert (near > 0).all() and (near < 1e-25).all() and (far == 0).all()      # not black / exactly black
    assert GOLDEN.stat().st_size < 1024 * 1024


def test_integer_emulation_of_the_accumulation_scheme_reproduces_the_golden(gold):
    worst = 0
    for c in gold["cases"]:
        xyz, rgb = golden_cloud(gold, c)
        fig = check_splat(c["name"], emulate_splat(xyz, rgb, c["K"], c["RT"], c["H"], c["W"], c["radius"]), c)
        worst = max(worst, fig["ulp"])
    print(f"worst image difference over the golden cases: {worst} ulp")


def test_integer_emulation_on_float_colours_tiny_and_above_one():
    """A channel's reference exponent is the largest l + ln c, so a near point with a colour of 1e-10 does not set the
    scale of the bright point behind it, and nothing is clamped before the final image."""
    xyz, rgb, K, RT, H, W = float_colour_cloud()
    for radius in (0, 2):
        img, pw, _, _ = emulate_splat(xyz, rgb, K, RT, H, W, radius)
        check_float_colours(img, pw, radius)
