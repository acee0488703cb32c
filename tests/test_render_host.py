"""CPU: the C ABI of libgcd_amd_render.so (include/gcd_amd_render.h) — header, binding table and exported symbols are one
set; the library builds from a tree that holds no build product, through build(); every entry validates its arguments
before any launch; the scratch sizes are what the header says; the host module refuses what is not a GPU tensor; and the
accumulation scheme of the splat (four reference exponents per pixel, l for the denominator and l + ln c per channel, integer maxima, fixed-point integer sums), restated
here with integer tensors, reproduces the reference's images of tests/golden/render_tiny.pt at the bars of DESIGN.md §12.2.
The last one keeps the scheme itself pinned where no GPU is present."""
import ctypes as C
import importlib.util
import math
import re
import shutil
import struct
from pathlib import Path

import pytest
import torch

from render_util import GOLDEN, check_float_colours, check_splat, float_colour_cloud, golden_cloud, load_golden

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


def test_render_header_binding_table_and_exports_are_one_set():
    from gcd_amd import _lib
    from gcd_amd.csrc import build as b
    b.build(verbose=False)                     # a no-op when the libraries are current
    header = (ROOT / "include" / "gcd_amd_render.h").read_text()
    declared = set(re.findall(DECL, header, flags=re.M))
    assert declared == set(_lib.RENDER_SIGNATURES), declared ^ set(_lib.RENDER_SIGNATURES)
    exported = {n for n in _dynamic_exports(_lib.RENDER_LIB_PATH) if n.startswith("gcd_")}
    assert exported == declared, exported ^ declared
    assert {"gcd_render_abi_version", "gcd_render_last_error", "gcd_render_scratch_bytes", "gcd_render_splat",
            "gcd_render_fill_resize_f32"} <= declared
    lib = _lib.load_render()
    assert lib.gcd_render_abi_version() == _lib.RENDER_ABI_VERSION == 1
    assert int(re.search(r"#define GCD_AMD_RENDER_ABI_VERSION (\d+)", header).group(1)) == 1
    for name in ("F16", "F32", "F64", "U8", "MAX_CAMERAS", "CAM_DOUBLES", "MAX_KERNEL"):
        assert int(re.search(rf"#define GCD_RENDER_{name} (\d+)", header).group(1)) == getattr(_lib, "RENDER_" + name), name
    # the descriptor of the binding has the header's fields, in the header's order
    body = re.search(r"typedef struct gcd_render_splat_desc \{(.*?)\} gcd_render_splat_desc;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].replace(
        "void*", "").replace("double*", "").replace("float*", "").replace("int64_t*", "").split(",")]
    assert fields == [f[0] for f in _lib.RenderSplatDesc._fields_], fields
    # a library of its own: the main header, its table, its ABI version and the step's source digest do not know it
    main_header = (ROOT / "include" / "gcd_amd.h").read_text()
    assert "gcd_render" not in main_header and not (declared & set(_lib.SIGNATURES)) and _lib.ABI_VERSION == 9
    assert set(re.findall(DECL, main_header, flags=re.M)) == set(_lib.SIGNATURES)
    assert not (set(b.RENDER_SOURCES) & set(b.SOURCES + b.TRAIN_SOURCES + b.SAMPLER_SOURCES + b.METRICS_SOURCES))
    assert not (set(b.RENDER_HEADERS) & set(b.HEADERS + b.TRAIN_HEADERS + b.SAMPLER_HEADERS + b.METRICS_HEADERS))


def test_render_library_builds_from_a_clean_tree_through_build(tmp_path):
    """A copy of the build script, the source and the header, and nothing built: build() makes the library even when
    the main library is current (it returns early then), and a second call compiles nothing."""
    (tmp_path / "gcd_amd" / "csrc").mkdir(parents=True)
    (tmp_path / "include").mkdir()
    for rel in ("gcd_amd/csrc/build.py", "gcd_amd/csrc/render.hip", "include/gcd_amd_render.h"):
        shutil.copy(ROOT / rel, tmp_path / rel)
    spec = importlib.util.spec_from_file_location("clean_tree_build_render", tmp_path / "gcd_amd" / "csrc" / "build.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert m.LIB_RENDER == tmp_path / "gcd_amd" / "libgcd_amd_render.so" and not m.LIB_RENDER.exists()
    called = []
    m.build_train = lambda **k: called.append("train")
    m.build_sampler = lambda **k: called.append("sampler")
    m.build_metrics = lambda **k: called.append("metrics")
    m._digest = lambda: "current"
    m.LIB.write_bytes(b"")
    m.STAMP.write_text("current")
    assert m.build(verbose=False) == m.LIB and called == ["train", "sampler", "metrics"]
    assert m.LIB_RENDER.exists() and m.STAMP_RENDER.exists()
    exported = {n for n in _dynamic_exports(m.LIB_RENDER) if n.startswith("gcd_")}
    assert "gcd_render_splat" in exported and "gcd_render_fill_resize_f32" in exported
    before = m.LIB_RENDER.stat().st_mtime_ns
    m.build(verbose=False)
    assert m.LIB_RENDER.stat().st_mtime_ns == before
    assert ".libgcd_amd_render.stamp" in (ROOT / ".gitignore").read_text().split()


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
