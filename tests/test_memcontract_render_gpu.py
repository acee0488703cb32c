"""The memory contract of the renderer (include/gcd_amd_render.h; tests/memcontract.py; DESIGN.md "Memory contract").

gcd_render_splat and gcd_render_fill_resize_f32 are called directly with guarded operands.  The cloud is two guarded
strided inputs (rows of 3 values, padded), the cameras a guarded flat input; `img` and `weights` are strided views (padded
rows, two cameras under each other) inside guarded allocations, `uv`, `depth`, `status` and the frames are store-only
too: zeros in run (a), NaN bytes in run (b), every payload element must be written and no guard touched.  `scratch` is
zeros in (a) and NaN bytes in (b) and must not reach a result: the splat clears its accumulators itself.  Integer
atomics only: run (b) is bit-identical to run (a).  Values: the golden file's reference (tools/make_golden_render.py).
"""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

import memcontract as mc
from render_util import golden_cloud, load_golden

pytestmark = pytest.mark.gpu
F32, F64, I64 = torch.float32, torch.float64, torch.int64
ROOT = Path(__file__).resolve().parent.parent
CASES = []


def _case(gold, name):
    return next(c for c in gold["cases"] if c["name"] == name)


def _splat(ctx, names, cloud_case):
    """One call for the cameras of the golden cases `names`, which share a cloud."""
    from gcd_amd import _lib, geometry as G
    lib = _lib.load_render()
    gold = load_golden()
    cs = [_case(gold, n) for n in names]
    c0 = cs[0]
    xyz_h, rgb_h = golden_cloud(gold, _case(gold, cloud_case))
    nc, H, W, N = len(cs), c0["H"], c0["W"], xyz_h.shape[0]
    codes = {torch.float16: _lib.RENDER_F16, torch.float32: _lib.RENDER_F32, torch.float64: _lib.RENDER_F64, torch.uint8: _lib.RENDER_U8}
    xyz = ctx.inp(xyz_h, name="xyz")
    rgb = ctx.inp(rgb_h, name="rgb")
    cams = ctx.inp_flat(G.pack_cameras(c0["K"], torch.stack([c["RT"] for c in cs]), "cpu"), name="cams")
    img = ctx.out("img", nc * H, W * 3, F32)
    weights = ctx.out("weights", nc * H, W, F64)
    uv = ctx.out_flat("uv", (nc, N, 2), F64)
    depth = ctx.out_flat("depth", (nc, N), F64)
    status = ctx.out_flat("status", (nc,), I64)
    nbytes = lib.gcd_render_scratch_bytes(nc, H, W)
    scratch = ctx.scratch(nbytes // 8, I64)
    d = _lib.RenderSplatDesc(
        xyz=xyz.data_ptr(), rgb=rgb.data_ptr(), xyz_ld=xyz.stride(0), rgb_ld=rgb.stride(0), N=N, xyz_dtype=codes[xyz_h.dtype],
        rgb_dtype=codes[rgb_h.dtype], cams=cams.data_ptr(), nc=nc, H=H, W=W, spread_radius=c0["radius"],
        img=img.data_ptr(), img_cs=H * img.stride(0), img_ld=img.stride(0), weights=weights.data_ptr(),
        weights_cs=H * weights.stride(0), weights_ld=weights.stride(0), uv=uv.data_ptr(), depth=depth.data_ptr(),
        status=status.data_ptr(), scratch=scratch.data_ptr(), scratch_bytes=nbytes)
    assert xyz.stride(0) > 3 and img.stride(0) > W * 3 and weights.stride(0) > W
    _lib.check_render(lib.gcd_render_splat(C.byref(d), torch.cuda.current_stream().cuda_stream), "gcd_render_splat")

    def ref():
        x = (xyz_h.float() if xyz_h.dtype == torch.float16 else xyz_h).double()
        uvs, ds = [], []
        for c in cs:
            RT, K = c["RT"].double(), c["K"].double()
            cam = (x - RT[0:3, 3]) @ RT[0:3, 0:3]
            p = cam @ K.T
            uvs.append(p[:, 0:2] / p[:, 2:3])
            ds.append(cam[:, 2])
        return {"img": (torch.cat([c["img"].reshape(H, W * 3) for c in cs]), ("maxabs", 2.0 ** -23)),
                "weights": (torch.cat([c["pixel_weights"].reshape(H, W) for c in cs]), 1e-9),
                "uv": (torch.stack(uvs).reshape(1, -1), 1e-12), "depth": (torch.stack(ds).reshape(1, -1), 1e-12),
                "status": (torch.tensor([[float(c["visible"]) for c in cs]], dtype=F64), 1e-12)}
    return ctx.ref(ref)


def _fill(ctx, src, k):
    from gcd_amd import _lib
    lib = _lib.load_render()
    gold = load_golden()
    f = next(f for f in gold["fills"] if f["src"] == src and f["k"] == k)
    img_h = _case(gold, src)["img"]
    H, W = img_h.shape[:2]
    Hp, Wp = f["frame_hw"]
    img = ctx.inp(img_h.reshape(H, W * 3), name="img")
    out = ctx.out("frames", 3 * Hp, Wp, F32)
    nbytes = lib.gcd_render_fill_scratch_bytes(H, W)
    scratch = ctx.scratch(nbytes // 8, F64)
    assert img.stride(0) > W * 3 and out.stride(0) > Wp
    _lib.check_render(lib.gcd_render_fill_resize_f32(
        img.data_ptr(), img.stride(0), H, W, k, f["sigma"], out.data_ptr(), Hp * out.stride(0), out.stride(0), 1, Hp, Wp, 2.0, -1.0,
        scratch.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream), "gcd_render_fill_resize_f32")
    return ctx.ref(lambda: {"frames": (f["frames_f64"].reshape(3 * Hp, Wp), ("maxabs", 2.0 ** -22))})


CASES.append(mc.Case("render_splat_two_cameras_f32", ("gcd_render_splat",), lambda ctx: _splat(ctx, ["base_r2", "base_r2_cam_b"], "base_r2")))
CASES.append(mc.Case("render_splat_ragged_f64_r2", ("gcd_render_splat",), lambda ctx: _splat(ctx, ["ragged_f64"], "ragged_f64")))
CASES.append(mc.Case("render_splat_f16_u8", ("gcd_render_splat",), lambda ctx: _splat(ctx, ["f16_u8"], "f16_u8")))
CASES.append(mc.Case("render_splat_radius3", ("gcd_render_splat",), lambda ctx: _splat(ctx, ["base_r3"], "base_r3")))
for _src, _k in (("base_r1", 21), ("ragged_f64", 21), ("ragged_f64", 3)):
    CASES.append(mc.Case(f"render_fill_{_src}_k{_k}", ("gcd_render_fill_resize_f32",), lambda ctx, _src=_src, _k=_k: _fill(ctx, _src, _k)))


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_render_memory_contract(gpu, c):
    assert not c.atomic, "integer atomics only: run (b) is bit-identical to run (a)"
    mc.run_contract(c, gpu)


def test_every_kernel_entry_of_the_render_header_has_a_contract_case():
    header = (ROOT / "include" / "gcd_amd_render.h").read_text()
    exports = set(re.findall(r"^\s*(?:int|int64_t)\s+(gcd_\w+)\s*\(", header, flags=re.M))
    kernels = exports - {"gcd_render_abi_version", "gcd_render_scratch_bytes", "gcd_render_fill_scratch_bytes"}
    covered = {e for c in CASES for e in c.entries}
    assert kernels == {"gcd_render_splat", "gcd_render_fill_resize_f32"} and kernels <= covered
