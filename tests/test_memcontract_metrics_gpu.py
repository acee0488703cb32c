"""The memory contract of the device metrics (include/gcd_amd_metrics.h; tests/memcontract.py; DESIGN.md "Memory
contract").

gcd_metrics_frames_f32 and gcd_metrics_diversity_f32 are called directly with guarded operands: `pred`, `gt` and
`reproject` are guarded read-only inputs, `out` and `uncertainty` are store-only (zeros in run (a), NaN in run (b), every
element must be written), `scratch` is zeros in (a) and NaN in (b) and must not reach a result.  No atomics: run (b) is
bit-identical to run (a).  Odd sizes (one tile with a ragged edge, and 2 x 2 tiles whose halos cross), with and without
`reproject`; the masks leave every value finite (the harness takes a NaN for an unwritten element).  Values: the host
function on float64 copies, rel-L2 1e-9 (the float32 uncertainty map: 1e-6).
"""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import memcontract as mc

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
ROOT = Path(__file__).resolve().parent.parent
S, T = 2, 2
CASES = []


def _inputs(H, W, with_mask):
    g = torch.Generator().manual_seed(31 + H)
    gt = torch.rand(T, 3, H, W, generator=g)
    pred = (gt[None] + 0.05 * torch.randn(S, T, 3, H, W, generator=g)).clamp(0, 1)
    rep = None
    if with_mask:
        # occluded: the L1 ball of radius 3 around (3, 3), and whatever lies left of it; the ball around (H - 4, W - 4)
        # is visible: both eroded masks keep a pixel of the cropped image even at 9 x 13
        y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        occ = ((y - 3).abs() + (x - 3).abs() <= 3) | (x + y < 4)
        assert not (occ & ((y - (H - 4)).abs() + (x - (W - 4)).abs() <= 3)).any()
        rep = ((0.2 + torch.rand(T, 3, H, W, generator=g)) * (~occ)).float()
    return pred.float(), gt.float(), rep


def _host64(pred, gt, rep):
    from gcd_amd import metrics as M
    return M.calculate_metrics(gt.numpy().astype(np.float64), None if rep is None else rep.numpy(),
                               [{"sampled_rgb": x} for x in pred.numpy().astype(np.float64)])


def _frames(ctx, H, W, with_mask):
    from gcd_amd import _lib
    lib = _lib.load_metrics()
    pred, gt, rep = _inputs(H, W, with_mask)
    p, g_ = ctx.inp_flat(pred, name="pred"), ctx.inp_flat(gt, name="gt")
    r = ctx.inp_flat(rep, name="reproject") if with_mask else None
    nbytes = lib.gcd_metrics_frames_scratch_bytes(S, T, H, W)
    scratch = ctx.scratch(nbytes // 8, F64)
    out = ctx.out_flat("out", (S, T, 6), F64)
    _lib.check_metrics(lib.gcd_metrics_frames_f32(
        p.data_ptr(), g_.data_ptr(), r.data_ptr() if with_mask else None, S, T, H, W, 0, scratch.data_ptr(), nbytes,
        out.data_ptr(), torch.cuda.current_stream().cuda_stream), "gcd_metrics_frames_f32")

    def ref():
        md, _ = _host64(pred, gt, rep)
        want = torch.zeros(S, T, 6, dtype=F64)
        names = ("psnr", "ssim", "psnr_vis", "ssim_vis", "psnr_occ", "ssim_occ")
        for i, n in enumerate(names if with_mask else names[:2]):
            want[:, :, i] = torch.from_numpy(md["frame_" + n])
        assert torch.isfinite(want).all()
        return {"out": (want.reshape(1, -1), 1e-9)}
    return ctx.ref(ref)


def _diversity(ctx, H, W, with_mask):
    from gcd_amd import _lib
    lib = _lib.load_metrics()
    pred, gt, rep = _inputs(H, W, with_mask)
    p = ctx.inp_flat(pred, name="pred")
    r = ctx.inp_flat(rep, name="reproject") if with_mask else None
    nbytes = lib.gcd_metrics_diversity_scratch_bytes(S, T, H, W)
    scratch = ctx.scratch(nbytes // 8, F64)
    unc = ctx.out_flat("uncertainty", (T, H, W), F32)
    out = ctx.out_flat("out", (T, 3), F64)
    _lib.check_metrics(lib.gcd_metrics_diversity_f32(
        p.data_ptr(), r.data_ptr() if with_mask else None, S, T, H, W, 0, unc.data_ptr(), scratch.data_ptr(), nbytes,
        out.data_ptr(), torch.cuda.current_stream().cuda_stream), "gcd_metrics_diversity_f32")

    def ref():
        md, u = _host64(pred, gt, rep)
        want = torch.zeros(T, 3, dtype=F64)
        want[:, 0] = torch.from_numpy(md["frame_diversity"])
        if with_mask:
            want[:, 1] = torch.from_numpy(md["frame_diversity_vis"])
            want[:, 2] = torch.from_numpy(md["frame_diversity_occ"])
        assert torch.isfinite(want).all()
        return {"out": (want.reshape(1, -1), 1e-9), "uncertainty": (torch.from_numpy(u).reshape(1, -1), 1e-6)}
    return ctx.ref(ref)


for _H, _W in ((9, 13), (19, 37)):
    for _m in (False, True):
        _tag = f"{_H}x{_W}_{'reproject' if _m else 'nomask'}"
        CASES.append(mc.Case(f"metrics_frames_{_tag}", ("gcd_metrics_frames_f32",),
                             lambda ctx, _H=_H, _W=_W, _m=_m: _frames(ctx, _H, _W, _m)))
        CASES.append(mc.Case(f"metrics_diversity_{_tag}", ("gcd_metrics_diversity_f32",),
                             lambda ctx, _H=_H, _W=_W, _m=_m: _diversity(ctx, _H, _W, _m)))


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_metrics_memory_contract(gpu, c):
    assert not c.atomic, "no spread rule here: run (b) is bit-identical to run (a)"
    mc.run_contract(c, gpu)


def test_every_kernel_entry_of_the_metrics_header_has_a_contract_case():
    header = (ROOT / "include" / "gcd_amd_metrics.h").read_text()
    exports = set(re.findall(r"^\s*(?:int|int64_t)\s+(gcd_\w+)\s*\(", header, flags=re.M))
    kernels = {e for e in exports if e.endswith("_f32")}          # the others launch nothing: version and scratch sizes
    assert exports - kernels == {"gcd_metrics_abi_version", "gcd_metrics_frames_scratch_bytes",
                                 "gcd_metrics_diversity_scratch_bytes"}
    covered = {e for c in CASES for e in c.entries}
    assert kernels == {"gcd_metrics_frames_f32", "gcd_metrics_diversity_f32"} and kernels <= covered
