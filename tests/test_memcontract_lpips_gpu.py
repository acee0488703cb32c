"""The memory contract (tests/memcontract.py; DESIGN.md "Memory contract") of the three launching entries of
libgcd_amd_lpips.so: operands are views in guarded allocations, outputs start as zeros in one run and as a NaN bit pattern
in the other (guards too), the two runs are bit-identical, every payload element is written, no guard is touched, null
destinations are honoured, and the clean run meets the bar of the entry's own test (tests/test_lpips_gpu.py: equality for
the packing and ReLU / max-pool, lpips_util.DISTANCE_BAR for the distance).  gcd_lpips_distance's partial sums are scratch:
written before they are read.  None reduces with atomics, so there is no bit-equality waiver."""
import pytest
import torch
import torch.nn.functional as F

import lpips_util as U
import memcontract as mc

pytestmark = pytest.mark.gpu
F16, F32, F64 = torch.float16, torch.float32, torch.float64
EQUAL = ("maxabs", 1e-30)          # the harness compares with <: any difference at all fails
CASES = []


def case(cid, entries, **kw):
    def deco(fn):
        CASES.append(mc.Case(cid, entries, fn, **kw))
        return fn
    return deco


def _pack_case(ctx, n, H, W, cpad, ab):
    from gcd_amd import lpips as L
    g = torch.Generator().manual_seed(H)
    x = torch.rand(n, 3, H, W, generator=g) * (1.0 if ab[0] == 2.0 else 2.0) - (0.0 if ab[0] == 2.0 else 1.0)
    shift, scale = torch.tensor(U.SHIFT), torch.tensor(U.SCALE)
    out = ctx.out("out16", n * H * W, cpad, F16, pad=0)
    L.pack(ctx.inp_flat(x, name="x"), out, ab, ctx.inp_flat(shift, name="shift"), ctx.inp_flat(scale, name="scale"))

    def ref():
        t = x * ab[0]
        t = t + ab[1]
        t = t - shift.view(1, 3, 1, 1)
        t = t / scale.view(1, 3, 1, 1)
        want = torch.zeros(n * H * W, cpad, dtype=F64)
        want[:, :3] = t.permute(0, 2, 3, 1).reshape(-1, 3).half().double()
        return {"out16": (want, EQUAL)}
    return ctx.ref(ref)


case("lpips_pack_signed_37x51", ("gcd_lpips_pack_f16",))(lambda ctx: _pack_case(ctx, 2, 37, 51, 64, (1.0, 0.0)))
case("lpips_pack_unit_16x16_cpad8", ("gcd_lpips_pack_f16",))(lambda ctx: _pack_case(ctx, 1, 16, 16, 8, (2.0, -1.0)))


def _relu_pool_case(ctx, n, H, W, C, want_full, want_pooled):
    from gcd_amd import lpips as L
    g = torch.Generator().manual_seed(H * W + C)
    src = (2.0 * torch.randn(n * H * W, C, generator=g)).half()
    full = ctx.out("full", n * H * W, C, F16, pad=0) if want_full else None
    pooled = ctx.out("pooled", n * (H // 2) * (W // 2), C, F16, pad=0) if want_pooled else None
    L.relu_pool(ctx.inp(src, pad=0, name="src"), full, pooled, n, H, W)

    def ref():
        r = torch.relu(src.float())
        refs = {}
        if want_full:
            refs["full"] = (r.double(), EQUAL)
        if want_pooled:
            p = F.max_pool2d(r.reshape(n, H, W, C).permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).reshape(-1, C)
            refs["pooled"] = (p.double(), EQUAL)
        return refs
    return ctx.ref(ref)


case("lpips_relu_pool_5x7_C32_both", ("gcd_lpips_relu_pool_f16",))(lambda ctx: _relu_pool_case(ctx, 2, 5, 7, 32, True, True))
case("lpips_relu_pool_6x8_C512_both", ("gcd_lpips_relu_pool_f16",))(lambda ctx: _relu_pool_case(ctx, 2, 6, 8, 512, True, True))
case("lpips_relu_5x7_C64_no_pool", ("gcd_lpips_relu_pool_f16",))(lambda ctx: _relu_pool_case(ctx, 3, 5, 7, 64, True, False))
case("lpips_pool_7x5_C64_no_full", ("gcd_lpips_relu_pool_f16",))(lambda ctx: _relu_pool_case(ctx, 3, 7, 5, 64, False, True))


def _distance_case(ctx, n, HW, C, blocks, taps, tap):
    from gcd_amd import lpips as L
    f0, f1, w = U.seeded_features(n, HW, C, 2000 + C)
    f0[3] = 0
    f1[-HW:] = f0[-HW:]                          # the last image: identical tensors
    others = torch.arange(1, taps * n + 1, dtype=F64).reshape(taps, n) / 64.0
    # rows of the other taps are inputs (what earlier calls left); with one tap the whole tensor is output
    tm = ctx.out_flat("tap_means", (taps, n), F64, init=others if taps > 1 else None)
    out = ctx.out_flat("out", (n,), F32)
    partials = ctx.scratch(n * blocks, F32, name="partials")
    L.distance(ctx.inp(f0, pad=0, name="f0"), ctx.inp(f1, pad=0, name="f1"), ctx.inp_flat(w, name="w"), n, HW, tm, tap, taps,
               out, blocks=blocks, partials=partials)

    def ref():
        want = others.clone()
        want[tap] = U.distance_ref(f0, f1, w, n, HW)
        return {"tap_means": (want.reshape(1, -1), U.DISTANCE_BAR), "out": (want.sum(0).reshape(1, -1), U.DISTANCE_BAR)}
    return ctx.ref(ref)


case("lpips_distance_C64_ragged", ("gcd_lpips_distance",))(lambda ctx: _distance_case(ctx, 3, 203, 64, 7, 1, 0))
case("lpips_distance_C512_strided_blocks", ("gcd_lpips_distance",))(lambda ctx: _distance_case(ctx, 2, 77, 512, 5, 3, 1))
case("lpips_distance_C32_idle_blocks", ("gcd_lpips_distance",))(lambda ctx: _distance_case(ctx, 2, 45, 32, 9, 1, 0))


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_contract(gpu, c):
    mc.run_contract(c, gpu)


def test_every_kernel_launching_export_has_a_case():
    from gcd_amd import _lib_lpips
    launching = set(_lib_lpips.LPIPS_SIGNATURES) - {"gcd_lpips_abi_version", "gcd_lpips_last_error"}
    covered = {e for c in CASES for e in c.entries}
    assert launching == covered, launching ^ covered
    assert all(not c.atomic for c in CASES), "no bit-equality waiver: there are no read-modify-write reductions here"
