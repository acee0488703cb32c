"""The memory contract (tests/memcontract.py; DESIGN.md "Memory contract") of the four launching entries of
libgcd_amd_clip.so: operands are strided views in guarded allocations, outputs start as zeros in one run and as a NaN bit
pattern in the other (guards, pad columns too), the two runs are bit-identical, every payload element is written, no
guard is touched, and the clean run meets the bar of the entry's own test (tests/test_clip_vision_gpu.py).  The entries
take no scratch; none reduces with atomics, so there is no bit-equality waiver."""
import math

import pytest
import torch
import torch.nn.functional as F

import memcontract as mc

pytestmark = pytest.mark.gpu
F16, F32 = torch.float16, torch.float32
CASES = []


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def case(cid, entries, **kw):
    def deco(fn):
        CASES.append(mc.Case(cid, entries, fn, **kw))
        return fn
    return deco


def _attn_case(ctx, n, S, heads):
    from gcd_amd import clip_vision as cv
    g = _gen(10 + S)
    C = heads * 80
    qkv = (torch.randn(n * S, 3 * C, generator=g) * 1.5).to(F16).float()
    qg = ctx.inp(qkv, dtype=F16, name="qkv")          # rows past n * S: the guard (keys past S of the last image)
    out = ctx.out("out", n * S, C, F16, pad=4)
    cv.attention(qg, out, n, S, heads)

    def ref():
        q, k, v = [t.reshape(n, S, heads, 80).permute(0, 2, 1, 3).double() for t in qkv.split(C, dim=1)]
        r = F.scaled_dot_product_attention(q, k, v)
        return {"out": (r.permute(0, 2, 1, 3).reshape(n * S, C).float(), 1.5e-3)}
    return ctx.ref(ref)


for _n, _S, _heads in [(2, 1, 1), (2, 17, 2), (1, 65, 3), (2, 257, 2)]:      # one kernel instantiation each + a lone key
    case(f"clip_attn_S{_S}", ("gcd_clip_attn_f16",))(lambda ctx, _a=(_n, _S, _heads): _attn_case(ctx, *_a))


def _preprocess_case(ctx, n, H, W, S, antialias):
    from gcd_amd import clip_vision as cv
    g = _gen(20 + H)
    P, kp = 14, 608
    raw = torch.rand(n, 3, H, W, generator=g) * 2 - 1
    rows = ctx.inp(raw.reshape(n * 3 * H, W), name="x")                      # pad columns after every image row
    x = rows.as_strided((n, 3, H, W), (3 * H * rows.stride(0), H * rows.stride(0), rows.stride(0), 1), rows.storage_offset())
    mean, std = ctx.inp_flat(torch.tensor(cv.CLIP_MEAN), name="mean"), ctx.inp_flat(torch.tensor(cv.CLIP_STD), name="std")
    G = S // P
    patches = ctx.out("patches", n * G * G, kp, F16, pad=0)
    img = ctx.out_flat("img", (n, 3, S, S), F32)
    lib = cv._lib_clip.load()
    cv._lib_clip.check(lib.gcd_clip_preprocess(x.data_ptr(), *x.stride(), n, H, W, S, P, int(antialias), mean.data_ptr(),
                                               std.data_ptr(), patches.data_ptr(), kp, img.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream), "gcd_clip_preprocess")

    def ref():
        r = cv.preprocess_reference(raw.double(), S, antialias, torch.tensor(cv.CLIP_MEAN), torch.tensor(cv.CLIP_STD))
        pm = torch.zeros(n * G * G, kp, dtype=torch.float64)
        pm[:, :3 * P * P] = r.reshape(n, 3, G, P, G, P).permute(0, 2, 4, 1, 3, 5).reshape(n * G * G, 3 * P * P)
        # max-abs bars: the fp32 tap sums (2e-5 is 4 x the smallest recorded float32-chain gap of a blurred case);
        # the patches add one rounding to fp16 of values within [-2, 2.3]: 2^-11 x 2.3
        return {"img": (r.reshape(1, -1), ("maxabs", 2e-5)), "patches": (pm, ("maxabs", 2.3 * 2.0 ** -11 + 2e-5))}
    return ctx.ref(ref)


case("clip_preprocess_72x200_blur", ("gcd_clip_preprocess",))(lambda ctx: _preprocess_case(ctx, 2, 72, 200, 56, True))
case("clip_preprocess_40x300_one_axis_up", ("gcd_clip_preprocess",))(lambda ctx: _preprocess_case(ctx, 1, 40, 300, 56, True))
case("clip_preprocess_30x30_upscale", ("gcd_clip_preprocess",))(lambda ctx: _preprocess_case(ctx, 2, 30, 30, 56, False))


def _tokens_case(ctx, n, G2, C):
    from gcd_amd import clip_vision as cv
    g = _gen(30 + C)
    patch = torch.randn(n * G2, C, generator=g)
    cls, pos = 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(G2 + 1, C, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    out = ctx.out("tok", n * (G2 + 1), C, F32)
    cv.tokens_ln_pre(ctx.inp(patch, name="patch"), ctx.inp_flat(cls, name="cls"), ctx.inp_flat(pos, name="pos"),
                     ctx.inp_flat(gamma, name="gamma"), ctx.inp_flat(beta, name="beta"), out, n)

    def ref():
        z = torch.cat([cls.double().expand(n, 1, C), patch.double().reshape(n, G2, C)], 1) + pos.double()
        return {"tok": (F.layer_norm(z, (C,), gamma.double(), beta.double(), 1e-5).reshape(n * (G2 + 1), C), 2e-6)}
    return ctx.ref(ref)


case("clip_tokens_ln_pre_C160", ("gcd_clip_tokens_ln_pre",))(lambda ctx: _tokens_case(ctx, 3, 16, 160))
case("clip_tokens_ln_pre_C1284", ("gcd_clip_tokens_ln_pre",))(lambda ctx: _tokens_case(ctx, 2, 7, 1284))


@case("clip_bias_gelu", ("gcd_clip_bias_gelu_f16",))
def _(ctx):
    from gcd_amd import clip_vision as cv
    M, N = 37, 172
    g = _gen(40)
    h, bias = 3.0 * torch.randn(M, N, generator=g), torch.randn(N, generator=g)
    out = ctx.out("out", M, N, F16, pad=4)
    cv.bias_gelu(ctx.inp(h, name="h"), ctx.inp_flat(bias, name="bias"), out)

    def ref():
        t = (h + bias).double()
        # rel-L2 of one rounding to fp16 is below 2^-11 / sqrt(3) = 2.8e-4 (uniform rounding error); 4e-4 with the tail's absolute term
        return {"out": (0.5 * t * (1.0 + torch.erf(t / math.sqrt(2.0))), 4e-4)}
    return ctx.ref(ref)


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_contract(gpu, c):
    mc.run_contract(c, gpu)


def test_every_kernel_launching_export_has_a_case():
    from gcd_amd import _lib_clip
    launching = set(_lib_clip.CLIP_SIGNATURES) - {"gcd_clip_abi_version", "gcd_clip_last_error"}
    covered = {e for c in CASES for e in c.entries}
    assert launching == covered, launching ^ covered
    assert all(not c.atomic for c in CASES), "no bit-equality waiver: there are no read-modify-write reductions here"
