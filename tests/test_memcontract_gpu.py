"""The memory contract of every forward entry point of gcd_amd.ops (tests/memcontract.py; DESIGN.md "Memory contract").

Operands are views into larger allocations whose guard rows, pad columns and scratch hold zeros in one run and a NaN
bit pattern in the other; outputs start as zeros / NaN.  Writes must stay inside the payload, every payload element must be
written, the poisoned run must be bit-identical to the clean one, and the clean one must meet the bar of the entry's
own parity test (test_kernels_gpu.py, test_decoder_gpu.py) against the same CPU reference.  Shapes are small and have an
overhanging tile in every tiled dimension.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import memcontract as mc

pytestmark = pytest.mark.gpu

TOL_F32 = 1e-4          # test_kernels_gpu.py
TOL_F16 = 6e-4
F16, F32, BF16, F64 = torch.float16, torch.float32, torch.bfloat16, torch.float64

_IMPLS = {"auto": 0, "tile256x320": 2, "ring32": 3, "tile64": 6}
_ATTN = {"attn-auto": 0, "attn-q32": 1, "attn-q64": 2, "attn-q64p": 3}

CASES = []


def _h(t):
    return t.to(F16).float()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def case(cid, entries, **kw):
    def deco(fn):
        CASES.append(mc.Case(cid, entries, fn, **kw))
        return fn
    return deco


def gemm_case(cid, entries=("gemm",), impls=tuple(_IMPLS), **kw):
    """One case per forced GEMM kernel choice (test_kernels_gpu.py's gemm_impl)."""
    def deco(fn):
        for name in impls:
            def run(ctx, _name=name):
                from gcd_amd import ops
                ops.tune_set(ops.TUNE_GEMM_IMPL, _IMPLS[_name])
                try:
                    return fn(ctx)
                finally:
                    torch.cuda.synchronize()
                    ops.tune_set(ops.TUNE_GEMM_IMPL, 0)
            CASES.append(mc.Case(f"{cid}[{name}]", entries, run, **kw))
        return fn
    return deco


# ------------------------------------------------------------------------------------------------------------- GEMM
def _plain_operands(ctx, M, N, K, seed, rows=50):
    g = _gen(seed)
    a = _h(torch.randn(M, K, generator=g))
    w = _h(torch.randn(N, K, generator=g) / math.sqrt(K))
    bias = torch.randn(N, generator=g)
    rv = torch.randn((M + rows - 1) // rows, N, generator=g)
    r1, r2 = torch.randn(M, N, generator=g), torch.randn(M, N, generator=g)
    alpha = torch.rand((M + rows - 1) // rows, generator=g)
    dev = dict(a=ctx.inp(a, dtype=F16, name="A"), w=ctx.inp_flat(w, dtype=F16, name="W"),
               bias=ctx.inp_flat(bias, name="bias"), rv=ctx.inp(rv, name="rowvec"), r1=ctx.inp(r1, name="r1"),
               r2=ctx.inp(r2, name="r2"), alpha=ctx.inp_flat(alpha, name="frame_alpha"))
    return dict(a=a, w=w, bias=bias, rv=rv, r1=r1, r2=r2, alpha=alpha), dev


@gemm_case("gemm_bias_rowvec_r1_r2_strided")
def _(ctx):
    from gcd_amd import ops
    M, N, K, rows = 333, 352, 128, 50             # ragged in M (64-, 128-, 256-row tiles) and N (160 / 320 columns)
    c, d = _plain_operands(ctx, M, N, K, 1, rows)
    out = ctx.out("out", M, N, F32)
    ops.gemm(d["a"], d["w"], out, M=M, bias=d["bias"], rowvec=d["rv"], rows_per_vec=rows, r1=d["r1"], r2=d["r2"],
             s_acc=0.7, s_r1=0.5, s_r2=-1.25)
    return ctx.ref(lambda: {"out": (0.7 * (c["a"] @ c["w"].t() + c["bias"] + c["rv"].repeat_interleave(rows, 0)[:M])
                                    + 0.5 * c["r1"] - 1.25 * c["r2"], TOL_F32)})


@gemm_case("gemm_inplace_out_is_r1")
def _(ctx):
    from gcd_amd import ops
    M, N, K = 500, 320, 192
    c, d = _plain_operands(ctx, M, N, K, 2)
    out = ctx.out("out", M, N, F32, init=c["r1"])
    ops.gemm(d["a"], d["w"], out, M=M, bias=d["bias"], r1=out)
    return ctx.ref(lambda: {"out": (c["a"] @ c["w"].t() + c["bias"] + c["r1"], TOL_F32)})


@gemm_case("gemm_f16_out")
def _(ctx):
    from gcd_amd import ops
    M, N, K = 257, 176, 128
    c, d = _plain_operands(ctx, M, N, K, 3)
    out = ctx.out("out", M, N, F16)
    ops.gemm(d["a"], d["w"], out, M=M, bias=d["bias"], out_kind=ops.OUT_F16)
    return ctx.ref(lambda: {"out": (c["a"] @ c["w"].t() + c["bias"], TOL_F16)})


@gemm_case("gemm_geglu_out")
def _(ctx):
    from gcd_amd import ops, packing
    g = _gen(4)
    M, C = 200, 64
    inner = 4 * C
    a = _h(torch.randn(M, C, generator=g))
    w = _h(torch.randn(2 * inner, C, generator=g) / math.sqrt(C))
    b = torch.randn(2 * inner, generator=g)
    wp, bp = packing.pack_geglu(w, b)
    out = ctx.out("out", M, inner, F16)
    ops.gemm(ctx.inp(a, dtype=F16, name="A"), ctx.inp_flat(wp, dtype=F16, name="W"), out, M=M,
             bias=ctx.inp_flat(bp, name="bias"), out_kind=ops.OUT_GEGLU)

    def ref():
        h = a @ w.t() + b
        return {"out": (h[:, :inner] * F.gelu(h[:, inner:]), TOL_F16)}
    return ctx.ref(ref)


@gemm_case("gemm_frame_alpha_blend")
def _(ctx):
    from gcd_amd import ops
    M, N, K, rows = 300, 160, 128, 48             # 6.25 frames of 48 rows: the last frame is cut, no tile holds whole frames
    c, d = _plain_operands(ctx, M, N, K, 5, rows)
    out = ctx.out("out", M, N, F32)
    out16 = ctx.out("out16", M, N, F16)
    res = ctx.out("resblock", M, N, F32)
    kw = dict(M=M, bias=d["bias"], r1=d["r1"], frame_alpha=d["alpha"], rows_per_alpha=rows)
    ops.gemm(d["a"], d["w"], out, r2=d["r2"], r1_blend=True, **kw)
    ops.gemm(d["a"], d["w"], out16, r2=d["r2"], r1_blend=True, out_kind=ops.OUT_F16, **kw)
    ops.gemm(d["a"], d["w"], res, r1_blend=False, **kw)

    def ref():
        al = c["alpha"].repeat_interleave(rows)[:M, None]
        acc = c["a"] @ c["w"].t() + c["bias"]
        blend = al * c["r2"] + (1 - al) * (acc + c["r1"])
        return {"out": (blend, TOL_F32), "out16": (blend, TOL_F16), "resblock": (c["r1"] + (1 - al) * acc, TOL_F32)}
    return ctx.ref(ref)


@gemm_case("gemm_split_k_poisoned_workspace", impls=("auto",))
def _(ctx):
    from gcd_amd import ops
    M, N, K = 300, 352, 7680                      # 2 x 2 tiles, K / 4 = 1920: four K slices through the fp32 scratch
    c, d = _plain_operands(ctx, M, N, K, 6)
    out = ctx.out("out", M, N, F32)
    ws = ctx.scratch(4 * M * N, F32, name="split-K workspace")
    ops.gemm(d["a"], d["w"], out, M=M, bias=d["bias"], r1=d["r1"], workspace=ws)
    # and through the persistent scratch of the inference engine, dirtied between the runs
    out2 = ctx.out("out_persistent_ws", M, N, F32)
    ctx.dirty(ops._splitk_ws(ctx.device))
    ops.gemm(d["a"], d["w"], out2, M=M, bias=d["bias"], r1=d["r1"])
    return ctx.ref(lambda: {k: (c["a"] @ c["w"].t() + c["bias"] + c["r1"], TOL_F32) for k in ("out", "out_persistent_ws")})


@gemm_case("gemm_bf16_operands", entries=("gemm", "cast_bf16"))
def _(ctx):
    from gcd_amd import ops
    g = _gen(51)
    M, N, K = 77, 48, 64
    a32, w32 = torch.randn(M, K, generator=g) * 3, torch.randn(N, K, generator=g) / math.sqrt(K)
    bias, r1 = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    a = ctx.out("a_bf16", M, K, BF16)
    ops.cast_bf16(ctx.inp(a32, name="a32"), a)                         # fp32 -> bf16
    w = ctx.out_flat("w_bf16", (N, K), BF16)
    ops.cast_bf16(ctx.inp(w32, dtype=F16, name="w16"), w)               # fp16 -> bf16
    out = ctx.out("out", M, N, F32)
    ops.gemm(a, w, out, M=M, bias=ctx.inp_flat(bias, name="bias"), r1=ctx.inp(r1, name="r1"), operand_bf16=True)

    def ref():
        ab, wb = a32.to(BF16), w32.half().to(BF16)
        return {"a_bf16": (ab.float(), 1e-30), "w_bf16": (wb.float(), 1e-30),
                "out": (ab.float() @ wb.float().t() + bias + r1, TOL_F32)}
    return ctx.ref(ref)


def _colsum_ref(out, rows=64):
    b = out.double().reshape(out.shape[0] // rows, rows, out.shape[1])
    return torch.stack([b.sum(1), (b * b).sum(1)], 1).reshape(-1, out.shape[1])


@gemm_case("gemm_colstats", impls=("tile256x320", "ring32"))
def _(ctx):
    from gcd_amd import ops
    M, N, K = 768, 320, 64
    c, d = _plain_operands(ctx, M, N, K, 31)
    out = ctx.out("out", M, N, F32)
    kw = dict(M=M, bias=d["bias"], r1=d["r1"])
    assert ops.gemm(d["a"], d["w"], out, probe_colstats=True, **kw), "gcd_gemm_colstats_supported says no"
    cs = ctx.out_flat("colstats", (2 * (M // 64), N), F32)
    ops.gemm(d["a"], d["w"], out, colstats=cs, **kw)

    def ref():
        torch.cuda.synchronize()
        return {"out": (c["a"] @ c["w"].t() + c["bias"] + c["r1"], TOL_F32),
                "colstats": (_colsum_ref(out.cpu()), 2e-6)}          # sums of what was actually stored
    return ctx.ref(ref)


@gemm_case("gemm_colstats_conv3x3_rowvec", impls=("tile256x320", "ring32"))
def _(ctx):
    from gcd_amd import ops, packing
    g = _gen(33)
    frames, H, W, Cin, N = 3, 16, 32, 64, 320            # H * W = 512: the per-frame vector is constant over every tile
    M = frames * H * W
    x = _h(torch.randn(frames, Cin, H, W, generator=g))
    wt = _h(torch.randn(N, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin))
    bias, rv = torch.randn(N, generator=g), torch.randn(frames, N, generator=g)
    out = ctx.out("out", M, N, F32)
    kw = dict(M=M, mode=ops.GEMM_CONV3X3, bias=ctx.inp_flat(bias, name="bias"), rowvec=ctx.inp(rv, name="rowvec"),
              rows_per_vec=H * W, conv=dict(Cin=Cin, Hi=H, Wi=W, Ho=H, Wo=W, stride=1, upsample=0))
    A_, Wp = ctx.inp(x.permute(0, 2, 3, 1).reshape(M, Cin), dtype=F16, name="A"), ctx.inp_flat(packing.pack_conv3x3(wt), dtype=F16, name="W")
    assert ops.gemm(A_, Wp, out, probe_colstats=True, **kw), "gcd_gemm_colstats_supported says no"
    cs = ctx.out_flat("colstats", (2 * (M // 64), N), F32)
    ops.gemm(A_, Wp, out, colstats=cs, **kw)

    def ref():
        torch.cuda.synchronize()
        y = (F.conv2d(x, wt, bias, padding=1) + rv[:, :, None, None]).permute(0, 2, 3, 1).reshape(M, N)
        return {"out": (y, TOL_F32), "colstats": (_colsum_ref(out.cpu()), 2e-6)}
    return ctx.ref(ref)


def _conv_case(ctx, frames, H, W, Cin, Cout, stride, up, seed, res=0, cin_real=None):
    from gcd_amd import ops, packing
    g = _gen(seed)
    creal = cin_real or Cin
    x = _h(torch.randn(frames, creal, H, W, generator=g))
    w = _h(torch.randn(Cout, creal, 3, 3, generator=g) / math.sqrt(9 * creal))
    b = torch.randn(Cout, generator=g)
    Ho, Wo = (2 * H, 2 * W) if up else ((H - 1) // stride + 1, (W - 1) // stride + 1)
    M = frames * Ho * Wo
    emb = torch.randn(frames, Cout, generator=g)
    r1 = torch.randn(M, Cout, generator=g)
    a = torch.zeros(frames * H * W, Cin)
    a[:, :creal] = x.permute(0, 2, 3, 1).reshape(frames * H * W, creal)
    out = ctx.out("out", M, Cout, F32)
    kw = dict(r1=ctx.inp(r1, name="r1")) if res else {}
    ops.gemm(ctx.inp(a, dtype=F16, name="A (token-major image)"),
             ctx.inp_flat(packing.pack_conv3x3(w, cin_pad=Cin if cin_real else 0), dtype=F16, name="W"), out, M=M,
             mode=ops.GEMM_CONV3X3, bias=ctx.inp_flat(b, name="bias"), rowvec=ctx.inp(emb, name="rowvec"),
             rows_per_vec=Ho * Wo, conv=dict(Cin=Cin, Hi=H, Wi=W, Ho=Ho, Wo=Wo, stride=stride, upsample=up), **kw)

    def ref():
        xin = F.interpolate(x, scale_factor=2, mode="nearest") if up else x
        y = F.conv2d(xin, w, b, stride=stride, padding=1) + emb[:, :, None, None]
        y = y.permute(0, 2, 3, 1).reshape(M, Cout)
        return {"out": (y + r1 if res else y, TOL_F32)}
    return ctx.ref(ref)


# W odd, H * W not a multiple of 64: halo / tail rows of the A panel fall into the guard rows
for _cid, _args in {"conv3x3_stride1": (2, 9, 7, 128, 320, 1, 0, 5), "conv3x3_stride2": (2, 9, 7, 64, 64, 2, 0, 6),
                    "conv3x3_fused_x2_up": (2, 5, 7, 128, 64, 1, 1, 7),
                    "conv3x3_halo_panel": (3, 4, 64, 64, 320, 1, 0, 8, 1),
                    "conv3x3_padded_channels": (2, 7, 9, 64, 64, 1, 0, 9, 0, 8)}.items():
    gemm_case(_cid)(lambda ctx, _a=_args: _conv_case(ctx, *_a))


@case("conv3x3_narrow_head", ("gemm", "conv3x3_narrow"))
def _(ctx):
    from gcd_amd import ops, packing
    g = _gen(31)
    frames, Cin, H, W = 5, 64, 7, 13              # 455 pixels: not a multiple of the 256-pixel task
    x = _h(torch.randn(frames, Cin, H, W, generator=g))
    w = _h(torch.randn(4, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin))
    b = torch.zeros(16)
    b[:4] = torch.randn(4, generator=g)
    M = frames * H * W
    a = x.permute(0, 2, 3, 1).reshape(M, Cin)
    out = ctx.out("out", M, 16, F32)
    ops.gemm(ctx.inp(a, dtype=F16, name="A"), ctx.inp_flat(packing.pack_conv3x3(w, cout_pad=16), dtype=F16, name="W"), out,
             M=M, mode=ops.GEMM_CONV3X3, bias=ctx.inp_flat(b, name="bias"),
             conv=dict(Cin=Cin, Hi=H, Wi=W, Ho=H, Wo=W, stride=1, upsample=0))

    def ref():
        y = torch.zeros(M, 16)
        y[:, :4] = F.conv2d(x, w, b[:4], padding=1).permute(0, 2, 3, 1).reshape(M, 4)
        return {"out": (y, TOL_F32)}
    return ctx.ref(ref)


def _temporal_case(ctx, clips, T, HW, C):
    from gcd_amd import ops, packing
    g = _gen(7 + T)
    x = _h(torch.randn(clips, C, T, HW, 1, generator=g))
    w = _h(torch.randn(C, C, 3, 1, 1, generator=g) / math.sqrt(3 * C))
    b = torch.randn(C, generator=g)
    M = clips * T * HW
    a = x[..., 0].permute(0, 2, 3, 1).reshape(M, C)
    out = ctx.out("out", M, C, F32)
    ops.gemm(ctx.inp(a, dtype=F16, name="A"), ctx.inp_flat(packing.pack_conv_t3(w), dtype=F16, name="W"), out, M=M,
             mode=ops.GEMM_TEMPORAL3, bias=ctx.inp_flat(b, name="bias"), conv=dict(Cin=C, T=T, HW=HW))
    return ctx.ref(lambda: {"out": (F.conv3d(x, w, b, padding=(1, 0, 0))[..., 0].permute(0, 2, 3, 1).reshape(M, C),
                                    TOL_F32)})


for _T, _clips, _HW in [(1, 3, 37), (5, 2, 12), (14, 2, 23)]:
    gemm_case(f"conv_temporal3_T{_T}")(lambda ctx, _a=(_clips, _T, _HW, 64): _temporal_case(ctx, *_a))


# ------------------------------------------------------------------------------------- the two fused C = 320 kernels
def _ff_weights(g, for_ln, ctx):
    from gcd_amd import ops, packing
    C, H = 320, 1280
    w1 = _h(torch.randn(2 * H, C, generator=g) / math.sqrt(C))
    b1 = torch.randn(2 * H, generator=g) * 0.5
    w2 = _h(torch.randn(C, H, generator=g) / math.sqrt(H))
    b2 = torch.randn(C, generator=g)
    w1p, b1p = packing.pack_geglu(w1.to(ctx.device), b1.to(ctx.device))
    wp = ops.ff_pack(w1p, w2.half().to(ctx.device), for_ln=for_ln)
    return w1, b1, w2, b2, ctx.inp_flat(wp.cpu(), name="wp"), ctx.inp_flat(b1p.cpu(), name="b1"), ctx.inp_flat(b2, name="b2")


def _ff_ref(xn, w1, b1, w2, b2):
    h = xn @ w1.t() + b1
    return _h(h[:, :1280] * F.gelu(h[:, 1280:])) @ w2.t() + b2


def _ff_case(ctx, M, form):
    from gcd_amd import ops
    g = _gen(611)
    C = 320
    x = _h(torch.randn(M, C, generator=g))
    w1, b1, w2, b2, wp, b1p, b2g = _ff_weights(g, False, ctx)
    r1, r2 = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g)
    rpa = 2048 if form == "blend32" else 1024
    alpha = torch.rand((M + rpa - 1) // rpa, generator=g)
    xg, r1g = ctx.inp(x, dtype=F16, name="X"), ctx.inp(r1, name="R1")
    if form == "plain":
        out = ctx.out("out", M, C, F32)
        ops.ff_fused(xg, wp, b1p, b2g, out, M=M, r1=r1g)
        inpl = ctx.out("in_place", M, C, F32, init=r1)         # as the engine calls it: out aliases the residual
        ops.ff_fused(xg, wp, b1p, b2g, inpl, M=M, r1=inpl)
    else:
        f16 = form == "blend16"
        out = ctx.out("out", M, C, F16 if f16 else F32)
        ops.ff_fused(xg, wp, b1p, b2g, out, M=M, r1=r1g, r2=ctx.inp(r2, name="R2"),
                     out_kind=ops.OUT_F16 if f16 else ops.OUT_F32, frame_alpha=ctx.inp_flat(alpha, name="frame_alpha"),
                     rows_per_alpha=rpa)

    def ref():
        ff = _ff_ref(x, w1, b1, w2, b2)
        if form == "plain":
            return {"out": (ff + r1, 3e-4), "in_place": (ff + r1, 3e-4)}
        a = alpha.repeat_interleave(rpa)[:M, None]
        return {"out": ((1 - a) * (ff + r1) + a * r2, TOL_F16 if form == "blend16" else 3e-4)}
    return ctx.ref(ref)


# 128-token tiles on a persistent grid, stores through buffer resources: rule 1 is a test of num_records
for _M, _form in [(1, "plain"), (5, "plain"), (128 * 256 + 77, "plain"), (4096 + 77, "blend32"), (2048 + 5, "blend16")]:
    case(f"ff_fused_{_form}_M{_M}", ("ff_fused", "ff_pack"))(lambda ctx, _a=(_M, _form): _ff_case(ctx, *_a))


def _ff_ln_case(ctx, M, form):
    from gcd_amd import ops
    g = _gen(612)
    C, rpv = 320, 1024
    x = torch.randn(M, C, generator=g) * 1.5 + 0.3
    w1, b1, w2, b2, wp, b1p, b2g = _ff_weights(g, True, ctx)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g) * 0.5
    r2 = torch.randn(M, C, generator=g)
    nvec = (M + rpv - 1) // rpv
    pos, alpha = torch.randn(nvec, C, generator=g) * 0.7, torch.rand(nvec, generator=g)
    ln = dict(gamma=ctx.inp_flat(gamma, name="ln_gamma"), beta=ctx.inp_flat(beta, name="ln_beta"))
    if form != "plain":
        ln.update(addvec=ctx.inp(pos, name="addvec"), rows_per_vec=rpv)
    f16 = form == "blend16"
    kw = dict(r2=ctx.inp(r2, name="R2"), out_kind=ops.OUT_F16, frame_alpha=ctx.inp_flat(alpha, name="frame_alpha"),
              rows_per_alpha=rpv) if f16 else {}
    out = ctx.out("out", M, C, F16 if f16 else F32)
    ops.ff_fused(ctx.inp(x, name="x32"), wp, b1p, b2g, out, M=M, ln=ln, **kw)
    if form == "plain":
        inpl = ctx.out("in_place", M, C, F32, init=x)
        ops.ff_fused(inpl, wp, b1p, b2g, inpl, M=M, ln=ln)

    def ref():
        z = x + pos.repeat_interleave(rpv, 0)[:M] if form != "plain" else x
        ff = _ff_ref(_h(F.layer_norm(z, (C,), gamma, beta, 1e-5)), w1, b1, w2, b2)
        if f16:
            a = alpha.repeat_interleave(rpv)[:M, None]
            return {"out": ((1 - a) * (ff + z) + a * r2, TOL_F16)}
        return {"out": (ff + z, 3e-4), **({"in_place": (ff + z, 3e-4)} if form == "plain" else {})}
    return ctx.ref(ref)


for _M, _form in [(5, "plain"), (128 * 256 + 77, "plain"), (2048 + 77, "pos"), (2048 + 5, "blend16")]:
    case(f"ff_fused_layernorm_{_form}_M{_M}", ("ff_fused", "ff_pack"))(lambda ctx, _a=(_M, _form): _ff_ln_case(ctx, *_a))


def _lnqkv_case(ctx, M, ld):
    from gcd_amd import ops
    g = _gen(77)
    C, N = 320, 960
    x = torch.randn(M, C, generator=g) * 1.3 + 0.4
    w = _h(torch.randn(N, C, generator=g) / math.sqrt(C))
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g) * 0.5
    wp = ops.lnqkv_pack(w.half().to(ctx.device))
    out = ctx.out("out", M, N, F16)
    rev = ctx.out("reverse_walk", M, N, F16)
    xv = ctx.inp(x, pad=ld - C, name="x32")
    gg, bg, wpg = ctx.inp_flat(gamma, name="gamma"), ctx.inp_flat(beta, name="beta"), ctx.inp_flat(wp.cpu(), name="wp")
    ops.lnqkv(xv, gg, bg, wpg, out, M=M, N=N)
    ops.lnqkv(xv, gg, bg, wpg, rev, M=M, N=N, sched=1)

    def ref():
        r = _h(F.layer_norm(x, (C,), gamma, beta, 1e-5)) @ w.t()
        return {"out": (r, TOL_F16), "reverse_walk": (r, TOL_F16)}
    return ctx.ref(ref)


for _M, _ld in [(5, 324), (256 * 70 + 77, 324), (1000, 384)]:
    case(f"lnqkv_M{_M}_ld{_ld}", ("lnqkv", "lnqkv_pack"))(lambda ctx, _a=(_M, _ld): _lnqkv_case(ctx, *_a))


# ------------------------------------------------------------------------------------------------ small-M Linear
def _smallm_case(ctx, M, N, K):
    from gcd_amd import ops
    g = _gen(12)
    x, w, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K), torch.randn(N, generator=g)
    y0 = torch.randn(M, N, generator=g)
    xg, wg, bg = ctx.inp(x, name="x"), ctx.inp_flat(w, name="w"), ctx.inp_flat(b, name="b")
    acc = ctx.out("accumulate", M, N, F32, init=y0)              # documented accumulate-into: old + contribution
    ops.linear_smallm(xg, wg, bg, acc, silu_in=True, silu_out=True, accumulate=True)
    y = ctx.out("y", M, N, F32)
    ops.linear_smallm(xg, wg, None, y)
    return ctx.ref(lambda: {"accumulate": (y0 + F.silu(F.linear(F.silu(x), w, b)), 1e-5), "y": (F.linear(x, w), 1e-5)})


for _M, _N, _K in [(5, 33, 20), (33, 64, 128), (28, 1280, 320), (14, 4101, 260), (5, 4096, 516)]:      # N >= 4096: the MFMA kernel
    case(f"linear_smallm_{_M}x{_N}x{_K}", ("linear_smallm",))(lambda ctx, _a=(_M, _N, _K): _smallm_case(ctx, *_a))


# -------------------------------------------------------------------------------------------------------- norms
def _layernorm_case(ctx, M, C, order):
    from gcd_amd import ops
    g = _gen(9)
    x = torch.randn(M, C, generator=g) * 2 + 0.5
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    rpv = 10
    add = torch.randn((M + 9) // 10, C, generator=g)
    xg, gg, bg = ctx.inp(x, name="x"), ctx.inp_flat(gamma, name="gamma"), ctx.inp_flat(beta, name="beta")
    y, s = ctx.out("y", M, C, F16), ctx.out("sum_out", M, C, F32)
    ops.layernorm(xg, gg, bg, y, addvec=ctx.inp(add, name="addvec"), rows_per_vec=rpv, sum_out=s, order=order)
    yb = ctx.out("y_no_addvec", M, C, F16)
    ops.layernorm(xg, gg, bg, yb, order=order)

    def ref():
        xs = x + add.repeat_interleave(rpv, 0)[:M]
        return {"y": (F.layer_norm(xs, (C,), gamma, beta, 1e-5), TOL_F16), "sum_out": (xs, 1e-6),
                "y_no_addvec": (F.layer_norm(x, (C,), gamma, beta, 1e-5), TOL_F16)}
    return ctx.ref(ref)


for _M, _C, _order in [(77, 640, 0), (1000, 320, 1), (70, 1280, 2), (16 * 1024 + 37, 320, 3)]:
    case(f"layernorm_M{_M}_C{_C}_order{_order}", ("layernorm",))(lambda ctx, _a=(_M, _C, _order): _layernorm_case(ctx, *_a))


def _groupnorm_case(ctx, frames, HW, C1, C2, per_clip_T, order):
    from gcd_amd import ops
    g = _gen(8)
    C = C1 + C2
    x = torch.randn(frames, C, HW, generator=g) * 3 + 1.5
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    eps = 1e-5
    rows = per_clip_T * HW if per_clip_T else HW
    tok = x.permute(0, 2, 1).reshape(frames * HW, C)
    x1 = ctx.inp(tok[:, :C1], name="x1")
    x2 = ctx.inp(tok[:, C1:], name="x2") if C2 else None
    nch = ops.gn_nchunks(rows)
    ninst = frames * HW // rows
    partial = ctx.scratch(ninst * nch * 64, F64, name="partial")
    stats = ctx.out_flat("stats", (ninst * 64,), F32)
    ops.groupnorm_stats(x1, x2, rows, eps, partial, stats, nch)
    y, raw = ctx.out("y", frames * HW, C, F16), ctx.out("raw16", frames * HW, C, F16)
    ops.groupnorm_apply(x1, x2, rows, stats, ctx.inp_flat(gamma, name="gamma"), ctx.inp_flat(beta, name="beta"), True, y, raw,
                        order=order)

    def ref():
        if per_clip_T:
            xr = x.reshape(frames // per_clip_T, per_clip_T, C, HW).permute(0, 2, 1, 3)
            r = F.group_norm(xr, 32, gamma, beta, eps).permute(0, 2, 1, 3).reshape(frames, C, HW)
        else:
            r = F.group_norm(x, 32, gamma, beta, eps)
        xg = x.double().reshape(ninst, rows // HW, 32, C // 32, HW)          # instance, frame, group, channel, pixel
        mean, rstd = xg.mean((1, 3, 4)), 1.0 / torch.sqrt(xg.var((1, 3, 4), unbiased=False) + eps)
        return {"y": (F.silu(r).permute(0, 2, 1).reshape(frames * HW, C), TOL_F16), "raw16": (tok, TOL_F16),
                "stats": (torch.stack([mean, rstd], -1).reshape(1, -1), 1e-5)}       # (mean, rstd) per group, as from_colsums
    return ctx.ref(ref)


for _a in [(4, 37, 64, 0, 0, 0), (3, 65, 640, 320, 0, 1), (4, 50, 128, 0, 2, 2), (2, 300, 320, 64, 0, 3)]:
    case("groupnorm_%dx%d_C%d+%d_T%d_order%d" % _a, ("groupnorm_stats", "groupnorm_apply"))(
        lambda ctx, _a=_a: _groupnorm_case(ctx, *_a))


@case("groupnorm_stats_from_colsums_virtual_concat", ("groupnorm_stats_from_colsums",))
def _(ctx):
    from gcd_amd import ops
    g = _gen(32)
    frames, HW, C1, C2 = 3, 128, 640, 320
    M = frames * HW
    x = torch.randn(M, C1 + C2, generator=g) * 2 + torch.randn(C1 + C2, generator=g)
    cs1 = ctx.inp_flat(_colsum_ref(x[:, :C1]).float(), name="cs1")
    cs2 = ctx.inp_flat(_colsum_ref(x[:, C1:]).float(), name="cs2")
    stats = ctx.out_flat("stats", (frames * 64,), F32)
    ops.groupnorm_stats_from_colsums(cs1, C1, cs2, C2, M, HW, 1e-6, stats)

    def ref():
        xg = x.double().reshape(frames, HW, 32, (C1 + C2) // 32)
        mean, rstd = xg.mean((1, 3)), 1.0 / torch.sqrt(xg.var((1, 3), unbiased=False) + 1e-6)
        return {"stats": (torch.stack([mean, rstd], -1).reshape(-1), 1e-5)}
    return ctx.ref(ref)


# ---------------------------------------------------------------------------------------------------- attention
def _attn_spatial_case(ctx, impl, frames, S, heads):
    from gcd_amd import ops
    g = _gen(10)
    C = heads * 64
    qkv = _h(torch.randn(frames * S, 3 * C, generator=g) * 1.5)
    if S >= 100:
        qkv[70, C:C + 64] *= 6.0                  # a spiked key: the online-softmax rescale path
    S_pad = (S + 63) // 64 * 64
    qg = ctx.inp(qkv, dtype=F16, name="qkv")      # rows past frames * S: the guard (keys past S of the last frame)
    vt = ctx.out_flat("vt", (frames * heads * 64, S_pad), F16)
    out = ctx.out("out", frames * S, C, F16, pad=4)               # ldo % 4 is what the entry asks for
    ops.tune_set(ops.TUNE_ATTN_IMPL, impl)
    try:
        ops.attn_transpose_v(qg, frames, S, heads, vt, S_pad)
        ops.attn_spatial(qg, vt, S_pad, out, frames, S, heads)
        torch.cuda.synchronize()
    finally:
        ops.tune_set(ops.TUNE_ATTN_IMPL, 0)

    def ref():
        q, k, v = [t.reshape(frames, S, heads, 64).permute(0, 2, 1, 3) for t in qkv.split(C, dim=1)]
        r = F.scaled_dot_product_attention(q.double(), k.double(), v.double())
        vt_ref = torch.zeros(frames, heads, 64, S_pad)
        vt_ref[..., :S] = v.permute(0, 1, 3, 2)
        perm = torch.arange(S_pad).reshape(-1, 4, 4)[:, [0, 2, 1, 3]].reshape(-1)     # 16-key groups as 0-3, 8-11, 4-7, 12-15
        return {"out": (r.permute(0, 2, 1, 3).reshape(frames * S, C).float(), 1.5e-3),
                "vt": (vt_ref[..., perm].reshape(frames * heads * 64, S_pad), 1e-30)}  # columns S..S_pad: written as zeros
    return ctx.ref(ref)


for _name, _impl in _ATTN.items():
    for _frames, _S, _heads in [(2, 4, 1), (2, 100, 3), (2, 144, 2), (1, 1300, 1)]:
        case(f"attn_spatial_S{_S}[{_name}]", ("attn_transpose_v", "attn_spatial"))(
            lambda ctx, _a=(_impl, _frames, _S, _heads): _attn_spatial_case(ctx, *_a))


def _attn_temporal_case(ctx, kernel, clips, T, HW, heads):
    from gcd_amd import ops
    g = _gen(11)
    C = heads * 64
    M = clips * T * HW
    qkv = _h(torch.randn(M, 3 * C, generator=g) * 1.5)
    out = ctx.out("out", M, C, F16, pad=4 if kernel == "long" else 8)      # ldo % 4 (long) / % 8: what each entry asks for
    ops.tune_set(ops.TUNE_ATTN_IMPL, 16 if kernel == "valu" else 0)
    try:
        ops.attn_temporal(ctx.inp(qkv, dtype=F16, name="qkv"), out, clips, T, HW, heads)
        torch.cuda.synchronize()
    finally:
        ops.tune_set(ops.TUNE_ATTN_IMPL, 0)

    def ref():
        q, k, v = [t.reshape(clips, T, HW, heads, 64).permute(0, 2, 3, 1, 4) for t in qkv.split(C, dim=1)]
        r = F.scaled_dot_product_attention(q.double(), k.double(), v.double())
        return {"out": (r.permute(0, 3, 1, 2, 4).reshape(M, C).float(), TOL_F16)}
    return ctx.ref(ref)


# clips * HW * heads problems: never a multiple of the waves per workgroup / of the 4 problems a VALU wave holds
for _kernel, _shapes in {"mfma": [(2, 14, 7, 3), (1, 4, 33, 1), (1, 1, 5, 1)], "valu": [(2, 14, 7, 3), (1, 4, 33, 1), (1, 1, 5, 1)],
                         "long": [(1, 17, 7, 3), (2, 33, 5, 1), (1, 64, 3, 1)]}.items():
    for _s in _shapes:
        case(f"attn_temporal_{_kernel}_T{_s[1]}_HW{_s[2]}", ("attn_temporal",))(
            lambda ctx, _a=(_kernel,) + _s: _attn_temporal_case(ctx, *_a))


# ------------------------------------------------------------------------------------------------- small pieces
@case("softmax_rows", ("softmax_rows",))
def _(ctx):
    from gcd_amd import ops
    g = _gen(130)
    R, C = 37, 1300                               # 1300 = 5 x 256 + 20: the row loop's tail
    x = torch.randn(R, C, generator=g) * 4.0
    x[0] += 30.0 * torch.randn(C, generator=g)
    y = ctx.out("y", R, C, F16, pad=4)
    ops.softmax_rows(ctx.inp(x, name="x"), y)
    return ctx.ref(lambda: {"y": (torch.softmax(x.double(), -1), ("maxabs", 6e-4))})


def _transpose_case(ctx, R, C):
    from gcd_amd import ops
    x = _h(torch.randn(R, C, generator=_gen(R)))
    y = ctx.out("y", C, R, F16)
    ops.transpose_f16(ctx.inp(x, dtype=F16, name="x"), y)
    return ctx.ref(lambda: {"y": (x.t(), 1e-30)})


for _R, _C in [(33, 130), (112, 72)]:            # the scalar kernel, and the vector kernel (R % 16 == 0, C % 8 == 0) on ragged 64-tiles
    case(f"transpose_f16_{_R}x{_C}", ("transpose_f16",))(lambda ctx, _a=(_R, _C): _transpose_case(ctx, *_a))


@case("time_mix_unpack", ("time_mix_unpack",))
def _(ctx):
    from gcd_amd import ops
    C, clips, T, HW = 3, 2, 3, 101
    g = _gen(C * 100 + T)
    N = clips * T
    tok = torch.randn(N * HW, C, generator=g)
    w, b = torch.randn(C, C, 3, 1, 1, generator=g), torch.randn(C, generator=g)
    out = ctx.out_flat("out", (N, C, HW), F32)
    ops.time_mix_unpack(ctx.inp(tok, pad=1, name="tok"), ctx.inp_flat(w.reshape(C, C, 3), name="w"), ctx.inp_flat(b, name="b"),
                        out, C, N, T, HW)

    def ref():
        x5 = tok.reshape(clips, T, HW, 1, C).permute(0, 4, 1, 2, 3).double()
        r = F.conv3d(x5, w.double(), b.double(), padding=(1, 0, 0))
        return {"out": (r.permute(0, 2, 1, 3, 4).reshape(N, C * HW).reshape(1, -1), ("maxabs", 1e-5))}
    return ctx.ref(ref)


@case("pack_unpack_cast", ("pack_input", "unpack_output", "cast_f16", "cast_bf16"))
def _(ctx):
    from gcd_amd import ops
    g = _gen(13)
    nx, N, H, W = 3, 6, 5, 7
    x, cc = torch.randn(nx, 4, H, W, generator=g), torch.randn(N, 4, H, W, generator=g)
    c_in = torch.rand(N, generator=g) + 0.5
    # gcd_pack_input takes no row stride (out16 is a dense [N * HW, Cpad]): only the row guards apply
    packed = ctx.out("packed", N * H * W, 64, F16, pad=0)
    ops.pack_input(ctx.inp_flat(x, name="x"), ctx.inp_flat(cc, name="concat"), ctx.inp_flat(c_in, name="c_in"), N, H * W,
                   packed, 64)
    tok = torch.randn(N * H * W, 16, generator=g)
    nchw = ctx.out_flat("nchw", (N, 4, H, W), F32)
    ops.unpack_output(ctx.inp(tok, name="tok"), nchw, 4, N, H * W)
    x32 = torch.randn(101, 72, generator=g)
    y16, yb = ctx.out("cast_f16", 101, 72, F16), ctx.out("cast_bf16", 101, 72, BF16)
    xg = ctx.inp(x32, name="x32")
    ops.cast_f16(xg, y16)
    ops.cast_bf16(xg, yb)

    def ref():
        p = torch.zeros(N, H * W, 64)
        p[:, :, :4] = (x.repeat(2, 1, 1, 1) * c_in[:, None, None, None]).permute(0, 2, 3, 1).reshape(N, H * W, 4)
        p[:, :, 4:8] = cc.permute(0, 2, 3, 1).reshape(N, H * W, 4)
        return {"packed": (p.reshape(-1, 64).half().float(), 1e-30),
                "nchw": (tok[:, :4].reshape(N, H, W, 4).permute(0, 3, 1, 2).reshape(1, -1), 1e-30),
                "cast_f16": (x32.half().float(), 1e-30), "cast_bf16": (x32.to(BF16).float(), 1e-30)}
    return ctx.ref(ref)


@case("sampler_kernels", ("cfg_euler_step", "edm_scalings", "timestep_embedding"))
def _(ctx):
    from gcd_amd import ops
    g = _gen(14)
    nx, T = 4, 2
    x = torch.randn(nx, 4, 7, 9, generator=g) * 50           # 252 elements per sample: not a multiple of 8
    net = torch.randn(2 * nx, 4, 7, 9, generator=g)
    scale = torch.tensor([1.0, 1.5])
    sigma, sigma_next = 37.5, 21.0
    sig = ctx.inp_flat(torch.tensor([sigma, sigma_next]), name="sig")
    out = ctx.out_flat("x_out", (nx, 4, 7, 9), F32)
    ops.cfg_euler_step(ctx.inp_flat(x, name="x"), ctx.inp_flat(net, name="net"), ctx.inp_flat(scale, name="scale"), sig, out, T)
    c_in, c_noise = ctx.out_flat("c_in", (7,), F32), ctx.out_flat("c_noise", (7,), F32)
    ops.edm_scalings(sig, c_in, c_noise)
    t = torch.tensor([0.0, 1.6378, -1.55, 13.0, 2.5])
    emb = ctx.out_flat("emb", (5, 324), F32)
    ops.timestep_embedding(ctx.inp_flat(t, name="t"), emb)

    def ref():
        c_skip, c_out = 1 / (sigma ** 2 + 1), -sigma / math.sqrt(sigma ** 2 + 1)
        den = net * c_out + torch.cat([x, x]) * c_skip
        du, dc = den.chunk(2)
        d_ = du + scale.repeat(nx // T)[:, None, None, None] * (dc - du)
        half = 162
        freqs = torch.exp(-math.log(10000) * torch.arange(half, dtype=torch.float32) / half)
        args = t[:, None] * freqs[None]
        return {"x_out": ((x + (sigma_next - sigma) * ((x - d_) / sigma)).reshape(1, -1), 1e-5),
                "c_in": (torch.full((1, 7), 1 / math.sqrt(sigma ** 2 + 1)), 1e-6),
                "c_noise": (torch.full((1, 7), 0.25 * math.log(sigma)), 1e-6),
                "emb": (torch.cat([torch.cos(args), torch.sin(args)], -1).reshape(1, -1), ("maxabs", 2e-6))}
    return ctx.ref(ref)


# ------------------------------------------------------------------------------------------------------ the test
@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_forward_memory_contract(gpu, c):
    mc.run_contract(c, gpu)


# ------------------------------------------------------------------------------------------------ engine level
def _net(gpu, cfg, train=False):
    from gcd_amd.video_model import VideoUNet
    from oracle import weights
    with torch.device("meta"):
        net = VideoUNet(**cfg.as_reference_kwargs())
    sd = weights.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()})
    net = net.to_empty(device=gpu)
    net.load_state_dict(sd)
    return (net.train() if train else net.eval()), sd


def _two_clips(cfg, T, H, W, seed):
    from oracle import weights
    noise, c, _ = weights.synth_inputs(2, T, H, W, cfg.context_dim, cfg.adm_in_channels + cfg.aux_emb_dim, seed)
    ioi = torch.zeros(2, T)
    ioi[1, 1] = 1.0
    return torch.cat([noise, c["concat"]], 1), torch.linspace(-1.2, 1.4, 2 * T), c["crossattn"], c["vector"], ioi


def _engine_forward(net, gpu, x, ts, ctx, y, T, ioi):
    out = net(x.to(gpu), ts.to(gpu), context=ctx.to(gpu), y=y.to(gpu), num_video_frames=T, image_only_indicator=ioi.to(gpu))
    torch.cuda.synchronize()
    return out


def _poison_engine_scratch(net, gpu):
    """Between two runs every slab of the engine's workspace is free; so is the persistent split-K scratch."""
    from gcd_amd import ops
    ws = net.engine.ws
    assert ws is not None and ws.slabs
    for slab in ws.slabs:
        mc.poison_scratch(slab)
    for w in ops._splitk.values():
        mc.poison_scratch(w)
    torch.cuda.synchronize()
    return len(ws.slabs), ws.nbytes()


@pytest.mark.parametrize("levels,H,W", [(4, 8, 24), (1, 9, 13)], ids=["tiny_8x24", "tiny_one_level_9x13"])
def test_engine_replays_bit_identically_over_a_poisoned_workspace(gpu, levels, H, W):
    """UNetEngine (width 64, two clips) run twice with the same signature, every recycled slab of engine.ws and the
    split-K scratch NaN-filled in between: the second output is bit-identical (what the hipGraph replay design requires)
    and both meet the forward bar of test_unet_gpu.py against the oracle.  The four-level TINY network needs H, W
    divisible by 8 (8 x 24: 192, 48, 12 and 3 tokens per frame down the levels); a one-level network of the same width
    takes 9 x 13 = 117 tokens per frame, a multiple of no tile."""
    import dataclasses
    from conftest import rel_l2
    from oracle import svd_unet_ref as O
    cfg = O.TINY if levels == 4 else dataclasses.replace(O.TINY, channel_mult=(1,), attention_resolutions=(1,))
    net, sd = _net(gpu, cfg)
    T = 3
    x, ts, ctx, y, ioi = _two_clips(cfg, T, H, W, 91)
    with torch.no_grad():
        ref = O.unet_forward(sd, cfg, x, ts, ctx, y, T, ioi)
        first = _engine_forward(net, gpu, x, ts, ctx, y, T, ioi).clone()
        nslab, nbytes = _poison_engine_scratch(net, gpu)
        second = _engine_forward(net, gpu, x, ts, ctx, y, T, ioi)
    e = rel_l2(first, ref)
    print(f"engine {levels} level(s) {H}x{W}: {nslab} slabs / {nbytes >> 20} MiB poisoned, rel-L2 vs oracle {e:.3e}")
    assert not torch.isnan(second).any(), "poison from a recycled slab reached the output"
    assert torch.equal(first, second), "the replay over a poisoned workspace is not bit-identical"
    assert e < 2e-3                                # TOL_FWD of test_unet_gpu.py


@pytest.mark.parametrize("H,W", [(8, 16), (9, 13)], ids=["HW128", "HW117_not_a_multiple_of_32"])
def test_engine_reaches_the_fused_c320_kernels_at_small_shapes(gpu, monkeypatch, H, W):
    """ops.ff_fused / ops.lnqkv exist for model width 320 only and the engine takes them from ~10^5 tokens: with the token
    thresholds at 1, a one-level network of width 320 runs them at H x W = 8 x 16 (every form: plain, per-frame
    position vector, blended fp16 result; M = 768 = six 128-token tiles) and is held to the oracle; at 9 x 13 a frame is
    117 tokens, no multiple of the kernel's 32-row wave tile: the per-frame forms must FALL BACK to LayerNorm + GEMMs
    (not raise) and the result must still be right.  Workspace poisoned between two bit-identical runs, as above."""
    import dataclasses
    from conftest import rel_l2
    from gcd_amd import ops
    from oracle import svd_unet_ref as O
    cfg = dataclasses.replace(O.TINY, model_channels=320, channel_mult=(1,), attention_resolutions=(1,), num_res_blocks=1)
    monkeypatch.setattr(ops, "FF_FUSED_MIN_TOKENS", 1)
    monkeypatch.setattr(ops, "LNQKV_MIN_TOKENS", 1)
    calls = {"ff_fused": [], "lnqkv": 0}
    real_ff, real_qkv = ops.ff_fused, ops.lnqkv

    def spy_ff(*a, **k):
        ln = k.get("ln") or {}
        calls["ff_fused"].append("blend" if k.get("frame_alpha") is not None else "addvec" if ln.get("addvec") is not None else "plain")
        return real_ff(*a, **k)

    def spy_qkv(*a, **k):
        calls["lnqkv"] += 1
        return real_qkv(*a, **k)
    monkeypatch.setattr(ops, "ff_fused", spy_ff)
    monkeypatch.setattr(ops, "lnqkv", spy_qkv)
    net, sd = _net(gpu, cfg)
    T = 3
    x, ts, ctx, y, ioi = _two_clips(cfg, T, H, W, 92)
    with torch.no_grad():
        ref = O.unet_forward(sd, cfg, x, ts, ctx, y, T, ioi)
        first = _engine_forward(net, gpu, x, ts, ctx, y, T, ioi).clone()
        _poison_engine_scratch(net, gpu)
        second = _engine_forward(net, gpu, x, ts, ctx, y, T, ioi)
    e = rel_l2(first, ref)
    print(f"width-320 engine {H}x{W}: ff_fused forms {sorted(set(calls['ff_fused']))} x{len(calls['ff_fused'])}, "
          f"lnqkv x{calls['lnqkv']}, rel-L2 vs oracle {e:.3e}")
    assert calls["lnqkv"] > 0 and "plain" in calls["ff_fused"], "the engine did not reach the fused kernels"
    if H * W % 32 == 0:
        assert {"plain", "addvec", "blend"} <= set(calls["ff_fused"])
    else:
        assert set(calls["ff_fused"]) == {"plain"}, "per-frame forms with H * W % 32 != 0 must fall back"
    assert torch.equal(first, second)
    assert e < 2e-3                                # TOL_FWD of test_unet_gpu.py


def test_planned_finetune_step_over_poisoned_plan_buffers(gpu):
    """One planned fine-tune step (unet_forward_planned, TINY) three times; between the steps the plan's un-zeroed few-row
    storage, its per-step arena of accumulators (the plan zeroes it itself) and the persistent split-K / attention scratch
    are NaN-filled.  Gradients of steps 2 and 3 against step 1 within max(10 x run-to-run spread, 1e-6) (the atomicAdd
    reductions are order-dependent), the spread taken from two clean steps and printed."""
    from conftest import rel_l2
    from gcd_amd import autograd_ops as A, ops
    from gcd_amd.train_plan import plan_for, unet_forward_planned
    from oracle import svd_unet_ref as O
    net, _ = _net(gpu, O.TINY, train=True)
    T, H, W = 4, 16, 24
    g = _gen(41)
    s = dict(x=torch.randn(2 * T, 8, H, W, generator=g).to(gpu), ts=torch.linspace(-1.0, 1.5, 2 * T).to(gpu),
             ctx=torch.randn(2 * T, 1, O.TINY.context_dim, generator=g).to(gpu),
             y=torch.randn(2 * T, O.TINY.adm_in_channels + O.TINY.aux_emb_dim, generator=g).clamp(-1, 1).to(gpu),
             tgt=torch.randn(2 * T, 4, H, W, generator=g).to(gpu), ioi=torch.zeros(2, T, device=gpu))

    def step():
        for p in net.parameters():
            p.grad = None
        out = unet_forward_planned(net, s["x"], s["ts"], s["ctx"], s["y"], T, s["ioi"], use_checkpoint=False)
        ((out - s["tgt"]) ** 2).mean().mul(64.0).backward()
        torch.cuda.synchronize()
        return out.detach().clone(), {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}

    def poison():
        plan = plan_for(net)
        bufs = [plan._sbuf, plan._arena] + list(A._WS.values()) + list(A._ATTN_WS.values()) + list(ops._splitk.values())
        for b in bufs:
            mc.poison_scratch(b)
        torch.cuda.synchronize()
        return len(bufs)
    o1, g1 = step()
    _, g1b = step()
    repeats = [g1b, step()[1], step()[1]]         # three more clean steps: the spread of a 1-element atomic sum is noisy
    spread = max((rel_l2(g1b[n], g1[n]) for n in g1 if g1[n].numel() >= 64), default=0.0)
    bar = max(10 * spread, 1e-6)
    # tensors of fewer than 64 elements (the blend factors, the 4-channel output bias): the same rule on the largest
    # element-wise difference relative to the tensor's largest element (a rel-L2 of one or four numbers says little)
    small = [n for n in g1 if g1[n].numel() < 64]

    def dmax(x, y):
        return float((x.double() - y.double()).abs().max() / y.double().abs().max().clamp_min(1e-30))
    spread_small = max((dmax(r[n], g1[n]) for r in repeats for n in small), default=0.0)
    bar_small = max(10 * spread_small, 1e-6)
    assert len(g1) > 100
    for k in (2, 3):
        nb = poison()
        ok, gk = step()
        assert not torch.isnan(ok).any() and torch.equal(ok, o1), f"step {k}: the forward result changed"
        bad = [n for n in gk if torch.isnan(gk[n]).any()]
        assert not bad, f"step {k}: NaN gradients after poisoning {nb} buffers: {bad[:5]}"
        worst = max(((n, rel_l2(gk[n], g1[n])) for n in g1 if g1[n].numel() >= 64), key=lambda t: t[1])
        print(f"planned step {k} over {nb} poisoned buffers: run-to-run spread {spread:.2e}, worst tensor {worst[0]} "
              f"rel-L2 {worst[1]:.2e} (bar {bar:.2e})")
        assert set(gk) == set(g1) and worst[1] <= bar
        worst_small = max(((n, dmax(gk[n], g1[n])) for n in small), key=lambda t: t[1], default=("", 0.0))
        print(f"  {len(small)} tensors of < 64 elements: spread {spread_small:.2e}, worst {worst_small[0]} {worst_small[1]:.2e} "
              f"(bar {bar_small:.2e})")
        assert worst_small[1] <= bar_small


# ------------------------------------------------------------------------------------------------- sensitivity
def _case_by_id(cid):
    return next(c for c in CASES if c.id == cid)


class _Shrunk(mc.Ctx):
    """A Ctx that tells the harness a payload one row (and one column) smaller than the one the kernel is given: the
    correct kernel's legitimate last row / column then lands in what the harness takes for guard.  Nothing leaves the
    allocation and no kernel is changed."""
    shrink = {}

    def out(self, name, rows, cols, dtype, *, pad=None, init=None, overhang=(0, 0)):
        dr, dc = self.shrink.get(name, (0, 0))
        if dr or dc:
            assert init is None
            return super().out(name, rows - dr, cols - dc, dtype, pad=(mc.min_pad(dtype) if pad is None else pad) + dc,
                               overhang=(dr, dc))
        return super().out(name, rows, cols, dtype, pad=pad, init=init, overhang=overhang)


@pytest.mark.parametrize("cid,name,shrink,row,col", [
    ("gemm_f16_out[auto]", "out", (1, 0), 256, 0),                 # last row of a 257-row output
    ("layernorm_M77_C640_order0", "sum_out", (1, 1), 0, 639),      # strided output: last column of row 0 comes first
])
def test_harness_sees_a_correct_kernel_as_overrunning_a_smaller_payload(gpu, monkeypatch, cid, name, shrink, row, col):
    c = _case_by_id(cid)
    monkeypatch.setattr(_Shrunk, "shrink", {name: shrink})
    monkeypatch.setattr(mc, "Ctx", _Shrunk)
    with pytest.raises(mc.MemContractError) as ei:
        mc.run_contract(c, gpu)
    msg = str(ei.value)
    assert "write outside" in msg and f"(row {row}, col {col})" in msg and name in msg, msg
