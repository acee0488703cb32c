"""The memory contract of the training library (tests/memcontract.py; DESIGN.md "Memory contract").

Two levels.  The C-ABI wrappers of gcd_amd.autograd_ops, the exports of include/gcd_amd_train.h and the backward exports of
include/gcd_amd.h (GEGLU, spatial and both temporal attention backwards) are called directly with guarded, strided
operands; `*_zeroed` arguments get zeros there (that is the ABI).  The torch.autograd functions run
forward + backward once clean and once with a dirty allocator: every torch.empty the wrappers make returns NaN bytes
(mc.record_empty fills each one as it is handed out, and the case asserts that some were), so a torch.empty where a
kernel needs zeros fails here.  The persistent scratch (_train_ws, _attn_ws, ops._splitk_ws)
is NaN-filled between the clean and the poisoned run.  References: fp32 / fp64 torch on the CPU at the bars of
test_backward_gpu.py / test_train_plan_gpu.py.  The outputs written by one of the five fp32 atomicAdd reductions
(rowblock_sum, LayerNorm-backward affine sums, cast + column sums, blend d_alpha, small-M dgrad with flag 4) are named in
`atomic=` and held to the run-to-run spread rule; every other output, of the same case too, to bit equality.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import memcontract as mc

pytestmark = pytest.mark.gpu

TOL_OP = 3e-3           # test_backward_gpu.py
F16, F32, BF16, F64, U8 = torch.float16, torch.float32, torch.bfloat16, torch.float64, torch.uint8

CASES = []


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dirty_persistent(ctx):
    from gcd_amd import autograd_ops as A, ops
    for w in list(A._WS.values()) + list(A._ATTN_WS.values()) + list(ops._splitk.values()):
        ctx.dirty(w)


def case(cid, entries, alloc=False, **kw):
    """alloc: the entry allocates its own outputs / scratch with torch.empty: the poisoned run happens under the dirty
    allocator (mc.record_empty(poison=True)), and must have handed out at least one poisoned tensor."""
    def deco(fn):
        def run(ctx):
            _dirty_persistent(ctx)
            if not alloc or not ctx.poisoned:
                return fn(ctx)
            before = len(ctx.arenas)
            with mc.record_empty(poison=True) as rec:
                r = fn(ctx)
            assert len(rec.sizes) > len(ctx.arenas) - before, f"{cid}: no torch.empty of the wrappers was poisoned"
            return r
        CASES.append(mc.Case(cid, entries, run, **kw))
        return fn
    return deco


# --------------------------------------------------------------------------------------------- C-ABI level
def _wgrad_case(ctx, M, N, K, impl, dt):
    from gcd_amd import autograd_ops as A
    g = _gen(5)
    dy = (torch.randn(M, N, generator=g) * 0.5).to(dt)
    x = torch.randn(M, K, generator=g).to(dt)
    dyg, xg = ctx.inp(dy, name="dy16"), ctx.inp(x, name="x16")          # strided in both forms ("gemm": transposed copies)
    old = A.WGRAD_IMPL
    try:
        A.set_wgrad_impl(impl)
        ctx.also("dw", A._wgrad(dyg, xg))
        torch.cuda.synchronize()
    finally:
        A.set_wgrad_impl(old)
    return ctx.ref(lambda: {"dw": (dy.float().t() @ x.float(), 1e-4)})


for _impl, _M, _N, _K, _dt in [("tr", 1000, 208, 336, F16), ("tr", 100, 8, 24, F16), ("tr", 4099, 320, 640, BF16),
                               ("gemm", 1000, 208, 336, F16), ("gemm", 4099, 320, 640, F16)]:
    case(f"wgrad_{_impl}_{_M}x{_N}x{_K}_{'bf16' if _dt == BF16 else 'fp16'}",
         ("_wgrad", "gcd_wgrad_tr_f16", "gcd_wgrad_tr_scratch_floats"), alloc=True)(
        lambda ctx, _a=(_M, _N, _K, _impl, _dt): _wgrad_case(ctx, *_a))


@case("wgrad_ex_parameter_layout", ("_wgrad", "gcd_wgrad_tr_f16_ex"), alloc=True)
def _(ctx):
    from gcd_amd import autograd_ops as A
    g = _gen(7)
    taps, N, Nr, Cp, Cr = 9, 64, 40, 64, 8
    M, K = 1003, taps * Cp
    dy, x = (torch.randn(M, N, generator=g) * 0.5).half(), torch.randn(M, K, generator=g).half()
    dst = ctx.out_flat("dest", (Nr, Cr, taps), F32)
    A._wgrad(ctx.inp(dy, name="dy16"), ctx.inp(x, name="x16"), dest=dst, taps=taps, n_real=Nr, c_real=Cr)
    return ctx.ref(lambda: {"dest": ((dy.float().t() @ x.float()).reshape(N, taps, Cp).permute(0, 2, 1)[:Nr, :Cr], 1e-4)})


def _wgrad_conv_case(ctx, conv):
    from gcd_amd import autograd_ops as A
    g = _gen(61)
    if conv == 1:
        frames, H, W, Cin, Cp, Cout, N = 3, 7, 9, 8, 64, 40, 40
        x = torch.randn(frames, Cin, H, W, generator=g).half().float()
        dy = (torch.randn(frames, Cout, H, W, generator=g) * 0.5).half().float()
        xt = torch.zeros(frames * H * W, Cp)
        xt[:, :Cin] = x.permute(0, 2, 3, 1).reshape(-1, Cin)
        dyt = dy.permute(0, 2, 3, 1).reshape(-1, Cout)
        geo, taps = dict(Ho=H, Wo=W), 9
        ref = lambda: torch.nn.grad.conv2d_weight(x, (Cout, Cin, 3, 3), dy, padding=1).reshape(Cout, Cin, 9)   # noqa: E731
    else:
        clips, T, HW, Cin, Cout = 3, 14, 35, 72, 40
        x = torch.randn(clips, Cin, T, HW, 1, generator=g).half().float()
        dy = (torch.randn(clips, Cout, T, HW, 1, generator=g) * 0.5).half().float()
        xt, dyt = x.permute(0, 2, 3, 4, 1).reshape(-1, Cin), dy.permute(0, 2, 3, 4, 1).reshape(-1, Cout)
        geo, taps = dict(T=T, HW=HW), 3
        ref = lambda: torch.nn.grad.conv3d_weight(x, (Cout, Cin, 3, 1, 1), dy, padding=(1, 0, 0)).reshape(Cout, Cin, 3)   # noqa: E731
    dst = ctx.out_flat("dest", (Cout, Cin, taps), F32)
    A._wgrad_conv(ctx.inp(dyt, dtype=F16, name="dy16"), ctx.inp(xt, dtype=F16, name="x16 (halo / tail rows in the guards)"),
                  dst, conv, Cout, Cin, **geo)
    return ctx.ref(lambda: {"dest": (ref(), 2e-4)})


for _conv in (1, 2):
    case(f"wgrad_conv_{'3x3' if _conv == 1 else 't3'}", ("_wgrad_conv", "gcd_wgrad_conv_tr_f16"), alloc=True)(
        lambda ctx, _c=_conv: _wgrad_conv_case(ctx, _c))


@case("grad_contractions", ("_grad_contractions",), alloc=True)
def _(ctx):
    from gcd_amd import autograd_ops as A
    g = _gen(1)
    M, K, N = 300, 64, 128
    x, w = torch.randn(M, K, generator=g).half(), (torch.randn(N, K, generator=g) / math.sqrt(K)).half()
    dy = torch.randn(M, N, generator=g)
    wt = ctx.inp_flat(w.t().contiguous(), name="W^T")                   # W operands carry no row stride: dense
    dx, dw = A._grad_contractions(ctx.inp(dy, name="dy32"), ctx.inp(x, name="x16"), lambda dt: wt.to(dt), True, True)
    ctx.also("dx", dx)
    ctx.also("dw", dw)
    return ctx.ref(lambda: {"dx": (dy.half().float() @ w.float(), 1e-4), "dw": (dy.half().float().t() @ x.float(), 1e-4)})


@case("cast16_colsum_and_colsum", ("_cast16_colsum", "_colsum"), alloc=True, atomic=("sums", "colsum_blocks", "colsum_all"))
def _(ctx):
    from gcd_amd import autograd_ops as A
    g = _gen(2)
    rows, blocks, N = 37, 6, 72
    M = rows * blocks
    dy = torch.randn(M, N, generator=g)
    dyg = ctx.inp(dy, name="dy32")
    y16, sums = A._cast16_colsum(dyg, F16, rows)
    ctx.also("y16", y16)
    ctx.also("sums", sums)
    ctx.also("colsum_blocks", A._colsum(dyg, rows))
    ctx.also("colsum_all", A._colsum(dyg))

    def ref():
        s = dy.double().reshape(blocks, rows, N).sum(1)
        return {"y16": (dy.half().float(), 1e-30), "sums": (s, 1e-5), "colsum_blocks": (s, 1e-5), "colsum_all": (s.sum(0, keepdim=True), 1e-5)}
    return ctx.ref(ref)


def _gn_bwd_case(ctx, frames, HW, C, per_clip_T, silu):
    from gcd_amd import autograd_ops as A
    g = _gen(4)
    M = frames * HW
    x = torch.randn(M, C, generator=g) * 2 + 0.7
    gamma, beta, dy = torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(M, C, generator=g)
    rows = (per_clip_T or 1) * HW
    xg = ctx.inp(x, name="x")
    _, stats, g32, b32 = A._gn_fwd(xg, gamma.to(ctx.device), beta.to(ctx.device), rows, 1e-5, silu)
    dx, dgamma, dbeta = A._gn_bwd(xg, ctx.inp(dy, name="dy"), stats, g32, b32, rows, silu)
    for n, t in (("dx", dx), ("dgamma", dgamma), ("dbeta", dbeta)):
        ctx.also(n, t)

    def ref():
        xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
        yr = F.group_norm(xr.reshape(M // rows, rows, C).permute(0, 2, 1), 32, gr, br, 1e-5)
        (F.silu(yr) if silu else yr).permute(0, 2, 1).reshape(M, C).backward(dy)
        return {"dx": (xr.grad, 1e-4), "dgamma": (gr.grad, 1e-4), "dbeta": (br.grad, 1e-4)}
    return ctx.ref(ref)


for _a in [(4, 50, 320, 2, True), (3, 33, 128, 0, False)]:
    case("gn_bwd_%dx%d_C%d_T%d" % _a[:4], ("_gn_bwd",), alloc=True)(lambda ctx, _a=_a: _gn_bwd_case(ctx, *_a))


@case("gn_affine_grads", ("gcd_gn_affine_grads",))
def _(ctx):
    from gcd_amd import _lib
    g = _gen(44)
    ninst, Cc = 5, 72
    AB = torch.randn(ninst, Cc, 2, generator=g, dtype=F64)
    dg, db = ctx.out_flat("dgamma", (Cc,), F32), ctx.out_flat("dbeta", (Cc,), F32)
    _lib.check_train(_lib.load_train().gcd_gn_affine_grads(ctx.inp_flat(AB, name="AB").data_ptr(), ninst, Cc, dg.data_ptr(),
                                                           db.data_ptr(), 0, _stream()), "gcd_gn_affine_grads")
    return ctx.ref(lambda: {"dgamma": (AB.sum(0)[:, 1].reshape(1, -1), 1e-6), "dbeta": (AB.sum(0)[:, 0].reshape(1, -1), 1e-6)})


def _ln_bwd_case(ctx, M, C):
    from gcd_amd import autograd_ops as A
    g = _gen(5)
    x = torch.randn(M, C, generator=g) * 1.5 + 0.3
    gamma, beta, dy = torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(M, C, generator=g)
    dx, dg, db = A._ln_bwd(ctx.inp(x, name="x"), ctx.inp(dy, name="dy"), ctx.inp_flat(gamma, name="gamma"), 1e-5)
    for n, t in (("dx", dx), ("dgamma", dg), ("dbeta", db)):
        ctx.also(n, t)

    def ref():
        xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
        F.layer_norm(xr, (C,), gr, br, 1e-5).backward(dy)
        return {"dx": (xr.grad, 1e-4), "dgamma": (gr.grad.reshape(1, -1), 1e-4), "dbeta": (br.grad.reshape(1, -1), 1e-4)}
    return ctx.ref(ref)


for _M, _C in [(100, 64), (501, 320), (33, 1280)]:
    case(f"ln_bwd_{_M}x{_C}", ("_ln_bwd",), alloc=True, atomic=("dgamma", "dbeta"))(lambda ctx, _a=(_M, _C): _ln_bwd_case(ctx, *_a))


@case("blend_fwd_bwd", ("gcd_blend_fwd_f32", "gcd_blend_bwd_f32"), atomic=("d_alpha",))
def _(ctx):
    from gcd_amd import _lib
    g = _gen(9)
    frames, rows, Cc = 6, 37, 64
    M = frames * rows
    xs, xt, dy = (torch.randn(M, Cc, generator=g) for _ in range(3))
    a = torch.rand(frames, generator=g)
    a[2] = 1.0
    lib = _lib.load_train()
    xsg, xtg, dyg, ag = ctx.inp(xs, name="xs"), ctx.inp(xt, name="xt"), ctx.inp(dy, name="dy"), ctx.inp_flat(a, name="alpha")
    y, dxs, dxt = ctx.out("y", M, Cc, F32), ctx.out("d_xs", M, Cc, F32), ctx.out("d_xt", M, Cc, F32)
    dal = ctx.out_flat("d_alpha", (frames,), F32, init=0.0)               # d_alpha_zeroed: zeros are the ABI
    ld = xsg.stride(0)
    _lib.check_train(lib.gcd_blend_fwd_f32(xsg.data_ptr(), ld, xtg.data_ptr(), ld, ag.data_ptr(), M, Cc, rows, y.data_ptr(), ld,
                                           _stream()), "blend_fwd")
    _lib.check_train(lib.gcd_blend_bwd_f32(dyg.data_ptr(), ld, xsg.data_ptr(), ld, xtg.data_ptr(), ld, ag.data_ptr(), M, Cc, rows,
                                           dxs.data_ptr(), ld, 0, dxt.data_ptr(), ld, dal.data_ptr(), _stream()), "blend_bwd")

    def ref():
        ar = a.repeat_interleave(rows)[:, None]
        return {"y": (ar * xs + (1 - ar) * xt, 1e-6), "d_xs": (ar * dy, 1e-6), "d_xt": ((1 - ar) * dy, 1e-6),
                "d_alpha": ((dy * (xs - xt)).reshape(frames, -1).double().sum(1).reshape(1, -1), 1e-5)}
    return ctx.ref(ref)


@case("smallm_fwd_dgrad_wgrad", ("gcd_smallm_fwd", "gcd_smallm_dgrad", "gcd_smallm_wgrad"), atomic=("dx0", "dx1", "dx2", "dx3"))
def _(ctx):
    from gcd_amd import _lib
    g = _gen(11)
    lib = _lib.load_train()
    shapes = [(28, 1280, 320, True), (28, 100, 72, False), (2, 64, 1280, False), (7, 36, 260, True)]      # (M, N, K, silu)
    items = []
    for M, N, K, silu in shapes:
        it = dict(x=torch.randn(M, K, generator=g), W=torch.randn(N, K, generator=g) / K ** 0.5, b=torch.randn(N, generator=g),
                  dy=torch.randn(M, N, generator=g), silu=silu, M=M, N=N, K=K)
        i = len(items)
        it["xg"] = ctx.inp(it["x"], name=f"x{i}")                          # strided: ldx is in the table
        it["Wg"], it["bg"] = ctx.inp_flat(it["W"], name=f"W{i}"), ctx.inp_flat(it["b"], name=f"b{i}")
        it["dyg"] = ctx.inp(it["dy"], name=f"dy{i}")                        # strided too: ldy is in the table
        it["yg"] = ctx.out(f"y{i}", M, N, F32)
        it["dxg"] = ctx.out(f"dx{i}", M, K, F32, init=0.0)                 # flag 4: atomicAdd into a zeroed dx (the ABI)
        it["dWg"], it["dbg"] = ctx.out_flat(f"dW{i}", (N, K), F32), ctx.out_flat(f"db{i}", (N,), F32)
        items.append(it)

    def table(mode):
        probs, b0 = [], 0
        for it in items:
            M, N, K = it["M"], it["N"], it["K"]
            p = _lib.SmallmProblem()
            p.x, p.ldx, p.W, p.b = it["xg"].data_ptr(), it["xg"].stride(0), it["Wg"].data_ptr(), it["bg"].data_ptr()
            p.M, p.N, p.K, p.block0 = M, N, K, b0
            if mode == "fwd":
                p.y, p.ldy, p.flags = it["yg"].data_ptr(), it["yg"].stride(0), int(it["silu"])
                b0 += (N + 15) // 16
            else:
                p.y, p.ldy = it["dyg"].data_ptr(), it["dyg"].stride(0)
                p.dx, p.lddx, p.dW, p.db = it["dxg"].data_ptr(), it["dxg"].stride(0), it["dWg"].data_ptr(), it["dbg"].data_ptr()
                p.flags = int(it["silu"]) | (4 if mode == "dgrad" else 0)
                b0 += ((K + 255) // 256) * ((N + 63) // 64)
            probs.append(p)
        arr = (_lib.SmallmProblem * len(probs))(*probs)
        d = torch.frombuffer(bytearray(bytes(arr)), dtype=U8).to(ctx.device)
        return d, len(probs), b0
    for mode, fn in (("fwd", lib.gcd_smallm_fwd), ("dgrad", lib.gcd_smallm_dgrad), ("wgrad", lib.gcd_smallm_wgrad)):
        tab, n, blocks = table(mode)
        _lib.check_train(fn(tab.data_ptr(), n, blocks, _stream()), mode)
    torch.cuda.synchronize()

    def ref():
        out = {}
        for i, it in enumerate(items):
            x, W, b = (it[k].double().requires_grad_(True) for k in ("x", "W", "b"))
            y = (F.silu(x) if it["silu"] else x) @ W.t() + b
            y.backward(it["dy"].double())
            out.update({f"y{i}": (y.detach(), 1e-5), f"dx{i}": (x.grad, 1e-5), f"dW{i}": (W.grad, 1e-5), f"db{i}": (b.grad, 1e-5)})
        return out
    return ctx.ref(ref)


@case("adam_step_multi", ("gcd_adam_step_multi",))
def _(ctx):
    from gcd_amd import _lib
    g = _gen(9)
    shapes = [(300, 7), (5,), (64, 64), (16 * 1024 + 3,)]
    lr, b1, b2, eps, wd, step, gs = 2e-3, 0.9, 0.999, 1e-8, 0.01, 3, 1.0 / 64.0
    ps, grads, ms, vs = ([torch.randn(s, generator=g) for s in shapes] for _ in range(4))
    vs = [v.abs() for v in vs]
    n = len(shapes)
    pg = [ctx.out_flat(f"p{i}", s, F32, init=ps[i]) for i, s in enumerate(shapes)]
    mg = [ctx.out_flat(f"m{i}", s, F32, init=ms[i]) for i, s in enumerate(shapes)]
    vg = [ctx.out_flat(f"v{i}", s, F32, init=vs[i]) for i, s in enumerate(shapes)]
    gg = [ctx.inp_flat(grads[i] * 64.0, name=f"g{i}") for i in range(n)]
    arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])      # noqa: E731
    _lib.check(_lib.load().gcd_adam_step_multi(n, arr(pg), arr(gg), arr(mg), arr(vg), (C.c_int64 * n)(*[t.numel() for t in pg]),
                                               lr, b1, b2, eps, wd, step, gs, _stream()), "gcd_adam_step_multi")

    def ref():
        out = {}
        for i in range(n):
            p, m, v = ps[i].double(), ms[i].double(), vs[i].double()
            gr = grads[i].double() + wd * p
            m = b1 * m + (1 - b1) * gr
            v = b2 * v + (1 - b2) * gr * gr
            p = p - lr / (1 - b1 ** step) * m / ((v / (1 - b2 ** step)).sqrt() + eps)
            out.update({f"p{i}": (p.reshape(1, -1), 1e-6), f"m{i}": (m.reshape(1, -1), 1e-6), f"v{i}": (v.reshape(1, -1), 1e-6)})
        return out
    return ctx.ref(ref)


@case("train_pack_weights", ("gcd_train_pack_weights",))
def _(ctx):
    from gcd_amd import _lib, autograd_ops as A, packing
    g = _gen(3)
    lin, c3, t3 = torch.randn(100, 72, generator=g), torch.randn(40, 8, 3, 3, generator=g), torch.randn(64, 32, 3, 1, 1, generator=g)
    entries = []

    def entry(src, N, Cc, taps, dst_f, f, dst_t, t, mirror=0):
        e = _lib.PackEntry()
        e.src, e.N, e.C, e.taps, e.mirror = ctx.inp_flat(src, name=f"src{len(entries)}").data_ptr(), N, Cc, taps, mirror
        e.dst_f, e.dst_t = dst_f.data_ptr(), dst_t.data_ptr()
        (e.f_ns, e.f_ts), (e.t_cs, e.t_ts) = f, t
        e.tiles_c = (Cc + 31) // 32
        entries.append(e)
    # a ragged Linear: every destination element is written; the padded 3x3 convolution (Cin 8 -> 64, Cout 40 -> 64): the
    # destinations are allocated zeroed by the caller (the ABI), only real elements are written
    lf, lt = ctx.out_flat("lin_f", (100, 72), F16), ctx.out_flat("lin_t", (72, 100), F16)
    entry(lin, 100, 72, 1, lf, (72, 0), lt, (100, 0))
    cf, cd = ctx.out_flat("c3_f", (64, 9 * 64), F16, init=0.0), ctx.out_flat("c3_dgrad", (64, 9 * 64), F16, init=0.0)
    entry(c3, 40, 8, 9, cf, (9 * 64, 64), cd, (9 * 64, 64), 1)
    tf, td = ctx.out_flat("t3_f", (64, 96), F16), ctx.out_flat("t3_dgrad", (32, 192), F16)
    entry(t3, 64, 32, 3, tf, (96, 32), td, (192, 64), 1)
    t0 = 0
    for e in entries:
        e.tile0 = t0
        t0 += ((e.N + 31) // 32) * e.tiles_c
    arr = (_lib.PackEntry * len(entries))(*entries)
    tab = torch.frombuffer(bytearray(bytes(arr)), dtype=U8).to(ctx.device)
    _lib.check_train(_lib.load_train().gcd_train_pack_weights(tab.data_ptr(), len(entries), t0, 0, _stream()), "pack")
    torch.cuda.synchronize()
    return ctx.ref(lambda: {"lin_f": (lin.half().float(), 1e-30), "lin_t": (lin.half().float().t(), 1e-30),
                            "c3_f": (packing.pack_conv3x3(c3, 64, 64, F16).float(), 1e-30),
                            "c3_dgrad": (A._pack_c3_dgrad(F16, 64, 64)(c3).float(), 1e-30),
                            "t3_f": (packing.pack_conv_t3(t3, F16).float(), 1e-30),
                            "t3_dgrad": (A._pack_t3_dgrad(F16)(t3).float(), 1e-30)})


@case("attn_spatial_bwd_direct", ("attn_spatial_bwd",))
def _(ctx):
    from gcd_amd import ops
    g = _gen(71)
    frames, S, heads = 2, 300, 3                  # S = 4 key blocks + 44: keys past S of the last frame are guard rows
    C_ = heads * 64
    qkv = (torch.randn(frames * S, 3 * C_, generator=g) * torch.linspace(0.3, 2.0, frames * S)[:, None]).half()
    dO = (torch.randn(frames * S, C_, generator=g) * torch.linspace(2.0, 0.1, frames * S)[:, None]).half()
    q, k, v = (t.double().reshape(frames, S, heads, 64).transpose(1, 2).requires_grad_(True) for t in qkv.chunk(3, dim=-1))
    o = F.scaled_dot_product_attention(q, k, v)
    o16 = o.detach().transpose(1, 2).reshape(frames * S, C_).half()
    dqkv = ctx.out("dqkv", frames * S, 3 * C_, F32)
    ws = ctx.scratch(ops.attn_spatial_bwd_ws_bytes(frames, S, heads), U8, name="ws")
    ops.attn_spatial_bwd(ctx.inp(qkv, name="qkv"), ctx.inp(o16, name="out16"), ctx.inp(dO, name="dout16"), dqkv, frames, S, heads, ws)

    def ref():
        o.backward(dO.double().reshape(frames, S, heads, 64).transpose(1, 2))
        return {"dqkv": (torch.cat([t.grad.transpose(1, 2).reshape(frames * S, C_) for t in (q, k, v)], 1), 1e-3)}
    return ctx.ref(ref)


@case("geglu_fwd_bwd_direct", ("gcd_geglu_fwd_f32", "gcd_geglu_bwd_f32"))
def _(ctx):
    from gcd_amd import _lib
    g = _gen(6)
    M, H = 201, 260                               # 260 = 65 float4 per row: the last wave's columns are a tail
    h, dout = torch.randn(M, 2 * H, generator=g) * 1.5, torch.randn(M, H, generator=g)
    hg, dog = ctx.inp(h, name="h"), ctx.inp(dout, name="dout")
    out, dh = ctx.out("out", M, H, F32), ctx.out("dh", M, 2 * H, F32)
    lib = _lib.load()
    _lib.check(lib.gcd_geglu_fwd_f32(hg.data_ptr(), hg.stride(0), out.data_ptr(), out.stride(0), M, H, _stream()), "gcd_geglu_fwd_f32")
    _lib.check(lib.gcd_geglu_bwd_f32(hg.data_ptr(), hg.stride(0), dog.data_ptr(), dog.stride(0), dh.data_ptr(), dh.stride(0), M, H,
                                     _stream()), "gcd_geglu_bwd_f32")

    def ref():
        hr = h.clone().requires_grad_(True)
        a, gate = hr.chunk(2, dim=-1)
        y = a * F.gelu(gate)
        y.backward(dout)
        return {"out": (y.detach(), 1e-5), "dh": (hr.grad, 1e-5)}
    return ctx.ref(ref)


def _temporal_bwd_direct(ctx, export, clips, T, HW, heads):
    """dqkv fp32 [M, 3C] from fp16 q|k|v and fp32 dO, every operand a strided view; fp64 math on the same fp16-rounded
    q|k|v as the reference (the bar of test_temporal_attention_backward)."""
    from gcd_amd import _lib
    g = _gen(8)
    Cc = heads * 64
    M = clips * T * HW
    qkv, dO = (torch.randn(M, 3 * Cc, generator=g)).half(), torch.randn(M, Cc, generator=g)
    qg, dg = ctx.inp(qkv, name="qkv16 (rows past clips * T * HW in the guard)"), ctx.inp(dO, name="dO")
    dqkv = ctx.out("dqkv", M, 3 * Cc, F32)
    _lib.check(getattr(_lib.load(), export)(qg.data_ptr(), qg.stride(0), dg.data_ptr(), dg.stride(0), dqkv.data_ptr(),
                                            dqkv.stride(0), clips, T, HW, heads, _stream()), export)

    def ref():
        qr = qkv.double().requires_grad_(True)
        q, k, v = (u.reshape(clips, T, HW, heads, 64).permute(0, 2, 3, 1, 4) for u in qr.chunk(3, dim=-1))
        F.scaled_dot_product_attention(q, k, v).permute(0, 3, 1, 2, 4).reshape(M, Cc).backward(dO.double())
        return {"dqkv": (qr.grad, 1e-3)}
    return ctx.ref(ref)


# clips * HW * heads problems: odd (gcd_attn_temporal_bwd takes two per workgroup), T below / at the 16-frame block and,
# on the long kernel, inside every number of 16-frame blocks (T padded to 16 / 32 / 48 / 64)
for _export, _shapes in (("gcd_attn_temporal_bwd", [(1, 14, 5, 3), (1, 1, 7, 1), (3, 16, 3, 1), (1, 4, 33, 1)]),
                         ("gcd_attn_temporal_long_bwd", [(1, 17, 7, 1), (1, 33, 5, 3), (1, 47, 3, 1), (1, 64, 3, 1), (1, 9, 5, 1)])):
    for _sh in _shapes:
        case("%s_%dx%dx%dx%d" % ((_export[4:],) + _sh), (_export,))(
            lambda ctx, _a=(_export,) + _sh: _temporal_bwd_direct(ctx, *_a))


# ------------------------------------------------------------------------------ torch.autograd functions, dirty allocator
def _leaf(t, dev=None):
    t = t.clone().to(dev) if dev is not None else t.clone()
    return t.requires_grad_(True)


def _tok(x):
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n * h * w, c).contiguous()


def _autograd(ctx, fn_gpu, fn_ref, tensors, dy, tol_y=TOL_OP, tols=None, tok_in=None, tok_out=None):
    """tensors: {name: CPU tensor} -> leaves on both sides; fn(**leaves) -> y.  Compares y and every gradient."""
    tols = tols or {}
    tok_in, tok_out = tok_in or {}, tok_out or (lambda t: t)
    gl = {k: _leaf(tok_in[k](v) if k in tok_in else v, ctx.device) for k, v in tensors.items()}
    y = fn_gpu(**gl)
    y.backward(tok_out(dy).to(ctx.device))
    torch.cuda.synchronize()
    ctx.also("y", y)
    for k, t in gl.items():
        if t.grad is not None:
            ctx.also("d" + k, t.grad)

    def ref():
        rl = {k: _leaf(v) for k, v in tensors.items()}
        yr = fn_ref(**rl)
        yr.backward(dy)
        out = {"y": (tok_out(yr.detach()), tol_y)}
        for k, t in rl.items():
            gr = tok_in[k](t.grad) if k in tok_in else t.grad
            out["d" + k] = (gr if gr.dim() == 2 else gr.reshape(1, -1), tols.get(k, TOL_OP))
        return out
    return ctx.ref(ref)


@case("A.linear", ("A.linear",), alloc=True, atomic=("db",))
def _(ctx):
    from gcd_amd import autograd_ops as A
    g = _gen(1)
    M, K, N = 300, 64, 128
    t = dict(x=torch.randn(M, K, generator=g), w=torch.randn(N, K, generator=g) / math.sqrt(K), b=torch.randn(N, generator=g))
    return _autograd(ctx, lambda x, w, b: A.linear(x, w, b), lambda x, w, b: F.linear(x, w, b), t,
                     torch.randn(M, N, generator=g), tols=dict(b=1e-5))


def _conv3x3_case(ctx, frames, H, W, Cin, Cout, stride, up):
    from gcd_amd import autograd_ops as A
    g = _gen(2)
    t = dict(x=torch.randn(frames, Cin, H, W, generator=g), w=torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin),
             b=torch.randn(Cout, generator=g))

    def fr(x, w, b):
        return F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest") if up else x, w, b, stride=stride, padding=1)
    with torch.no_grad():
        shape = fr(**t).shape
    return _autograd(ctx, lambda x, w, b: A.conv3x3(x, w, b, frames, H, W, stride=stride, upsample=up), fr, t,
                     torch.randn(shape, generator=g), tols=dict(b=1e-5), tok_in=dict(x=_tok), tok_out=_tok)


for _a in [(2, 7, 9, 64, 64, 1, False), (3, 6, 10, 64, 128, 2, False), (2, 4, 6, 128, 64, 1, True), (2, 8, 8, 8, 64, 1, False),
           (2, 8, 8, 64, 4, 1, False)]:
    case("A.conv3x3_%dx%dx%d_%d-%d_s%d_up%d" % _a, ("A.conv3x3",), alloc=True, atomic=("db",))(
        lambda ctx, _a=_a: _conv3x3_case(ctx, *_a))


@case("A.conv_t3", ("A.conv_t3",), alloc=True, atomic=("db",))
def _(ctx):
    from gcd_amd import autograd_ops as A
    g = _gen(3)
    clips, T, HW, Cc = 2, 5, 12, 64
    t = dict(x=torch.randn(clips, Cc, T, HW, 1, generator=g), w=torch.randn(Cc, Cc, 3, 1, 1, generator=g) / math.sqrt(3 * Cc),
             b=torch.randn(Cc, generator=g))
    tok = lambda v: v[..., 0].permute(0, 2, 3, 1).reshape(clips * T * HW, Cc).contiguous()      # noqa: E731
    return _autograd(ctx, lambda x, w, b: A.conv_t3(x, w, b, T, HW), lambda x, w, b: F.conv3d(x, w, b, padding=(1, 0, 0)), t,
                     torch.randn(clips, Cc, T, HW, 1, generator=g), tols=dict(b=1e-5), tok_in=dict(x=tok), tok_out=tok)


@case("A.group_norm", ("A.group_norm",), alloc=True)
def _(ctx):
    from gcd_amd import autograd_ops as A
    g = _gen(4)
    frames, HW, Cc, T = 4, 50, 320, 2
    rows = T * HW
    t = dict(x=torch.randn(frames * HW, Cc, generator=g) * 2 + 0.7, gamma=torch.randn(Cc, generator=g), beta=torch.randn(Cc, generator=g))

    def fr(x, gamma, beta):
        y = F.group_norm(x.reshape(frames * HW // rows, rows, Cc).permute(0, 2, 1), 32, gamma, beta, 1e-5)
        return F.silu(y).permute(0, 2, 1).reshape(frames * HW, Cc)
    return _autograd(ctx, lambda x, gamma, beta: A.group_norm(x, gamma, beta, rows, 1e-5, True), fr, t,
                     torch.randn(frames * HW, Cc, generator=g), tol_y=6e-4, tols=dict(x=1e-4, gamma=1e-4, beta=1e-4))


@case("A.layer_norm", ("A.layer_norm",), alloc=True, atomic=("dgamma", "dbeta"))
def _(ctx):
    from gcd_amd import autograd_ops as A
    g = _gen(5)
    M, Cc = 501, 320
    t = dict(x=torch.randn(M, Cc, generator=g) * 1.5 + 0.3, gamma=torch.randn(Cc, generator=g), beta=torch.randn(Cc, generator=g))
    return _autograd(ctx, lambda x, gamma, beta: A.layer_norm(x, gamma, beta),
                     lambda x, gamma, beta: F.layer_norm(x, (Cc,), gamma, beta, 1e-5), t, torch.randn(M, Cc, generator=g),
                     tol_y=6e-4, tols=dict(x=1e-4, gamma=1e-4, beta=1e-4))


@case("A.geglu", ("A.geglu",), alloc=True)
def _(ctx):
    from gcd_amd import autograd_ops as A
    g = _gen(6)
    t = dict(h=torch.randn(201, 512, generator=g) * 1.5)

    def fr(h):
        a, gate = h.chunk(2, dim=-1)
        return a * F.gelu(gate)
    return _autograd(ctx, lambda h: A.geglu(h), fr, t, torch.randn(201, 256, generator=g), tol_y=1e-5, tols=dict(h=1e-5))


def _spatial_case(ctx, frames, S, heads):
    from gcd_amd import autograd_ops as A
    g = _gen(7)
    Cc = heads * 64
    t = dict(qkv=torch.randn(frames * S, 3 * Cc, generator=g))

    def fr(qkv):
        q, k, v = (u.reshape(frames, S, heads, 64).transpose(1, 2) for u in qkv.chunk(3, dim=-1))
        return F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(frames * S, Cc)
    return _autograd(ctx, lambda qkv: A.spatial_attention(qkv, frames, S, heads), fr, t, torch.randn(frames * S, Cc, generator=g),
                     tol_y=1.5e-3)


for _a in [(2, 100, 2), (2, 201, 1), (1, 33, 1)]:
    case("A.spatial_attention_%dx%dx%d" % _a, ("A.spatial_attention", "attn_spatial_bwd"), alloc=True)(
        lambda ctx, _a=_a: _spatial_case(ctx, *_a))


def _temporal_case(ctx, clips, T, HW, heads):
    from gcd_amd import autograd_ops as A
    g = _gen(8)
    Cc = heads * 64
    M = clips * T * HW
    t = dict(qkv=torch.randn(M, 3 * Cc, generator=g))

    def fr(qkv):
        q, k, v = (u.reshape(clips, T, HW, heads, 64).permute(0, 2, 3, 1, 4) for u in qkv.chunk(3, dim=-1))
        return F.scaled_dot_product_attention(q, k, v).permute(0, 3, 1, 2, 4).reshape(M, Cc)
    return _autograd(ctx, lambda qkv: A.temporal_attention(qkv, clips, T, HW, heads), fr, t, torch.randn(M, Cc, generator=g),
                     tol_y=1.5e-3, tols=dict(qkv=1e-3))


# T <= 16: gcd_attn_temporal_bwd; 17..64: gcd_attn_temporal_long_bwd
for _a in [(2, 14, 6, 2), (1, 4, 33, 1), (1, 25, 7, 2), (1, 64, 3, 1)]:
    case("A.temporal_attention_%dx%dx%dx%d" % _a, ("A.temporal_attention",), alloc=True)(
        lambda ctx, _a=_a: _temporal_case(ctx, *_a))


def _fused_case(ctx, form):
    """The three forms of test_fused_node_norm_contraction_vector_residual."""
    from gcd_amd import autograd_ops as A
    g = _gen(43)
    frames, H, W, Cc, Co = 4, 8, 8, 64, 128
    HW, M = H * W, 4 * 64
    dev = ctx.device
    if form == "ln_linear":
        t = dict(x=torch.randn(M, Cc, generator=g), w=torch.randn(Co, Cc, generator=g) / math.sqrt(Cc), b=torch.randn(Co, generator=g),
                 vec=torch.randn(frames, Co, generator=g), res=torch.randn(M, Co, generator=g),
                 gamma=1 + 0.2 * torch.randn(Cc, generator=g), beta=0.1 * torch.randn(Cc, generator=g))

        def fg(x, w, b, vec, res, gamma, beta):
            ln = torch.nn.LayerNorm(Cc).to(dev)
            ln.weight, ln.bias = torch.nn.Parameter(gamma), torch.nn.Parameter(beta)
            mods.append(ln)
            return A.linear(x, w, b, norm=("ln", ln, 1e-5), residual=res, rowvec=(vec, HW))

        def fr(x, w, b, vec, res, gamma, beta):
            return F.linear(F.layer_norm(x, (Cc,), gamma, beta, 1e-5), w, b) + vec.repeat_interleave(HW, 0) + res
        dy, kw = torch.randn(M, Co, generator=g), {}
    elif form == "gn_conv3x3":
        t = dict(x=torch.randn(frames, Cc, H, W, generator=g), w=torch.randn(Co, Cc, 3, 3, generator=g) / math.sqrt(9 * Cc),
                 b=torch.randn(Co, generator=g), vec=torch.randn(frames, Co, generator=g), res=torch.randn(frames, Co, H, W, generator=g),
                 gamma=1 + 0.2 * torch.randn(Cc, generator=g), beta=0.1 * torch.randn(Cc, generator=g))

        def fg(x, w, b, vec, res, gamma, beta):
            gn = torch.nn.GroupNorm(32, Cc).to(dev)
            gn.weight, gn.bias = torch.nn.Parameter(gamma), torch.nn.Parameter(beta)
            mods.append(gn)
            return A.conv3x3(x, w, b, frames, H, W, norm=("gn", gn, HW, 1e-5, True), residual=res, rowvec=(vec, HW))

        def fr(x, w, b, vec, res, gamma, beta):
            return F.conv2d(F.silu(F.group_norm(x, 32, gamma, beta, 1e-5)), w, b, padding=1) + vec[:, :, None, None] + res
        dy, kw = torch.randn(frames, Co, H, W, generator=g), dict(tok_in=dict(x=_tok, res=_tok), tok_out=_tok)
    else:
        clips, T = 2, 2
        tok5 = lambda v: v.permute(0, 2, 3, 4, 1).reshape(clips * T * HW, Cc).contiguous()    # noqa: E731
        t = dict(x=torch.randn(clips, Cc, T, H, W, generator=g), w=torch.randn(Cc, Cc, 3, 1, 1, generator=g) / math.sqrt(3 * Cc),
                 gamma=1 + 0.2 * torch.randn(Cc, generator=g), beta=0.1 * torch.randn(Cc, generator=g))

        def fg(x, w, gamma, beta):
            gn = torch.nn.GroupNorm(32, Cc).to(dev)
            gn.weight, gn.bias = torch.nn.Parameter(gamma), torch.nn.Parameter(beta)
            mods.append(gn)
            return A.conv_t3(x, w, None, T, HW, norm=("gn", gn, T * HW, 1e-5, True), residual=x)

        def fr(x, w, gamma, beta):
            return F.conv3d(F.silu(F.group_norm(x, 32, gamma, beta, 1e-5)), w, None, padding=(1, 0, 0)) + x
        dy, kw = torch.randn(clips, Cc, T, H, W, generator=g), dict(tok_in=dict(x=tok5), tok_out=tok5)
    mods = []
    refs = _autograd(ctx, fg, fr, t, dy, tol_y=1e-3, **kw)
    # The norm's affine gradients arrive on the MODULE's parameters: fg re-wraps the leaves gamma / beta in nn.Parameter,
    # so _autograd finds no .grad on those leaves and records no "dgamma" / "dbeta" for the GPU side, while its CPU
    # reference (plain leaves) does produce them.  They are added here under exactly those keys: "d" + the names in `t`.
    ctx.extra_outs["dgamma"], ctx.extra_outs["dbeta"] = mods[0].weight.grad, mods[0].bias.grad
    return refs


# the outputs that atomicAdd reductions write: bias / per-frame-vector gradients (cast + column sums, rowblock_sum) and the
# LayerNorm backward's affine sums; GroupNorm's affine gradients are a plain sum over instances
for _form, _atomic in (("ln_linear", ("db", "dvec", "dgamma", "dbeta")), ("gn_conv3x3", ("db", "dvec")), ("gn_conv_t3", ())):
    case(f"A.Fused_{_form}", ("A.Fused",), alloc=True, atomic=_atomic)(lambda ctx, _f=_form: _fused_case(ctx, _f))


# ------------------------------------------------------------------------------------------------------ the test
@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_backward_memory_contract(gpu, c):
    from gcd_amd import autograd_ops as A
    A.PACK.clear()
    mc.run_contract(c, gpu)
