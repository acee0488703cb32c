"""The memory contract of the deterministic reductions (include/gcd_amd_train_det.h; tests/memcontract.py; DESIGN.md
"Memory contract" and "Deterministic reductions").

Every export of the header is called directly with guarded, strided operands, a destination that already holds non-zero
values (the entries ADD) and a guarded scratch (zeros in run (a), NaN in run (b)).  No case uses the run-to-run spread
rule: run (b) is bit-identical to run (a).  Values: the fp64 / fp32 torch references and the bars of the default entries'
cases in test_memcontract_train_gpu.py.  Then, per entry: three launches on the same inputs are torch.equal, and the outputs
that are not reductions (LayerNorm's dx, the 16-bit copy of dY) are torch.equal to what the default entry writes.
"""
import re
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import memcontract as mc

pytestmark = pytest.mark.gpu

F16, F32, BF16, U8 = torch.float16, torch.float32, torch.bfloat16, torch.uint8
ROOT = Path(__file__).resolve().parent.parent
CASES = []


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _lt():
    from gcd_amd import _lib
    return _lib, _lib.load_train()


def _r4(n):
    """Scratch sizes handed to the harness: >= the entry's figure, rounded up to whole 16-byte units (the guarded scratch
    then starts 16-byte aligned, which the entries require)."""
    return (int(n) + 3) // 4 * 4


def case(cid, entries):
    def deco(fn):
        CASES.append(mc.Case(cid, entries, fn))
        return fn
    return deco


# ------------------------------------------------------------------------------------------------ launchers (device tensors)
def launch_rowblock(x, rows, out, scratch):
    _lib, lib = _lt()
    M, N = x.shape
    _lib.check_train(lib.gcd_rowblock_sum_det_f32(x.data_ptr(), x.stride(0), M, N, rows, out.data_ptr(), scratch.data_ptr(),
                                                  scratch.numel(), _stream()), "gcd_rowblock_sum_det_f32")


def launch_ln(x, dy, gamma, dx, dg, db, scratch, dx_add=None):
    _lib, lib = _lt()
    M, C = x.shape
    _lib.check_train(lib.gcd_layernorm_bwd_det(
        x.data_ptr(), x.stride(0), dy.data_ptr(), dy.stride(0), M, C, gamma.data_ptr(), 1e-5, dx.data_ptr(), dx.stride(0),
        dg.data_ptr(), db.data_ptr(), 0 if dx_add is None else dx_add.data_ptr(), 0 if dx_add is None else dx_add.stride(0),
        scratch.data_ptr(), scratch.numel(), _stream()), "gcd_layernorm_bwd_det")


def launch_cast(x, y16, rows, sums, total, scratch):
    _lib, lib = _lt()
    M, C = x.shape
    _lib.check_train(lib.gcd_cast_colsum_det_f32(
        x.data_ptr(), x.stride(0), y16.data_ptr(), y16.stride(0), M, C, rows, sums.data_ptr(), int(y16.dtype == BF16),
        0 if total is None else total.data_ptr(), scratch.data_ptr(), scratch.numel(), _stream()), "gcd_cast_colsum_det_f32")


def launch_blend(dy, xs, xt, a, rows, dxs, dxt, dal, scratch):
    _lib, lib = _lt()
    M, C = dy.shape
    _lib.check_train(lib.gcd_blend_bwd_det_f32(
        dy.data_ptr(), dy.stride(0), xs.data_ptr(), xs.stride(0), xt.data_ptr(), xt.stride(0), a.data_ptr(), M, C, rows,
        dxs.data_ptr(), dxs.stride(0), 0, dxt.data_ptr(), dxt.stride(0), dal.data_ptr(), scratch.data_ptr(), scratch.numel(),
        _stream()), "gcd_blend_bwd_det_f32")


def smallm_table(items, device):
    """items: dicts with device tensors x [M, K], W [N, K], dy [M, N], dx [M, K], silu.  Problems with the same dx form
    a group: `reserved` = table index of the group's first problem.  -> (table, n, blocks)."""
    _lib, _ = _lt()
    probs, b0, heads = [], 0, {}
    for it in items:
        M, K = it["x"].shape
        N = it["W"].shape[0]
        p = _lib.SmallmProblem()
        p.x, p.ldx, p.W = it["x"].data_ptr(), it["x"].stride(0), it["W"].data_ptr()
        p.y, p.ldy = it["dy"].data_ptr(), it["dy"].stride(0)
        p.dx, p.lddx = it["dx"].data_ptr(), it["dx"].stride(0)
        p.M, p.N, p.K, p.flags, p.block0 = M, N, K, (1 if it["silu"] else 0) | 4, b0
        p.reserved = heads.setdefault(it["dx"].data_ptr(), len(probs))
        b0 += (K + 255) // 256
        probs.append(p)
    arr = (_lib.SmallmProblem * len(probs))(*probs)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=U8).to(device), len(probs), b0


def launch_smallm(tab, n, blocks, scratch):
    _lib, lib = _lt()
    _lib.check_train(lib.gcd_smallm_dgrad_det(tab.data_ptr(), n, blocks, scratch.data_ptr(), scratch.numel(), _stream()),
                     "gcd_smallm_dgrad_det")


# ------------------------------------------------------------------------------------------------------------ contract cases
# (blocks, rows per block, N, pad): rows not a multiple of the 4-row lanes / of 256; one block over > 64 x 256 rows (the
# split cap); C = 320, 640, 1280 and a width that is not a multiple of 64
_ROWBLOCK = [(6, 37, 72, 4), (3, 1001, 320, 8), (1, 17000, 640, 4), (2, 515, 1280, 4), (5, 300, 100, 12)]


def _rowblock_case(ctx, blocks, rows, N, pad):
    _, lib = _lt()
    g = _gen(2)
    M = blocks * rows
    x, init = torch.randn(M, N, generator=g), torch.randn(blocks, N, generator=g)
    out = ctx.out_flat("out", (blocks, N), F32, init=init)
    scratch = ctx.scratch(_r4(lib.gcd_rowblock_sum_det_scratch_floats(M, N, rows)), F32)
    launch_rowblock(ctx.inp(x, pad=pad, name="x"), rows, out, scratch)
    return ctx.ref(lambda: {"out": ((init.double() + x.double().reshape(blocks, rows, N).sum(1)).reshape(1, -1), 1e-5)})


for _a in _ROWBLOCK:
    case("rowblock_sum_det_%dx%d_N%d_pad%d" % _a, ("gcd_rowblock_sum_det_f32", "gcd_rowblock_sum_det_scratch_floats"))(
        lambda ctx, _a=_a: _rowblock_case(ctx, *_a))

# (M, C, pad, dx_add): M not a multiple of the 4 rows of a workgroup; more rows than 4 x 768 (several rows per wave)
_LN = [(100, 64, 4, False), (501, 320, 8, True), (3301, 640, 4, False), (33, 1280, 4, False), (257, 100, 4, True)]


def _ln_case(ctx, M, C, pad, add):
    _, lib = _lt()
    g = _gen(5)
    x = torch.randn(M, C, generator=g) * 1.5 + 0.3
    gamma, beta, dy = torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(M, C, generator=g)
    ig, ib = torch.randn(C, generator=g), torch.randn(C, generator=g)
    xadd = torch.randn(M, C, generator=g) if add else None
    dx = ctx.out("dx", M, C, F32, pad=pad)
    dg, db = ctx.out_flat("dgamma", (C,), F32, init=ig), ctx.out_flat("dbeta", (C,), F32, init=ib)
    scratch = ctx.scratch(_r4(lib.gcd_layernorm_bwd_det_scratch_floats(M, C)), F32)
    launch_ln(ctx.inp(x, pad=pad, name="x"), ctx.inp(dy, pad=pad, name="dy"), ctx.inp_flat(gamma, name="gamma"), dx, dg, db,
              scratch, None if xadd is None else ctx.inp(xadd, pad=pad, name="dx_add"))

    def ref():
        xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
        F.layer_norm(xr, (C,), gr, br, 1e-5).backward(dy)
        return {"dx": (xr.grad if xadd is None else xr.grad + xadd, 1e-4), "dgamma": ((ig + gr.grad).reshape(1, -1), 1e-4),
                "dbeta": ((ib + br.grad).reshape(1, -1), 1e-4)}
    return ctx.ref(ref)


for _a in _LN:
    case("ln_bwd_det_%dx%d_pad%d_add%d" % _a, ("gcd_layernorm_bwd_det", "gcd_layernorm_bwd_det_scratch_floats"))(
        lambda ctx, _a=_a: _ln_case(ctx, *_a))

# (blocks, rows per block, C, dtype, total, pad of x)
_CAST = [(6, 37, 72, F16, False, 4), (6, 37, 72, BF16, True, 4), (1, 2003, 320, F16, True, 8), (4, 129, 640, BF16, True, 4),
         (2, 70, 1280, F16, False, 4), (28, 33, 320, BF16, True, 4)]


def _cast_case(ctx, blocks, rows, C, dt, want_total, pad):
    _, lib = _lt()
    g = _gen(3)
    M = blocks * rows
    x = torch.randn(M, C, generator=g)
    isum, itot = torch.randn(blocks, C, generator=g), torch.randn(C, generator=g)
    y16 = ctx.out("y16", M, C, dt, pad=8)
    sums = ctx.out_flat("sums", (blocks, C), F32, init=isum)
    total = ctx.out_flat("total", (C,), F32, init=itot) if want_total else None
    scratch = ctx.scratch(_r4(lib.gcd_cast_colsum_det_scratch_floats(M, C, rows)), F32)
    launch_cast(ctx.inp(x, pad=pad, name="x"), y16, rows, sums, total, scratch)

    def ref():
        s = x.double().reshape(blocks, rows, C).sum(1)
        out = {"y16": (x.to(dt).float(), 1e-30), "sums": ((isum.double() + s).reshape(1, -1), 1e-5)}
        if want_total:
            out["total"] = ((itot.double() + s.sum(0)).reshape(1, -1), 1e-5)
        return out
    return ctx.ref(ref)


for _a in _CAST:
    case("cast_colsum_det_%dx%d_C%d_%s_total%d_pad%d" % (_a[:3] + ("bf16" if _a[3] == BF16 else "fp16",) + _a[4:]),
         ("gcd_cast_colsum_det_f32", "gcd_cast_colsum_det_scratch_floats"))(lambda ctx, _a=_a: _cast_case(ctx, *_a))

# (frames, rows per frame, C, pad)
_BLEND = [(6, 37, 64, 4), (8, 256, 320, 8), (1, 700, 640, 4), (3, 50, 1280, 4), (5, 41, 100, 4)]


def _blend_case(ctx, frames, rows, C, pad):
    _, lib = _lt()
    g = _gen(9)
    M = frames * rows
    xs, xt, dy = (torch.randn(M, C, generator=g) for _ in range(3))
    a, ial = torch.rand(frames, generator=g), torch.randn(frames, generator=g)
    dxs, dxt = ctx.out("d_xs", M, C, F32, pad=pad), ctx.out("d_xt", M, C, F32, pad=pad)
    dal = ctx.out_flat("d_alpha", (frames,), F32, init=ial)
    scratch = ctx.scratch(_r4(lib.gcd_blend_bwd_det_scratch_floats(M, C, rows)), F32)
    launch_blend(ctx.inp(dy, pad=pad, name="dy"), ctx.inp(xs, pad=pad, name="xs"), ctx.inp(xt, pad=pad, name="xt"),
                 ctx.inp_flat(a, name="alpha"), rows, dxs, dxt, dal, scratch)

    def ref():
        ar = a.repeat_interleave(rows)[:, None]
        return {"d_xs": (ar * dy, 1e-6), "d_xt": ((1 - ar) * dy, 1e-6),
                "d_alpha": ((ial.double() + (dy * (xs - xt)).reshape(frames, -1).double().sum(1)).reshape(1, -1), 1e-5)}
    return ctx.ref(ref)


for _a in _BLEND:
    case("blend_bwd_det_%dx%d_C%d_pad%d" % _a, ("gcd_blend_bwd_det_f32", "gcd_blend_bwd_det_scratch_floats"))(
        lambda ctx, _a=_a: _blend_case(ctx, *_a))

# problems (M, N, K, silu, dx slot): slots 0 and 1 are shared by several problems (the time embedding's gradient is the
# sum over all emb_layers); N not a multiple of 64 and of 4; K not a multiple of 256; 1 and 32 rows
_SMALLM = [(28, 1280, 320, True, 0), (28, 100, 320, True, 0), (28, 320, 320, True, 0), (2, 64, 1280, False, 1),
           (7, 37, 260, True, 2), (2, 640, 1280, False, 1), (32, 70, 72, False, 3), (1, 7, 640, True, 4), (28, 64, 320, True, 0)]


def _smallm_operands(g):
    its, slots = [], {}
    for M, N, K, silu, slot in _SMALLM:
        shape = slots.setdefault(slot, (M, K))
        assert shape == (M, K)
        its.append(dict(W=torch.randn(N, K, generator=g) / K ** 0.5, dy=torch.randn(M, N, generator=g), silu=silu, slot=slot))
    xs = {s: torch.randn(m, k, generator=g) for s, (m, k) in slots.items()}          # problems of a group share x too
    inits = {s: torch.randn(m, k, generator=g) for s, (m, k) in slots.items()}
    return its, xs, inits


def _smallm_case(ctx):
    _, lib = _lt()
    its, xs, inits = _smallm_operands(_gen(11))
    xg = {s: ctx.inp(v, name=f"x{s}") for s, v in xs.items()}
    dxg = {s: ctx.out(f"dx{s}", *v.shape, F32, pad=8, init=v) for s, v in inits.items()}
    items = [dict(x=xg[it["slot"]], W=ctx.inp_flat(it["W"], name=f"W{i}"), dy=ctx.inp(it["dy"], name=f"dy{i}"),
                  dx=dxg[it["slot"]], silu=it["silu"]) for i, it in enumerate(its)]
    tab, n, blocks = smallm_table(items, ctx.device)
    scratch = ctx.scratch(_r4(lib.gcd_smallm_dgrad_det_scratch_floats(blocks)), F32)
    launch_smallm(tab, n, blocks, scratch)
    torch.cuda.synchronize()

    def ref():
        out = {}
        for s, x in xs.items():
            xr = x.double().requires_grad_(True)
            for it in its:
                if it["slot"] == s:
                    ((F.silu(xr) if it["silu"] else xr) @ it["W"].double().t()).backward(it["dy"].double())
            out[f"dx{s}"] = (inits[s].double() + xr.grad, 1e-5)
        return out
    return ctx.ref(ref)


case("smallm_dgrad_det_shared_dx", ("gcd_smallm_dgrad_det", "gcd_smallm_dgrad_det_scratch_floats"))(_smallm_case)


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_deterministic_memory_contract(gpu, c):
    assert not c.atomic, "no spread rule here: run (b) is bit-identical to run (a)"
    mc.run_contract(c, gpu)


def test_every_export_of_the_det_header_has_a_contract_case():
    header = (ROOT / "include" / "gcd_amd_train_det.h").read_text()
    exports = set(re.findall(r"^\s*(?:int|int64_t)\s+(gcd_\w+)\s*\(", header, flags=re.M))
    covered = {e for c in CASES for e in c.entries}
    assert exports and exports <= covered, exports - covered
    assert not any(c.atomic for c in CASES)


# --------------------------------------------------------------------------- three launches; equality with the default entries
def _three(run):
    outs = [run() for _ in range(3)]
    torch.cuda.synchronize()
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert torch.equal(a, b)


def _scratch(n, gpu):
    return torch.empty(int(n), dtype=F32, device=gpu)


def test_rowblock_three_launches_bit_equal(gpu):
    _, lib = _lt()
    for blocks, rows, N, _ in _ROWBLOCK:
        x = torch.randn(blocks * rows, N, generator=_gen(2)).to(gpu)
        sc = _scratch(lib.gcd_rowblock_sum_det_scratch_floats(blocks * rows, N, rows), gpu)

        def run():
            out = torch.full((blocks, N), 0.25, device=gpu)
            launch_rowblock(x, rows, out, sc)
            return [out]
        _three(run)


def test_ln_three_launches_bit_equal_and_dx_equals_default_entry(gpu):
    from gcd_amd import _lib
    _, lib = _lt()
    for M, C, _, add in _LN + [(43008 // 4, 320, 0, True)]:
        g = _gen(5)
        x, dy = (torch.randn(M, C, generator=g) * 1.5 + 0.3).to(gpu), torch.randn(M, C, generator=g).to(gpu)
        gamma = torch.randn(C, generator=g).to(gpu)
        xadd = torch.randn(M, C, generator=g).to(gpu) if add else None
        sc = _scratch(lib.gcd_layernorm_bwd_det_scratch_floats(M, C), gpu)

        def run():
            dx, dg, db = torch.empty_like(x), torch.zeros(C, device=gpu), torch.zeros(C, device=gpu)
            launch_ln(x, dy, gamma, dx, dg, db, sc, xadd)
            return [dx, dg, db]
        _three(run)
        dx, dg, db = run()
        dx0, dg0, db0 = torch.empty_like(x), torch.zeros(C, device=gpu), torch.zeros(C, device=gpu)
        _lib.check(_lib.load().gcd_layernorm_bwd(
            x.data_ptr(), C, dy.data_ptr(), C, M, C, gamma.data_ptr(), 1e-5, dx0.data_ptr(), C, dg0.data_ptr(), db0.data_ptr(),
            0 if xadd is None else xadd.data_ptr(), 0 if xadd is None else C, _stream()), "gcd_layernorm_bwd")
        torch.cuda.synchronize()
        assert torch.equal(dx, dx0), (M, C)
        assert mc._rel_l2(dg, dg0) < 1e-5 and mc._rel_l2(db, db0) < 1e-5


def test_cast_three_launches_bit_equal_and_copy_equals_default_entry(gpu):
    from gcd_amd import _lib
    _, lib = _lt()
    for blocks, rows, C, dt, want_total, _ in _CAST + [(1, 10752, 640, BF16, True, 0)]:
        M = blocks * rows
        x = torch.randn(M, C, generator=_gen(3)).to(gpu)
        sc = _scratch(lib.gcd_cast_colsum_det_scratch_floats(M, C, rows), gpu)

        def run():
            y, sums = torch.empty(M, C, dtype=dt, device=gpu), torch.zeros(blocks, C, device=gpu)
            total = torch.zeros(C, device=gpu) if want_total else None
            launch_cast(x, y, rows, sums, total, sc)
            return [y, sums] + ([total] if want_total else [])
        _three(run)
        got = run()
        y0, s0, t0 = torch.empty(M, C, dtype=dt, device=gpu), torch.zeros(blocks, C, device=gpu), torch.zeros(C, device=gpu)
        _lib.check(_lib.load().gcd_cast_colsum_f32(x.data_ptr(), C, y0.data_ptr(), C, M, C, rows, s0.data_ptr(), int(dt == BF16),
                                                   t0.data_ptr() if want_total else 0, _stream()), "gcd_cast_colsum_f32")
        torch.cuda.synchronize()
        assert torch.equal(got[0].view(torch.int16), y0.view(torch.int16)), (blocks, rows, C)
        assert mc._rel_l2(got[1], s0) < 1e-5
        if want_total:
            assert mc._rel_l2(got[2], t0) < 1e-5


def test_blend_three_launches_bit_equal(gpu):
    _, lib = _lt()
    for frames, rows, C, _ in _BLEND:
        g = _gen(9)
        M = frames * rows
        xs, xt, dy = (torch.randn(M, C, generator=g).to(gpu) for _ in range(3))
        a = torch.rand(frames, generator=g).to(gpu)
        sc = _scratch(lib.gcd_blend_bwd_det_scratch_floats(M, C, rows), gpu)

        def run():
            dxs, dxt, dal = torch.empty_like(dy), torch.empty_like(dy), torch.full((frames,), 0.5, device=gpu)
            launch_blend(dy, xs, xt, a, rows, dxs, dxt, dal, sc)
            return [dxs, dxt, dal]
        _three(run)


def test_smallm_three_launches_bit_equal(gpu):
    _, lib = _lt()
    its, xs, inits = _smallm_operands(_gen(11))
    xg = {s: v.to(gpu) for s, v in xs.items()}
    for it in its:
        it["Wg"], it["dyg"] = it["W"].to(gpu), it["dy"].to(gpu)

    def run():
        dx = {s: v.to(gpu) for s, v in inits.items()}
        items = [dict(x=xg[it["slot"]], W=it["Wg"], dy=it["dyg"], dx=dx[it["slot"]], silu=it["silu"]) for it in its]
        tab, n, blocks = smallm_table(items, gpu)
        sc = _scratch(lib.gcd_smallm_dgrad_det_scratch_floats(blocks), gpu)
        launch_smallm(tab, n, blocks, sc)
        torch.cuda.synchronize()
        return [dx[s] for s in sorted(dx)]
    _three(run)
