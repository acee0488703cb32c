"""The phase form of the x2 up-convolution (gcd_gemm_desc.upsample = 2, gemm_p8.hip MODE 4) on the GPU.

Two references per case:
  (i)  torch fp32 phase convolutions on the SAME fp16 phase weights and fp16 x: operands are exact, only the fp32
       accumulation order differs -> TOL_F32 of tests/test_kernels_gpu.py (1e-4).  The sharp check of the indexing.
  (ii) the fp32-weight truth conv2d(interpolate(x), w): the phase form rounds four folded taps where the 3 x 3 form rounds
       nine, so it is held to 1.1 x the error of the existing upsample = 1 launch on the same inputs, not to that launch.
The 256 x 320 tile kernels are forced (GCD_TUNE_GEMM_IMPL = 2) as test_conv3x3_pingpong_full_tiles does: the automatic
choice takes them from 192 tiles only.
"""
import math

import pytest
import torch

from conftest import rel_l2
from memcontract import Case, run_contract
from test_up_phases_host import phase_conv, up_conv

pytestmark = pytest.mark.gpu

TOL_F32 = 1e-4            # tests/test_kernels_gpu.py: fp32 outputs of contractions on exact operands
TOL_FWD = 2e-3            # tests/test_unet_gpu.py: one UNet forward against its golden

#        frames Hi  Wi  Cin  Cout
CASES = {
    "wi16_colsums": (28, 12, 16, 320, 320),      # four image rows per wave; Hi Wi = 192: column sums on
    "wi64": (2, 4, 64, 320, 320),                # one image row per wave
    "wi32": (2, 6, 32, 320, 320),                # two image rows per wave; 1.5 M-tiles per phase
    "net_9x16": (3, 9, 16, 640, 640),            # the network's own shape: partial tiles, 64-row blocks straddle frames
    "odd_h_cin64": (2, 7, 24, 64, 320),          # odd Hi, Cin != Cout, borders in every lane position
}
COLSUM_CASES = ("wi16_colsums", "wi64", "wi32")


@pytest.fixture(autouse=True)
def tile_kernels():
    from gcd_amd import ops
    ops.tune_set(ops.TUNE_GEMM_IMPL, 2)
    yield
    ops.tune_set(ops.TUNE_GEMM_IMPL, 0)


def _tok(t):      # NCHW -> token-major [n h w, C]
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


_made = {}


def _case(name):
    """Operands and both references of a case, made once (CPU, fp32) and shared."""
    if name not in _made:
        from gcd_amd import packing
        frames, hi, wi, cin, cout = CASES[name]
        g = torch.Generator().manual_seed(sorted(CASES).index(name) + 50)
        x = torch.randn(frames, cin, hi, wi, generator=g).half().float()
        w = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)       # the fp32 parameter, unrounded
        b = torch.randn(cout, generator=g)
        wp = packing.pack_conv3x3_up_phases(w)
        _made[name] = dict(x=x, w=w, b=b, wp=wp, a=_tok(x).half().contiguous(),
                           ref_phase=_tok(phase_conv(x, wp, b)), truth=_tok(up_conv(x, w, b)),
                           conv=dict(Cin=cin, Hi=hi, Wi=wi, Ho=2 * hi, Wo=2 * wi, stride=1), M=frames * 4 * hi * wi, N=cout)
    return _made[name]


def _phase_block_sums(out, frames, hi, wi):
    """[sum | sumsq] rows in the phase form's block order: frame n owns blocks [n Ho Wo / 64, (n + 1) Ho Wo / 64), inside
    it phase-major, then 64 consecutive low-res tokens."""
    n = out.shape[1]
    v = out.double().reshape(frames, hi, 2, wi, 2, n).permute(0, 2, 4, 1, 3, 5).reshape(-1, 64, n)
    return torch.stack([v.sum(1), (v * v).sum(1)], 1).reshape(-1, n)


@pytest.mark.parametrize("name", list(CASES))
def test_up_phases_conv(gpu, name):
    from gcd_amd import ops, packing
    c = _case(name)
    frames, hi, wi, cin, cout = CASES[name]
    M, N = c["M"], c["N"]
    a, wp, b = c["a"].to(gpu), c["wp"].to(gpu), c["b"].to(gpu)
    kw = dict(M=M, mode=ops.GEMM_CONV3X3, bias=b, conv=dict(c["conv"], upsample=2))
    out = torch.full((M, N), float("nan"), device=gpu)
    want_cs = name in COLSUM_CASES
    assert ops.gemm(a, wp, out, probe_colstats=True, **kw) == want_cs
    cs = torch.full((2 * (M // 64), N), float("nan"), device=gpu)
    if want_cs:
        ops.gemm(a, wp, out, colstats=cs, **kw)
    else:
        with pytest.raises(Exception, match="colstats"):
            ops.gemm(a, wp, out, colstats=cs, **kw)
        ops.gemm(a, wp, out, **kw)
    out9 = torch.empty(M, N, device=gpu)
    ops.gemm(a, packing.pack_conv3x3(c["w"]).to(gpu), out9, M=M, mode=ops.GEMM_CONV3X3, bias=b,
             conv=dict(c["conv"], upsample=1))
    torch.cuda.synchronize()
    assert not torch.isnan(out).any()
    e_idx = rel_l2(out, c["ref_phase"])
    e_phase, e_nine = rel_l2(out, c["truth"]), rel_l2(out9, c["truth"])
    print(f"{name}: vs fp32 phase conv on the same operands {e_idx:.3e}; vs the fp32-weight truth: phase form "
          f"{e_phase:.3e}, upsample=1 launch {e_nine:.3e}")
    assert e_idx < TOL_F32, f"{name}: rel-L2 {e_idx:.3e} against the phase convolution on the same operands"
    assert e_phase <= 1.1 * e_nine, f"{name}: {e_phase:.3e} against the truth, the 3x3 form makes {e_nine:.3e}"
    if not want_cs:
        return
    # the sums of what was stored, in the documented block order; then statistics from the sums == statistics from a
    # pass over the tensor (the bars of test_gemm_column_sums_for_groupnorm), one instance per frame and one in all
    want = _phase_block_sums(out.cpu(), frames, hi, wi)
    assert not torch.isnan(cs).any()
    assert rel_l2(cs[0::2], want[0::2]) < 2e-6 and rel_l2(cs[1::2], want[1::2]) < 2e-6
    for rows in (4 * hi * wi, M):
        ninst = M // rows
        st_a = torch.empty(ninst * 64, device=gpu)
        st_b = torch.empty(ninst * 64, device=gpu)
        ops.groupnorm_stats_from_colsums(cs, N, None, 0, M, rows, 1e-5, st_a)
        nch = ops.gn_nchunks(rows, ninst)
        partial = torch.empty(ninst * nch * 64, dtype=torch.float64, device=gpu)
        ops.groupnorm_stats(out, None, rows, 1e-5, partial, st_b, nch)
        torch.cuda.synchronize()
        assert torch.allclose(st_a, st_b, rtol=2e-5, atol=2e-6), f"rows={rows}: {(st_a - st_b).abs().max()}"


def test_up_phases_refusals(gpu):
    """Argument errors, never another kernel: Wi % 8 != 0, Cin % 64 != 0, a residual, an fp16 output, and a shape the
    automatic choice would send to the general kernel or split-K."""
    from gcd_amd import ops, packing
    g = torch.Generator().manual_seed(9)

    def launch(frames, hi, wi, cin, cout, out_kind=None, r1=False):
        M = frames * 4 * hi * wi
        a = torch.zeros(frames * hi * wi, cin, device=gpu, dtype=torch.float16)
        wp = packing.pack_conv3x3_up_phases(torch.randn(cout, cin, 3, 3, generator=g)).to(gpu)
        f16 = out_kind == ops.OUT_F16
        out = torch.zeros(M, cout, device=gpu, dtype=torch.float16 if f16 else torch.float32)
        kw = dict(out_kind=out_kind) if f16 else {}
        if r1:
            kw["r1"] = torch.zeros(M, cout, device=gpu)
        ops.gemm(a, wp, out, M=M, mode=ops.GEMM_CONV3X3, bias=torch.zeros(cout, device=gpu),
                 conv=dict(Cin=cin, Hi=hi, Wi=wi, Ho=2 * hi, Wo=2 * wi, stride=1, upsample=2), **kw)

    with pytest.raises(Exception, match="Wi"):
        launch(2, 5, 13, 64, 320)
    with pytest.raises(Exception, match="Cin"):
        launch(2, 4, 8, 96, 320)
    with pytest.raises(Exception, match="residual"):
        launch(2, 4, 8, 64, 320, r1=True)
    with pytest.raises(Exception, match="residual"):
        launch(2, 4, 8, 64, 320, out_kind=ops.OUT_F16)
    ops.tune_set(ops.TUNE_GEMM_IMPL, 0)      # 4 tiles: the automatic choice is the general kernel / split-K
    with pytest.raises(Exception, match="tile kernel"):
        launch(2, 4, 8, 64, 320)
    launch_ok = ops.up_phases_ok(2, 4, 8, 64, 320)
    assert not launch_ok and ops.up_phases_ok(28, 9, 16, 1280, 1280) and not ops.up_phases_ok(28, 9, 12, 1280, 1280)


def test_up_phases_memory_contract(gpu):
    """One phase-form launch with column sums on guarded, poisoned operands (tests/memcontract.py): strided A and out,
    1.5 M-tiles per phase (a whole overhanging half tile), every element of out and colstats written, nothing else."""
    from gcd_amd import ops
    name = "wi32"
    c = _case(name)
    frames, hi, wi, cin, cout = CASES[name]
    M, N = c["M"], c["N"]

    def run(ctx):
        a = ctx.inp(c["a"], name="A")
        wp = ctx.inp_flat(c["wp"], name="W phases")
        b = ctx.inp_flat(c["b"], name="bias")
        out = ctx.out("out", M, N, torch.float32)
        cs = ctx.out_flat("colstats", (2 * (M // 64), N), torch.float32)
        ops.gemm(a, wp, out, M=M, mode=ops.GEMM_CONV3X3, bias=b, conv=dict(c["conv"], upsample=2), colstats=cs)
        return ctx.ref(lambda: {"out": (c["ref_phase"], TOL_F32),
                                "colstats": (_phase_block_sums(c["ref_phase"], frames, hi, wi), TOL_F32)})

    run_contract(Case("gemm_up_phases", ["gemm"], run), gpu)


def test_up_phases_in_the_engine(gpu, monkeypatch):
    """A narrow VideoUNet forward (2 x 2 frames of 8 x 64 latents: Wi = 8, 16, 32 at the three Upsamples) with the phase
    form against the same forward on the 3 x 3 form, at the forward tolerance of the tiny-UNet golden test; and with the
    switch off, the bits of an engine that never packed phase weights."""
    from gcd_amd import engine, ops
    from oracle import svd_unet_ref as O
    from test_unet_gpu import _build, _unet_inputs
    T, h, w = 2, 8, 64
    x, ts, ctx, y, ioi = _unet_inputs(O.TINY, T, h, w, 71)
    args = (x.to(gpu), ts.to(gpu))
    kw = dict(context=ctx.to(gpu), y=y.to(gpu), num_video_frames=T, image_only_indicator=ioi.to(gpu))
    ups = []
    real_gemm = ops.gemm

    def spy(*a, **k):
        if k.get("mode") == ops.GEMM_CONV3X3 and k["conv"].get("upsample") and not k.get("probe_colstats"):
            ups.append(int(k["conv"]["upsample"]))
        return real_gemm(*a, **k)

    monkeypatch.setattr(ops, "gemm", spy)
    monkeypatch.setattr(engine, "_UP_PHASES", False)
    net, _ = _build(O.TINY, gpu)
    off_never = net(*args, **kw).clone()
    assert ups == [1, 1, 1]
    assert all("wp" not in L for blk in net.engine.packed["output"] for L in blk if L["kind"] == "up")
    del ups[:]
    monkeypatch.setattr(engine, "_UP_PHASES", True)
    net.engine.invalidate()
    on = net(*args, **kw).clone()
    assert ups == [2, 2, 2], ups
    assert all(L["w"] is None for blk in net.engine.packed["output"] for L in blk if L["kind"] == "up")
    monkeypatch.setattr(engine, "_UP_PHASES", False)
    net.engine.invalidate()
    off_again = net(*args, **kw).clone()
    torch.cuda.synchronize()
    e = rel_l2(on, off_never)
    print(f"tiny UNet forward, phase form vs 3x3 form: rel-L2 {e:.3e}")
    assert torch.isfinite(on).all() and e <= TOL_FWD
    assert torch.equal(off_again, off_never)
