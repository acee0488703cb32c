"""GPU: `gcd_gemm_desc` bit for bit — a pairwise covering sweep of the descriptor over every GEMM kernel, and split-K at
every slice count.

Operands are exact (tests/gemm_model.py): small integers in A and W, addends in eighths, dyadic scales and blend
factors, so every correct evaluation order gives the same bits and the kernels are held to `torch.equal` against the
fp64 model — one wrong element, one dropped or doubled K sub-tile, one row with its neighbour's frame vector fails.
The only bound in this file is the per-element GEGLU bound of test_conditioning_gpu.py, applied to exactly known
(value, gate) pairs.  Weights are drawn in the reference layout and reach the GPU through gcd_amd.packing.
"""
import pytest
import torch

import gemm_model as G
from test_conditioning_gpu import _check_geglu_pointwise

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _pack_weights(c, o, dt):
    from gcd_amd import packing
    w = o["w"].float()
    if c["mode"] == "plain":
        w16 = packing.pack_linear(w) if dt == torch.float16 else w.to(dt).contiguous()
    elif c["mode"] == "temporal":
        w16 = packing.pack_conv_t3(w, dtype=dt)
    elif c["mode"] == "phase":
        w16 = packing.pack_conv3x3_up_phases(w)
    else:
        w16 = packing.pack_conv3x3(w, dtype=dt)
    bias = o["bias"].float()
    if c["out"] == "geglu":
        w16, bias = packing.pack_geglu(w16, bias)
    return w16, bias


def _padded(t, pad, dev, dtype=None):
    """t [R, C] -> (buffer, view): a NaN-filled device buffer [R, C + pad] and its first C columns holding t."""
    t = t if dtype is None else t.to(dtype)
    buf = torch.full((t.shape[0], t.shape[1] + pad), NAN, dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    buf = buf.to(dev)
    return buf, buf[:, :t.shape[1]]


def _launch(c, o, dev, *, sched=None, workspace=None):
    """Run one case.  -> (out buffer [M, ldo] on the CPU, colstats or None)."""
    from gcd_amd import ops
    dt = torch.bfloat16 if c["bf16"] else torch.float16
    M, N = c["M"], c["N"]
    p = c["padded"]
    _, a = _padded(o["a"], 8 if p else 0, dev, dt)
    w16, bias = _pack_weights(c, o, dt)
    ncols = N // 2 if c["out"] == "geglu" else N
    odt = torch.float32 if c["out"] == "f32" else torch.float16
    init = o["R1"] if c["r1"] == "inplace" else torch.full((M, ncols), NAN, dtype=torch.float64)
    obuf, out = _padded(init, 8 if p else 0, dev, odt)
    kw = {}
    if c["rpv"]:
        kw.update(rowvec=_padded(o["rowvec"], 4 if (p or workspace is not None) else 0, dev, torch.float32)[1],
                  rows_per_vec=c["rpv"])
    if c["r1"] == "sep":
        kw["r1"] = _padded(o["R1"], 4 if p else 0, dev, torch.float32)[1]
    elif c["r1"] == "inplace":
        kw["r1"] = out
    if c["r2"]:
        kw["r2"] = _padded(o["R2"], 12 if p else 0, dev, torch.float32)[1]
    if c["alpha"] != "none":
        kw.update(frame_alpha=o["alpha"].float().to(dev), rows_per_alpha=c["rpa"], r1_blend=c["alpha"] == "b1")
    cs = None
    if c["colstats"]:
        cs = torch.full((2 * (M // 64), N), NAN, dtype=torch.float32, device=dev)
        kw["colstats"] = cs
    s_acc, s_r1, s_r2 = c["scales"]
    mode = {"plain": ops.GEMM_PLAIN, "temporal": ops.GEMM_TEMPORAL3}.get(c["mode"], ops.GEMM_CONV3X3)
    out_kind = {"f32": ops.OUT_F32, "f16": ops.OUT_F16, "geglu": ops.OUT_GEGLU}[c["out"]]
    common = dict(M=M, mode=mode, out_kind=out_kind, bias=bias.to(dev) if c["bias"] else None, s_acc=s_acc, s_r1=s_r1,
                  s_r2=s_r2, conv=G.conv_args(c), operand_bf16=c["bf16"], workspace=workspace,
                  sched=c["sched"] if sched is None else sched, **kw)
    ops.tune_set(ops.TUNE_GEMM_IMPL, c["knob"])
    try:
        if c["colstats"]:      # "where gcd_gemm_colstats_supported says yes": the static rules must agree with the library
            assert ops.gemm(a, w16.to(dev), out, probe_colstats=True, **{k: v for k, v in common.items() if k != "colstats"}), \
                "gcd_gemm_colstats_supported refuses a row the static rules allow"
        ops.gemm(a, w16.to(dev), out, **common)      # a refusal of a generated row raises: the test fails
        torch.cuda.synchronize()
    finally:
        ops.tune_set(ops.TUNE_GEMM_IMPL, 0)
    return obuf.cpu(), None if cs is None else cs.cpu()


def _first_mismatch(got, want):
    bad = (got != want) | got.isnan()
    rows = bad.any(1).nonzero().flatten()
    cols = bad.any(0).nonzero().flatten()
    i, j = int(rows[0]), int(bad[int(rows[0])].nonzero()[0])
    return (f"{int(bad.sum())} of {bad.numel()} elements differ: rows {int(rows[0])}..{int(rows[-1])} ({len(rows)}), "
            f"columns {int(cols[0])}..{int(cols[-1])} ({len(cols)}); first [{i}, {j}] = {float(got[i, j])!r}, "
            f"model {float(want[i, j])!r}")


def _assert_out(name, c, obuf, exp):
    ncols = c["N"] // 2 if c["out"] == "geglu" else c["N"]
    assert obuf[:, ncols:].isnan().all(), f"{name}: padding columns beyond N were written"
    got = obuf[:, :ncols]
    if c["out"] == "geglu":
        _check_geglu_pointwise(name, got, exp["value"], exp["gate"])
        return
    assert torch.equal(got, exp["out"]), f"{name}: {_first_mismatch(got, exp['out'])}"


def _assert_colstats(name, c, cs, exp):
    want = exp["colstats"]
    if c["mode"] == "phase":
        # the blocks of a frame are written in an order the header leaves open: compare them as a multiset per frame
        per = 2 * (c["Ho"] * c["Wo"] // 64)
        N = c["N"]

        def canon(t):
            t = t.reshape(c["frames"], per // 2, 2 * N)                 # one row per block: (sums | sums of squares)
            return torch.stack([f[sorted(range(f.shape[0]), key=lambda i: f[i].tolist())] for f in t])
        cs, want = canon(cs), canon(want)
        cs, want = cs.reshape(-1, N), want.reshape(-1, N)
    assert torch.equal(cs, want), f"{name}: column statistics: {_first_mismatch(cs, want)}"


# =====================================================================================================================
# 1. the covering sweep
# =====================================================================================================================
_ROWS, _ALLOWED, _EXCLUDED = G.sweep_rows()


@pytest.mark.parametrize("i", range(len(_ROWS)), ids=[G.row_id(i, r) for i, r in enumerate(_ROWS)])
def test_descriptor_row(gpu, i):
    r = _ROWS[i]
    c = G.sweep_case(r)
    o = G.make_operands(c, seed=1000 + i)
    exp = G.expected(c, o)                     # raises InexactCase before anything reaches the GPU
    name = G.row_id(i, r)
    obuf, cs = _launch(c, o, gpu)
    _assert_out(name, c, obuf, exp)
    if c["colstats"]:
        _assert_colstats(name, c, cs, exp)
    if c["sched"] & 1:                         # the reversed tile walk is pure scheduling: the same bits as its twin
        twin, tcs = _launch(c, o, gpu, sched=0)
        assert torch.equal(twin.nan_to_num(nan=12345.0), obuf.nan_to_num(nan=12345.0)), f"{name}: sched=1 differs from sched=0"
        if c["colstats"] and c["mode"] != "phase":
            assert torch.equal(tcs, cs), f"{name}: colstats of sched=1 differ from sched=0"


# =====================================================================================================================
# 2. split-K at every slice count
# =====================================================================================================================
def _run_splitk(name, c, gpu, seed, ws_slabs):
    """Runs the case on a NaN-filled workspace of `ws_slabs` slabs (+ one guard slab the library is not told about),
    asserts the output and returns the number of slabs the launch wrote."""
    o = G.make_operands(c, seed)
    exp = G.expected(c, o)
    M, N = c["M"], c["N"]
    slab = M * N
    ws = torch.full(((ws_slabs + 1) * slab,), NAN, dtype=torch.float32, device=gpu)
    obuf, _ = _launch(c, o, gpu, workspace=ws[:ws_slabs * slab])
    _assert_out(name, c, obuf, exp)
    written = ~ws.cpu().reshape(ws_slabs + 1, slab).isnan()
    ran = int(written.any(1).sum())
    assert written[:ran].all(), f"{name}: a slab among the first {ran} was only partly written"
    assert not written[ran:].any(), f"{name}: scratch beyond slab {ran} was written"
    return ran


_DIAL = G.splitk_dial()


@pytest.mark.parametrize("i", range(len(_DIAL)), ids=[c["name"] for c in _DIAL])
def test_splitk_finetune_rule(gpu, i):
    """sched bit 1 with a scratch of exactly s M N 4 bytes: s slices run (read off the sentinel), the result is the
    model's bits — unequal slices, trailing slices of length 0 and -1, slices that start inside a tap, both kernels, both
    operand types, and the reduce pass's own epilogue in every form."""
    c = _DIAL[i]
    ran = _run_splitk(c["name"], c, gpu, 5000 + i, c["s"])
    assert ran == c["s"], f"{c['name']}: {ran} slices ran, the case intends {c['s']}"


_INFER = G.splitk_inference()


@pytest.mark.parametrize("i", range(len(_INFER)), ids=[c["name"] for c in _INFER])
def test_splitk_inference_rule(gpu, i):
    """No sched bit, 65 resp. 88 tiles: 3 resp. 2 slices of K / slices >= 1920, on ragged M and N."""
    c = _INFER[i]
    ran = _run_splitk(c["name"], c, gpu, 7000 + i, 4)
    assert ran == c["s"], f"{c['name']}: {ran} slices ran, the case intends {c['s']}"
