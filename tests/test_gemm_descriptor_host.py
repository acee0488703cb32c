"""Host: the fp64 model of `gcd_gemm_desc` (tests/gemm_model.py) against independent torch on non-exact data, its
exactness guard, the covering arrays' properties and the split-K slice arithmetic.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import gemm_model as G


def _randn_operands(c, seed):
    """Non-exact operands of the right shapes: the exact ones with a random-normal fp64 value in every position."""
    g = torch.Generator().manual_seed(seed)
    o = G.make_operands(c, seed)
    return {k: torch.randn(v.shape, generator=g, dtype=torch.float64) for k, v in o.items()}


def _loop_reference(c, o):
    """The documented formulas, element by element where the model uses torch's convolutions: out[m, n] from explicit
    tap loops over a zero-padded NCHW tensor, the epilogue row by row."""
    M, N = c["M"], c["N"]
    a, w = o["a"], o["w"]
    m = c["mode"]
    if m == "plain":
        acc = torch.einsum("mk,nk->mn", a, w)
    elif m == "temporal":
        x = a.reshape(c["clips"], c["T"], c["HW"], c["Cin"])
        xp = F.pad(x, (0, 0, 0, 0, 1, 1))
        acc = sum(torch.einsum("bthc,nc->bthn", xp[:, kt:kt + c["T"]], w[:, :, kt, 0, 0]) for kt in range(3)).reshape(M, N)
    else:
        x = a.reshape(c["frames"], c["Hi"], c["Wi"], c["Cin"])
        if m in ("conv_up", "phase"):
            x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
        s = 2 if m in ("conv_s2", "conv_s2a") else 1
        xp = F.pad(x, (0, 0, 0, 2, 0, 2)) if m == "conv_s2a" else F.pad(x, (0, 0, 1, 1, 1, 1))
        Ho, Wo = c["Ho"], c["Wo"]
        acc = sum(torch.einsum("fyxc,nc->fyxn", xp[:, kh:kh + s * (Ho - 1) + 1:s, kw:kw + s * (Wo - 1) + 1:s], w[:, :, kh, kw])
                  for kh in range(3) for kw in range(3)).reshape(M, N)
    if c["out"] == "geglu":
        return acc + o["bias"] if c["bias"] else acc
    out = torch.empty(M, N, dtype=torch.float64)
    for i in range(M):
        v = acc[i].clone()
        if c["bias"]:
            v += o["bias"]
        if c["rpv"]:
            v += o["rowvec"][i // c["rpv"]]
        s_acc, s_r1, s_r2 = c["scales"]
        if c["alpha"] != "none":
            al = float(o["alpha"][i // c["rpa"]])
            s_acc, s_r2 = 1.0 - al, al
            if c["alpha"] == "b1":
                s_r1 = s_r1 * (1.0 - al)
        v *= s_acc
        if c["r1"] != "none":
            v += s_r1 * o["R1"][i]
        if c["r2"]:
            v += s_r2 * o["R2"][i]
        out[i] = v
    return out


_EPILOGUES = [
    dict(),
    dict(bias=True, rpv=37),
    dict(bias=True, r1="sep", scales=G.SCALES_SET),
    dict(r1="inplace", r2=True, scales=G.SCALES_SET, rpv=64),
    dict(bias=True, rpv=37, r1="sep", r2=True, alpha="b0", rpa=40, scales=G.SCALES_SET),
    dict(bias=True, rpv=256, r1="sep", r2=True, alpha="b1", rpa=40, scales=G.SCALES_SET),
    dict(bias=True, out="geglu"),
    dict(bias=True, out="f16", r2=True),
]


@pytest.mark.parametrize("mode", G.FACTORS["mode"])
def test_model_against_independent_torch(mode):
    """Every mode / geometry with every epilogue form, on random-normal fp64 data: model == explicit tap loops to fp64
    round-off, and the im2col gather x [N, K] matrix (what the guard re-evaluates) agrees with torch's convolutions."""
    for j, (medge, epi) in enumerate([(("sub", "ragged")[k % 2], e) for k, e in enumerate(_EPILOGUES)]):
        row = dict(mode=mode, knob=2, out="f32", bias=False, rowvec="none", r1="none", r2=False, scales="default",
                   alpha="none", bf16=False, padded=False, medge=medge, N=48 if epi.get("out") != "geglu" else 160,
                   kdiv=64, colstats=False, sched=0)
        c = G.complete_case({**G.case_of_row(row), **epi})
        o = _randn_operands(c, 11 * j + 1)
        got, ref = G.model(c, o), _loop_reference(c, o)
        assert got.shape == ref.shape == (c["M"], c["N"])
        err = float((got - ref).abs().max() / ref.abs().max())
        assert err < 1e-12, (mode, epi, err)
        acc = G.im2col(c, o["a"]) @ G.weights_2d(c, o["w"]).T
        ref_acc = G.contraction(c, o["a"], o["w"])
        assert float((acc - ref_acc).abs().max() / ref_acc.abs().max()) < 1e-12, (mode, "im2col")
        assert float((G.epilogue(c, o, ref_acc, 1) - G.epilogue(c, o, ref_acc, 0)).abs().max()) < 1e-9 * float(ref.abs().max())


def test_model_column_sums():
    row = dict(mode="plain", knob=2, out="f32", bias=True, rowvec="tile", r1="sep", r2=False, scales="set", alpha="b1",
               bf16=False, padded=False, medge="full", N=320, kdiv=64, colstats=True, sched=0)
    c = G.case_of_row(row)
    o = G.make_operands(c, 3)
    exp = G.expected(c, o)
    out = exp["out"].double()
    cs = exp["colstats"].double()
    assert cs.shape == (2 * c["M"] // 64, c["N"])
    for b in range(c["M"] // 64):
        blk = out[64 * b:64 * b + 64]
        assert torch.equal(cs[2 * b], blk.sum(0)) and torch.equal(cs[2 * b + 1], (blk * blk).sum(0))
    # the phase form: blocks of 64 low-res tokens of one phase; the per-frame totals are those of the frame's rows
    row.update(mode="phase", rowvec="none", r1="none", alpha="none")
    c = G.case_of_row(row)
    exp = G.expected(c, G.make_operands(c, 4))
    per = c["Ho"] * c["Wo"]
    cs = exp["colstats"].double().reshape(c["frames"], per // 64, 2, c["N"])
    out = exp["out"].double().reshape(c["frames"], per, c["N"])
    assert torch.equal(cs[:, :, 0].sum(1), out.sum(1)) and torch.equal(cs[:, :, 1].sum(1), (out * out).sum(1))
    blk = G.colstats_blocks(c, torch.arange(c["M"], dtype=torch.float64)[:, None].expand(c["M"], 2))[:, :, 0]
    y, x = (blk[0] % per) // c["Wo"], (blk[0] % per) % c["Wo"]
    assert bool((y % 2 == 0).all()) and bool((x % 2 == 0).all()) and sorted(blk.flatten().tolist()) == list(range(c["M"]))


def test_exactness_guard_trips():
    row = dict(mode="conv_s2", knob=2, out="f16", bias=True, rowvec="ragged", r1="sep", r2=True, scales="set", alpha="b1",
               bf16=False, padded=False, medge="ragged", N=48, kdiv=32, colstats=False, sched=0)
    c = G.case_of_row(row)
    o = G.make_operands(c, 5)
    G.expected(c, o)                                            # the exact set passes
    for key, make in (("a", lambda t: t / 3.0),                 # not representable in fp16
                      ("a", lambda t: t * 1024.0 + (t == 0) * 2.0 ** -10),      # fp16-exact, but the sums span more than 24 bits
                      ("bias", lambda t: t + 0.1),              # an inexact addend
                      ("alpha", lambda t: t * 0 + 0.3),         # a non-dyadic blend factor
                      ("R1", lambda t: t * (1 + 2.0 ** -20))):  # 1/8 . (1 + 2^-20): the scaled residual rounds in fp32
        bad = dict(o)
        bad[key] = make(o[key])
        with pytest.raises(G.InexactCase):
            G.expected(c, bad)
    cb = dict(c, bf16=True)
    bad = dict(o)
    bad["a"] = o["a"] + 0.001953125 * (o["a"] == 3)            # 3 + 2^-9: fp16-exact, not bf16-exact
    with pytest.raises(G.InexactCase):
        G.expected(cb, bad)


def test_covering_array_properties():
    rows, allowed, excluded = G.sweep_rows()
    n_array = len(rows) - len(G.DIRECTED_ROWS)
    print(f"descriptor sweep: {n_array} covering rows + {len(G.DIRECTED_ROWS)} directed, {len(allowed)} pairs covered, "
          f"{len(excluded)} pairs excluded by the static rules")
    assert 60 <= n_array <= 120
    for r in rows:                                              # no row needs a run-time skip: each satisfies every rule
        assert G._violated({k: v for k, v in r.items() if k in G.FACTORS}, G.RULES) is None, r
        assert all(r[f] in lv for f, lv in G.FACTORS.items())
    got = G.covered_pairs(rows[:n_array], G.FACTORS)
    assert allowed <= got, sorted(allowed - got, key=repr)[:5]
    assert not (got & excluded)
    times = {p: 0 for p in allowed}                             # the two passes: every pair in at least two rows
    for r in rows[:n_array]:
        for p in G._pairs_of(r, list(G.FACTORS)):
            times[p] += 1
    assert min(times.values()) >= 2
    # every excluded pair is excluded BY a rule: no valid completion exists, and a rule text says why
    total = sum(len(a) * len(b) for i, a in enumerate(G.FACTORS.values()) for b in list(G.FACTORS.values())[i + 1:])
    assert len(allowed) + len(excluded) == total
    for fi, li, fj, lj in excluded:
        assert G._complete({fi: li, fj: lj}, G.FACTORS, G.RULES, None) is None
    # deterministic
    again, _, _ = G.sweep_rows()
    assert again == rows
    # every level of every factor is in the array
    for f, lv in G.FACTORS.items():
        assert {r[f] for r in rows} == set(lv), f
    # every generated case is exact (the guard would otherwise stop the GPU test) — checked for a sample here, the GPU
    # test runs the guard on every row
    for i in range(0, len(rows), 9):
        c = G.sweep_case(rows[i])
        G.expected(c, G.make_operands(c, 1000 + i))


def test_epilogue_array_and_dial():
    rows, allowed, excluded = G.epi_rows()
    assert allowed <= G.covered_pairs(rows, G.EPI_FACTORS)
    print(f"reduce epilogue: {len(rows)} rows, {len(excluded)} pairs excluded")
    dial = G.splitk_dial()
    assert {c["s"] for c in dial} == set(range(2, 33))
    assert {(c["sub"], c["bf16"]) for c in dial} == {(32, False), (32, True), (64, False), (64, True)}
    assert {c["mode"] for c in dial} >= {"plain", "conv_s1", "temporal"}
    seen = set()
    for c in dial:
        # the documented fine-tune rule picks exactly the intended count from a scratch of s M N 4 bytes
        assert G.finetune_slices(c["M"], c["N"], c["K"], c["s"] * c["M"] * c["N"] * 4) == c["s"], c["name"]
        # which kernel takes it: the 8-phase one needs K % 64 == 0 and, with bf16 operands, no second residual
        assert c["sub"] == (64 if c["K"] % 64 == 0 and not (c["bf16"] and c["r2"]) else 32), c["name"]
        if c["mode"] != "plain":
            assert c["Cin"] % 32 == 0 and c["K"] == (3 if c["mode"] == "temporal" else 9) * c["Cin"]
        seen |= {k for k in ("out", "rpv", "alpha", "r1", "padded") if c[k] not in (0, "none", False, "f32")}
        seen |= {f"alpha={c['alpha']}", f"r1={c['r1']}", f"scales={c['scales'] != G.DEFAULT_SCALES}"}
    assert seen >= {"out", "rpv", "padded", "alpha=b0", "alpha=b1", "r1=inplace", "r1=sep", "scales=True"}
    for c in G.splitk_inference():
        tiles = ((c["M"] + 255) // 256) * ((c["N"] + 319) // 320)
        assert min(4, 256 // tiles) == c["s"] and tiles <= 96 and c["K"] // c["s"] >= 1920
        assert c["K"] - 64 * c["s"] < 1920 * c["s"] and c["M"] % 16 and c["N"] % 320      # K just large enough; ragged


def test_slice_arithmetic():
    """per = ceil(subtiles / s): the lengths each (K, s) of the GPU test produces, with the intended 0 / negative tail."""
    assert G.slice_lengths(7744, 12, 64) == [11] * 11 + [0]
    assert G.slice_lengths(14112, 22, 32) == [21] * 21 + [0]
    assert G.slice_lengths(14752, 23, 32) == [21] * 21 + [20, -1]
    assert G.slice_lengths(4608, 5, 64) == [15, 15, 15, 15, 12]          # Cin = 512: slices start at k = 960 = tap 1 + 448
    assert (15 * 64) % 512 != 0 and (23 * 32) % 480 != 0 and (17 * 64) % 1408 != 0
    unequal = 0
    for c in G.splitk_dial() + G.splitk_inference():
        ln = G.slice_lengths(c["K"], c["s"], c["sub"])
        assert len(ln) == c["s"] and sum(max(v, 0) for v in ln) == c["K"] // c["sub"] and all(v > 0 for v in ln[:-1]), c["name"]
        if c["tail"] is None:
            assert ln[-1] > 0, c["name"]
        else:
            assert ln[-1] == c["tail"], c["name"]
        unequal += len(set(ln)) > 1
        if c["name"].startswith("s"):
            assert len(set(ln)) > 1, c["name"]                          # the dial's own cases: never divisible
    assert unequal >= 31
