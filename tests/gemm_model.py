"""An fp64 model of `gcd_gemm_desc` (include/gcd_amd.h), exact operands for it, and the covering arrays of its tests.

The model is plain torch on the CPU, written from the header's documentation: weights in the REFERENCE layout
([N, K], [Cout, Cin, 3, 3], [Cout, Cin, 3, 1, 1]), activations token-major, the contraction through `a @ w.T`,
`F.conv2d` (stride / padding, the asymmetric-pad form, nearest x2 upsample) or `F.conv3d`, then the documented epilogue

    out = s_acc * (acc + bias + rowvec[m // rows_per_vec]) + s_r1 * R1 + s_r2 * R2

with the `frame_alpha` substitution, the fp32 / fp16 / GEGLU output kinds and the per-64-row column sums.

Exact operands.  `make_operands` draws small integers for A and W, multiples of 1/8 for every addend and dyadic scales
and blend factors, seeded and independent per position.  Every intermediate of any correct evaluation order is then
exactly representable in fp32, so the kernels are compared with `torch.equal`, not with a tolerance.  `expected` is the
guard of that claim: it evaluates the model a second and third time in fp32 (natural and reversed K through an explicit
im2col gather, the epilogue addends in two orders), bounds every partial sum by sum |a| |w| < 2^24, and raises
`InexactCase` unless all evaluations agree with the fp64 result bit for bit.  A case that is not order-independent is
a mistake of the test and never reaches a GPU assertion.

A case is a dict:
    mode     plain | conv_s1 | conv_s2 | conv_s2a (asymmetric pad) | conv_up (gathered x2) | phase (upsample = 2) | temporal
    M N K Cin, frames Hi Wi Ho Wo (conv), clips T HW (temporal)
    out      f32 | f16 | geglu          bias  bool          rpv  rows_per_vec, 0 = no rowvec
    r1       none | sep | inplace       r2    bool          scales (s_acc, s_r1, s_r2)
    alpha    none | b0 | b1 (r1_blend)  rpa   rows_per_alpha
    bf16, padded, colstats, sched, knob
"""
from __future__ import annotations

import functools
import random
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F


class InexactCase(AssertionError):
    """The operands of a case are not order-independent in fp32: the test is wrong, not the kernel."""


CONV_MODES = ("conv_s1", "conv_s2", "conv_s2a", "conv_up", "phase")
DEFAULT_SCALES = (1.0, 1.0, 1.0)


def complete_case(c: dict) -> dict:
    """Fill the epilogue / layout keys a hand-written case leaves out with their neutral values."""
    d = dict(out="f32", bias=False, rpv=0, r1="none", r2=False, scales=DEFAULT_SCALES, alpha="none", rpa=1,
             bf16=False, padded=False, colstats=False, sched=0, knob=0, sparse_w=False, small=False)
    d.update(c)
    if d["out"] == "geglu":
        d["sparse_w"] = True
    if d["colstats"]:
        d["small"] = True
    return d


def rows_in(c: dict) -> int:
    """Rows of the token-major activation A."""
    if c["mode"] in CONV_MODES:
        return c["frames"] * c["Hi"] * c["Wi"]
    return c["M"]


def conv_args(c: dict) -> Optional[dict]:
    """The `conv=` argument of ops.gemm for a case."""
    m = c["mode"]
    if m == "plain":
        return None
    if m == "temporal":
        return dict(Cin=c["Cin"], T=c["T"], HW=c["HW"])
    return dict(Cin=c["Cin"], Hi=c["Hi"], Wi=c["Wi"], Ho=c["Ho"], Wo=c["Wo"], stride=2 if m in ("conv_s2", "conv_s2a") else 1,
                upsample={"conv_up": 1, "phase": 2}.get(m, 0), asym_pad=int(m == "conv_s2a"))


# ---------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------
def make_operands(c: dict, seed: int) -> dict:
    """fp64 CPU tensors holding exactly representable values (see the module docstring).  `small` (the column-statistics
    cases, whose sums of SQUARES must stay exact too): entries of A, W in -1 .. 1, addends in halves, blend factors in
    halves.  `sparse_w` (GEGLU): about six +-1 entries per weight row, so value and gate stay within +-16 and the product
    within fp16 range."""
    g = torch.Generator().manual_seed(seed)

    def ri(shape, lo, hi):
        return torch.randint(lo, hi + 1, shape, generator=g).double()

    M, N, K = c["M"], c["N"], c["K"]
    amp = 1 if c["small"] else 3
    den, top = (2.0, 4) if c["small"] else (8.0, 16)
    o = {}
    o["a"] = ri((rows_in(c), c["Cin"] if c["mode"] != "plain" else K), -amp, amp)
    if c["mode"] == "plain":
        wshape = (N, K)
    elif c["mode"] == "temporal":
        wshape = (N, c["Cin"], 3, 1, 1)
    else:
        wshape = (N, c["Cin"], 3, 3)
    w = ri(wshape, -amp, amp)
    if c["sparse_w"]:
        per_row = w[0].numel()
        keep = torch.rand(wshape, generator=g) < 6.0 / per_row
        w = torch.where(keep, torch.where(w >= 0, 1.0, -1.0).double(), torch.zeros_like(w))
    o["w"] = w
    o["bias"] = ri((N,), -top, top) / den
    if c["rpv"]:
        o["rowvec"] = ri(((M + c["rpv"] - 1) // c["rpv"], N), -top, top) / den
    if c["r1"] != "none":
        o["R1"] = ri((M, N), -4 * top, 4 * top) / den
    if c["r2"]:
        o["R2"] = ri((M, N), -4 * top, 4 * top) / den
    if c["alpha"] != "none":
        steps = 2 if c["small"] else 4
        o["alpha"] = ri(((M + c["rpa"] - 1) // c["rpa"],), 0, steps) / steps
    return o


# ---------------------------------------------------------------------------------------------------------------------
# contraction: fp64 through torch's own convolutions; and the explicit gather + [N, K] matrix for the fp32 re-evaluation
# ---------------------------------------------------------------------------------------------------------------------
def contraction(c: dict, a: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """acc [M, N] in the dtype of a / w (fp64 in the model)."""
    m, M, N = c["mode"], c["M"], c["N"]
    if m == "plain":
        return a @ w.T
    if m == "temporal":
        x = a.reshape(c["clips"], c["T"], c["HW"], c["Cin"]).permute(0, 3, 1, 2)[..., None]     # [clips, Cin, T, HW, 1]
        y = F.conv3d(x, w, padding=(1, 0, 0))
        return y.permute(0, 2, 3, 1, 4).reshape(M, N)
    x = a.reshape(c["frames"], c["Hi"], c["Wi"], c["Cin"]).permute(0, 3, 1, 2)
    if m in ("conv_up", "phase"):
        y = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1)
    elif m == "conv_s2a":
        y = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2)
    else:
        y = F.conv2d(x, w, stride=2 if m == "conv_s2" else 1, padding=1)
    assert tuple(y.shape[2:]) == (c["Ho"], c["Wo"]), (tuple(y.shape), c["Ho"], c["Wo"])
    return y.permute(0, 2, 3, 1).reshape(M, N)


def im2col(c: dict, a: torch.Tensor) -> torch.Tensor:
    """The implicit GEMM's A operand [M, K] as the header words it: K order (kh, kw, cin) resp. (kt, cin), zeros where a
    tap leaves the image / the clip."""
    m, M = c["mode"], c["M"]
    if m == "plain":
        return a
    rows = torch.arange(M)
    cols = []
    if m == "temporal":
        T, HW = c["T"], c["HW"]
        t = (rows // HW) % T
        for kt in range(3):
            tt = t + kt - 1
            ok = (tt >= 0) & (tt < T)
            src = (rows + (kt - 1) * HW).clamp(0, M - 1)
            cols.append(torch.where(ok[:, None], a[src], torch.zeros((), dtype=a.dtype)))
        return torch.cat(cols, 1)
    Hi, Wi, Ho, Wo = c["Hi"], c["Wi"], c["Ho"], c["Wo"]
    f = rows // (Ho * Wo)
    rem = rows % (Ho * Wo)
    y, x = rem // Wo, rem % Wo
    for kh in range(3):
        for kw in range(3):
            if m in ("conv_up", "phase"):
                uy, ux = y + kh - 1, x + kw - 1
                ok = (uy >= 0) & (uy < Ho) & (ux >= 0) & (ux < Wo)
                iy, ix = uy.clamp(0) // 2, ux.clamp(0) // 2
            else:
                s = 2 if m in ("conv_s2", "conv_s2a") else 1
                off = 0 if m == "conv_s2a" else -1
                iy, ix = y * s + kh + off, x * s + kw + off
                ok = (iy >= 0) & (iy < Hi) & (ix >= 0) & (ix < Wi)
            src = (f * Hi + iy.clamp(0, Hi - 1)) * Wi + ix.clamp(0, Wi - 1)
            cols.append(torch.where(ok[:, None], a[src], torch.zeros((), dtype=a.dtype)))
    return torch.cat(cols, 1)


def weights_2d(c: dict, w: torch.Tensor) -> torch.Tensor:
    """Reference-layout weights as the [N, K] matrix that goes with `im2col`."""
    m = c["mode"]
    if m == "plain":
        return w
    if m == "temporal":
        return w.reshape(w.shape[0], w.shape[1], 3).permute(0, 2, 1).reshape(w.shape[0], -1)
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


# ---------------------------------------------------------------------------------------------------------------------
# epilogue
# ---------------------------------------------------------------------------------------------------------------------
def epilogue(c: dict, o: dict, acc: torch.Tensor, order: int = 0) -> torch.Tensor:
    """The documented epilogue in acc's dtype.  order 1 adds the same terms in another order (for the guard)."""
    dt = acc.dtype
    M = acc.shape[0]
    rows = torch.arange(M)
    bias = o["bias"].to(dt)[None, :] if c["bias"] else None
    rv = o["rowvec"].to(dt)[rows // c["rpv"]] if c["rpv"] else None
    R1 = o["R1"].to(dt) if c["r1"] != "none" else None
    R2 = o["R2"].to(dt) if c["r2"] else None
    s_acc, s_r1, s_r2 = (torch.tensor(s, dtype=dt) for s in c["scales"])
    if c["alpha"] != "none":
        al = o["alpha"].to(dt)[rows // c["rpa"]][:, None]
        s_acc, s_r2 = 1 - al, al
        if c["alpha"] == "b1":
            s_r1 = s_r1 * (1 - al)
    if order == 0:
        v = acc
        if bias is not None:
            v = v + bias
        if rv is not None:
            v = v + rv
        v = s_acc * v
        if R1 is not None:
            v = v + s_r1 * R1
        if R2 is not None:
            v = v + s_r2 * R2
        return v
    add = None
    for t in (rv, bias):
        if t is not None:
            add = t if add is None else add + t
    v = acc if add is None else add + acc
    res = None
    for s, t in ((s_r2, R2), (s_r1, R1)):
        if t is not None:
            res = t * s if res is None else res + t * s
    v = v * s_acc
    return v if res is None else res + v


def model(c: dict, o: dict) -> torch.Tensor:
    """fp64 `out` [M, N] before the output conversion (GEGLU: acc + bias, [value columns | gate columns])."""
    acc = contraction(c, o["a"], o["w"])
    if c["out"] == "geglu":
        return acc + o["bias"][None, :] if c["bias"] else acc
    return epilogue(c, o, acc)


def colstats_blocks(c: dict, out: torch.Tensor) -> torch.Tensor:
    """out [M, N] -> [M / 64, 64, N]: the rows of each statistics block.  The phase form sums 64 consecutive LOW-RES
    tokens of one phase (py, px); which block of a frame holds which of them is left open by the header."""
    M, N = out.shape
    if c["mode"] != "phase":
        return out.reshape(M // 64, 64, N)
    Hi, Wi, Wo = c["Hi"], c["Wi"], c["Wo"]
    idx = []
    for f in range(c["frames"]):
        for py in range(2):
            for px in range(2):
                for i in range(Hi):
                    for j in range(Wi):
                        idx.append(f * 4 * Hi * Wi + (2 * i + py) * Wo + 2 * j + px)
    return out[torch.tensor(idx)].reshape(M // 64, 64, N)


def expected(c: dict, o: dict) -> dict:
    """The exactness guard and the expected tensors:
        out       [M, N] in the output dtype (fp32 / fp16), or for GEGLU `value`, `gate` [M, N / 2] fp64 (exact)
        colstats  [2 M / 64, N] fp32 when the case asks for them (phase form: see `colstats_blocks`)
    Raises InexactCase unless the fp64 model and two fp32 evaluations in different summation orders agree bit for bit."""
    a, w = o["a"], o["w"]
    lim = torch.bfloat16 if c["bf16"] else torch.float16
    for name, t in (("A", a), ("W", w)):
        if not torch.equal(t.to(lim).double(), t):
            raise InexactCase(f"{name} is not representable in {lim}")
    acc64 = contraction(c, a, w)
    col, w2 = im2col(c, a.float()), weights_2d(c, w.float())
    if float((col.abs() @ w2.abs().T).max()) >= 2.0 ** 24:
        raise InexactCase("sum |a| |w| reaches 2^24: a partial sum of some order may round")
    accs = (col @ w2.T, col.flip(1) @ w2.flip(1).T)
    for acc in accs:
        if not torch.equal(acc.double(), acc64):
            raise InexactCase("the fp32 contraction depends on the summation order")
    res = {}
    if c["out"] == "geglu":
        t64 = acc64 + o["bias"][None, :] if c["bias"] else acc64
        t32 = accs[1] + o["bias"].float()[None, :] if c["bias"] else accs[1]
        if not torch.equal(t32.double(), t64):
            raise InexactCase("GEGLU value / gate are not exact in fp32")
        inner = c["N"] // 2
        res["value"], res["gate"] = t64[:, :inner], t64[:, inner:]
        return res
    out64 = epilogue(c, o, acc64)
    for acc, order in zip(accs, (0, 1)):
        if not torch.equal(epilogue(c, o, acc, order).double(), out64):
            raise InexactCase(f"the fp32 epilogue (term order {order}) differs from fp64")
    res["out"] = out64.to(torch.float16 if c["out"] == "f16" else torch.float32)
    if c["colstats"]:
        blk = colstats_blocks(c, out64)
        unit = next((u for u in (1, 2, 4, 8, 16, 32, 64) if torch.equal((blk * u).round(), blk * u)), None)
        if unit is None or float(((blk * unit) ** 2).sum(1).max()) >= 2.0 ** 24:
            raise InexactCase("the per-block sums of squares are not exact in fp32")
        s64, q64 = blk.sum(1), (blk * blk).sum(1)
        b32 = blk.float()
        for t in (b32, b32.flip(1)):
            if not (torch.equal(t.sum(1).double(), s64) and torch.equal((t * t).sum(1).double(), q64)):
                raise InexactCase("the fp32 column statistics depend on the summation order")
        res["colstats"] = torch.stack([s64, q64], 1).reshape(-1, c["N"]).float()
    return res


# ---------------------------------------------------------------------------------------------------------------------
# covering arrays
# ---------------------------------------------------------------------------------------------------------------------
# (the refusal it mirrors, the levels that trigger it, the levels each other factor may then take)
Rule = Tuple[str, Dict[str, list], Dict[str, list]]


def _violated(row: dict, rules: Sequence[Rule]) -> Optional[str]:
    """The text of the first rule a (partial) row breaks: its trigger levels are all there and a factor it constrains
    holds another level than it allows.  Factors not yet in the row break nothing."""
    for text, when, then in rules:
        if all(f in row and row[f] in lv for f, lv in when.items()) and any(f in row and row[f] not in lv for f, lv in then.items()):
            return text
    return None


def _complete(row: dict, factors: Dict[str, list], rules: Sequence[Rule], rng: Optional[random.Random]) -> Optional[dict]:
    """Depth-first completion of a partial row under the rules (exhaustive: None means no row holds it)."""
    if _violated(row, rules):
        return None
    todo = [f for f in factors if f not in row]
    if not todo:
        return dict(row)
    f = todo[0]
    levels = list(factors[f])
    if rng is not None:
        rng.shuffle(levels)
    for lv in levels:
        row[f] = lv
        got = _complete(row, factors, rules, rng)
        del row[f]
        if got is not None:
            return got
    return None


def _pairs_of(row: dict, names: List[str]):
    return {(names[i], row[names[i]], names[j], row[names[j]]) for i in range(len(names)) for j in range(i + 1, len(names))}


def covering_array(factors: Dict[str, list], rules: Sequence[Rule], seed: int, candidates: int = 48, passes: int = 1):
    """A deterministic greedy pairwise covering array.  -> (rows, allowed pairs, excluded pairs): every pair of levels
    that some row satisfying all rules can hold is in `allowed` and appears in at least one row; `excluded` are the
    pairs no valid row holds.  passes > 1 appends that many independent arrays: every allowed pair then appears in
    several rows, in different company."""
    names = list(factors)
    allowed, excluded = set(), set()
    for i in range(len(names)):
        for j in range(i + 1, len(names)):
            for li in factors[names[i]]:
                for lj in factors[names[j]]:
                    p = (names[i], li, names[j], lj)
                    (allowed if _complete({names[i]: li, names[j]: lj}, factors, rules, None) is not None else excluded).add(p)
    rng = random.Random(seed)
    order = sorted(allowed, key=repr)
    todo = set()
    rows = []
    while todo or passes > 0:
        if not todo:
            todo, passes = set(allowed), passes - 1
        fi, li, fj, lj = next(p for p in order if p in todo)
        best, best_gain = None, -1
        for _ in range(candidates):
            cand = _complete({fi: li, fj: lj}, factors, rules, rng)
            gain = len(_pairs_of(cand, names) & todo)
            if gain > best_gain:
                best, best_gain = cand, gain
        rows.append({n: best[n] for n in names})
        todo -= _pairs_of(best, names)
    return rows, allowed, excluded


def covered_pairs(rows: Sequence[dict], factors: Dict[str, list]) -> set:
    names = list(factors)
    got = set()
    for r in rows:
        got |= _pairs_of(r, names)
    return got


# ---- the descriptor sweep ------------------------------------------------------------------------------------------
FACTORS = {
    "mode": ["plain", "conv_s1", "conv_s2", "conv_s2a", "conv_up", "phase", "temporal"],
    "knob": [0, 2, 3, 6],                  # GCD_TUNE_GEMM_IMPL: automatic, tile kernels, ring kernel only, general 64-row
    "out": ["f32", "f16", "geglu"],
    "bias": [False, True],
    "rowvec": ["none", "tile", "div", "ragged"],   # rows_per_vec 256 (uniform over a tile), 64 (divides it), 37
    "r1": ["none", "sep", "inplace"],
    "r2": [False, True],
    "scales": ["default", "set"],
    "alpha": ["none", "b0", "b1"],         # frame_alpha with r1_blend 0 / 1
    "bf16": [False, True],
    "padded": [False, True],
    "medge": ["sub", "ragged", "full"],    # less than one tile / ragged / whole 256-row tiles
    "N": [16, 48, 160, 320, 336],
    "kdiv": [32, 64],                      # K (and Cin) a multiple of 32 only / of 64
    "colstats": [False, True],
    "sched": [0, 1],
}

RULES: List[Rule] = [
    ("gcd_gemm_f16: GEGLU takes bias only",
     {"out": ["geglu"]}, {"rowvec": ["none"], "r1": ["none"], "r2": [False]}),
    ("GCD_OUT_GEGLU is documented as out = a * gelu(g): it has no scale or blend inputs",
     {"out": ["geglu"]}, {"scales": ["default"], "alpha": ["none"]}),
    ("gcd_gemm_f16: GEGLU needs N %% 32 == 0 (N=%d)",
     {"out": ["geglu"]}, {"N": [160, 320]}),
    ("gcd_gemm_f16: bf16 operands are implemented for fp32 output, without fused LayerNorm / colstats / blocked layouts",
     {"bf16": [True]}, {"out": ["f32"], "colstats": [False]}),
    ("gcd_gemm_f16: bf16 operands with mode %d / K=%d need the ping-pong kernel, which the shape or "
     "GCD_TUNE_GEMM_IMPL=%d rules out",
     {"bf16": [True], "knob": [6]}, {"mode": ["plain"]}),
    ("gcd_gemm_f16: upsample=2 (phase form) writes fp32 rows + bias only: no residual, per-frame vector, blend, "
     "fp16 / GEGLU output or bf16 operands",
     {"mode": ["phase"]}, {"out": ["f32"], "rowvec": ["none"], "r1": ["none"], "r2": [False], "alpha": ["none"], "bf16": [False]}),
    ("gcd_gemm_f16: upsample=2 (phase form) needs the 8-phase 256x320 tile kernel, which the shape (%lld tiles: the "
     "automatic choice takes the general kernel or split-K) or GCD_TUNE_GEMM_IMPL=%d rules out",
     {"mode": ["phase"]}, {"knob": [2]}),
    ("gcd_gemm_f16: upsample=2 (phase form) needs Cin %% 64 == 0 and K == 4*Cin (Cin=%d K=%d)",
     {"mode": ["phase"]}, {"kdiv": [64]}),
    ("gcd_gemm_f16: K=%d (Cin=%d) needs the ping-pong kernel, which the shape or GCD_TUNE_GEMM_IMPL=%d rules out",
     {"knob": [6]}, {"kdiv": [64]}),
    ("gcd_gemm_f16: colstats cannot be honoured for this descriptor (M=%d N=%d; see gcd_gemm_colstats_supported): "
     "fp32 out, no second residual, M %% 256 == 0, N %% 320 == 0, rowvec / frame_alpha constant over each 256-row tile, "
     "a kernel choice that lands on the 256x320 tile kernels",
     {"colstats": [True]}, {"out": ["f32"], "r2": [False], "medge": ["full"], "N": [320], "rowvec": ["none", "tile"], "knob": [2, 3]}),
    ("R1 is an fp32 tensor: it can alias only an fp32 `out`",
     {"r1": ["inplace"]}, {"out": ["f32"]}),
]

SCALES_SET = (0.5, -2.0, 0.25)
SCALES_SET_SMALL = (-2.0, 2.0, 1.0)          # column-statistics rows: results stay in quarters

_PLAIN_M = {"sub": 77, "ragged": 2 * 256 + 77, "full": 512}
_PLAIN_K = {32: 352, 64: 448}
# (frames, Hi, Wi, Ho, Wo) per M edge; `full` of conv_s1 is 4 x 64 so that the halo-panel K loop of gemm_p8.hip takes it
_CONV_GEOM = {
    "conv_s1": {"sub": (3, 8, 8, 8, 8), "ragged": (7, 5, 8, 5, 8), "full": (2, 4, 64, 4, 64)},
    "conv_s2": {"sub": (3, 16, 16, 8, 8), "ragged": (7, 9, 15, 5, 8), "full": (4, 16, 32, 8, 16)},
    "conv_s2a": {"sub": (3, 16, 16, 8, 8), "ragged": (7, 10, 16, 5, 8), "full": (4, 16, 32, 8, 16)},
    "conv_up": {"sub": (3, 4, 4, 8, 8), "ragged": (5, 3, 5, 6, 10), "full": (4, 4, 8, 8, 16)},
    # the phase form walks LOW-RES tokens: 64 / 280 / 256 of them (M = 4 x that is always a multiple of 32)
    "phase": {"sub": (2, 4, 8, 8, 16), "ragged": (7, 5, 8, 10, 16), "full": (1, 16, 16, 32, 32)},
}
_TEMPORAL_GEOM = {"sub": (1, 5, 15), "ragged": (17, 3, 11), "full": (2, 4, 64)}      # (clips, T, HW)
_ROWVEC_PERIOD = {"none": 0, "tile": 256, "div": 64, "ragged": 37}


def case_of_row(r: dict) -> dict:
    """A covering-array row -> the smallest case that still has the row's edges."""
    c = dict(mode=r["mode"], N=r["N"], knob=r["knob"], out=r["out"], bias=r["bias"], r1=r["r1"], r2=r["r2"],
             alpha=r["alpha"], bf16=r["bf16"], padded=r["padded"], colstats=r["colstats"], sched=r["sched"])
    m = r["mode"]
    if m == "plain":
        c.update(M=_PLAIN_M[r["medge"]], K=_PLAIN_K[r["kdiv"]], Cin=0)
    elif m == "temporal":
        clips, T, HW = _TEMPORAL_GEOM[r["medge"]]
        cin = 96 if r["kdiv"] == 32 else 128
        c.update(clips=clips, T=T, HW=HW, M=clips * T * HW, Cin=cin, K=3 * cin)
    else:
        frames, Hi, Wi, Ho, Wo = _CONV_GEOM[m][r["medge"]]
        cin = r["kdiv"]                      # 32 or 64 channels per tap
        c.update(frames=frames, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo, M=frames * Ho * Wo, Cin=cin, K=(4 if m == "phase" else 9) * cin)
    c["rpv"] = _ROWVEC_PERIOD[r["rowvec"]]
    # frame_alpha on a period different from rowvec's: constant over a tile where the row allows it (the AlphaBlender
    # fast paths, and what column statistics need), ragged inside a tile otherwise
    if r["colstats"] and r["rowvec"] == "tile":
        c["rpa"] = 512
    elif r["medge"] == "full" and r["rowvec"] != "tile":
        c["rpa"] = 256
    else:
        c["rpa"] = 40
    c["scales"] = DEFAULT_SCALES if r["scales"] == "default" else (SCALES_SET_SMALL if r["colstats"] else SCALES_SET)
    return complete_case(c)


# Rows the pairwise array cannot be counted on to produce: each needs five or more levels at once.
DIRECTED_ROWS = [
    # the narrow output-head kernel (conv_narrow.hip): N = 16, stride 1, Cin 64 / 320, fp32 rows + bias, automatic choice
    dict(mode="conv_s1", knob=0, out="f32", bias=True, rowvec="none", r1="none", r2=False, scales="set", alpha="none",
         bf16=False, padded=True, medge="ragged", N=16, kdiv=64, colstats=False, sched=0),
    dict(mode="conv_s1", knob=0, out="f32", bias=True, rowvec="none", r1="none", r2=False, scales="default", alpha="none",
         bf16=False, padded=False, medge="sub", N=16, kdiv=64, colstats=False, sched=0, Cin=320),
    # the halo-panel K loop of the 8-phase kernel: full tiles of 4 x 64 frames, both residuals / column statistics
    dict(mode="conv_s1", knob=2, out="f32", bias=True, rowvec="tile", r1="sep", r2=True, scales="set", alpha="b1",
         bf16=False, padded=True, medge="full", N=336, kdiv=64, colstats=False, sched=0),
    dict(mode="conv_s1", knob=2, out="f32", bias=True, rowvec="tile", r1="inplace", r2=False, scales="set", alpha="b0",
         bf16=False, padded=False, medge="full", N=320, kdiv=64, colstats=True, sched=1),
]


@functools.lru_cache(maxsize=None)
def sweep_rows(seed: int = 20260):
    """-> (rows, allowed, excluded) of the descriptor sweep: two independent pairwise arrays, then the directed rows."""
    rows, allowed, excluded = covering_array(FACTORS, RULES, seed, passes=2)
    return rows + [dict(r) for r in DIRECTED_ROWS], allowed, excluded


def sweep_case(r: dict) -> dict:
    c = case_of_row({k: v for k, v in r.items() if k in FACTORS})
    if "Cin" in r:                           # a directed row with its own channel count
        c["Cin"], c["K"] = r["Cin"], 9 * r["Cin"]
    return c


def row_id(i: int, r: dict) -> str:
    bits = [f"{i:03d}", r["mode"], f"k{r['knob']}", r["out"], f"N{r['N']}", r["medge"], f"K{r['kdiv']}"]
    for key, tag in (("bias", "b"), ("r2", "r2"), ("bf16", "bf16"), ("padded", "pad"), ("colstats", "cs"), ("sched", "rev")):
        if r[key]:
            bits.append(tag)
    for key in ("rowvec", "r1", "alpha"):
        if r[key] != "none":
            bits.append(f"{key}={r[key]}")
    if r["scales"] != "default":
        bits.append("sc")
    return "-".join(bits)


# ---- split-K -------------------------------------------------------------------------------------------------------
def slice_lengths(K: int, s: int, sub: int) -> List[int]:
    """Length in `sub`-deep K sub-tiles (64: the 8-phase kernel, 32: the ring kernel) of each of the s slices as the
    kernels cut them: per = ceil(subtiles / s), slice z = [z per, min((z + 1) per, subtiles)).  Not clamped: a trailing
    slice can come out as 0 or negative, and its workgroups must still write a slab of zeros."""
    n = K // sub
    per = (n + s - 1) // s
    return [min(per, n - z * per) for z in range(s)]


def finetune_slices(M: int, N: int, K: int, workspace_bytes: int) -> int:
    """The slice count the fine-tune rule (gcd_gemm_desc.sched bit 1) is documented to choose: up to 32 slices of at
    least 640, as many as the scratch holds; 1 = no split."""
    tiles = ((M + 255) // 256) * ((N + 319) // 320)
    if tiles > 32 or K < 4096:
        return 1
    s = min(32, 256 // tiles)
    while s > 1 and (K // s < 640 or workspace_bytes < s * M * N * 4):
        s -= 1
    return s


EPI_FACTORS = {
    "out": ["f32", "f16"],
    "bias": [False, True],
    "rowvec": [False, True],                # period 37, ld_rowvec always padded
    "scales": ["default", "set"],
    "alpha": ["none", "b0", "b1"],
    "padded": [False, True],                # ldo / ldr1 / ldr2 (and lda)
    "r1": ["none", "sep", "inplace"],
    "r2": [False, True],
}
EPI_RULES: List[Rule] = [RULES[-1]]


@functools.lru_cache(maxsize=None)
def epi_rows(seed: int = 7):
    return covering_array(EPI_FACTORS, EPI_RULES, seed)


def _dial_K(s: int, ring: bool) -> int:
    """The smallest K >= max(4096, 640 s) of the kernel's residue mod 64 that gives slices of unequal, positive length."""
    sub, res = (32, 32) if ring else (64, 0)
    K = max(4096, 640 * s)
    K += (res - K) % 64
    while (K // sub) % s == 0 or slice_lengths(K, s, sub)[-1] <= 0:
        K += 64
    return K


def splitk_dial() -> List[dict]:
    """The fine-tune-rule cases: every slice count 2 .. 32 once with slices of unequal length, alternately on the
    8-phase kernel (K % 64 == 0) and the ring kernel (K % 64 == 32), then the directed ones.  Each case names the slice
    count it intends (`s`), the sub-tile depth of the kernel that must take it (`sub`) and whether it wants a trailing
    slice of length 0 or below (`tail`)."""
    cases = []
    for s in range(2, 33):
        ring = s % 2 == 1
        c = dict(mode="plain", M=200 if s % 3 else 300, N=176 if s % 4 else 336, K=_dial_K(s, ring), s=s,
                 sub=32 if ring else 64, bf16=s % 5 == 0, tail=None, name=f"s{s:02d}-{'ring' if ring else 'p8'}")
        if ((c["M"] + 255) // 256) * ((c["N"] + 319) // 320) * s > 256:
            c["M"], c["N"] = 200, 176
        cases.append(c)
    conv = dict(frames=3, Hi=8, Wi=8, Ho=8, Wo=8, M=192, N=176)
    temporal = dict(clips=4, T=3, HW=16, M=192, N=176)
    cases += [
        dict(mode="plain", M=200, N=176, K=4096, s=2, sub=64, name="equal-p8"),
        dict(mode="plain", M=200, N=336, K=7744, s=12, sub=64, tail=0, name="zero-tail-p8"),
        dict(mode="plain", M=200, N=176, K=14112, s=22, sub=32, tail=0, name="zero-tail-ring"),
        dict(mode="plain", M=300, N=176, K=14752, s=23, sub=32, tail=-1, name="negative-tail-ring"),
        dict(mode="plain", M=200, N=176, K=14752, s=23, sub=32, tail=-1, bf16=True, name="negative-tail-ring-bf16"),
        dict(mode="conv_s1", Cin=512, K=4608, s=5, sub=64, name="conv-midtap-p8", **conv),
        dict(mode="conv_s1", Cin=480, K=4320, s=6, sub=32, name="conv-midtap-ring", **conv),
        dict(mode="conv_s2a", Cin=512, K=4608, s=7, sub=64, name="conv-s2a-p8", bf16=True,
             frames=3, Hi=16, Wi=16, Ho=8, Wo=8, M=192, N=176),
        dict(mode="temporal", Cin=1408, K=4224, s=4, sub=64, name="temporal-p8", **temporal),
        dict(mode="temporal", Cin=1376, K=4128, s=5, sub=32, name="temporal-ring", **temporal),
        dict(mode="temporal", Cin=1408, K=4224, s=6, sub=64, bf16=True, name="temporal-p8-bf16", **temporal),
        # empty trailing slices in the conv modes: set_tile forms a tap index of 9 (3) there, which must stay unused
        dict(mode="conv_s1", Cin=1024, K=9216, s=13, sub=64, tail=0, name="conv-zero-tail-p8", **conv),
        dict(mode="conv_s1", Cin=1152, K=10368, s=16, sub=64, tail=-3, name="conv-negative-tail-p8", **conv),
        dict(mode="conv_s1", Cin=1568, K=14112, s=22, sub=32, tail=0, name="conv-zero-tail-ring", **conv),
        dict(mode="conv_s1", Cin=1952, K=17568, s=26, sub=32, tail=-1, name="conv-negative-tail-ring", **conv),
        dict(mode="temporal", Cin=3008, K=9024, s=14, sub=64, tail=-2, name="temporal-negative-tail-p8", **temporal),
        dict(mode="temporal", Cin=4704, K=14112, s=22, sub=32, tail=0, name="temporal-zero-tail-ring", **temporal),
        # bf16 with the second residual is not on the 8-phase kernel: the ring kernel at K % 64 == 0
        dict(mode="plain", M=200, N=176, K=4160, s=3, sub=32, bf16=True, force=dict(r2=True), name="bf16-r2-ring"),
    ]
    epi, _, _ = epi_rows()
    out = []
    for i, c in enumerate(cases):
        c.setdefault("bf16", False)
        c.setdefault("tail", None)
        c.setdefault("Cin", 0)
        j = i
        e = dict(epi[j % len(epi)])
        while c["bf16"] and e["out"] != "f32":                     # bf16 operands: fp32 output only
            j += 1
            e = dict(epi[j % len(epi)])
        e.update(c.pop("force", {}))
        if c["bf16"] and c["sub"] == 64:
            e["r2"] = False                                        # (keeps a bf16 case on the 8-phase kernel)
        c.update(out=e["out"], bias=e["bias"], rpv=37 if e["rowvec"] else 0, r1=e["r1"], r2=e["r2"],
                 scales=DEFAULT_SCALES if e["scales"] == "default" else SCALES_SET, alpha=e["alpha"], rpa=40,
                 padded=e["padded"], sched=2, knob=0)
        out.append(complete_case(c))
    return out


# The inference rule (no sched bit): min(4, 256 / tiles) slices for <= 96 tiles when K / slices >= 1920.
def splitk_inference() -> List[dict]:
    cases = [
        # 13 x 5 = 65 tiles -> 3 slices; K = 5824 = 91 k-tiles of 64: slices of 31, 31, 29
        dict(mode="plain", M=12 * 256 + 77, N=4 * 320 + 48, K=5824, s=3, sub=64, name="infer-3"),
        # 11 x 8 = 88 tiles -> 2 slices; K = 3872 = 121 sub-tiles of 32 (ring kernel): 61 + 60
        dict(mode="plain", M=10 * 256 + 77, N=7 * 320 + 48, K=3872, s=2, sub=32, name="infer-2"),
    ]
    out = []
    for c in cases:
        c.update(Cin=0, tail=None, out="f32", bias=True, rpv=1000, r1="sep", r2=True, alpha="b1", rpa=777, padded=True,
                 sched=0, knob=0)
        out.append(complete_case(c))
    return out
