"""Kernels across the 2^31- and 2^32-byte marks of an operand, and on both sides of the size limits they declare.

Part A.  A token-major operand gets a row stride of 65 536 bytes, so that row 32 768 starts at byte 2^31 and row 65 536 at
byte 2^32 while the compute stays that of ~66 k tokens of 64 (320) channels.  One operand at a time is far, inputs and outputs
alike, the others are compact; every operand is a view into a `memcontract.Arena` (512 guard rows on both sides, pad columns
and guards poisoned and compared as integers afterwards), so a wrapped or overhanging store lands in memory the test owns and
is reported as (row, column).  The reference is plain torch in fp64 over all rows, the bar is the entry's own
(test_kernels_gpu.py, as cited by test_memcontract_gpu.py), and the error is taken per row band — the first and last 256
rows, the 512 rows around each byte mark, the rest — so that one wrong band is not diluted.  `gcd_lnqkv_f16` and
`gcd_ff_fused_f16` keep their result below 2^31 bytes (32-bit buffer offsets): their far `out` runs at the largest M the
predicate admits at that stride, one row more must be refused, and neither is ever launched beyond it.

Part B.  The tile GEMM kernels pack (frame, y, x) of a 3 x 3 convolution in 11 + 10 + 11 bits and take T <= 31 in the temporal
mode: both sides of frames = 2046, Ho = 1024, Wo = 2048 and T = 31, under the forced tile kernels and the automatic choice.
The temporal mode's third limit, M + 256 < 2^26 tokens, needs about 13 GB of operands and is left out.

Part C.  `gcd_groupnorm_apply` beyond 65 535 row chunks (the re-chunking branch of its launch arithmetic).

Part D.  The width-320 engine at 2 clips x 64 frames x 72 x 128 (M = 1 179 648 tokens, q | k | v = 2.26 GB): before the
size-aware predicates this raised GcdError from `_ln_qkv`.
"""
import collections
import gc
import math

import pytest
import torch
import torch.nn.functional as F

import memcontract as mc
from test_kernels_gpu import TOL_F16, TOL_F32          # the bars of the entries' own parity tests

pytestmark = pytest.mark.gpu

F16, F32, BF16, F64 = torch.float16, torch.float32, torch.bfloat16, torch.float64
LD_BYTES = 65536
ROWS = 65536 + 333                 # crosses both marks away from the first and the last tile; ragged against 64 / 128 / 256
TOL_FF32 = 3e-4                    # test_ff_fused_one_kernel / test_ff_fused_with_its_layernorm (fp32 result)
TOL_ATTN = 1.5e-3                  # test_attn_spatial
INT_MAX = 2 ** 31 - 1
_IMPLS = {"auto": 0, "tile256x320": 2, "ring32": 3, "tile64": 6}          # test_kernels_gpu.py's gemm_impl


def _es(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def _h(t):
    return t.to(F16).to(t.dtype)


class Run:
    """The operands of one launch: the one named `far` with the 65 536-byte row stride, the others compact."""

    def __init__(self, dev, far, limit=None):
        self.dev, self.far, self.limit, self.arenas, self.outs, self.hit = dev, far, limit, [], {}, False

    def _arena(self, name, rows, cols, dtype):
        far = name == self.far
        a = mc.Arena(rows, cols, dtype, self.dev, pad=LD_BYTES // _es(dtype) - cols if far else None, name=name)
        if far:
            es, self.hit = _es(dtype), True
            assert a.ld * es == LD_BYTES
            if self.limit is None:           # not vacuous: the last payload element lies beyond byte 2^32
                assert (rows - 1) * a.ld * es + cols * es > 2 ** 32, (name, rows)
            else:                            # an output that its kernel keeps below 2^31: one row more is past the limit
                assert rows * a.ld * es <= self.limit < (rows + 1) * a.ld * es, (name, rows)
        self.arenas.append(a)
        return a

    def inp(self, name, value):
        return self._arena(name, value.shape[0], value.shape[1], value.dtype).set(value).view

    def out(self, name, rows, cols, dtype, init=None):
        a = self._arena(name, rows, cols, dtype).set("poison" if init is None else init)
        self.outs[name] = a
        return a.view

    def finish(self):
        torch.cuda.synchronize()
        assert self.hit, f"no operand named {self.far}"
        for a in self.arenas:
            a.assert_untouched(f"[far {self.far}] ")


def _bands(rows):
    if rows < 1024:                                       # a small result (a weight gradient, column sums): one figure
        return {"all rows": (0, rows)}
    b = {"rows [0, 256)": (0, 256), "the last 256 rows": (rows - 256, rows)}
    for mark, row in (("2^31", 32768), ("2^32", 65536)):            # (may overlap the last 256 rows: both are held)
        if row < rows:
            b[f"the 512 rows around byte {mark}"] = (row - 256, min(row + 256, rows))
    return b


def check_bands(what, got, ref, bar):
    """rel-L2 per row band (max-abs for a bar ("maxabs", x)), each band held to the bar; NaN (an element never written)
    fails every comparison."""
    got, ref = got.double(), ref.double().reshape(got.shape)
    maxabs = isinstance(bar, tuple)
    if maxabs:
        assert bar[0] == "maxabs"
        bar, d = bar[1], (got - ref).abs().amax(1)
        d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
        n = torch.ones_like(d)
    else:
        d, n = ((got - ref) ** 2).sum(1), (ref ** 2).sum(1)
    rest, fig = torch.ones_like(d, dtype=torch.bool), {}

    def err(dd, nn):
        return float(dd.max()) if maxabs else float(torch.sqrt(dd.sum() / nn.sum()))
    for name, (a, b) in _bands(got.shape[0]).items():
        fig[name] = err(d[a:b], n[a:b])
        rest[a:b] = False
    if got.shape[0] > 1024:
        fig["the rest"] = err(d[rest], n[rest])
    print(f"{what}: " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()) + f" (bar {bar:.1e}{', max-abs' if maxabs else ''})")
    for name, e in fig.items():
        assert e < bar, f"{what}: {'max-abs' if maxabs else 'rel-L2'} {e:.3e} in {name} (bar {bar:.1e})"


@pytest.fixture
def spy(monkeypatch):
    """Counts the calls of every C entry of libgcd_amd.so and libgcd_amd_train.so (the wrappers look them up on the loaded
    library per call)."""
    from gcd_amd import _lib
    counts = collections.Counter()

    def wrap(name, real):
        def f(*a):
            counts[name] += 1
            return real(*a)
        return f
    for lib, names in ((_lib.load(), _lib.SIGNATURES),
                       (_lib.load_train(), list(_lib.TRAIN_SIGNATURES) + list(_lib.TRAIN_DET_SIGNATURES))):
        for name in names:
            if not name.endswith(("_last_error", "abi_version")):
                monkeypatch.setattr(lib, name, wrap(name, getattr(lib, name)))
    return counts


def drive(dev, spy, entry, what, case, fars, limit_for=lambda far: None):
    """One run per far operand: guards, the spy, the bands; the buffer is freed between the runs."""
    for far in fars:
        torch.cuda.reset_peak_memory_stats()
        run, n0 = Run(dev, far, limit_for(far)), spy[entry]
        refs = case(run)
        run.finish()
        assert spy[entry] > n0, f"{entry} was not called"
        for name, (ref, bar) in refs.items():
            check_bands(f"{what}, far {far}: {name}", run.outs[name].payload, ref, bar)
        print(f"{what}, far {far}: peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
        del run, refs
        gc.collect()
        torch.cuda.empty_cache()


def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _randn(g, *shape, dtype=F32):
    return torch.randn(*shape, device=g.device, generator=g).to(dtype)


@pytest.fixture
def impl(request):
    from gcd_amd import ops
    ops.tune_set(ops.TUNE_GEMM_IMPL, _IMPLS[request.param])
    yield request.param
    torch.cuda.synchronize()
    ops.tune_set(ops.TUNE_GEMM_IMPL, 0)


all_impls = pytest.mark.parametrize("impl", list(_IMPLS), indirect=True)
tile_impls = pytest.mark.parametrize("impl", ["auto", "tile256x320", "tile64"], indirect=True)


# ============================================================================================ part A: gcd_gemm_f16
def _plain_case(M, N, K, kind):
    from gcd_amd import ops, packing

    def case(run):
        g = _gen(run.dev, 1)
        a = _randn(g, M, K, dtype=F16)
        geglu = kind == ops.OUT_GEGLU
        w = _h(_randn(g, (2 * N if geglu else N), K) / math.sqrt(K))
        bias = _randn(g, w.shape[0])
        wd, bd = (packing.pack_geglu(w, bias) if geglu else (w, bias))
        kw = {}
        if not geglu:
            r1, r2 = _randn(g, M, N), _randn(g, M, N)
            kw = dict(r1=run.inp("r1", r1), r2=run.inp("r2", r2), s_acc=0.7, s_r1=0.5, s_r2=-1.25)
        out = run.out("out", M, N, F32 if kind == ops.OUT_F32 else F16)
        ops.gemm(run.inp("A", a), wd.to(F16).contiguous(), out, M=M, bias=bd.contiguous(), out_kind=kind, **kw)
        acc = a.double() @ w.double().t() + bias.double()
        if geglu:
            return {"out": (acc[:, :N] * F.gelu(acc[:, N:]), TOL_F16)}
        return {"out": (0.7 * acc + 0.5 * r1.double() - 1.25 * r2.double(), TOL_F32 if kind == ops.OUT_F32 else TOL_F16)}
    return case


@all_impls
@pytest.mark.parametrize("kind,N", [("f32", 64), ("f32", 320), ("f16", 64), ("f16", 320), ("geglu", 64), ("geglu", 320)])
def test_gemm_plain_far_operands(gpu, spy, impl, kind, N):
    """A far A fails the tile kernels' extent check (gcd_gemm_p8_supported): the call must land on a kernel with 64-bit
    addresses and be right; `out`, `R1`, `R2` are 64-bit in every kernel."""
    from gcd_amd import ops
    k = dict(f32=ops.OUT_F32, f16=ops.OUT_F16, geglu=ops.OUT_GEGLU)[kind]
    fars = ("A", "out") if kind == "geglu" else ("A", "out", "r1", "r2")
    drive(gpu, spy, "gcd_gemm_f16", f"gemm plain {kind} N={N} [{impl}]", _plain_case(ROWS, N, 64, k), fars)


def _conv_ref(x_tok, frames, H, W, w, b, stride, up):
    """fp64 conv2d on the CPU of the token-major fp16 image; token-major result."""
    x = x_tok.cpu().double().reshape(frames, H, W, -1).permute(0, 3, 1, 2)
    if up:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    y = F.conv2d(x, w.cpu().double(), b.cpu().double(), stride=stride, padding=1)
    return y.permute(0, 2, 3, 1).reshape(-1, w.shape[0])


def _conv_case(frames, H, W, Cin, Cout, stride, up, res=True):
    from gcd_amd import ops, packing

    def case(run):
        g = _gen(run.dev, 5)
        a = _randn(g, frames * H * W, Cin, dtype=F16)
        w = _h(_randn(g, Cout, Cin, 3, 3) / math.sqrt(9 * Cin))
        b = _randn(g, Cout)
        Ho, Wo = (2 * H, 2 * W) if up else ((H - 1) // stride + 1, (W - 1) // stride + 1)
        M = frames * Ho * Wo
        r1 = _randn(g, M, Cout)
        out = run.out("out", M, Cout, F32)
        kw = dict(r1=run.inp("r1", r1)) if res else {}
        ops.gemm(run.inp("A", a), packing.pack_conv3x3(w.cpu()).to(run.dev), out, M=M, mode=ops.GEMM_CONV3X3, bias=b,
                 conv=dict(Cin=Cin, Hi=H, Wi=W, Ho=Ho, Wo=Wo, stride=stride, upsample=up), **kw)
        ref = _conv_ref(a, frames, H, W, w, b, stride, up).to(run.dev)
        return {"out": (ref + r1.double() if res else ref, TOL_F32)}
    return case


@all_impls
@pytest.mark.parametrize("form,frames,H,stride,up,fars", [
    ("stride1", 1030, 8, 1, 0, ("A", "out", "r1")), ("stride2", 1030, 16, 2, 0, ("out",)), ("stride2_far_A", 260, 16, 2, 0, ("A",)),
    ("fused_up", 1030, 4, 1, 1, ("out",)), ("fused_up_far_A", 4120, 4, 1, 1, ("A",))])
def test_gemm_conv3x3_far_operands(gpu, spy, impl, form, frames, H, stride, up, fars):
    """8 x 8 output frames (stride 2: 16 x 16 in, fused x2 up: 4 x 4 in); the far side has about 66 k rows."""
    drive(gpu, spy, "gcd_gemm_f16", f"conv3x3 {form} [{impl}]", _conv_case(frames, H, H, 64, 64, stride, up), fars)


def _temporal_ref(a, clips, T, HW, w, b):
    """(3, 1, 1) convolution over time, zero padded, as three fp64 products; w is [Cout, Cin, 3]."""
    x = a.double().reshape(clips, T, HW, -1)
    y = torch.zeros(clips, T, HW, w.shape[0], dtype=F64, device=a.device) + b.double()
    for dt in range(3):
        lo, hi = max(0, 1 - dt), min(T, T + 1 - dt)
        y[:, lo:hi] += x[:, lo + dt - 1:hi + dt - 1] @ w[:, :, dt].double().t()
    return y.reshape(clips * T * HW, -1)


def _temporal_case(clips, T, HW, C, Cout=None):
    from gcd_amd import ops, packing
    Cout = Cout or C

    def case(run):
        g = _gen(run.dev, 7)
        M = clips * T * HW
        a = _randn(g, M, C, dtype=F16)
        w = _h(_randn(g, Cout, C, 3, 1, 1) / math.sqrt(3 * C))
        b, r1 = _randn(g, Cout), _randn(g, M, Cout)
        out = run.out("out", M, Cout, F32)
        ops.gemm(run.inp("A", a), packing.pack_conv_t3(w.cpu()).to(run.dev), out, M=M, mode=ops.GEMM_TEMPORAL3, bias=b,
                 r1=run.inp("r1", r1), conv=dict(Cin=C, T=T, HW=HW))
        return {"out": (_temporal_ref(a, clips, T, HW, w[..., 0, 0], b) + r1.double(), TOL_F32)}
    return case


@all_impls
def test_gemm_temporal3_far_operands(gpu, spy, impl):
    drive(gpu, spy, "gcd_gemm_f16", f"temporal3 [{impl}]", _temporal_case(2, 16, 2059, 64), ("A", "out", "r1"))


def _p8_extent_ok(a_rows, lda, K, HW=0):
    """The A-extent line of gcd_gemm_p8_supported (gemm_p8.hip)."""
    return (a_rows + 256 + HW) * lda * 2 + K * 2 < 0xFFFFFF00


@tile_impls
@pytest.mark.parametrize("mode,step", [("plain", 0), ("plain", 1), ("plain", 300), ("conv3x3", 0), ("conv3x3", 1), ("conv3x3", 5),
                                       ("temporal3", 0), ("temporal3", 1), ("temporal3", 10)])
def test_gemm_straddles_the_tile_kernels_extent_check(gpu, spy, impl, mode, step):
    """lda = 32 768: the largest A the tile kernels admit (offsets up to the 0xFFFFFF00 marker), one unit more and well past
    it — in rows (PLAIN), 8 x 8 frames (CONV3X3) and pixels per frame of 2 clips x 16 frames (TEMPORAL3, whose formula
    adds HW).  N = 320, so that the automatic choice too takes a tile kernel where the check admits one (>= 192 tiles of
    256 x 320).  The library exports nothing that tells which kernel ran (`gcd_gemm_p8_supported` is internal), so the test
    holds what a caller can see: on either side of the limit, whichever kernel the dispatcher picks, every band is right."""
    lda = LD_BYTES // 2
    if mode == "plain":
        m = max(r for r in range(65000, 65536) if _p8_extent_ok(r, lda, 64))
        assert _p8_extent_ok(m, lda, 64) and not _p8_extent_ok(m + 1, lda, 64)
        case = _plain_case(m + step, 320, 64, 0)
    elif mode == "conv3x3":
        f = max(f for f in range(1000, 1030) if _p8_extent_ok(64 * f, lda, 9 * 64))
        assert not _p8_extent_ok(64 * (f + 1), lda, 9 * 64)
        case = _conv_case(f + step, 8, 8, 64, 320, 1, 0)
    else:
        hw = max(h for h in range(1900, 2048) if _p8_extent_ok(32 * h, lda, 3 * 64, h))
        assert not _p8_extent_ok(32 * (hw + 1), lda, 3 * 64, hw + 1)
        case = _temporal_case(2, 16, hw + step, 64, 320)

    class Near(Run):                         # the far A of these runs ends just below / above 2^32 by construction
        def _arena(self, name, rows, cols, dtype):
            far = name == self.far
            a = mc.Arena(rows, cols, dtype, self.dev, pad=lda - cols if far else None, name=name)
            if far:
                self.hit = True
                assert 0xF0000000 < rows * LD_BYTES < 2 ** 32 + 400 * LD_BYTES
            self.arenas.append(a)
            return a
    torch.cuda.reset_peak_memory_stats()
    run, n0 = Near(gpu, "A"), spy["gcd_gemm_f16"]
    refs = case(run)
    run.finish()
    assert spy["gcd_gemm_f16"] > n0
    check_bands(f"{mode} +{step} [{impl}]", run.outs["out"].payload, *refs["out"])
    print(f"{mode} +{step} [{impl}]: peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    del run, refs
    gc.collect()
    torch.cuda.empty_cache()


# ============================================================================= part A: the two fused C = 320 kernels
def _lnqkv_largest(ldo):
    return (INT_MAX - 1) // (2 * ldo)                   # M ldo 2 < 2^31 - 1 (gcd_lnqkv_f16's check)


def _ff_largest(ldo, es):
    """The largest M with M ldo es <= 2^31 - 1 and ((Mpad - 1) ldo + 316) es <= 2^31 - 1, Mpad = M rounded up to 128."""
    def fits(M):
        return M * ldo * es <= INT_MAX and (((M + 127) // 128 * 128 - 1) * ldo + 316) * es <= INT_MAX
    m = INT_MAX // (ldo * es)
    while not fits(m):
        m -= 1
    assert fits(m) and not fits(m + 1)
    return m


def _lnqkv_case(M, N):
    from gcd_amd import ops

    def case(run):
        g = _gen(run.dev, 77)
        C = 320
        x = _randn(g, M, C) * 1.3 + 0.4
        w = _h(_randn(g, N, C) / math.sqrt(C))
        gamma, beta = _randn(g, C), _randn(g, C) * 0.5
        out = run.out("out", M, N, F16)
        ops.lnqkv(run.inp("x32", x), gamma, beta, ops.lnqkv_pack(w.half()), out, M=M, N=N)
        xn = _h(F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), 1e-5))
        return {"out": (xn @ w.double().t(), TOL_F16)}
    return case


def test_lnqkv_far_operands(gpu, spy, monkeypatch):
    from gcd_amd import _lib, ops
    monkeypatch.setattr(ops, "LNQKV_MIN_TOKENS", 1)
    drive(gpu, spy, "gcd_lnqkv_f16", "lnqkv", _lnqkv_case(ROWS, 192), ("x32",))
    ldo = LD_BYTES // 2
    m = _lnqkv_largest(ldo)
    assert ops.lnqkv_ok(m, 320, 192, enabled=True, ldo=ldo) and not ops.lnqkv_ok(m + 1, 320, 192, enabled=True, ldo=ldo)
    drive(gpu, spy, "gcd_lnqkv_f16", f"lnqkv at its largest M = {m}", _lnqkv_case(m, 192), ("out",), lambda far: INT_MAX - 1)


def test_engine_layernorm_qkv_falls_back_one_row_past_the_limit(gpu, spy, monkeypatch):
    """`UNetEngine._ln_qkv` with a q | k | v buffer of 65 536-byte rows and one row more than `gcd_lnqkv_f16` admits: the
    fused kernel is not launched, LayerNorm + GEMM write the far buffer, and the result is right to its last row."""
    import types
    from gcd_amd import ops
    from gcd_amd.engine import UNetEngine
    monkeypatch.setattr(ops, "LNQKV_MIN_TOKENS", 1)
    M, C, N = _lnqkv_largest(LD_BYTES // 2) + 1, 320, 192
    g = _gen(gpu, 78)
    x = _randn(g, M, C) * 1.3 + 0.4
    w = _h(_randn(g, N, C) / math.sqrt(C)).half()
    gamma, beta = _randn(g, C), _randn(g, C) * 0.5
    far = mc.Arena(M, N, F16, gpu, pad=LD_BYTES // 2 - N, name="qkv").set("poison")
    assert M * far.ld * 2 >= 2 ** 31

    def ln(x32, affine):
        y = torch.empty(x32.shape, dtype=F16, device=gpu)
        return ops.layernorm(x32, affine[0], affine[1], y)
    eng = types.SimpleNamespace(fuse_layernorm=False, _next_dir=lambda: 0, _ln=ln,
                                ws=types.SimpleNamespace(alloc=lambda shape, dtype: far.view, release=lambda t: None),
                                _gemm=lambda a16, w16, out, **kw: ops.gemm(a16, w16, out, **kw))
    qkv = UNetEngine._ln_qkv(eng, dict(wqkv=w, wqkv_p=ops.lnqkv_pack(w)), x, (gamma, beta), M)
    torch.cuda.synchronize()
    assert spy["gcd_lnqkv_f16"] == 0 and spy["gcd_layernorm_f16"] == 1 and spy["gcd_gemm_f16"] == 1
    assert qkv.data_ptr() == far.view.data_ptr()
    far.assert_untouched("[engine fallback] ")
    xn = _h(F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), 1e-5))
    check_bands("engine fallback q | k | v", far.payload, xn @ w.double().t(), TOL_F16)


def _ff_weights(g, for_ln):
    from gcd_amd import ops, packing
    C, H = 320, 1280
    w1 = _h(_randn(g, 2 * H, C) / math.sqrt(C))
    b1 = _randn(g, 2 * H) * 0.5
    w2 = _h(_randn(g, C, H) / math.sqrt(H))
    b2 = _randn(g, C)
    w1p, b1p = packing.pack_geglu(w1, b1)
    return w1, b1, w2, b2, ops.ff_pack(w1p.half().contiguous(), w2.half(), for_ln=for_ln), b1p.contiguous()


def _ff_ref(xn, w1, b1, w2, b2):
    out = torch.empty(xn.shape[0], 320, dtype=F64, device=xn.device)
    for r in range(0, xn.shape[0], 8192):                # row chunks: the fp64 hidden tensor of all rows would be 1.3 GB
        h = xn[r:r + 8192] @ w1.double().t() + b1.double()
        out[r:r + 8192] = _h(h[:, :1280] * F.gelu(h[:, 1280:])) @ w2.double().t() + b2.double()
    return out


def _ff_case(M, form):
    """form: ln_plain | ln_addvec | ln_blend16 (the LayerNorm forms the engine uses) | x_plain | x_blend32 | x_blend16."""
    from gcd_amd import ops

    def case(run):
        g = _gen(run.dev, 611)
        C, rpv = 320, 1024
        ln_form, f16 = form.startswith("ln"), form.endswith("16")
        w1, b1, w2, b2, wp, b1p = _ff_weights(g, ln_form)
        nvec = (M + rpv - 1) // rpv
        alpha, r2 = torch.rand(nvec, device=run.dev, generator=g), _randn(g, M, C)
        kw = {}
        if "blend" in form:
            kw = dict(r2=run.inp("R2", r2), out_kind=ops.OUT_F16 if f16 else ops.OUT_F32, frame_alpha=alpha, rows_per_alpha=rpv)
        out = run.out("out", M, C, F16 if f16 else F32)
        if ln_form:
            x = _randn(g, M, C) * 1.5 + 0.3
            gamma, beta, pos = _randn(g, C), _randn(g, C) * 0.5, _randn(g, nvec, C) * 0.7
            ln = dict(gamma=gamma, beta=beta)
            if form != "ln_plain":
                ln.update(addvec=pos, rows_per_vec=rpv)
            ops.ff_fused(run.inp("x32", x), wp, b1p, b2, out, M=M, ln=ln, **kw)
            z = x.double() + (pos.double().repeat_interleave(rpv, 0)[:M] if form != "ln_plain" else 0)
            xn = _h(F.layer_norm(z, (C,), gamma.double(), beta.double(), 1e-5))
        else:
            x, r1 = _randn(g, M, C, dtype=F16), _randn(g, M, C)
            ops.ff_fused(run.inp("X", x), wp, b1p, b2, out, M=M, r1=run.inp("R1", r1), **kw)
            z, xn = r1.double(), x.double()
        res = _ff_ref(xn, w1, b1, w2, b2) + z
        if "blend" in form:
            a = alpha.double().repeat_interleave(rpv)[:M, None]
            res = (1 - a) * res + a * r2.double()
        return {"out": (res, TOL_F16 if f16 else TOL_FF32)}
    return case


@pytest.mark.parametrize("form,fars", [("ln_plain", ("x32",)), ("ln_addvec", ("x32",)), ("ln_blend16", ("x32", "R2")),
                                        ("x_plain", ("X", "R1")), ("x_blend32", ("R2",)), ("x_blend16", ("R1", "R2"))])
def test_ff_fused_far_inputs(gpu, spy, form, fars):
    """x32, X, R1 and R2 are read through 64-bit pointers: full size, across both marks."""
    drive(gpu, spy, "gcd_ff_fused_f16", f"ff_fused {form}", _ff_case(ROWS, form), fars)


@pytest.mark.parametrize("form", ["ln_plain", "ln_addvec", "ln_blend16", "x_plain", "x_blend32", "x_blend16"])
def test_ff_fused_far_out_at_its_largest_M(gpu, spy, monkeypatch, form):
    """The largest M `gcd_ff_fused_fits` admits at the 65 536-byte stride runs and is right to its last row (its last
    128-token tile overhangs); one row more is refused by the predicate and by `_ff_ln`, and nothing is launched."""
    import types
    from gcd_amd import ops
    from gcd_amd.engine import UNetEngine
    monkeypatch.setattr(ops, "FF_FUSED_MIN_TOKENS", 1)
    f16 = form.endswith("16")
    es, kind = (2, ops.OUT_F16) if f16 else (4, ops.OUT_F32)
    ldo = LD_BYTES // es
    m = _ff_largest(ldo, es)
    assert m % 128 != 0
    assert ops.ff_fused_ok(m, 320, 1280, enabled=True, ldo=ldo, out_kind=kind)
    assert not ops.ff_fused_ok(m + 1, 320, 1280, enabled=True, ldo=ldo, out_kind=kind)
    drive(gpu, spy, "gcd_ff_fused_f16", f"ff_fused {form} at its largest M = {m}", _ff_case(m, form), ("out",), lambda far: INT_MAX)
    n0 = spy["gcd_ff_fused_f16"]
    eng = types.SimpleNamespace(fuse_layernorm=False, _next_dir=lambda: 0)
    wide = torch.empty(m + 1, ldo, dtype=F16 if f16 else F32, device="meta")[:, :320]      # a shape and a stride, no memory
    Fw = dict(wp=object(), w1=torch.empty(2560, 320, device="meta"))
    assert UNetEngine._ff_ln(eng, Fw, None, (None, None), m + 1, out=wide, out_kind=kind) is False
    assert wide.stride(0) == ldo
    assert spy["gcd_ff_fused_f16"] == n0


# ======================================================================================= part A: norms, casts, attention
def _layernorm_case(M, C):
    from gcd_amd import ops

    def case(run):
        g = _gen(run.dev, 9)
        rpv = 1030
        x, add = _randn(g, M, C) * 2 + 0.5, _randn(g, (M + rpv - 1) // rpv, C)
        gamma, beta = _randn(g, C), _randn(g, C)
        y, s = run.out("y", M, C, F16), run.out("sum_out", M, C, F32)
        ops.layernorm(run.inp("x", x), gamma, beta, y, addvec=add, rows_per_vec=rpv, sum_out=s)
        xs = x.double() + add.double().repeat_interleave(rpv, 0)[:M]
        return {"y": (F.layer_norm(xs, (C,), gamma.double(), beta.double(), 1e-5), TOL_F16), "sum_out": (xs, 1e-6)}
    return case


@pytest.mark.parametrize("C", [64, 320])                 # the wave-per-row kernel and the 16-lanes-per-row kernel of C = 320
def test_layernorm_far_operands(gpu, spy, C):
    drive(gpu, spy, "gcd_layernorm_f16", f"layernorm C={C}", _layernorm_case(ROWS + 3, C), ("x", "y", "sum_out"))


def _groupnorm_case(frames, HW, C, per_clip_T):
    from gcd_amd import ops

    def case(run):
        g = _gen(run.dev, 8)
        M = frames * HW
        tok = _randn(g, M, C) * 3 + 1.5
        gamma, beta = _randn(g, C), _randn(g, C)
        rows = (per_clip_T or 1) * HW
        ninst, nch = M // rows, ops.gn_nchunks(rows)
        x1 = run.inp("x1", tok)
        stats = torch.empty(ninst * 64, device=run.dev)
        ops.groupnorm_stats(x1, None, rows, 1e-5, torch.empty(ninst * nch * 64, dtype=F64, device=run.dev), stats, nch)
        y, raw = run.out("y", M, C, F16), run.out("raw16", M, C, F16)
        ops.groupnorm_apply(x1, None, rows, stats, gamma, beta, True, y, raw)
        xg = tok.double().reshape(ninst, rows, 32, C // 32)
        mean, var = xg.mean((1, 3), keepdim=True), xg.var((1, 3), unbiased=False, keepdim=True)
        r = ((xg - mean) / torch.sqrt(var + 1e-5)).reshape(M, C) * gamma.double() + beta.double()
        torch.cuda.synchronize()
        st = torch.stack([mean.reshape(ninst, 32), 1 / torch.sqrt(var.reshape(ninst, 32) + 1e-5)], -1).reshape(-1)
        e = float((stats.double() - st).norm() / st.norm())
        print(f"groupnorm far {run.far}: statistics rel-L2 {e:.2e}")
        assert e < 1e-5                                   # the statistics bar of test_memcontract_gpu.py's groupnorm cases
        return {"y": (F.silu(r), TOL_F16), "raw16": (tok, TOL_F16)}
    return case


@pytest.mark.parametrize("frames,HW,T", [(1030, 64, 0), (1030, 64, 103), (2, 32967, 0)], ids=["per_frame", "per_clip", "two_instances"])
def test_groupnorm_far_operands(gpu, spy, frames, HW, T):
    drive(gpu, spy, "gcd_groupnorm_apply", f"groupnorm {frames}x{HW} T={T}", _groupnorm_case(frames, HW, 64, T), ("x1", "y", "raw16"))
    assert spy["gcd_groupnorm_stats"] == 3


def _cast_case(M, C):
    from gcd_amd import ops

    def case(run):
        x = _randn(_gen(run.dev, 13), M, C)
        xv = run.inp("x32", x)
        ops.cast_f16(xv, run.out("f16", M, C, F16))
        ops.cast_bf16(xv, run.out("bf16", M, C, BF16))
        return {"f16": (x.half(), 1e-30), "bf16": (x.to(BF16), 1e-30)}
    return case


def test_cast_far_operands(gpu, spy):
    drive(gpu, spy, "gcd_cast_f32_f16", "cast", _cast_case(ROWS, 72), ("x32", "f16", "bf16"))
    assert spy["gcd_cast_f32_bf16"] == 3


def _attn_spatial_case(frames, S, heads):
    from gcd_amd import ops

    def case(run):
        C = heads * 64
        qkv = _randn(_gen(run.dev, 10), frames * S, 3 * C, dtype=F16) * 1.5
        S_pad = (S + 63) // 64 * 64
        vt = torch.empty(frames * heads * 64, S_pad, dtype=F16, device=run.dev)
        qv, out = run.inp("qkv", qkv), run.out("out", frames * S, C, F16)
        ops.attn_transpose_v(qv, frames, S, heads, vt, S_pad)
        ops.attn_spatial(qv, vt, S_pad, out, frames, S, heads)
        q, k, v = [t.reshape(frames, S, heads, 64).permute(0, 2, 1, 3).double() for t in qkv.split(C, dim=1)]
        p = torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1)
        return {"out": ((p @ v).permute(0, 2, 1, 3).reshape(frames * S, C), TOL_ATTN)}
    return case


def test_attn_spatial_far_operands(gpu, spy):
    drive(gpu, spy, "gcd_attn_spatial_f16", "spatial attention 257 x 257", _attn_spatial_case(257, 257, 1), ("qkv", "out"))
    assert spy["gcd_attn_transpose_v"] == 2


def _attn_temporal_case(clips, T, HW, heads):
    from gcd_amd import ops

    def case(run):
        C, M = heads * 64, clips * T * HW
        qkv = _randn(_gen(run.dev, 11), M, 3 * C, dtype=F16) * 1.5
        out = run.out("out", M, C, F16)
        ops.attn_temporal(run.inp("qkv", qkv), out, clips, T, HW, heads)
        q, k, v = [t.reshape(clips, T, HW, heads, 64).permute(0, 2, 3, 1, 4).double() for t in qkv.split(C, dim=1)]
        p = torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1)
        return {"out": ((p @ v).permute(0, 3, 1, 2, 4).reshape(M, C), TOL_F16)}
    return case


@pytest.mark.parametrize("entry,T,HW", [("gcd_attn_temporal_f16", 16, 2059), ("gcd_attn_temporal_long_f16", 33, 999)])
def test_attn_temporal_far_operands(gpu, spy, entry, T, HW):
    drive(gpu, spy, entry, f"temporal attention T={T} HW={HW}", _attn_temporal_case(2, T, HW, 1), ("qkv", "out"))


def _smallm_case(M, N, K):
    from gcd_amd import ops

    def case(run):
        g = _gen(run.dev, 12)
        x, w, b = _randn(g, M, K), _randn(g, N, K) / math.sqrt(K), _randn(g, N)
        ops.linear_smallm(run.inp("x", x), w, b, run.out("y", M, N, F32))
        return {"y": (x.double() @ w.double().t() + b.double(), 1e-5)}        # test_linear_smallm's bar (test_kernels_gpu.py)
    return case


def test_linear_smallm_far_operands(gpu, spy):
    drive(gpu, spy, "gcd_linear_smallm_f32", "linear_smallm", _smallm_case(ROWS, 64, 64), ("x", "y"))


def _softmax_case(R, C):
    from gcd_amd import ops

    def case(run):
        x = _randn(_gen(run.dev, 130), R, C) * 4.0
        ops.softmax_rows(run.inp("x", x), run.out("y", R, C, F16))
        return {"y": (torch.softmax(x.double(), -1), ("maxabs", 6e-4))}        # test_softmax_rows' max-abs bar
    return case


def test_softmax_rows_far_operands(gpu, spy):
    drive(gpu, spy, "gcd_softmax_rows_f16", "softmax_rows", _softmax_case(ROWS, 300), ("x", "y"))


def _transpose_case(R, C):
    from gcd_amd import ops

    def case(run):
        x = _randn(_gen(run.dev, R), R, C, dtype=F16)
        ops.transpose_f16(run.inp("x", x), run.out("y", C, R, F16))
        return {"y": (x.t(), 1e-30)}
    return case


@pytest.mark.parametrize("rows", [ROWS, ROWS + 3])       # the scalar kernel, and the vector kernel (R % 16 == 0, C % 8 == 0)
def test_transpose_f16_far_operands(gpu, spy, rows):
    drive(gpu, spy, "gcd_transpose_f16", f"transpose {rows} x 72", _transpose_case(rows, 72), ("x",))
    drive(gpu, spy, "gcd_transpose_f16", f"transpose 80 x {rows}", _transpose_case(80, rows), ("y",))


def test_unpack_output_and_time_mix_unpack_far_tokens(gpu, spy):
    """Both read far token-major rows and write a contiguous NCHW tensor (no stride to move)."""
    from gcd_amd import ops
    N, T, HW, C = 199, 1, 331, 3                          # 199 x 331 = 65 869 rows
    torch.cuda.reset_peak_memory_stats()
    g = _gen(gpu, 14)
    run = Run(gpu, "tok")
    tok = _randn(g, N * HW, 16)
    tv = run.inp("tok", tok)
    nchw = mc.poison_scratch(torch.empty(N, 4, HW, device=gpu))
    ops.unpack_output(tv, nchw, 4, N, HW)
    run.finish()
    assert spy["gcd_unpack_output"] == 1
    assert torch.equal(nchw, tok[:, :4].reshape(N, HW, 4).permute(0, 2, 1)), "unpack_output"      # a copy: exact
    print(f"unpack_output far tok: peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    del run
    torch.cuda.empty_cache()
    N, T = 200, 2                                         # 100 clips of two frames: 66 200 rows
    run = Run(gpu, "tok")
    tok = _randn(g, N * HW, C)
    w, b = _randn(g, C, C, 3), _randn(g, C)
    out = mc.poison_scratch(torch.empty(N, C, HW, device=gpu))
    ops.time_mix_unpack(run.inp("tok", tok), w, b, out, C, N, T, HW)
    run.finish()
    assert spy["gcd_time_mix_unpack"] == 1
    ref = _temporal_ref(tok, N // T, T, HW, w, b).reshape(N, HW, C).permute(0, 2, 1)
    e = float((out.double() - ref).abs().max())
    print(f"time_mix_unpack far tok: max-abs {e:.2e}, peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    assert e < 1e-5                                       # test_time_mix_unpack's max-abs bar (test_decoder_gpu.py)
    del run
    gc.collect()
    torch.cuda.empty_cache()


# ================================================================== part A: the backward and fine-tune entries
class FarCtx(mc.Ctx):
    """memcontract's operand factory with ONE operand, chosen by the first word of its name, on the 65 536-byte stride (all
    guards and outputs poisoned).  The shape-parametrised cases of test_memcontract_train_gpu.py and
    test_memcontract_det_gpu.py run through it unchanged at ~66 k rows: their operands, their CPU references in fp32 / fp64
    and their bars, which are those of test_backward_gpu.py / test_train_plan_gpu.py / test_deterministic_gpu.py."""

    def __init__(self, dev, far):
        super().__init__(dev, True, True)
        self.far, self.hit = far, False

    def _new(self, rows, cols, dtype, pad, name, overhang=(0, 0)):
        if name.split(" ")[0] == self.far:
            pad, self.hit = LD_BYTES // _es(dtype) - cols, True
            assert (rows - 1) * LD_BYTES + cols * _es(dtype) > 2 ** 32, (name, rows)
        return super()._new(rows, cols, dtype, pad, name, overhang)


def drive_ctx(dev, spy, entries, what, fn, fars):
    for far in fars:
        torch.cuda.reset_peak_memory_stats()
        ctx, n0 = FarCtx(dev, far), {e: spy[e] for e in entries}
        refs = fn(ctx)
        torch.cuda.synchronize()
        assert ctx.hit, f"no operand named {far}"
        for a in ctx.arenas:
            a.assert_untouched(f"[{what}, far {far}] ")
        for e in entries:
            assert spy[e] > n0[e], f"{e} was not called"
        assert refs
        for name, (ref, bar) in refs.items():
            got = ctx.outs[name].payload if name in ctx.outs else ctx.extra_outs[name]
            ref = ref.reshape(ref.shape[0], -1) if ref.dim() >= 2 else ref.reshape(1, -1)
            check_bands(f"{what}, far {far}: {name}", got.reshape(ref.shape), ref.to(dev), bar)
        print(f"{what}, far {far}: peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
        del ctx, refs
        gc.collect()
        torch.cuda.empty_cache()


def _cpu_gen(seed):
    return torch.Generator().manual_seed(seed)


def test_wgrad_tr_far_operands(gpu, spy):
    """dW = dY^T X over ~66 k tokens, N = K = 64; and the parameter-layout form (9 taps, padded channels)."""
    import test_memcontract_train_gpu as T
    from gcd_amd import autograd_ops as A
    drive_ctx(gpu, spy, ("gcd_wgrad_tr_f16",), "wgrad_tr", lambda ctx: T._wgrad_case(ctx, ROWS, 64, 64, "tr", F16), ("dy16", "x16"))

    def ex(ctx):                                          # test_memcontract_train_gpu.py's wgrad_ex_parameter_layout at M = ROWS
        g = _cpu_gen(7)
        taps, N, Nr, Cp, Cr = 9, 64, 40, 64, 8
        M, K = ROWS, taps * Cp
        dy, x = (torch.randn(M, N, generator=g) * 0.5).half(), torch.randn(M, K, generator=g).half()
        dst = ctx.out_flat("dest", (Nr, Cr, taps), F32)
        A._wgrad(ctx.inp(dy, name="dy16"), ctx.inp(x, name="x16"), dest=dst, taps=taps, n_real=Nr, c_real=Cr)
        return ctx.ref(lambda: {"dest": ((dy.float().t() @ x.float()).reshape(N, taps, Cp).permute(0, 2, 1)[:Nr, :Cr]
                                         .reshape(1, -1), 1e-4)})
    drive_ctx(gpu, spy, ("gcd_wgrad_tr_f16_ex",), "wgrad_tr_ex", ex, ("dy16", "x16"))


@pytest.mark.parametrize("conv", [1, 2], ids=["3x3", "t3"])
def test_wgrad_conv_tr_far_operands(gpu, spy, conv):
    """test_memcontract_train_gpu.py's wgrad_conv cases at 1030 frames of 8 x 8 / 2 clips x 16 frames x 2059 pixels."""
    from gcd_amd import autograd_ops as A

    def case(ctx):
        g = _cpu_gen(61)
        if conv == 1:
            frames, H, W, Cin, Cp, Cout = 1030, 8, 8, 8, 64, 40
            x = torch.randn(frames, Cin, H, W, generator=g).half().float()
            dy = (torch.randn(frames, Cout, H, W, generator=g) * 0.5).half().float()
            xt = torch.zeros(frames * H * W, Cp)
            xt[:, :Cin] = x.permute(0, 2, 3, 1).reshape(-1, Cin)
            dyt = dy.permute(0, 2, 3, 1).reshape(-1, Cout)
            geo, taps = dict(Ho=H, Wo=W), 9
            ref = lambda: torch.nn.grad.conv2d_weight(x, (Cout, Cin, 3, 3), dy, padding=1).reshape(1, -1)   # noqa: E731
        else:
            clips, T, HW, Cin, Cout = 2, 16, 2059, 72, 40
            x = torch.randn(clips, Cin, T, HW, 1, generator=g).half().float()
            dy = (torch.randn(clips, Cout, T, HW, 1, generator=g) * 0.5).half().float()
            xt, dyt = x.permute(0, 2, 3, 4, 1).reshape(-1, Cin), dy.permute(0, 2, 3, 4, 1).reshape(-1, Cout)
            geo, taps = dict(T=T, HW=HW), 3
            ref = lambda: torch.nn.grad.conv3d_weight(x, (Cout, Cin, 3, 1, 1), dy, padding=(1, 0, 0)).reshape(1, -1)   # noqa: E731
        dst = ctx.out_flat("dest", (Cout, Cin, taps), F32)
        A._wgrad_conv(ctx.inp(dyt, dtype=F16, name="dy16"), ctx.inp(xt, dtype=F16, name="x16"), dst, conv, Cout, Cin, **geo)
        return ctx.ref(lambda: {"dest": (ref(), 2e-4)})
    drive_ctx(gpu, spy, ("gcd_wgrad_conv_tr_f16",), f"wgrad_conv {conv}", case, ("dy16", "x16"))


def test_blend_far_operands(gpu, spy):
    """test_memcontract_train_gpu.py's blend_fwd_bwd at 1030 frames of 64 rows, every operand with its own stride."""
    from gcd_amd import _lib

    def case(ctx):
        g = _cpu_gen(9)
        frames, rows, Cc = 1030, 64, 64
        M = frames * rows
        xs, xt, dy = (torch.randn(M, Cc, generator=g) for _ in range(3))
        a = torch.rand(frames, generator=g)
        a[2] = 1.0
        lib, st = _lib.load_train(), torch.cuda.current_stream().cuda_stream
        xsg, xtg, dyg, ag = ctx.inp(xs, name="xs"), ctx.inp(xt, name="xt"), ctx.inp(dy, name="dy"), ctx.inp_flat(a, name="alpha")
        y, dxs, dxt = ctx.out("y", M, Cc, F32), ctx.out("d_xs", M, Cc, F32), ctx.out("d_xt", M, Cc, F32)
        dal = ctx.out_flat("d_alpha", (frames,), F32, init=0.0)
        _lib.check_train(lib.gcd_blend_fwd_f32(xsg.data_ptr(), xsg.stride(0), xtg.data_ptr(), xtg.stride(0), ag.data_ptr(), M, Cc,
                                               rows, y.data_ptr(), y.stride(0), st), "blend_fwd")
        _lib.check_train(lib.gcd_blend_bwd_f32(dyg.data_ptr(), dyg.stride(0), xsg.data_ptr(), xsg.stride(0), xtg.data_ptr(),
                                               xtg.stride(0), ag.data_ptr(), M, Cc, rows, dxs.data_ptr(), dxs.stride(0), 0,
                                               dxt.data_ptr(), dxt.stride(0), dal.data_ptr(), st), "blend_bwd")

        def ref():
            ar = a.repeat_interleave(rows)[:, None]
            return {"y": (ar * xs + (1 - ar) * xt, 1e-6), "d_xs": (ar * dy, 1e-6), "d_xt": ((1 - ar) * dy, 1e-6),
                    "d_alpha": ((dy * (xs - xt)).reshape(frames, -1).double().sum(1).reshape(1, -1), 1e-5)}
        return ctx.ref(ref)
    drive_ctx(gpu, spy, ("gcd_blend_fwd_f32", "gcd_blend_bwd_f32"), "blend", case, ("xs", "xt", "dy", "y", "d_xs", "d_xt"))


def test_deterministic_reductions_far_operands(gpu, spy):
    """The four strided exports of gcd_amd_train_det.h through test_memcontract_det_gpu.py's cases: 1030 blocks of 64 rows."""
    import test_memcontract_det_gpu as D
    drive_ctx(gpu, spy, ("gcd_rowblock_sum_det_f32",), "rowblock_sum_det", lambda ctx: D._rowblock_case(ctx, 1030, 64, 64, 4), ("x",))
    drive_ctx(gpu, spy, ("gcd_layernorm_bwd_det",), "layernorm_bwd_det", lambda ctx: D._ln_case(ctx, ROWS + 3, 64, 4, True),
              ("x", "dy", "dx", "dx_add"))
    drive_ctx(gpu, spy, ("gcd_cast_colsum_det_f32",), "cast_colsum_det", lambda ctx: D._cast_case(ctx, 1030, 64, 64, F16, True, 4),
              ("x", "y16"))
    drive_ctx(gpu, spy, ("gcd_blend_bwd_det_f32",), "blend_bwd_det", lambda ctx: D._blend_case(ctx, 1030, 64, 64, 4),
              ("dy", "xs", "xt", "d_xs", "d_xt"))


def test_norm_backwards_and_column_sums_far_operands(gpu, spy):
    """gcd_groupnorm_bwd, gcd_layernorm_bwd, gcd_rowblock_sum_f32 and gcd_cast_colsum_f32 through the wrappers of
    gcd_amd.autograd_ops (which allocate their results compactly: the far operands are the inputs)."""
    import test_memcontract_train_gpu as T
    from gcd_amd import autograd_ops as A
    drive_ctx(gpu, spy, ("gcd_groupnorm_bwd",), "groupnorm_bwd",
              lambda ctx: T._gn_bwd_case(ctx, 1030, 64, 64, 0, True), ("x", "dy"))
    drive_ctx(gpu, spy, ("gcd_layernorm_bwd",), "layernorm_bwd", lambda ctx: T._ln_bwd_case(ctx, ROWS + 3, 64), ("x", "dy"))

    def sums(ctx):                                        # test_memcontract_train_gpu.py's cast16_colsum_and_colsum, 1030 x 64 rows
        rows, blocks, N = 64, 1030, 72
        dy = torch.randn(rows * blocks, N, generator=_cpu_gen(2))
        dyg = ctx.inp(dy, name="dy32")
        y16, s1 = A._cast16_colsum(dyg, F16, rows)
        for n, t in (("y16", y16), ("sums", s1), ("colsum_blocks", A._colsum(dyg, rows)), ("colsum_all", A._colsum(dyg))):
            ctx.also(n, t)

        def ref():
            s = dy.double().reshape(blocks, rows, N).sum(1)
            return {"y16": (dy.half().float(), 1e-30), "sums": (s, 1e-5), "colsum_blocks": (s, 1e-5),
                    "colsum_all": (s.sum(0, keepdim=True), 1e-5)}
        return ctx.ref(ref)
    drive_ctx(gpu, spy, ("gcd_cast_colsum_f32", "gcd_rowblock_sum_f32"), "cast + column sums", sums, ("dy32",))


@pytest.mark.parametrize("export,T,HW", [("gcd_attn_temporal_bwd", 16, 2059), ("gcd_attn_temporal_long_bwd", 33, 999)])
def test_attn_temporal_bwd_far_operands(gpu, spy, export, T, HW):
    import test_memcontract_train_gpu as M
    drive_ctx(gpu, spy, (export,), export, lambda ctx: M._temporal_bwd_direct(ctx, export, 2, T, HW, 1), ("qkv16", "dO", "dqkv"))


def test_attn_spatial_bwd_far_operands(gpu, spy):
    """test_memcontract_train_gpu.py's attn_spatial_bwd_direct at frames x S = 257 x 257."""
    from gcd_amd import ops

    def case(ctx):
        g = _cpu_gen(71)
        frames, S, heads = 257, 257, 1
        C_ = heads * 64
        qkv = (torch.randn(frames * S, 3 * C_, generator=g) * torch.linspace(0.3, 2.0, frames * S)[:, None]).half()
        dO = (torch.randn(frames * S, C_, generator=g) * torch.linspace(2.0, 0.1, frames * S)[:, None]).half()
        q, k, v = (t.double().reshape(frames, S, heads, 64).transpose(1, 2).requires_grad_(True) for t in qkv.chunk(3, dim=-1))
        o = F.scaled_dot_product_attention(q, k, v)
        o16 = o.detach().transpose(1, 2).reshape(frames * S, C_).half()
        dqkv = ctx.out("dqkv", frames * S, 3 * C_, F32)
        # (whole 16-byte units: the guarded scratch then starts 16-byte aligned, which the entry requires)
        ws = ctx.scratch((ops.attn_spatial_bwd_ws_bytes(frames, S, heads) + 15) // 16 * 16, torch.uint8, name="ws")
        ops.attn_spatial_bwd(ctx.inp(qkv, name="qkv"), ctx.inp(o16, name="out16"), ctx.inp(dO, name="dout16"), dqkv, frames, S,
                             heads, ws)

        def ref():
            o.backward(dO.double().reshape(frames, S, heads, 64).transpose(1, 2))
            return {"dqkv": (torch.cat([t.grad.transpose(1, 2).reshape(frames * S, C_) for t in (q, k, v)], 1), 1e-3)}
        return ctx.ref(ref)
    drive_ctx(gpu, spy, ("gcd_attn_spatial_bwd",), "spatial attention backward", case, ("qkv", "out16", "dout16", "dqkv"))


def test_geglu_softmax_bwd_and_scaled_cast_far_operands(gpu, spy):
    """The strided main-library exports without a wrapper in ops.py: GEGLU forward (fp32 / fp16 / bf16 result) and backward at
    the bars of test_memcontract_train_gpu.py's geglu case and test_conditioning_gpu.py's half-ulp bound (as rel-L2: 2^-11 /
    2^-8 plus the 1e-5 of the fp32 form); gcd_cast_f16_bf16 and gcd_cast_scale_f32_f16 (a power-of-two scale: one rounding,
    exact against torch); gcd_softmax_bwd_rows, which has no parity test of its own: one fp16 rounding of an fp32 result,
    2^-11 per element, against the fp64 formula on the same operands, at TOL_F16 like every fp16 result here."""
    from gcd_amd import _lib
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    M, H = ROWS, 72

    def geglu(ctx):
        g = _cpu_gen(6)
        h, dout = torch.randn(M, 2 * H, generator=g) * 1.5, torch.randn(M, H, generator=g)
        hg, dog = ctx.inp(h, name="h"), ctx.inp(dout, name="dout")
        out, dh = ctx.out("out", M, H, F32), ctx.out("dh", M, 2 * H, F32)
        o16, ob = ctx.out("out16", M, H, F16, pad=8), ctx.out("outbf", M, H, BF16, pad=8)
        _lib.check(lib.gcd_geglu_fwd_f32(hg.data_ptr(), hg.stride(0), out.data_ptr(), out.stride(0), M, H, st), "geglu_fwd_f32")
        _lib.check(lib.gcd_geglu_fwd_f16(hg.data_ptr(), hg.stride(0), o16.data_ptr(), o16.stride(0), M, H, st), "geglu_fwd_f16")
        _lib.check(lib.gcd_geglu_fwd_bf16(hg.data_ptr(), hg.stride(0), ob.data_ptr(), ob.stride(0), M, H, st), "geglu_fwd_bf16")
        _lib.check(lib.gcd_geglu_bwd_f32(hg.data_ptr(), hg.stride(0), dog.data_ptr(), dog.stride(0), dh.data_ptr(), dh.stride(0),
                                         M, H, st), "geglu_bwd_f32")

        def ref():
            hr = h.double().requires_grad_(True)
            a, gate = hr.chunk(2, dim=-1)
            y = a * F.gelu(gate)
            y.backward(dout.double())
            yd = y.detach()
            return {"out": (yd, 1e-5), "dh": (hr.grad, 1e-5), "out16": (yd, 2.0 ** -11 + 1e-5), "outbf": (yd, 2.0 ** -8 + 1e-5)}
        return ctx.ref(ref)
    drive_ctx(gpu, spy, ("gcd_geglu_fwd_f32", "gcd_geglu_fwd_f16", "gcd_geglu_fwd_bf16", "gcd_geglu_bwd_f32"), "geglu", geglu,
              ("h", "dout", "out", "dh", "out16", "outbf"))

    def casts(ctx):
        g = _cpu_gen(15)
        x, x16 = torch.randn(M, 72, generator=g) * 3, torch.randn(M, 72, generator=g).half()
        xg, hg = ctx.inp(x, name="x32"), ctx.inp(x16, name="x16")
        ys, yb = ctx.out("scaled", M, 72, F16, pad=8), ctx.out("bf16", M, 72, BF16, pad=8)
        _lib.check(lib.gcd_cast_scale_f32_f16(xg.data_ptr(), xg.stride(0), ys.data_ptr(), ys.stride(0), M, 72, 64.0, st), "cast_scale")
        _lib.check(lib.gcd_cast_f16_bf16(hg.data_ptr(), hg.stride(0), yb.data_ptr(), yb.stride(0), M, 72, st), "cast_f16_bf16")
        return ctx.ref(lambda: {"scaled": ((x * 64.0).half().float(), 1e-30), "bf16": (x16.to(BF16).float(), 1e-30)})
    drive_ctx(gpu, spy, ("gcd_cast_scale_f32_f16", "gcd_cast_f16_bf16"), "casts", casts, ("x32", "x16", "scaled", "bf16"))

    def softmax_bwd(ctx):
        g = _cpu_gen(16)
        S, scale = 300, 0.125
        P = torch.softmax(torch.randn(M, S, generator=g) * 2, -1).half()
        dP = torch.randn(M, S, generator=g)
        pg, dg = ctx.inp(P, name="P16"), ctx.inp(dP, name="dP")
        dS = ctx.out("dS16", M, S, F16, pad=4)
        _lib.check(lib.gcd_softmax_bwd_rows(pg.data_ptr(), pg.stride(0), dg.data_ptr(), dg.stride(0), dS.data_ptr(), dS.stride(0),
                                            M, S, scale, st), "gcd_softmax_bwd_rows")

        def ref():
            p, d = P.double(), dP.double()
            return {"dS16": (p * (d - (p * d).sum(-1, keepdim=True)) * scale, TOL_F16)}
        return ctx.ref(ref)
    drive_ctx(gpu, spy, ("gcd_softmax_bwd_rows",), "softmax_bwd_rows", softmax_bwd, ("P16", "dP", "dS16"))


# ============================================================================== part B: the tile kernels' packed fields
def _first_last_overall(what, out, ref, rows_per_frame, bar):
    from conftest import rel_l2
    fig = {"first frame": rel_l2(out[:rows_per_frame], ref[:rows_per_frame]),
           "last frame": rel_l2(out[-rows_per_frame:], ref[-rows_per_frame:]), "overall": rel_l2(out, ref)}
    print(f"{what}: " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    for k, v in fig.items():
        assert v < bar, f"{what}: rel-L2 {v:.3e} on the {k}"


@tile_impls
@pytest.mark.parametrize("frames,H,W", [(2046, 8, 8), (2047, 8, 8), (1, 1024, 8), (1, 1032, 8), (1, 2, 2048), (1, 2, 2056)])
def test_conv3x3_at_the_packed_field_limits(gpu, impl, frames, H, W):
    """frames <= 2046, Ho <= 1024, Wo <= 2048 (11 + 10 + 11 bits): the last admitted value and the first refused one."""
    from gcd_amd import ops, packing
    g = _gen(gpu, 21)
    a = _randn(g, frames * H * W, 64, dtype=F16)
    w, b = _h(_randn(g, 64, 64, 3, 3) / 24.0), _randn(g, 64)
    out = torch.empty(frames * H * W, 64, device=gpu)
    ops.gemm(a, packing.pack_conv3x3(w.cpu()).to(gpu), out, M=frames * H * W, mode=ops.GEMM_CONV3X3, bias=b,
             conv=dict(Cin=64, Hi=H, Wi=W, Ho=H, Wo=W, stride=1, upsample=0))
    torch.cuda.synchronize()
    _first_last_overall(f"conv3x3 {frames}x{H}x{W} [{impl}]", out, _conv_ref(a, frames, H, W, w, b, 1, 0), H * W, TOL_F32)


@tile_impls
@pytest.mark.parametrize("T", [31, 32])
def test_conv_temporal3_at_T_31_and_32(gpu, impl, T):
    from gcd_amd import ops, packing
    g = _gen(gpu, 22)
    clips, HW, C = 2, 40, 64
    a = _randn(g, clips * T * HW, C, dtype=F16)
    w, b = _h(_randn(g, C, C, 3, 1, 1) / math.sqrt(3 * C)), _randn(g, C)
    out = torch.empty(clips * T * HW, C, device=gpu)
    ops.gemm(a, packing.pack_conv_t3(w.cpu()).to(gpu), out, M=clips * T * HW, mode=ops.GEMM_TEMPORAL3, bias=b,
             conv=dict(Cin=C, T=T, HW=HW))
    torch.cuda.synchronize()
    x5 = a.cpu().double().reshape(clips, T, HW, 1, C).permute(0, 4, 1, 2, 3)
    ref = F.conv3d(x5, w.cpu().double(), b.cpu().double(), padding=(1, 0, 0))[..., 0].permute(0, 2, 3, 1).reshape(-1, C)
    _first_last_overall(f"temporal3 T={T} [{impl}]", out, ref, HW, TOL_F32)


# =========================================================================== part C: gcd_groupnorm_apply past 65 535 chunks
@pytest.mark.parametrize("silu", [True, False])
def test_groupnorm_apply_beyond_65535_row_chunks(gpu, silu):
    """C = 32, one instance of 65 535 x 512 + 4 099 rows (4.3 GB of fp32 in, 2.1 GB of fp16 out per result)."""
    from gcd_amd import ops
    C, rows = 32, 65535 * 512 + 4099
    rpc = (16384 + C - 1) // C                            # the launch arithmetic of gcd_groupnorm_apply (norm.hip)
    assert (rows + rpc - 1) // rpc > 65535
    rpc2 = (rows + 65535 - 1) // 65535
    assert rpc2 > rpc and (rows + rpc2 - 1) // rpc2 <= 65535
    torch.cuda.reset_peak_memory_stats()
    g = _gen(gpu, 8)
    x = torch.empty(rows, C, device=gpu)
    step = 1 << 22
    for r in range(0, rows, step):
        x[r:r + step] = torch.randn(min(step, rows - r), C, device=gpu, generator=g) * 3 + 1.5
    gamma, beta = _randn(g, C), _randn(g, C)
    nch = ops.gn_nchunks(rows)
    stats = torch.empty(64, device=gpu)
    ops.groupnorm_stats(x, None, rows, 1e-5, torch.empty(nch * 64, dtype=F64, device=gpu), stats, nch)
    y = mc.poison_scratch(torch.empty(rows, C, dtype=F16, device=gpu))          # NaN: a row never written fails its band
    raw = mc.poison_scratch(torch.empty(rows, C, dtype=F16, device=gpu)) if silu else None
    ops.groupnorm_apply(x, None, rows, stats, gamma, beta, silu, y, raw)
    torch.cuda.synchronize()
    s, q = torch.zeros(C, dtype=F64, device=gpu), torch.zeros(C, dtype=F64, device=gpu)
    for r in range(0, rows, step):
        xd = x[r:r + step].double()
        s, q = s + xd.sum(0), q + (xd * xd).sum(0)
    mean = s / rows                                       # C / 32 = 1 channel per group
    rstd = 1 / torch.sqrt(q / rows - mean * mean + 1e-5)
    st = torch.stack([mean, rstd], -1).reshape(-1)
    e = float((stats.double() - st).norm() / st.norm())
    print(f"groupnorm statistics of {rows} rows: rel-L2 {e:.2e}")
    assert e < 1e-5
    fig = {}                                               # band -> [d(y), n(y), d(raw16), n(raw16)]
    for r in range(0, rows, step):
        xd = x[r:r + step].double()
        ref = (xd - mean) * rstd * gamma.double() + beta.double()
        ref = F.silu(ref) if silu else ref
        acc = fig.setdefault("first rows" if r == 0 else "last rows" if r + step >= rows else "the rest", [0.0] * 4)
        acc[0] += float(((y[r:r + step].double() - ref) ** 2).sum())
        acc[1] += float((ref ** 2).sum())
        if raw is not None:
            acc[2] += float(((raw[r:r + step].double() - xd) ** 2).sum())
            acc[3] += float((xd ** 2).sum())
    assert len(fig) == 3
    print(f"groupnorm_apply silu={silu}: " + ", ".join(f"{k} y {math.sqrt(v[0] / v[1]):.2e}" for k, v in fig.items())
          + f", peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    for k, v in fig.items():
        assert math.sqrt(v[0] / v[1]) < TOL_F16, (k, v)
        assert raw is None or math.sqrt(v[2] / v[3]) < TOL_F16, (k, v)
    del x, y, raw
    gc.collect()
    torch.cuda.empty_cache()


# ================================================================== part D: the engine at 64 frames under CFG, 72 x 128
def test_engine_64_frames_under_cfg_at_72x128(gpu, monkeypatch):
    """The one-level width-320 network at 2 clips x 64 frames x 72 x 128: M = 1 179 648 tokens, q | k | v = 2.26 GB, past
    the 2^31 bytes `gcd_lnqkv_f16` can address, so `_ln_qkv` must take LayerNorm + GEMM for the joint call (it raised
    GcdError before `ops.lnqkv_ok` knew the size) while each clip alone (M = 589 824) keeps the fused kernel.  There is no
    oracle at this size: the clips are independent, so each half of the joint output is held to its clip run alone.  Two
    correct paths differ by their rounding points; the bar is 4 x the rel-L2 measured here between the SAME one-clip
    forward with the fused kernels on and off, and never above TOL_FWD = 2e-3 of test_unet_gpu.py.
    Measured: fused vs unfused at M = 589 824 7.0e-4 (so the bar is 2e-3), the halves of the joint call against each clip
    alone 7.0e-4 / 6.6e-4, peak memory 12.8 GiB ("Capacity")."""
    import dataclasses
    from conftest import rel_l2
    from gcd_amd import ops
    from oracle import svd_unet_ref as O
    from test_memcontract_gpu import _engine_forward, _net, _two_clips
    cfg = dataclasses.replace(O.TINY, model_channels=320, channel_mult=(1,), attention_resolutions=(1,), num_res_blocks=1)
    T, H, W = 64, 72, 128
    M = 2 * T * H * W
    assert M == 1179648 and not ops.lnqkv_ok(M, 320, 960) and ops.lnqkv_ok(M // 2, 320, 960)
    calls = {"lnqkv": [], "ff_fused": []}
    real_qkv, real_ff = ops.lnqkv, ops.ff_fused
    monkeypatch.setattr(ops, "lnqkv", lambda *a, **k: (calls["lnqkv"].append(k["M"]), real_qkv(*a, **k))[1])
    monkeypatch.setattr(ops, "ff_fused", lambda *a, **k: (calls["ff_fused"].append(k["M"]), real_ff(*a, **k))[1])
    x, ts, ctx, y, ioi = _two_clips(cfg, T, H, W, 93)

    def clip(net, c):
        sl = slice(c * T, (c + 1) * T)
        return _engine_forward(net, gpu, x[sl], ts[sl], ctx[sl], y[sl], T, ioi[c:c + 1]).clone()
    torch.cuda.reset_peak_memory_stats()
    net, _ = _net(gpu, cfg)
    with torch.no_grad():
        joint = _engine_forward(net, gpu, x, ts, ctx, y, T, ioi).clone()
        assert calls["lnqkv"] == [], "gcd_lnqkv_f16 was launched on 2.26 GB of q | k | v"
        assert calls["ff_fused"] and set(calls["ff_fused"]) == {M}       # 1.5 GB of fp32 rows: within ff_fused's limit
        alone = [clip(net, 0), clip(net, 1)]
        assert calls["lnqkv"] and set(calls["lnqkv"]) == {M // 2}
        peak = torch.cuda.max_memory_allocated() / 2 ** 30
        del net                                           # a fresh engine: its workspace replays one allocation trace per shape
        gc.collect()
        torch.cuda.empty_cache()
        n = len(calls["lnqkv"]), len(calls["ff_fused"])
        monkeypatch.setattr(ops, "LNQKV_MIN_TOKENS", 10 ** 9)
        monkeypatch.setattr(ops, "FF_FUSED_MIN_TOKENS", 10 ** 9)
        net, _ = _net(gpu, cfg)
        unfused = clip(net, 0)
        assert (len(calls["lnqkv"]), len(calls["ff_fused"])) == n
        del net
    assert torch.isfinite(joint).all()
    spread = rel_l2(alone[0], unfused)
    bar = min(4 * spread, 2e-3)
    figs = [rel_l2(joint[c * T:(c + 1) * T], alone[c]) for c in range(2)]
    print(f"engine 2 x 64 x 72 x 128: fused vs unfused at M = {M // 2}: {spread:.3e} -> bar {bar:.3e}; joint halves vs each "
          f"clip alone {figs[0]:.3e} {figs[1]:.3e}; peak memory {peak:.2f} GiB")
    assert spread > 0 and all(f < bar for f in figs), (figs, bar)
    gc.collect()
    torch.cuda.empty_cache()


# ======================================================================================= coverage table (read on the CPU)
# wrapper of gcd_amd/ops.py or export of the fine-tune headers that takes a row stride -> the part-A test that runs it far
FAR_CASES = {
    "gemm": "test_gemm_plain_far_operands, test_gemm_conv3x3_far_operands, test_gemm_temporal3_far_operands",
    "ff_fused": "test_ff_fused_far_inputs, test_ff_fused_far_out_at_its_largest_M",
    "lnqkv": "test_lnqkv_far_operands",
    "layernorm": "test_layernorm_far_operands",
    "groupnorm_stats": "test_groupnorm_far_operands",
    "groupnorm_apply": "test_groupnorm_far_operands",
    "cast_f16": "test_cast_far_operands",
    "cast_bf16": "test_cast_far_operands",
    "attn_transpose_v": "test_attn_spatial_far_operands",
    "attn_spatial": "test_attn_spatial_far_operands",
    "attn_temporal": "test_attn_temporal_far_operands",
    "linear_smallm": "test_linear_smallm_far_operands",
    "softmax_rows": "test_softmax_rows_far_operands",
    "transpose_f16": "test_transpose_f16_far_operands",
    "unpack_output": "test_unpack_output_and_time_mix_unpack_far_tokens",
    "time_mix_unpack": "test_unpack_output_and_time_mix_unpack_far_tokens",
    "attn_spatial_bwd": "test_attn_spatial_bwd_far_operands",
    "gcd_wgrad_tr_f16": "test_wgrad_tr_far_operands",
    "gcd_wgrad_tr_f16_ex": "test_wgrad_tr_far_operands",
    "gcd_wgrad_conv_tr_f16": "test_wgrad_conv_tr_far_operands",
    "gcd_blend_fwd_f32": "test_blend_far_operands",
    "gcd_blend_bwd_f32": "test_blend_far_operands",
    "gcd_rowblock_sum_det_f32": "test_deterministic_reductions_far_operands",
    "gcd_layernorm_bwd_det": "test_deterministic_reductions_far_operands",
    "gcd_cast_colsum_det_f32": "test_deterministic_reductions_far_operands",
    "gcd_blend_bwd_det_f32": "test_deterministic_reductions_far_operands",
    # strided exports of include/gcd_amd.h that gcd_amd/ops.py does not wrap (called from gcd_amd/autograd_ops.py)
    "gcd_groupnorm_bwd": "test_norm_backwards_and_column_sums_far_operands",
    "gcd_layernorm_bwd": "test_norm_backwards_and_column_sums_far_operands",
    "gcd_rowblock_sum_f32": "test_norm_backwards_and_column_sums_far_operands",
    "gcd_cast_colsum_f32": "test_norm_backwards_and_column_sums_far_operands",
    "gcd_attn_temporal_bwd": "test_attn_temporal_bwd_far_operands",
    "gcd_attn_temporal_long_bwd": "test_attn_temporal_bwd_far_operands",
    "gcd_geglu_fwd_f32": "test_geglu_softmax_bwd_and_scaled_cast_far_operands",
    "gcd_geglu_fwd_f16": "test_geglu_softmax_bwd_and_scaled_cast_far_operands",
    "gcd_geglu_fwd_bf16": "test_geglu_softmax_bwd_and_scaled_cast_far_operands",
    "gcd_geglu_bwd_f32": "test_geglu_softmax_bwd_and_scaled_cast_far_operands",
    "gcd_softmax_bwd_rows": "test_geglu_softmax_bwd_and_scaled_cast_far_operands",
    "gcd_cast_scale_f32_f16": "test_geglu_softmax_bwd_and_scaled_cast_far_operands",
}
# one line each: why a far operand cannot exist for the entry
EXEMPT = {
    "gcd_im2col3x3_f16": "writes the contiguous col tensor [M, 9 Cin], whose size is inherent: 66 k tokens of it stay far below 2^31 bytes",
    "gcd_col2im3x3_f32": "reads the contiguous col tensor [M, 9 Cin] and adds into a dx of as many pixels: sizes inherent, as im2col",
    "gcd_im2col_t3_f16": "writes the contiguous col tensor [M, 3 C] of the (3, 1, 1) convolution: size inherent",
    "gcd_col2im_t3_f32": "reads the contiguous col tensor [M, 3 C] of the (3, 1, 1) convolution: size inherent",
}
