"""CPU: the size limits of the two fused C = 320 kernels, as their predicates, their entries and the engine see them.

gcd_lnqkv_f16 and gcd_ff_fused_f16 store their result through one buffer descriptor with 32-bit byte offsets.  The limits
below are worked out here, in Python integers, from the kernels' own arithmetic and not from what the library answers:

  lnqkv     num_records = M ldo 2 bytes, refused from 2^31 - 1 (gcd_lnqkv_f16's check): M ldo 2 < 2^31 - 1.
  ff_fused  num_records = M ldo es and every store offset (m ldo + 16 cb + 4 g) es are formed as `int`
            (ff_fused_kernel.h: rsrcO, store_cb), es = 4 (fp32) or 2 (fp16); m runs over the whole last 128-token tile, so
            to Mpad - 1 with Mpad = M rounded up to 128, and 16 cb + 4 g to 316.  Both <= 2^31 - 1.

The predicates are host code: they answer without a GPU, and so do the entries' argument checks, which return before
any launch.  No entry is called here with arguments it would accept.
"""
import ctypes
import types

import pytest
import torch

from gcd_amd import _lib, ops

INT_MAX = 2 ** 31 - 1
WIDE16, WIDE32 = 32768, 16384                  # a 65 536-byte row stride in fp16 / fp32 elements
FAR_M = (3 * 10 ** 6, 10 ** 7, 2 ** 31 - 1, 2 ** 32 + 5, 2 ** 40)       # int products of these wrap back into range


def lnqkv_fits(M, ldo):
    return M * ldo * 2 < INT_MAX


def ff_fits(M, ldo, es):
    mpad = (M + 127) // 128 * 128
    return M * ldo * es <= INT_MAX and ((mpad - 1) * ldo + 316) * es <= INT_MAX


def largest(fits):
    """The largest M of a monotone predicate, by bisection."""
    lo, hi = 1, 2 ** 33
    assert fits(lo) and not fits(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    return lo


@pytest.fixture
def every_size(monkeypatch):
    """The token thresholds below which the engine does not bother with the fused kernels are not the subject here."""
    monkeypatch.setattr(ops, "LNQKV_MIN_TOKENS", 1)
    monkeypatch.setattr(ops, "FF_FUSED_MIN_TOKENS", 1)


# ---------------------------------------------------------------------------------------------------------- predicates
@pytest.mark.parametrize("N,ldo", [(960, 960), (960, 1024), (960, WIDE16), (64, WIDE16), (4096, 4096)])
def test_lnqkv_predicate_ends_where_the_entry_check_does(every_size, N, ldo):
    lib = _lib.load()
    m = largest(lambda M: lnqkv_fits(M, ldo))
    assert m == (INT_MAX - 1) // (2 * ldo)                   # what gcd_lnqkv_f16's check states
    for M, want in [(1, True), (m - 1, True), (m, True), (m + 1, False), (m + 300, False)] + [(M, False) for M in FAR_M]:
        assert bool(lib.gcd_lnqkv_fits(320, N, M, ldo)) is want, (M, ldo)
        assert ops.lnqkv_ok(M, 320, N, enabled=True, ldo=ldo) is want, (M, ldo)
    assert not lib.gcd_lnqkv_fits(320, N, 0, ldo) and not lib.gcd_lnqkv_fits(320, N, -5, ldo)
    assert not lib.gcd_lnqkv_fits(320, N, 1, N - 8) and not lib.gcd_lnqkv_fits(320, N, 1, 2 ** 40)
    assert not lib.gcd_lnqkv_fits(640, N, 1, ldo)
    assert lib.gcd_lnqkv_supported(320, N)                   # the shape-only question keeps its answer


def test_lnqkv_predicate_at_the_documented_clip_sizes(every_size):
    """CFG at 72 x 128 latents: 2 x frames x 9216 tokens, q | k | v = 960 columns.  60 frames fit, 61 do not."""
    assert ops.lnqkv_ok(2 * 60 * 9216, 320, 960, enabled=True)
    assert not ops.lnqkv_ok(2 * 61 * 9216, 320, 960, enabled=True)
    assert not ops.lnqkv_ok(2 * 64 * 9216, 320, 960, enabled=True)
    assert ops.lnqkv_ok(64 * 9216, 320, 960, enabled=True)   # one clip of 64 frames


@pytest.mark.parametrize("kind,es,ldo", [(ops.OUT_F32, 4, 320), (ops.OUT_F32, 4, 324), (ops.OUT_F32, 4, WIDE32),
                                          (ops.OUT_F16, 2, 320), (ops.OUT_F16, 2, 328), (ops.OUT_F16, 2, WIDE16)])
def test_ff_fused_predicate_ends_at_the_kernels_int_arithmetic(every_size, kind, es, ldo):
    lib = _lib.load()
    m = largest(lambda M: ff_fits(M, ldo, es))
    # (3 * 10^6 rows of 640 bytes are 1.92 GB: the compact fp16 result alone still admits the first of FAR_M)
    for M, want in [(1, True), (m - 1, True), (m, True), (m + 1, False), (m + 128, False), (m + 300, False)] + \
                   [(M, M <= m) for M in FAR_M]:
        assert want is ff_fits(M, ldo, es) and (want or M > m) and not (want and M >= 10 ** 7)
        assert bool(lib.gcd_ff_fused_fits(M, 320, 1280, ldo, kind)) is want, (M, ldo, kind)
        assert ops.ff_fused_ok(M, 320, 1280, enabled=True, ldo=ldo, out_kind=kind) is want, (M, ldo, kind)
    assert not lib.gcd_ff_fused_fits(0, 320, 1280, ldo, kind)
    assert not lib.gcd_ff_fused_fits(1, 320, 1280, 316, kind) and not lib.gcd_ff_fused_fits(1, 320, 1280, 2 ** 40, kind)
    assert not lib.gcd_ff_fused_fits(1, 640, 2560, ldo, kind) and not lib.gcd_ff_fused_fits(1, 320, 1280, ldo, 2)


def test_ff_fused_predicate_at_the_documented_clip_sizes(every_size):
    """Compact fp32 rows of 1280 bytes: two 64-frame clips under CFG (1.5 GB) fit, three (2.26 GB) do not; and the
    defaults of `ff_fused_ok` are the compact fp32 result."""
    assert ops.ff_fused_ok(2 * 64 * 9216, 320, 1280, enabled=True)
    assert ops.ff_fused_ok(2 * 64 * 9216, 320, 1280, enabled=True, ldo=320, out_kind=ops.OUT_F32)
    assert not ops.ff_fused_ok(3 * 64 * 9216, 320, 1280, enabled=True)
    assert ops.ff_fused_ok(3 * 64 * 9216, 320, 1280, enabled=True, out_kind=ops.OUT_F16)     # 1.13 GB of fp16
    assert not ops.ff_fused_ok(2 * 64 * 9216, 320, 1280, enabled=True, ldo=640)               # a view of wider rows


# ------------------------------------------------------------------------------------- the entries refuse where they say no
def _small():
    """Real, 16-byte aligned host memory for every pointer argument; no entry below gets as far as reading it."""
    return types.SimpleNamespace(x32=torch.zeros(4, 320), vec=torch.zeros(2560), wp=torch.zeros(4096, dtype=torch.float16),
                                 out32=torch.zeros(4, 320), out16=torch.zeros(4, 960, dtype=torch.float16),
                                 x16=torch.zeros(4, 320, dtype=torch.float16))


@pytest.mark.parametrize("ldo", [960, WIDE16])
def test_lnqkv_entry_refuses_one_row_past_the_predicate(ldo):
    lib, t = _lib.load(), _small()
    m = largest(lambda M: lnqkv_fits(M, ldo))
    assert lib.gcd_lnqkv_fits(320, 960, m, ldo) and not lib.gcd_lnqkv_fits(320, 960, m + 1, ldo)
    for M in (m + 1, INT_MAX):
        rc = lib.gcd_lnqkv_f16(t.x32.data_ptr(), 320, t.vec.data_ptr(), t.vec.data_ptr(), 1e-5, t.wp.data_ptr(),
                               t.out16.data_ptr(), ldo, M, 320, 960, 0, None)
        assert rc != 0
        with pytest.raises(_lib.GcdError, match=r"32-bit buffer offsets \(M ldo 2 < 2\^31 - 1 bytes\)"):
            _lib.check(rc, "gcd_lnqkv_f16")


@pytest.mark.parametrize("form", ["layernorm", "x16"])
@pytest.mark.parametrize("kind,es,ldo", [(ops.OUT_F32, 4, 320), (ops.OUT_F32, 4, WIDE32), (ops.OUT_F16, 2, 320),
                                          (ops.OUT_F16, 2, WIDE16)])
def test_ff_fused_entry_refuses_one_row_past_the_predicate(form, kind, es, ldo):
    lib, t = _lib.load(), _small()
    m = largest(lambda M: ff_fits(M, ldo, es))
    assert lib.gcd_ff_fused_fits(m, 320, 1280, ldo, kind) and not lib.gcd_ff_fused_fits(m + 1, 320, 1280, ldo, kind)
    d = _lib.FfDesc()
    d.wp, d.b1, d.b2 = t.wp.data_ptr(), t.vec.data_ptr(), t.vec.data_ptr()
    if form == "layernorm":
        d.x32, d.ldx32, d.ln_gamma, d.ln_beta, d.ln_eps = t.x32.data_ptr(), 320, t.vec.data_ptr(), t.vec.data_ptr(), 1e-5
    else:
        d.X, d.ldx, d.R1, d.ldr1 = t.x16.data_ptr(), 320, t.x32.data_ptr(), 320
    d.R2, d.ldr2 = t.x32.data_ptr(), 320
    d.out, d.ldo, d.out_kind = (t.out32 if kind == ops.OUT_F32 else t.out16).data_ptr(), ldo, kind
    d.s_acc = d.s_r2 = 1.0
    d.C, d.hidden = 320, 1280
    for M in (m + 1, INT_MAX):
        d.M = M
        rc = lib.gcd_ff_fused_f16(ctypes.byref(d), None)
        assert rc != 0
        with pytest.raises(_lib.GcdError, match=r"exceeds the 32-bit buffer offsets \(2\^31 - 1 bytes\)"):
            _lib.check(rc, "gcd_ff_fused_f16")


# ---------------------------------------------------------------------------------------------------- the engine's choice
class _Recorder:
    """Stands in for the engine's `self`: the two methods under test touch the workspace, the LayerNorm and the GEMM
    only through it.  Tensors live on the `meta` device: shapes and strides without memory."""

    fuse_layernorm = False

    def __init__(self):
        self.calls = []
        self.ws = types.SimpleNamespace(alloc=lambda shape, dtype: torch.empty(shape, dtype=dtype, device="meta"),
                                        release=lambda t: None)

    def _ln(self, x32, affine):
        self.calls.append("layernorm")
        return torch.empty(x32.shape, dtype=torch.float16, device="meta")

    def _gemm(self, a16, w16, out, **kw):
        self.calls.append(("gemm", kw["M"], tuple(out.shape)))

    def _next_dir(self):
        return 0


def _raise(name):
    def spy(*a, **k):
        raise AssertionError(f"{name} would have been launched")
    return spy


def test_engine_takes_layernorm_and_gemm_where_lnqkv_does_not_fit(monkeypatch):
    from gcd_amd.engine import UNetEngine
    M = 2 * 64 * 9216                                         # CFG, 64 frames, 72 x 128 latents
    A = dict(wqkv=torch.empty(960, 320, dtype=torch.float16, device="meta"), wqkv_p=object())
    x32, affine = torch.empty(M, 320, device="meta"), (None, None)
    fused = []
    monkeypatch.setattr(ops, "lnqkv", lambda *a, **k: fused.append(k["M"]))
    rec = _Recorder()
    UNetEngine._ln_qkv(rec, A, torch.empty(M // 2, 320, device="meta"), affine, M // 2)        # one clip: the fused kernel
    assert fused == [M // 2] and rec.calls == []
    monkeypatch.setattr(ops, "lnqkv", _raise("gcd_lnqkv_f16"))
    qkv = UNetEngine._ln_qkv(rec, A, x32, affine, M)
    assert rec.calls == ["layernorm", ("gemm", M, (M, 960))] and tuple(qkv.shape) == (M, 960)


def test_engine_takes_layernorm_and_two_gemms_where_ff_fused_does_not_fit(monkeypatch):
    """The compact fp32 result of M = 1 179 648 tokens is 1.5 GB and fits; the first engine-shaped call that does not is
    three 64-frame clips, and a result with wider rows at two."""
    from gcd_amd.engine import UNetEngine
    M = 2 * 64 * 9216
    Fw = dict(wp=object(), w1=torch.empty(2560, 320, dtype=torch.float16, device="meta"), b1=None, b2=None)
    fused = []
    monkeypatch.setattr(ops, "ff_fused", lambda *a, **k: fused.append(k["M"]))
    rec = _Recorder()
    assert UNetEngine._ff_ln(rec, Fw, torch.empty(M, 320, device="meta"), (None, None), M,
                             out=torch.empty(M, 320, device="meta")) is True
    assert fused == [M]
    monkeypatch.setattr(ops, "ff_fused", _raise("gcd_ff_fused_f16"))
    M3 = 3 * 64 * 9216
    assert UNetEngine._ff_ln(rec, Fw, torch.empty(M3, 320, device="meta"), (None, None), M3,
                             out=torch.empty(M3, 320, device="meta")) is False
    wide = torch.empty(M, 640, device="meta")[:, :320]
    assert wide.stride(0) == 640
    assert UNetEngine._ff_ln(rec, Fw, torch.empty(M, 320, device="meta"), (None, None), M, out=wide) is False
    assert rec.calls == []                                    # False: the caller runs LayerNorm + two GEMMs itself


# ------------------------------------------------------------------------------------------ coverage of the far-operand table
def test_every_strided_entry_is_in_the_far_operand_tables():
    """Every entry that takes a row stride has a far-operand case in tests/test_capacity_gpu.py or a one-line written
    exemption there, and nothing else counts.  The entries: every public wrapper of gcd_amd/ops.py that hands a row stride to
    the library (`_ld(...)` next to `check(...)` in its body); every export of include/gcd_amd.h with an `int64_t ld*`
    parameter that ops.py does not wrap (the backward kernels, called from gcd_amd/autograd_ops.py); every export of the
    two fine-tune headers with such a parameter.  A new strided entry fails here until it has one or the other."""
    import ast
    import re
    from pathlib import Path
    import test_capacity_gpu as cap
    root = Path(__file__).resolve().parent.parent
    ops_src = (root / "gcd_amd" / "ops.py").read_text()
    strided = []
    for f in ast.parse(ops_src).body:
        if isinstance(f, ast.FunctionDef) and not f.name.startswith("_"):
            called = {getattr(n.func, "id", "") for n in ast.walk(f) if isinstance(n, ast.Call)}
            if {"check", "_ld"} <= called:
                strided.append(f.name)
    assert len(strided) >= 15, strided

    def exports(header):
        text = (root / "include" / header).read_text()
        return [m.group(1) for m in re.finditer(r"^int (gcd_\w+)\(([^;]*?)\);", text, flags=re.M | re.S)
                if re.search(r"int64_t ld\w*", m.group(2))]
    unwrapped = [e for e in exports("gcd_amd.h") if not re.search(r"\b%s\b" % e, ops_src)]
    assert len(unwrapped) >= 15 and "gcd_groupnorm_bwd" in unwrapped and "gcd_gemm_f16" not in unwrapped, unwrapped
    train = exports("gcd_amd_train.h") + exports("gcd_amd_train_det.h")
    assert len(train) >= 9, train
    strided += unwrapped + train
    assert not hasattr(cap, "NOT_YET")
    for name in strided:
        assert (name in cap.FAR_CASES) != (name in cap.EXEMPT), f"{name}: needs a far-operand case or a written exemption"
    assert set(cap.FAR_CASES) | set(cap.EXEMPT) <= set(strided), (set(cap.FAR_CASES) | set(cap.EXEMPT)) - set(strided)
    src = (root / "tests" / "test_capacity_gpu.py").read_text()
    for name, tests in cap.FAR_CASES.items():
        for t in tests.split(", "):
            assert f"def {t}(" in src, (name, t)
    assert all(len(why) > 20 and "\n" not in why for why in cap.EXEMPT.values())
