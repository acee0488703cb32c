"""The memory contract of the device-resident optimizer step (include/gcd_amd_train_optim.h; tests/memcontract.py;
DESIGN.md "Memory contract" and §11.2).

Every kernel-launching export of the header is called directly with guarded operands: parameters, moments and shadows
are in-place arguments (they start from the same values in both runs), the gradients, the device table and — for the
entries that only read it — the state block are guarded inputs, the reduction scratch is guarded and holds zeros in run
(a) and NaN in run (b), and so do the state-block fields the kernels own.  There are no read-modify-write reductions
here, so no case uses the run-to-run spread rule: run (b) is bit-identical to run (a).  On a SKIPPED step the rule "every
payload element is written" is replaced by "no payload element changes": the case's references for p, m and v are their
initial values at a bar that only bit-equal data meets.
Tensor sizes: not multiples of 4 (their guarded views are not 16-byte aligned: the scalar path), multiples of 4 (the
vector path), one past a chunk boundary."""
import ctypes
import math

import pytest
import torch

import memcontract as mc

pytestmark = pytest.mark.gpu

F32, I32, U8 = torch.float32, torch.int32, torch.uint8
CASES = []
EXACT = 1e-12          # a rel-L2 bar that only identical values meet
CHUNK = 16384
SIZES = [5, 64, 16384 + 4, 1001, 2 * 16384, 16385]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _lt():
    from gcd_amd import _lib
    return _lib, _lib.load_train()


def case(cid, entries):
    def deco(fn):
        CASES.append(mc.Case(cid, entries, fn, no_ref=("state",)))
        return fn
    return deco


def _config(**kw):
    _lib, _ = _lt()
    c = _lib.OptimConfig()
    c.beta1, c.beta2, c.eps, c.weight_decay, c.grad_scale = 0.9, 0.999, 1e-8, 0.0, 1.0
    c.growth_factor, c.backoff_factor, c.growth_interval, c.ema_decay = 2.0, 0.5, 3, 0.99
    for k, v in kw.items():
        setattr(c, k, v)
    return c


_OWNED = ("found_inf", "grad_norm", "clip_coef", "gfactor", "bc1", "bc2_sqrt", "ema_omd")


def _state_words(poison_owned, **fields):
    """A gcd_optim_state as 16 int32 words; the fields the kernels own hold the NaN pattern when `poison_owned`."""
    _lib, _ = _lt()
    st = _lib.OptimState()
    st.loss_scale = 1.0
    for k, v in fields.items():
        setattr(st, k, v)
    words = torch.frombuffer(bytearray(bytes(st)), dtype=I32).clone()
    if poison_owned:
        for name in _OWNED:
            if name not in fields:
                words[getattr(_lib.OptimState, name).offset // 4] = mc.POISON[I32]
    return words


class Operands:
    """The tensor set of one run, every tensor in its own guarded arena, and the device table over them."""

    def __init__(self, ctx, seed, *, with_g=True, with_ema=True, with_mv=True, bad=None, null_g=()):
        g = _gen(seed)
        self.p0 = [torch.randn(n, generator=g) for n in SIZES]
        self.g0 = [torch.randn(n, generator=g) for n in SIZES]
        self.m0 = [torch.randn(n, generator=g) * 0.1 for n in SIZES]
        self.v0 = [torch.rand(n, generator=g) * 0.1 for n in SIZES]
        self.e0 = [torch.randn(n, generator=g) for n in SIZES]
        if bad is not None:
            self.g0[bad[0]][bad[1]] = bad[2]
        self.null_g = set(null_g)
        flat = lambda name, vals: [ctx.out_flat(f"{name}{i}", (v.numel(),), F32, init=v) for i, v in enumerate(vals)]  # noqa: E731
        self.p = flat("p", self.p0)
        self.m = flat("m", self.m0) if with_mv else None
        self.v = flat("v", self.v0) if with_mv else None
        self.e = flat("ema", self.e0) if with_ema else None
        self.g = [ctx.inp_flat(v, name=f"g{i}") for i, v in enumerate(self.g0)] if with_g else None
        _lib, _ = _lt()
        arr = (_lib.OptimTensor * len(SIZES))()
        chunk0 = 0
        for i, n in enumerate(SIZES):
            t = arr[i]
            t.p, t.n, t.chunk0 = self.p[i].data_ptr(), n, chunk0
            t.g = self.g[i].data_ptr() if with_g and i not in self.null_g else None
            t.m = self.m[i].data_ptr() if with_mv else None
            t.v = self.v[i].data_ptr() if with_mv else None
            t.ema = self.e[i].data_ptr() if with_ema else None
            chunk0 += -(-n // CHUNK)
        self.chunks = chunk0
        self.table = ctx.inp_flat(torch.frombuffer(bytearray(bytes(arr)), dtype=U8).clone(), name="table")
        assert self.table.data_ptr() % 8 == 0


def _adam_ref(o, cfg, lr, step, gfactor, *, skipped=False, omd=None):
    """fp64: what gcd_optim_apply leaves in p, m, v (and ema) — torch.optim.Adam / AdamW's arithmetic."""
    out = {}
    bc1, bc2 = 1.0 - cfg.beta1 ** step, 1.0 - cfg.beta2 ** step
    for i in range(len(SIZES)):
        p, m, v = o.p0[i].double(), o.m0[i].double(), o.v0[i].double()
        if not skipped and i not in o.null_g:
            gr = o.g0[i].double() * gfactor
            if cfg.decoupled:
                p = p * (1.0 - lr * cfg.weight_decay)
            elif cfg.weight_decay:
                gr = gr + cfg.weight_decay * p
            m = cfg.beta1 * m + (1.0 - cfg.beta1) * gr
            v = cfg.beta2 * v + (1.0 - cfg.beta2) * gr * gr
            p = p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + cfg.eps)
        exact = skipped or i in o.null_g
        out[f"p{i}"], out[f"m{i}"], out[f"v{i}"] = (p, EXACT if exact else 1e-6), (m, EXACT if exact else 1e-6), \
            (v, EXACT if exact else 1e-6)
        if omd is not None:
            e = o.e0[i].double()
            out[f"ema{i}"] = (e - omd * (e - p), 1e-6)
    return {k: (t.reshape(1, -1), bar) for k, (t, bar) in out.items()}


def _also_state(ctx, state, floats, ints):
    """The state block's fields as two extra outputs (the block itself is compared between the runs, bit for bit)."""
    _lib, _ = _lt()
    f32 = state.view(F32)
    ctx.also("state_floats", torch.stack([f32[getattr(_lib.OptimState, n).offset // 4] for n in floats]))
    ctx.also("state_ints", torch.stack([state[getattr(_lib.OptimState, n).offset // 4] for n in ints]).double())


_F = ("lr", "loss_scale", "grad_norm", "clip_coef", "gfactor", "bc1", "bc2_sqrt")
_I = ("step", "growth_tracker", "found_inf", "skipped_total", "ema_num_updates")


@case("gradstat/finite-clip-dynamic", ["gcd_optim_gradstat"])
def _gradstat_finite(ctx):
    _lib, lib = _lt()
    o = Operands(ctx, 1, with_ema=False, with_mv=False, null_g=(3,))
    cfg = _config(grad_scale=0.5, max_norm=2.0, dynamic_scale=1, use_ema=1)
    state = ctx.out_flat("state", (16,), I32, init=_state_words(ctx.poisoned, step=4, lr=1e-3, loss_scale=8.0,
                                                                growth_tracker=2, skipped_total=1, ema_num_updates=6))
    scratch = ctx.scratch((lib.gcd_optim_gradstat_scratch_floats(o.chunks) + 3) // 4 * 4, F32)
    _lib.check_train(lib.gcd_optim_gradstat(o.table.data_ptr(), len(SIZES), o.chunks, ctypes.byref(cfg), state.data_ptr(),
                                            scratch.data_ptr(), scratch.numel(), _stream()), "gcd_optim_gradstat")
    _also_state(ctx, state, _F + ("ema_omd",), _I)

    def ref():
        total = sum(float((o.g0[i].double() * 0.5).pow(2).sum()) for i in range(len(SIZES)) if i != 3)
        norm = math.sqrt(total) / 8.0
        clip = min(1.0, 2.0 / (norm + 1e-6))
        floats = [1e-3, 16.0, norm, clip, 0.5 / 8.0 * clip, 1 - 0.9 ** 5, math.sqrt(1 - 0.999 ** 5), 1 - min(0.99, 8 / 17)]
        out = {"state_floats": (torch.tensor(floats, dtype=torch.float64).reshape(1, -1), 1e-6),
               "state_ints": (torch.tensor([5, 0, 0, 1, 7], dtype=torch.float64).reshape(1, -1), EXACT)}
        out.update({f"p{i}": (o.p0[i].reshape(1, -1), EXACT) for i in range(len(SIZES))})      # pass 1 writes no tensor
        return out
    return ctx.ref(ref)


@case("gradstat/overflow-skips", ["gcd_optim_gradstat"])
def _gradstat_overflow(ctx):
    _lib, lib = _lt()
    o = Operands(ctx, 2, with_ema=False, with_mv=False, bad=(5, 16384, math.inf))
    cfg = _config(dynamic_scale=1)
    state = ctx.out_flat("state", (16,), I32, init=_state_words(ctx.poisoned, step=4, lr=1e-3, loss_scale=8.0,
                                                                growth_tracker=2, skipped_total=1, ema_num_updates=-1,
                                                                ema_omd=0.0))      # (no EMA: ema_omd is not written)
    scratch = ctx.scratch((o.chunks + 3) // 4 * 4, F32)
    _lib.check_train(lib.gcd_optim_gradstat(o.table.data_ptr(), len(SIZES), o.chunks, ctypes.byref(cfg), state.data_ptr(),
                                            scratch.data_ptr(), scratch.numel(), _stream()), "gcd_optim_gradstat")
    _also_state(ctx, state, ("lr", "loss_scale", "clip_coef", "gfactor", "bc1"), _I)

    def ref():
        out = {"state_floats": (torch.tensor([1e-3, 4.0, 0.0, 0.0, 1 - 0.9 ** 4], dtype=torch.float64).reshape(1, -1), 1e-6),
               "state_ints": (torch.tensor([4, 0, 1, 2, -1], dtype=torch.float64).reshape(1, -1), EXACT)}
        out.update({f"p{i}": (o.p0[i].reshape(1, -1), EXACT) for i in range(len(SIZES))})
        return out
    return ctx.ref(ref)


@case("advance", ["gcd_optim_advance"])
def _advance(ctx):
    _lib, lib = _lt()
    cfg = _config(grad_scale=0.25, use_ema=1, ema_decay=0.5)
    state = ctx.out_flat("state", (16,), I32, init=_state_words(ctx.poisoned, step=9, lr=2e-5, loss_scale=4.0,
                                                                ema_num_updates=20))
    _lib.check_train(lib.gcd_optim_advance(ctypes.byref(cfg), state.data_ptr(), _stream()), "gcd_optim_advance")
    _also_state(ctx, state, _F + ("ema_omd",), _I)
    return ctx.ref(lambda: {
        "state_floats": (torch.tensor([2e-5, 4.0, -1.0, 1.0, 0.25 / 4.0, 1 - 0.9 ** 10, math.sqrt(1 - 0.999 ** 10), 0.5],
                                      dtype=torch.float64).reshape(1, -1), 1e-6),
        "state_ints": (torch.tensor([10, 0, 0, 0, 21], dtype=torch.float64).reshape(1, -1), EXACT)})


def _apply_case(ctx, seed, cfg, *, found_inf=0, null_g=()):
    """gcd_optim_apply only READS the state block: it is a guarded input here, and an output nobody may change."""
    _lib, lib = _lt()
    o = Operands(ctx, seed, null_g=null_g)
    lr, step, gf, omd = 1e-2, 3, 0.125, 0.25
    words = _state_words(False, step=step, lr=lr, found_inf=found_inf, gfactor=gf, bc1=1 - cfg.beta1 ** step,
                         bc2_sqrt=math.sqrt(1 - cfg.beta2 ** step), ema_omd=omd, clip_coef=1.0)
    state = ctx.out_flat("state", (16,), I32, init=words)
    _lib.check_train(lib.gcd_optim_apply(o.table.data_ptr(), len(SIZES), o.chunks, ctypes.byref(cfg), state.data_ptr(),
                                         _stream()), "gcd_optim_apply")
    ctx.also("state_ints", state.double())

    def ref():
        out = _adam_ref(o, cfg, lr, step, gf, skipped=bool(found_inf), omd=omd if cfg.use_ema else None)
        if not cfg.use_ema:
            out.update({f"ema{i}": (o.e0[i].reshape(1, -1), EXACT) for i in range(len(SIZES))})
        out["state_ints"] = (words.double().reshape(1, -1), EXACT)
        return out
    return ctx.ref(ref)


@case("apply/adam-l2-ema", ["gcd_optim_apply"])
def _apply_adam(ctx):
    return _apply_case(ctx, 3, _config(weight_decay=0.01, use_ema=1), null_g=(1,))


@case("apply/adamw-no-ema", ["gcd_optim_apply"])
def _apply_adamw(ctx):
    return _apply_case(ctx, 4, _config(weight_decay=0.01, decoupled=1))


@case("apply/skipped-step-changes-no-payload-element", ["gcd_optim_apply"])
def _apply_skipped(ctx):
    """found_inf = 1: "every payload element is written" does not apply — no element of p, m, v changes (references =
    the initial values, exact); the EMA still moves."""
    return _apply_case(ctx, 5, _config(weight_decay=0.01, use_ema=1), found_inf=1)


@case("ema_update/num-updates-in-the-callers-counter", ["gcd_ema_update"])
def _ema_update(ctx):
    _lib, lib = _lt()
    o = Operands(ctx, 6, with_g=False, with_mv=False)
    count = ctx.out_flat("count", (4,), I32, init=torch.tensor([2, 0, 0, 0], dtype=I32))
    cfg = _config(use_ema=1, ema_decay=0.9999, ema_count=count.data_ptr())
    state = ctx.out_flat("state", (16,), I32, init=_state_words(
        ctx.poisoned, step=1, lr=1.0, ema_num_updates=77,      # (the optimizer's own fields are not written here)
        found_inf=0, grad_norm=0.0, clip_coef=0.0, gfactor=0.0, bc1=0.0, bc2_sqrt=0.0))
    _lib.check_train(lib.gcd_ema_update(o.table.data_ptr(), len(SIZES), o.chunks, ctypes.byref(cfg), state.data_ptr(),
                                        _stream()), "gcd_ema_update")
    ctx.also("state_ints", state[8:9].double())

    def ref():
        omd = 1.0 - 4.0 / 13.0
        out = {f"p{i}": (o.p0[i].reshape(1, -1), EXACT) for i in range(len(SIZES))}
        out.update({f"ema{i}": ((o.e0[i].double() - omd * (o.e0[i].double() - o.p0[i].double())).reshape(1, -1), 1e-6)
                    for i in range(len(SIZES))})
        out["count"] = (torch.tensor([3, 0, 0, 0], dtype=torch.float64).reshape(1, -1), EXACT)
        out["state_ints"] = (torch.tensor([3.0], dtype=torch.float64).reshape(1, -1), EXACT)
        return out
    return ctx.ref(ref)


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_contract(gpu, c):
    mc.run_contract(c, gpu)


def test_every_kernel_launching_export_has_a_case():
    from gcd_amd import _lib
    launching = {n for n in _lib.TRAIN_OPTIM_SIGNATURES if not n.endswith("_scratch_floats")}
    covered = {e for c in CASES for e in c.entries}
    assert launching == covered, launching ^ covered
    assert all(not c.atomic for c in CASES), "no bit-equality waiver: there are no read-modify-write reductions here"


def test_the_harness_sees_a_write_on_a_skipped_step(gpu):
    """Sensitivity of the skipped-step rule: the same case with found_inf = 0 does change p, so its 'initial values'
    references fail."""
    c = mc.Case("apply/not-skipped-against-skipped-references", ["gcd_optim_apply"],
                _apply_case_forced, no_ref=("state",))
    with pytest.raises(mc.MemContractError):
        mc.run_contract(c, gpu)


def _apply_case_forced(ctx):
    refs = _apply_case(ctx, 5, _config(weight_decay=0.01, use_ema=1), found_inf=0)
    if not refs:
        return refs
    g = _gen(5)                             # the skipped step's references: the initial values
    p0 = [torch.randn(n, generator=g) for n in SIZES]
    for i in range(len(SIZES)):
        refs[f"p{i}"] = (p0[i].reshape(1, -1), EXACT)
    return refs
