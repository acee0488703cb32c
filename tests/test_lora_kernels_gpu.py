"""GPU: the two grouped kernels of libgcd_amd_lora.so (include/gcd_amd_lora.h) against fp64 torch on the CPU, with every
operand inside a guarded, poisoned arena (tests/memcontract.py): writes stay inside the payloads, every payload element is
written, nothing outside an input's payload and nothing of the un-initialised scratch reaches a result.

The bar is derived, not measured.  An n-term fp32 sum, in any order, of terms that are formed exactly (fma) is within
    gamma * sum |terms|,   gamma = (n + 2) u / (1 - (n + 2) u),   u = 2^-24
of the exact value (n roundings of the sum at most, one for the scale, one to spare); it is checked ELEMENTWISE against
sum |terms| in fp64.  n = r + 1 for the merge (the r products and W0), K for dB, N for dA."""
import ctypes as C

import pytest
import torch

from memcontract import POISON, Arena

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# the smallest shapes that cross every boundary: one element; ragged in both tiles; several row and column tiles of both
# kernels (64 and 256); the largest rank with many column regions; many row regions — and, beyond that list, an odd K
# (rows that are not 16-byte aligned: the scalar loads and stores) with a rank that is no multiple of 4 above 16
SHAPES = [(1, 1, 1), (70, 100, 3), (300, 700, 16), (64, 2048, 64), (2048, 64, 16), (129, 259, 17)]
_CACHE = {}


def gamma(n: int) -> float:
    return (n + 2) * U / (1.0 - (n + 2) * U)


def _operands(N, K, r):
    """Seeded fp32 operands on the CPU with their fp64 references and elementwise bounds; made once per shape."""
    key = (N, K, r)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(1000 * N + 10 * K + r)
        W0 = torch.randn(N, K, generator=g)
        A = (torch.rand(r, K, generator=g) * 2 - 1) / K ** 0.5
        B = torch.randn(N, r, generator=g) * 0.3
        dW = torch.randn(N, K, generator=g) * 0.01 + 0.003          # an offset: sums that do not cancel to nothing
        s = 1.0 / 16 if r == 16 else 0.37
        s32 = float(torch.tensor(s, dtype=torch.float32))           # the scale as the kernel sees it
        W0d, Ad, Bd, dWd = W0.double(), A.double(), B.double(), dW.double()
        ref = dict(W=W0d + s32 * (Bd @ Ad), dB=s32 * (dWd @ Ad.T), dA=s32 * (Bd.T @ dWd))
        mag = dict(W=W0d.abs() + s32 * (Bd.abs() @ Ad.abs()), dB=s32 * (dWd.abs() @ Ad.abs().T), dA=s32 * (Bd.abs().T @ dWd.abs()))
        _CACHE[key] = dict(W0=W0, A=A, B=B, dW=dW, s=s, ref=ref, mag=mag, n=dict(W=r + 1, dB=K, dA=N))
    return _CACHE[key]


class Layer:
    """One entry's operands in arenas on the device."""

    def __init__(self, gpu, N, K, r, *, null_dw=False, zero_b=False):
        from gcd_amd import _lib_lora
        self.N, self.K, self.r, self.null_dw, self.zero_b = N, K, r, null_dw, zero_b
        self.op = _operands(N, K, r)
        self.ins = {}
        for name, shape in (("W0", (N, K)), ("A", (r, K)), ("B", (N, r)), ("dW", (N, K))):
            a = Arena.flat(shape[0] * shape[1], torch.float32, gpu, name=name, last=shape[1])
            v = self.op[name]
            a.set(torch.zeros_like(v) if (name == "B" and zero_b) else v)
            self.ins[name] = a
        self.outs = {name: Arena.flat(shape[0] * shape[1], torch.float32, gpu, name=name, last=shape[1]).set("poison")
                     for name, shape in (("W", (N, K)), ("dA", (r, K)), ("dB", (N, r)))}
        e = _lib_lora.LoraEntry()
        ptr = lambda a: a.payload.data_ptr()      # noqa: E731
        e.W0, e.A, e.B = ptr(self.ins["W0"]), ptr(self.ins["A"]), ptr(self.ins["B"])
        e.dW = None if null_dw else ptr(self.ins["dW"])
        e.W, e.dA, e.dB = ptr(self.outs["W"]), ptr(self.outs["dA"]), ptr(self.outs["dB"])
        e.N, e.K, e.r, e.scale = N, K, r, self.op["s"]
        self.entry = e

    def result(self, name):
        shape = {"W": (self.N, self.K), "dA": (self.r, self.K), "dB": (self.N, self.r)}[name]
        return self.outs[name].shaped(*shape).cpu()

    def check_memory(self, names):
        for a in self.ins.values():
            a.assert_untouched()
        for n in ("W", "dA", "dB"):
            self.outs[n].assert_untouched()
            got = self.outs[n].payload.view(torch.int32)
            if n in names:
                assert not bool((got == POISON[torch.float32]).any()), f"{n}: a payload element was not written"
                assert bool(torch.isfinite(self.outs[n].payload).all()), f"{n}: a guard or scratch value reached the result"
            else:
                assert bool((got == POISON[torch.float32]).all()), f"{n}: written by a call that does not own it"

    def check_values(self, names):
        for n in names:
            got = self.result(n).double()
            if n in ("dA", "dB") and self.null_dw:
                assert bool((got == 0).all()) and not bool(torch.signbit(got).any()), f"{n}: zeros for an entry without dW"
                continue
            if n == "W" and self.zero_b:
                assert torch.equal(self.result(n).view(torch.int32), self.op["W0"].view(torch.int32)), "B == 0: W is W0's bits"
                continue
            err = (got - self.op["ref"][n]).abs()
            bound = gamma(self.op["n"][n]) * self.op["mag"][n]
            worst = float((err / bound.clamp_min(1e-300)).max())
            print(f"({self.N}, {self.K}, {self.r}) {n}: worst |err| / bound = {worst:.3f}")
            assert bool((err <= bound).all()), (n, worst)


def _launch(gpu, layers, what, scratch_poison=True):
    from gcd_amd import _lib_lora
    arr = (_lib_lora.LoraEntry * len(layers))(*[l.entry for l in layers])
    mt, pt, sf = _lib_lora.fill_table(arr)
    tab = Arena.flat(C.sizeof(arr), torch.uint8, gpu, name="table")
    tab.set(torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8))
    lib, stream = _lib_lora.load(), torch.cuda.current_stream().cuda_stream
    scratch = None
    if what == "merge":
        _lib_lora.check(lib.gcd_lora_merge(tab.payload.data_ptr(), len(layers), mt, stream), "gcd_lora_merge")
    else:
        scratch = Arena.flat(sf, torch.float32, gpu, poison=scratch_poison, name="scratch")
        scratch.set("poison" if scratch_poison else 0.0)
        _lib_lora.check(lib.gcd_lora_project(tab.payload.data_ptr(), len(layers), pt, max(l.r for l in layers),
                                             scratch.payload.data_ptr(), sf, stream), "gcd_lora_project")
    torch.cuda.synchronize()
    tab.assert_untouched()
    if scratch is not None:
        scratch.assert_untouched()
    return scratch


@pytest.mark.parametrize("N,K,r", SHAPES)
def test_merge_and_project_one_layer(gpu, N, K, r):
    layer = Layer(gpu, N, K, r)
    _launch(gpu, [layer], "merge")
    layer.check_memory(["W"])
    _launch(gpu, [layer], "project")
    layer.check_memory(["W", "dA", "dB"])
    layer.check_values(["W", "dA", "dB"])


@pytest.mark.parametrize("order", [(2, 0, 4, 5, 1, 3), (1, 2, 0, 4)])
def test_grouped_launch_mixed_order_with_a_null_gradient(gpu, order):
    """All the shapes in one launch, not sorted by anything (ranks up to 64: the wide kernel; the second order holds ranks
    up to 16 only: the narrow one), one entry without dW in the middle."""
    layers = [Layer(gpu, *SHAPES[i]) for i in order]
    layers.insert(2, Layer(gpu, 70, 100, 3, null_dw=True))
    _launch(gpu, layers, "merge")
    _launch(gpu, layers, "project")
    for l in layers:
        l.check_memory(["W", "dA", "dB"])
        l.check_values(["W", "dA", "dB"])


def test_merge_with_zero_b_is_bitwise_w0(gpu):
    """Negative zeros and subnormals of W0 included; A is not zero."""
    layers = [Layer(gpu, 300, 700, 16, zero_b=True), Layer(gpu, 129, 259, 17, zero_b=True)]
    for l in layers:
        w0 = l.op["W0"].clone()
        w0.view(-1)[::7] = -0.0
        w0.view(-1)[3::11] = 1e-41
        l.ins["W0"].set(w0)
        l.op = dict(l.op, W0=w0)
    _launch(gpu, layers, "merge")
    for l in layers:
        l.check_memory(["W"])
        l.check_values(["W"])


def test_project_is_bit_reproducible(gpu):
    """Two calls, the second over a scratch that holds other bits: the same bits out."""
    layers = [Layer(gpu, 300, 700, 16), Layer(gpu, 2048, 64, 16), Layer(gpu, 64, 2048, 64)]
    _launch(gpu, layers, "project", scratch_poison=False)
    first = [(l.result("dA").clone(), l.result("dB").clone()) for l in layers]
    for l in layers:
        l.outs["dA"].set("poison")
        l.outs["dB"].set("poison")
    _launch(gpu, layers, "project", scratch_poison=True)
    for l, (da, db) in zip(layers, first):
        assert torch.equal(l.result("dA").view(torch.int32), da.view(torch.int32))
        assert torch.equal(l.result("dB").view(torch.int32), db.view(torch.int32))
        l.check_values(["dA", "dB"])


def test_entries_that_do_not_fit_are_skipped_not_followed(gpu):
    """A table that lies about its scratch (too short for the entry) makes the call a no-op for that entry: the outputs
    keep their bits and nothing outside any arena is written."""
    from gcd_amd import _lib_lora
    layer = Layer(gpu, 300, 700, 16)
    arr = (_lib_lora.LoraEntry * 1)(layer.entry)
    _, pt, sf = _lib_lora.fill_table(arr)
    tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(gpu)
    scratch = Arena.flat(sf // 2, torch.float32, gpu, name="scratch").set("poison")
    _lib_lora.check(_lib_lora.load().gcd_lora_project(tab.data_ptr(), 1, pt, 16, scratch.payload.data_ptr(), sf // 2,
                                                      torch.cuda.current_stream().cuda_stream), "gcd_lora_project")
    torch.cuda.synchronize()
    scratch.assert_untouched()
    assert bool((scratch.payload.view(torch.int32) == POISON[torch.float32]).all())
    layer.check_memory([])


def test_entry_above_the_stated_rank_is_skipped_by_both_stages(gpu):
    """max_rank below an entry's r (10 for r = 16, 16 for r = 17): neither stage touches that entry — no partial sum in
    the scratch, dA and dB keep their bits — while the other entry of the table is computed."""
    for big, small, stated in (((300, 700, 16), (70, 100, 3), 10), ((129, 259, 17), (300, 700, 16), 16)):
        from gcd_amd import _lib_lora
        skipped, done = Layer(gpu, *big), Layer(gpu, *small)
        arr = (_lib_lora.LoraEntry * 2)(skipped.entry, done.entry)
        _, pt, sf = _lib_lora.fill_table(arr)
        tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(gpu)
        scratch = Arena.flat(sf, torch.float32, gpu, name="scratch").set("poison")
        _lib_lora.check(_lib_lora.load().gcd_lora_project(tab.data_ptr(), 2, pt, stated, scratch.payload.data_ptr(), sf,
                                                          torch.cuda.current_stream().cuda_stream), "gcd_lora_project")
        torch.cuda.synchronize()
        scratch.assert_untouched()
        own = int(arr[1].scratch0)
        assert bool((scratch.payload.view(torch.int32)[0, :own] == POISON[torch.float32]).all())
        skipped.check_memory([])
        done.check_memory(["dA", "dB"])
        done.check_values(["dA", "dB"])
