"""Memory-contract harness for the kernel tests (a helper module like gloo_util.py, not a conftest).

A kernel's operands are handed to it as views into larger allocations laid out as

    front guard | payload rows, each followed by pad columns up to the row stride | back guard

and the entry point is held to five rules ("Memory contract"):

  1. writes stay inside the output's [rows, cols] payload;
  2. every payload element is written, whatever the output held before;
  3. nothing outside an input's payload reaches the result;
  4. scratch is written before it is read;
  5. the value is right against the entry's usual high-precision reference at its usual bar.

`run_contract(case)` runs the entry twice: (a) zeros in every guard / pad / scratch byte and a zero-filled output,
(b) a NaN bit pattern in all of them and a NaN-filled output, and requires the guards unchanged in both, no NaN in
any payload, (a) within the bar of the reference and (b) bit-identical to (a).  The kernels that reduce with fp32
atomicAdd are not bit-reproducible from run to run; for the outputs they write (`Case.atomic` names them, and only
them) run (a) is repeated, the run-to-run spread is measured and printed, and (b) must lie within
max(10 * spread, 1e-6) of (a) (rel-L2).  Every output needs a reference unless the case lists it in `no_ref`.

Everything here is plain torch and works on CPU tensors too (tests/test_memcontract_host.py runs it over wrong
torch stand-ins for a kernel).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

# One recognisable quiet-NaN bit pattern per dtype (payload bits survive torch copies and integer views).
_INT_VIEW = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32,
             torch.float64: torch.int64, torch.uint8: torch.uint8, torch.int32: torch.int32, torch.int64: torch.int64}
POISON = {torch.float16: 0x7E5A, torch.bfloat16: 0x7FDA, torch.float32: 0x7FC5A5A5,
          torch.float64: 0x7FF8A5A5A5A5A5A5, torch.uint8: 0xA5, torch.int32: 0x7FC5A5A5,
          torch.int64: 0x7FF8A5A5A5A5A5A5}
GUARD_ROWS = 512          # twice the tallest tile in the tree (256 rows): a whole overhanging tile stays inside


class MemContractError(AssertionError):
    """A rule of the memory contract is broken; the message names the rule and the first offending (row, column)."""


def min_pad(dtype) -> int:
    """The smallest non-zero pad the entries' own alignment checks accept: rows stay 16-byte aligned."""
    return 16 // torch.empty(0, dtype=dtype).element_size()


def _ints(t: torch.Tensor) -> torch.Tensor:
    return t.view(_INT_VIEW[t.dtype])


def poison_scratch(t: torch.Tensor) -> torch.Tensor:
    """Fill a (contiguous) scratch buffer with the NaN pattern of its dtype."""
    _ints(t).fill_(POISON[t.dtype])
    return t


def _first(mask2d: torch.Tensor) -> Optional[Tuple[int, int]]:
    """(row, column) of the first True of a 2-D mask in row-major order, or None."""
    flat = mask2d.reshape(-1)
    if not bool(flat.any()):
        return None
    i = int(torch.nonzero(flat)[0, 0])
    return i // mask2d.shape[1], i % mask2d.shape[1]


class Arena:
    """One operand as a view [rows, cols] with row stride `ld` inside an allocation the test owns.

    `poison`: guards and pad columns hold the dtype's NaN pattern (True) or zeros (False).
    `overhang=(dr, dc)`: the view handed to the kernel is [rows + dr, cols + dc] while the harness keeps believing in
    [rows, cols] — for the sensitivity tests: a correct kernel then writes its legitimate last row / column into what the
    harness takes for guard, still inside the allocation."""

    def __init__(self, rows: int, cols: int, dtype, device, *, pad: Optional[int] = None, poison: bool = True,
                 guard_rows: int = GUARD_ROWS, overhang: Tuple[int, int] = (0, 0), name: str = "operand"):
        if pad is None:
            pad = min_pad(dtype)
        assert guard_rows >= GUARD_ROWS and pad >= 0 and overhang[0] < guard_rows and overhang[1] <= max(pad, 0)
        self.name, self.rows, self.cols, self.ld, self.g = name, rows, cols, cols + pad, guard_rows
        self.dtype, self.over = dtype, overhang
        self.pattern = POISON[dtype] if poison else 0
        self.buf = torch.empty((2 * guard_rows + rows) * self.ld, dtype=dtype, device=device)
        _ints(self.buf).fill_(self.pattern)

    @classmethod
    def flat(cls, numel: int, dtype, device, *, poison: bool = True, name: str = "operand", last: int = 0):
        """A contiguous operand of `numel` elements (1-D, NCHW, ...): front / back guards only, each 512 rows of the
        operand's innermost extent `last` and never less than 4096 elements."""
        a = cls.__new__(cls)
        g = -(-max(4096, GUARD_ROWS * max(last, 1)) // max(numel, 1))        # guard "rows" of numel elements
        a.name, a.rows, a.cols, a.ld, a.g, a.dtype, a.over = name, 1, numel, numel, g, dtype, (0, 0)
        a.pattern = POISON[dtype] if poison else 0
        a.buf = torch.empty((2 * g + 1) * numel, dtype=dtype, device=device)
        _ints(a.buf).fill_(a.pattern)
        return a

    # -- views -------------------------------------------------------------------------------------------------------
    def _grid(self) -> torch.Tensor:
        return self.buf.view(2 * self.g + self.rows, self.ld)

    @property
    def view(self) -> torch.Tensor:
        """What the kernel gets: [rows (+ overhang), cols (+ overhang)], row stride ld."""
        return self._grid()[self.g:self.g + self.rows + self.over[0], :self.cols + self.over[1]]

    def shaped(self, *shape) -> torch.Tensor:
        """The payload of a flat arena as a contiguous tensor of `shape`."""
        assert self.rows == 1 and self.ld == self.cols
        return self._grid()[self.g].view(*shape)

    @property
    def payload(self) -> torch.Tensor:
        return self._grid()[self.g:self.g + self.rows, :self.cols]

    def set(self, value) -> "Arena":
        """Payload := value (a tensor of the payload's shape or a scalar); 'poison' fills it with the NaN pattern."""
        if isinstance(value, str):
            assert value == "poison"
            _ints(self._grid())[self.g:self.g + self.rows, :self.cols] = POISON[self.dtype]
        elif torch.is_tensor(value):
            self.payload.copy_(value.reshape(self.rows, self.cols))
        else:
            self.payload.fill_(value)
        return self

    # -- rule 1 ------------------------------------------------------------------------------------------------------
    def assert_untouched(self, what: str = "") -> None:
        """Guards and pad columns, compared as integers with their initial pattern; reports the first changed element
        as (row, column) relative to the payload (row < 0: front guard, row >= rows: back guard, column >= cols: pad)."""
        changed = _ints(self._grid()) != self.pattern
        changed[self.g:self.g + self.rows, :self.cols] = False
        at = _first(changed)
        if at is not None:
            r, c = at[0] - self.g, at[1]
            where = "front guard" if r < 0 else "back guard" if r >= self.rows else "pad column"
            raise MemContractError(
                f"{what}{self.name}: write outside the [{self.rows}, {self.cols}] payload (ld {self.ld}): first changed "
                f"element at (row {r}, col {c}) in the {where}; {int(changed.sum())} elements changed")


@dataclass
class Case:
    """One row of a contract table.  `run(ctx)` builds its operands through `ctx`, launches the entry and returns
    {output name: (reference on the CPU, rel-L2 bar)}; the reference callable may be built lazily with `ctx.ref`."""
    id: str
    entries: Sequence[str]                     # the wrappers / exports this case covers (for the coverage check)
    run: Callable[["Ctx"], Dict[str, tuple]]
    atomic: Sequence[str] = ()                 # the OUTPUTS that an fp32 atomicAdd reduction writes: spread rule for (b)
    expect_error: Optional[type] = None        # a documented restriction: the entry must refuse these strides
    no_ref: Sequence[str] = ()                 # outputs checked between the runs only (every other one needs a reference)


class Ctx:
    """Operand factory of one run of a case."""

    def __init__(self, device, poisoned: bool, want_ref: bool):
        self.device, self.poisoned, self.want_ref = torch.device(device), poisoned, want_ref
        self.arenas: List[Arena] = []
        self.outs: Dict[str, Arena] = {}
        self.extra_outs: Dict[str, torch.Tensor] = {}

    def _new(self, rows, cols, dtype, pad, name, overhang=(0, 0)) -> Arena:
        a = Arena(rows, cols, dtype, self.device, pad=pad, poison=self.poisoned, name=name, overhang=overhang)
        self.arenas.append(a)
        return a

    def inp(self, value: torch.Tensor, *, pad: Optional[int] = None, name: str = "input", dtype=None) -> torch.Tensor:
        """A 2-D input [rows, cols] as a guarded strided view holding `value` (CPU tensor, converted to `dtype`)."""
        value = value if dtype is None else value.to(dtype)
        assert value.dim() == 2
        a = self._new(value.shape[0], value.shape[1], value.dtype, pad, name)
        a.set(value.to(self.device))
        return a.view

    def inp_flat(self, value: torch.Tensor, *, name: str = "input", dtype=None) -> torch.Tensor:
        """A contiguous input of any shape with front / back guards."""
        value = (value if dtype is None else value.to(dtype)).contiguous()
        a = Arena.flat(value.numel(), value.dtype, self.device, poison=self.poisoned, name=name,
                       last=value.shape[-1] if value.dim() else 1)
        self.arenas.append(a)
        a.set(value.reshape(1, -1).to(self.device))
        return a.shaped(*value.shape)

    def out(self, name: str, rows: int, cols: int, dtype, *, pad: Optional[int] = None, init=None,
            overhang=(0, 0)) -> torch.Tensor:
        """A 2-D output.  Without `init` it starts as zeros in run (a) and as NaN in run (b); with `init` (in-place
        and accumulate-into arguments) it starts from that value in both."""
        a = self._new(rows, cols, dtype, pad, name, overhang)
        self._init_out(a, init)
        self.outs[name] = a
        return a.view

    def out_flat(self, name: str, shape, dtype, *, init=None) -> torch.Tensor:
        numel = 1
        for s in shape:
            numel *= s
        a = Arena.flat(numel, dtype, self.device, poison=self.poisoned, name=name, last=shape[-1])
        self.arenas.append(a)
        self._init_out(a, init)
        self.outs[name] = a
        return a.shaped(*shape)

    def _init_out(self, a: Arena, init) -> None:
        if init is not None:
            a.set(init.to(self.device) if torch.is_tensor(init) else init)
        else:
            a.set("poison" if self.poisoned else 0)

    def scratch(self, numel: int, dtype, name: str = "scratch") -> torch.Tensor:
        """A guarded scratch buffer: zeros in run (a), NaN in run (b)."""
        a = Arena.flat(numel, dtype, self.device, poison=self.poisoned, name=name)
        self.arenas.append(a)
        a.set("poison" if self.poisoned else 0)
        return a.shaped(numel)

    def dirty(self, t: torch.Tensor) -> torch.Tensor:
        """A persistent scratch tensor the library owns: NaN-filled before run (b), zeroed before run (a)."""
        if self.poisoned:
            poison_scratch(t)
        else:
            t.zero_()
        return t

    def also(self, name: str, t: torch.Tensor) -> None:
        """An unguarded result (what an autograd function returned) to compare between the runs."""
        self.extra_outs[name] = t

    def ref(self, fn: Callable[[], Dict[str, tuple]]) -> Dict[str, tuple]:
        return fn() if self.want_ref else {}


def _rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _sync(device) -> None:
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def _one_run(case: Case, device, poisoned: bool, want_ref: bool):
    ctx = Ctx(device, poisoned, want_ref)
    refs = case.run(ctx) or {}
    _sync(device)
    tag = f"[{case.id}] run ({'b: poisoned' if poisoned else 'a: zeros'}) "
    for a in ctx.arenas:
        a.assert_untouched(tag)
    res = {k: a.payload.clone() for k, a in ctx.outs.items()}
    res.update({k: (t.detach().clone() if t.dim() == 2 else t.detach().reshape(1, -1).clone())
                for k, t in ctx.extra_outs.items()})
    return res, refs


def _nan_check(case: Case, name: str, t: torch.Tensor, which: str) -> None:
    if not t.dtype.is_floating_point:
        return
    at = _first(torch.isnan(t))
    if at is not None:
        raise MemContractError(
            f"[{case.id}] run ({which}) {name}: NaN in the payload at (row {at[0]}, col {at[1]}), "
            f"{int(torch.isnan(t).sum())} in all: an element was not written, or poison outside an operand's "
            "payload / in scratch reached the result")


def run_contract(case: Case, device) -> Dict[str, float]:
    """Hold one entry to the contract; returns the measured rel-L2 figures (printed too)."""
    if case.expect_error is not None:
        for poisoned in (False, True):
            try:
                _one_run(case, device, poisoned, False)
            except case.expect_error:
                continue
            raise MemContractError(f"[{case.id}] expected {case.expect_error.__name__}: the entry documents that it "
                                   "refuses these strides, and accepted them")
        return {}
    atomic = set(case.atomic)
    a, refs = _one_run(case, device, False, True)
    a2 = _one_run(case, device, False, False)[0] if atomic else None
    b, _ = _one_run(case, device, True, False)
    figures = {}
    assert atomic <= set(a) and set(case.no_ref) <= set(a), f"[{case.id}] atomic / no_ref name an unknown output"
    missing, unknown = set(a) - set(refs) - set(case.no_ref), set(refs) - set(a)
    assert not missing and not unknown, f"[{case.id}] outputs without a reference: {missing}; references without an output: {unknown}"
    for name in a:
        _nan_check(case, name, a[name], "a: zeros")
        _nan_check(case, name, b[name], "b: poisoned")
    for name in a:
        if name in atomic:
            spread = _rel_l2(a2[name], a[name])
            d = _rel_l2(b[name], a[name])
            bar = max(10.0 * spread, 1e-6)
            figures[name + ":spread"], figures[name + ":b-a"] = spread, d
            print(f"[{case.id}] {name}: run-to-run spread {spread:.3e}, poisoned vs clean {d:.3e} (bar {bar:.3e})")
            if not d <= bar:
                raise MemContractError(f"[{case.id}] {name}: poisoned run differs from the clean run by rel-L2 {d:.3e} "
                                       f"> max(10 * spread {spread:.3e}, 1e-6)")
        else:
            at = _first(_ints(a[name].contiguous()) != _ints(b[name].contiguous()))
            if at is not None:
                raise MemContractError(
                    f"[{case.id}] {name}: poisoned run is not bit-identical to the clean run: first difference at "
                    f"(row {at[0]}, col {at[1]}): {a[name][at].item()!r} vs {b[name][at].item()!r}: the result depends "
                    "on bytes outside the operands' payloads, on scratch, or on what the output held before")
    for name, (ref, bar) in refs.items():
        got = a[name].detach().cpu().double().reshape(ref.shape)
        if isinstance(bar, tuple):                 # ("maxabs", x): the entries whose own tests use a max-abs bar
            assert bar[0] == "maxabs"
            e, kind, bar = float((got - ref.double()).abs().max()), "max-abs", bar[1]
        else:
            e, kind = _rel_l2(got, ref), "rel-L2"
        figures[name] = e
        print(f"[{case.id}] {name}: {kind} vs reference {e:.3e} (bar {bar:.1e})")
        if not e < bar:
            raise MemContractError(f"[{case.id}] {name}: {kind} {e:.3e} vs the reference, bar {bar:.1e}")
    return figures


class record_empty:
    """The dirty allocator of the contract tests: with `poison=True` every `torch.empty` / `empty_like` / `new_empty`
    made inside the block is filled with 0xFF bytes (a NaN in every float format) as it is handed out, so a wrapper that
    allocates with torch.empty where its kernel needs zeros computes NaN.  This does not rest on how torch's caching
    allocator recycles blocks (poisoning freed blocks and waiting for the allocator to hand them back proved to
    depend on the allocator's state: free neighbours merge, other streams own free blocks); `sizes` records
    (numel, dtype) of what was handed out, and a test asserts that it is not empty, so the rule cannot pass vacuously."""

    def __init__(self, poison: bool = False):
        self.poison, self.sizes = poison, []

    def _wrap(self, fn):
        def wrapped(*a, **k):
            t = fn(*a, **k)
            if torch.is_tensor(t) and t.device.type != "meta" and t.dim() and t.numel() and t.is_contiguous():
                self.sizes.append((t.numel(), t.dtype))
                if self.poison and (t.dtype.is_floating_point or t.dtype == torch.uint8):
                    t.view(torch.uint8).fill_(0xFF)
            return t
        return wrapped

    def __enter__(self):
        self._saved = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
        torch.empty, torch.empty_like = self._wrap(torch.empty), self._wrap(torch.empty_like)
        torch.Tensor.new_empty = self._wrap(torch.Tensor.new_empty)
        return self

    def __exit__(self, *exc):
        torch.empty, torch.empty_like, torch.Tensor.new_empty = self._saved
        return False
