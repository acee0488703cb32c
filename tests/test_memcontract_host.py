"""The memory-contract harness (tests/memcontract.py) must itself fail on a subtly wrong kernel: run_contract over
three deliberately wrong torch stand-ins for a kernel (a store one row past the payload, an unwritten last row, a pad
column summed into the result), each reported with the right (row, column), and over a correct one on strided views.
Plain torch on the CPU: no GPU is touched and nothing is provoked."""
import re

import pytest
import torch

import memcontract as mc

R, C = 37, 24


def _case(kernel, name):
    """y[R, C] = 2 x + 1 with x, y fp32 strided views; `kernel(xv, yv)` is the stand-in for a launch."""
    def run(ctx):
        x = torch.randn(R, C, generator=torch.Generator().manual_seed(5))
        xv = ctx.inp(x, name="x")
        yv = ctx.out("y", R, C, torch.float32)
        assert xv.stride(0) == C + 4 and yv.stride(0) == C + 4 and not yv.is_contiguous()
        kernel(xv, yv)
        return ctx.ref(lambda: {"y": (2 * x.double() + 1, 1e-6)})
    return mc.Case(name, ["standin"], run)


def _full(v, extra_rows=0, extra_cols=0):
    """The stand-in's out-of-payload access: the same storage with more rows / columns, still inside the arena."""
    return v.as_strided((v.shape[0] + extra_rows, v.shape[1] + extra_cols), v.stride(), v.storage_offset())


def k_correct(x, y):
    y.copy_(2 * x + 1)


def k_row_after(x, y):
    y.copy_(2 * x + 1)
    _full(y, extra_rows=1)[R, 3] = 7.0


def k_last_row_unwritten(x, y):
    y[:R - 1].copy_(2 * x[:R - 1] + 1)


def k_reads_pad_column(x, y):
    y.copy_(2 * x + 1)
    y[:, 5] += 0.0 * _full(x, extra_cols=1)[:, C]          # 0 * pad: nothing with zeros there, NaN with NaN there


def test_correct_standin_on_strided_views_passes():
    fig = mc.run_contract(_case(k_correct, "correct"), "cpu")
    assert fig["y"] < 1e-6


@pytest.mark.parametrize("kernel,row,col,what", [
    (k_row_after, R, 3, "write outside"),
    (k_last_row_unwritten, R - 1, 0, "NaN in the payload"),
    (k_reads_pad_column, 0, 5, "NaN in the payload"),
], ids=["store_one_row_past_payload", "last_row_unwritten", "pad_column_in_result"])
def test_wrong_standins_are_reported_with_row_and_column(kernel, row, col, what):
    with pytest.raises(mc.MemContractError) as ei:
        mc.run_contract(_case(kernel, kernel.__name__), "cpu")
    msg = str(ei.value)
    assert what in msg, msg
    m = re.search(r"\(row (-?\d+), col (\d+)\)", msg)
    assert m and (int(m.group(1)), int(m.group(2))) == (row, col), msg


def test_output_that_keeps_its_old_value_is_not_bit_identical():
    """Rule 2 for an output that accumulates where it should store: caught by bit comparison even when no NaN survives
    (the stand-in adds into an output whose poisoned run starts from NaN, the clean one from zero)."""
    def k(x, y):
        y.copy_(torch.nan_to_num(y, nan=3.0) * 0 + torch.where(torch.isnan(y), 1.0, 0.0) + 2 * x + 1)
    with pytest.raises(mc.MemContractError, match=r"not bit-identical.*\(row 0, col 0\)"):
        mc.run_contract(_case(k, "depends_on_old_output"), "cpu")


def test_arena_layout_patterns_and_overhang():
    for dt in (torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.uint8):
        a = mc.Arena(5, 16, dt, "cpu")
        assert a.ld == 16 + mc.min_pad(dt) and a.ld % mc.min_pad(dt) == 0 and a.g >= 512
        assert a.view.shape == (5, 16) and a.view.stride() == (a.ld, 1)
        if dt != torch.uint8:
            assert bool(torch.isnan(a.buf).all())          # guards, pads and the fresh payload: NaN in every format
        a.set(1)
        a.assert_untouched()
        c = a.buf.clone()                                   # the pattern survives a torch copy and an integer view
        assert torch.equal(mc._ints(c), mc._ints(a.buf))
        a._grid()[a.g - 1, 2] = 0
        with pytest.raises(mc.MemContractError, match=r"\(row -1, col 2\).*front guard"):
            a.assert_untouched()
    # sensitivity device: the kernel's view is one row and one column larger than the payload the harness believes in
    a = mc.Arena(5, 16, torch.float32, "cpu", overhang=(1, 1))
    assert a.view.shape == (6, 17)
    a.view.fill_(1.0)
    with pytest.raises(mc.MemContractError, match=r"\(row 0, col 16\).*pad column"):
        a.assert_untouched()
    f = mc.Arena.flat(10, torch.float32, "cpu", last=10)
    assert f.g * 10 >= 512 * 10 and f.shaped(2, 5).is_contiguous()
    f.shaped(10).fill_(2.0)
    f.assert_untouched()


def test_atomic_spread_rule_and_expected_error():
    calls = []

    def k(x, y):                                            # "atomics": a run-to-run wobble of ~1e-7
        calls.append(1)
        y.copy_((2 * x + 1) * (1 + 1e-7 * (len(calls) % 2)))
    c = _case(k, "wobble")
    c.atomic = ("y",)
    fig = mc.run_contract(c, "cpu")
    assert len(calls) == 3 and fig["y:b-a"] <= max(10 * fig["y:spread"], 1e-6)

    def refuses(x, y):
        raise ValueError("ld != cols")
    c = _case(refuses, "refuses")
    c.expect_error = ValueError
    assert mc.run_contract(c, "cpu") == {}
    c = _case(k_correct, "accepts")
    c.expect_error = ValueError
    with pytest.raises(mc.MemContractError, match="expected ValueError"):
        mc.run_contract(c, "cpu")


def test_record_empty_restores_torch_and_poisons():
    e0, l0, n0 = torch.empty, torch.empty_like, torch.Tensor.new_empty
    with mc.record_empty(poison=True) as rec:
        t = torch.empty(7, dtype=torch.float32)
        u = torch.empty_like(t)
        v = t.new_empty((3, 2))
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == (e0, l0, n0)
    assert rec.sizes == [(7, torch.float32), (7, torch.float32), (6, torch.float32)]
    assert all(bool(torch.isnan(w).all()) for w in (t, u, v))


# ------------------------------------------------------------------------------------------------ coverage of the tables
_NO_KERNEL = {"tune_set"}                       # gcd_tune_set: a host-side knob, launches nothing


def _table_entries():
    import test_memcontract_gpu as fwd
    import test_memcontract_train_gpu as bwd
    names = set()
    for c in fwd.CASES + bwd.CASES:
        names.update(c.entries)
    return names, fwd.CASES + bwd.CASES


def test_every_kernel_wrapper_and_training_export_has_a_contract_case():
    """A new entry point without a contract case fails here: every public function of gcd_amd/ops.py that calls into the
    library (`check(...)` in its body) and every `int gcd_*(` export of include/gcd_amd_train.h (all of them launch
    kernels) must be named by at least one case of the two tables."""
    import ast
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    covered, cases = _table_entries()
    tree = ast.parse((root / "gcd_amd" / "ops.py").read_text())
    wrappers = [f.name for f in tree.body if isinstance(f, ast.FunctionDef) and not f.name.startswith("_")
                and any(isinstance(n, ast.Call) and getattr(n.func, "id", "") == "check" for n in ast.walk(f))]
    assert len(wrappers) >= 25, wrappers
    missing = [w for w in wrappers if w not in covered and w not in _NO_KERNEL]
    assert not missing, f"ops.py wrappers without a memory-contract case: {missing}"
    header = (root / "include" / "gcd_amd_train.h").read_text()
    exports = re.findall(r"^int (gcd_\w+)\(", header, flags=re.M)
    exports = [e for e in exports if e != "gcd_train_abi_version"]
    assert len(exports) >= 10, exports
    missing = [e for e in exports if e not in covered]
    assert not missing, f"gcd_amd_train.h exports without a memory-contract case: {missing}"
    ids = [c.id for c in cases]
    assert len(ids) == len(set(ids)), "duplicate case ids"
    for c in cases:                                                   # none may be left out of the bit-equality rule
        assert isinstance(c.atomic, tuple) and all(isinstance(n, str) for n in c.atomic) and c.expect_error is None
    # bit equality is waived per OUTPUT, and only in cases built on the five atomicAdd reductions
    waived = {c.id.split("[")[0].split("_")[0] for c in cases if c.atomic}
    assert waived <= {"cast16", "ln", "blend", "smallm", "A.linear", "A.conv3x3", "A.conv", "A.layer", "A.Fused"}, waived
