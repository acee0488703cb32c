"""The memory contract of the ParallelDomain colours (include/gcd_amd_pardom.h; tests/memcontract.py; DESIGN.md "Memory
contract").

gcd_pardom_colours is called directly with guarded operands: the ids and the stored colours are guarded strided inputs
(rows of 1 and of 3 bytes, padded), the palette a guarded flat input, `out` a strided view (rows of 3 doubles, padded to 5)
inside a guarded allocation and `status` a guarded counter: zeros in run (a), NaN bytes in run (b), every payload element
must be written and no guard touched.  The only atomic is an integer one: run (b) is bit-identical to run (a).  The cloud
is the golden's, twice over (1 360 points: two workgroups, the second one ragged); values: the colours the reference built
(tools/make_golden_render_pardom.py), which the kernel must equal.
"""
import re
from pathlib import Path

import pytest
import torch

import memcontract as mc

pytestmark = pytest.mark.gpu
F64, I64 = torch.float64, torch.int64
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "render_pardom_tiny.pt"
EXACT = 1e-15            # run_contract wants error < bar; the error of equal values is 0
CASES = []
_GOLD = None


def gold():
    global _GOLD
    if _GOLD is None:
        _GOLD = torch.load(GOLDEN, map_location="cpu", weights_only=False)
    return _GOLD


def _colours(ctx, case, t, mode, alpha):
    from gcd_amd import _lib_pardom
    lib = _lib_pardom.load()
    g = gold()
    c = next(c for c in g["cases"] if c["name"] == case)
    pcl = g["clouds"][c["cloud"]]
    ids_h, rgb_h = pcl["segm"][t].reshape(-1, 1).repeat(2, 1), pcl["rgb"][t].reshape(-1, 3).repeat(2, 1)
    N = ids_h.shape[0]
    ids = ctx.inp(ids_h, name="ids")
    rgb = ctx.inp(rgb_h, name="rgb")
    palette = ctx.inp_flat(g["palette"], name="palette")
    out = ctx.out("out", N, 3, F64)
    status = ctx.out_flat("status", (1,), I64)
    assert ids.stride(0) > 1 and rgb.stride(0) > 3 and out.stride(0) == 5 and N > 1024
    _lib_pardom.check(lib.gcd_pardom_colours(
        ids.data_ptr(), ids.stride(0), rgb.data_ptr(), rgb.stride(0), N, palette.data_ptr(), g["n_classes"], alpha, mode,
        out.data_ptr(), out.stride(0), status.data_ptr(), torch.cuda.current_stream().cuda_stream), "gcd_pardom_colours")
    return ctx.ref(lambda: {"out": (c["frames"][t]["colours"].repeat(2, 1), EXACT), "status": (torch.zeros(1, 1, dtype=F64), EXACT)})


CASES.append(mc.Case("pardom_colours_blend_third", ("gcd_pardom_colours",), lambda ctx: _colours(ctx, "segm_m3", 1, 1, 1.0 / 3.0)))
CASES.append(mc.Case("pardom_colours_blend_two_thirds", ("gcd_pardom_colours",), lambda ctx: _colours(ctx, "segm_m3", 2, 1, 2.0 / 3.0)))
CASES.append(mc.Case("pardom_colours_palette", ("gcd_pardom_colours",), lambda ctx: _colours(ctx, "segm_m0", 1, 2, 1.0)))
CASES.append(mc.Case("pardom_colours_rgb", ("gcd_pardom_colours",), lambda ctx: _colours(ctx, "segm_m3", 0, 0, 0.0)))


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_pardom_memory_contract(gpu, c):
    assert not c.atomic, "an integer atomic only: run (b) is bit-identical to run (a)"
    mc.run_contract(c, gpu)


def test_every_kernel_entry_of_the_pardom_header_has_a_contract_case():
    from gcd_amd import _lib_pardom
    header = (ROOT / "include" / "gcd_amd_pardom.h").read_text()
    exports = set(re.findall(r"^\s*(?:int|int64_t)\s+(gcd_\w+)\s*\(", header, flags=re.M))
    kernels = exports - {"gcd_pardom_abi_version"}
    covered = {e for c in CASES for e in c.entries}
    assert kernels == {"gcd_pardom_colours"} and kernels <= covered
    assert (_lib_pardom.PARDOM_RGB, _lib_pardom.PARDOM_BLEND, _lib_pardom.PARDOM_PALETTE) == (0, 1, 2)      # the modes of CASES
