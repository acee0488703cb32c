"""The memory contract of the sampler-stage kernel (include/gcd_amd_sampler.h; tests/memcontract.py; DESIGN.md "Memory
contract").

gcd_sampler_stage_f32 is called directly with guarded operands for every kind of row its table builder emits.  Per row,
an optional buffer plays one of four parts: read and stored (in place, starts from a value in both runs), stored only
(an output: zeros in run (a), NaN in run (b), every element must be written), read only (a guarded input), or neither —
then it is handed over as scratch (zeros, then NaN) and must not reach any result.  `cur` is always in place.  No case
uses the run-to-run spread rule: run (b) is bit-identical to run (a).  Values: fp64 torch at rel-L2 1e-6.
"""
import re
from pathlib import Path

import pytest
import torch

import memcontract as mc
import sampler_cases as sc

pytestmark = pytest.mark.gpu
F32 = torch.float32
ROOT = Path(__file__).resolve().parent.parent
ROWS = sc.row_kinds()
CASES = []
NX, T = 6, 3


def _case(ctx, row, chw):
    from gcd_amd import _lib
    g = torch.Generator().manual_seed(23)
    r = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
    val = dict(cur=r(NX, chw) * 3.0 + 0.5, net=r(2 * NX, chw), h0=r(NX, chw) * 2.0, h1=r(NX, chw), noise=r(NX, chw))
    scale = torch.linspace(1.0, 1.5, T)
    need_net = any(float(row[i]) != 0.0 for i in (2, 7, 9))
    reads = {"h0": float(row[3]) != 0.0, "h1": float(row[4]) != 0.0, "noise": float(row[5]) != 0.0, "net": need_net}
    stores = {"h0": float(row[6]) != 0.0 or float(row[7]) != 0.0, "h1": float(row[8]) != 0.0 or float(row[9]) != 0.0}
    dev = {"cur": ctx.out_flat("cur", (NX, chw), F32, init=val["cur"])}
    for k in ("net", "h0", "h1", "noise"):
        shape = val[k].shape
        if stores.get(k):
            dev[k] = ctx.out_flat(k, shape, F32, init=val[k] if reads[k] else None)
        elif reads[k]:
            dev[k] = ctx.inp_flat(val[k], name=k)
        else:
            dev[k] = ctx.scratch(val[k].numel(), F32, name=k).view(shape)
    coef, sc_dev = ctx.inp_flat(row.clone(), name="coef"), ctx.inp_flat(scale, name="scale")
    lib = _lib.load_sampler()
    _lib.check_sampler(lib.gcd_sampler_stage_f32(
        dev["cur"].data_ptr(), dev["net"].data_ptr(), sc_dev.data_ptr(), coef.data_ptr(), dev["h0"].data_ptr(),
        dev["h1"].data_ptr(), dev["noise"].data_ptr(), NX, T, chw, torch.cuda.current_stream().cuda_stream),
        "gcd_sampler_stage_f32")

    def ref():
        d = {k: v.double() for k, v in val.items()}
        rr = row.double()
        s2 = rr[0] * rr[0] + 1.0
        c_skip, c_out = 1.0 / s2, -rr[0] / s2.sqrt()
        s = scale.double()[torch.arange(NX) % T].reshape(NX, 1)
        du, dc = d["net"][:NX] * c_out + d["cur"] * c_skip, d["net"][NX:] * c_out + d["cur"] * c_skip
        D = du + s * (dc - du)
        new = torch.zeros_like(d["cur"])
        for coef_, t in ((rr[1], d["cur"]), (rr[2], D), (rr[3], d["h0"]), (rr[4], d["h1"]), (rr[5], d["noise"])):
            if float(coef_) != 0.0:
                new = new + coef_ * t
        out = {"cur": (new.reshape(1, -1), 1e-6)}
        if stores["h0"]:
            out["h0"] = ((rr[6] * d["cur"] + rr[7] * D).reshape(1, -1), 1e-6)
        if stores["h1"]:
            out["h1"] = ((rr[8] * d["cur"] + rr[9] * D).reshape(1, -1), 1e-6)
        return out
    return ctx.ref(ref)


for _name, _row in ROWS.items():
    for _chw in (36, 15):          # the 16-byte path and the scalar path
        CASES.append(mc.Case(f"sampler_stage_{_name}_chw{_chw}", ("gcd_sampler_stage_f32",),
                             lambda ctx, _row=_row, _chw=_chw: _case(ctx, _row, _chw)))


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_sampler_stage_memory_contract(gpu, c):
    assert not c.atomic, "no spread rule here: run (b) is bit-identical to run (a)"
    mc.run_contract(c, gpu)


def test_every_kernel_entry_of_the_sampler_header_has_a_contract_case():
    header = (ROOT / "include" / "gcd_amd_sampler.h").read_text()
    exports = set(re.findall(r"^\s*(?:int|int64_t)\s+(gcd_\w+)\s*\(", header, flags=re.M)) - {"gcd_sampler_abi_version"}
    covered = {e for c in CASES for e in c.entries}
    assert exports == {"gcd_sampler_stage_f32"} and exports <= covered
