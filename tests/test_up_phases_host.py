"""The phase form of the x2 up-convolution, host side: `packing.pack_conv3x3_up_phases` against its definition, and the
code generation of the kernel instantiation that runs it (no GPU needed: hipcc cross-compiles).

out[2i+py, 2j+px] = b + sum_{a,c in {0,1}} Wp[2py+px][a][c] . x[i+py-1+a, j+px-1+c]  must be
F.conv2d(F.interpolate(x, 2, "nearest"), w, b, padding=1): the four folded taps are sums of the nine, formed in fp32 and
rounded to fp16 ONCE, so the phase form is held to the error the nine individually rounded taps make against the same
fp32-weight truth (x 1.1: two rounding errors of equal size scatter by under 1 % from case to case), not to them.
"""
import math
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2


def phase_conv(x, wp, b):
    """The four 2 x 2 phase convolutions on the low-res x [n, Cin, Hi, Wi] with packed weights wp [4, Cout, 4 Cin]
    (K order (a, c, cin)), scattered to (py::2, px::2); computed in x's dtype."""
    n, cin, hi, wi = x.shape
    cout = wp.shape[1]
    xp = F.pad(x, (1, 1, 1, 1))
    out = x.new_empty(n, cout, 2 * hi, 2 * wi)
    for py in range(2):
        for px in range(2):
            k = wp[2 * py + px].to(x.dtype).reshape(cout, 2, 2, cin).permute(0, 3, 1, 2)
            out[:, :, py::2, px::2] = F.conv2d(xp[:, :, py:py + hi + 1, px:px + wi + 1], k, b)
    return out


def up_conv(x, w, b):
    return F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b, padding=1)


@pytest.mark.parametrize("n,cin,h,w_", [(2, 64, 5, 8), (2, 320, 9, 16), (1, 640, 6, 8)])
def test_pack_up_phases_matches_the_definition(n, cin, h, w_):
    from gcd_amd import packing
    g = torch.Generator().manual_seed(100 + cin)
    cout = 48
    x = torch.randn(n, cin, h, w_, generator=g).half().double()
    w = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)          # the fp32 parameter, unrounded
    b = torch.randn(cout, generator=g).double()
    wp = packing.pack_conv3x3_up_phases(w)
    assert wp.dtype == torch.float16 and tuple(wp.shape) == (4, cout, 4 * cin) and wp.is_contiguous()
    truth = up_conv(x, w.double(), b)
    e_nine = rel_l2(up_conv(x, w.half().double(), b), truth)
    e_phase = rel_l2(phase_conv(x, wp, b), truth)
    print(f"{n}x{cin}x{h}x{w_}: nine rounded taps {e_nine:.3e}, phase form {e_phase:.3e}")
    assert 1e-5 < e_nine < 1e-3
    assert e_phase <= 1.1 * e_nine, f"phase form {e_phase:.3e} vs nine rounded taps {e_nine:.3e}"


def test_pack_up_phases_is_exact_on_small_integers():
    """No sum rounds: every tap set and every border must agree to the bit."""
    from gcd_amd import packing
    g = torch.Generator().manual_seed(7)
    for (n, cin, cout, h, w_) in [(2, 64, 16, 5, 8), (1, 128, 32, 1, 1), (1, 64, 16, 2, 3)]:
        x = torch.randint(-3, 4, (n, cin, h, w_), generator=g).double()
        w = torch.randint(-4, 5, (cout, cin, 3, 3), generator=g).float()
        b = torch.randint(-8, 9, (cout,), generator=g).double()
        wp = packing.pack_conv3x3_up_phases(w)
        assert torch.equal(phase_conv(x, wp, b), up_conv(x, w.double(), b))


def test_up_phase_kernels_compile_without_scratch():
    """gemm_p8.hip's phase-form instantiations (MODE 4, with and without column sums) hold 160 accumulator registers and
    the eight scalar row bases of the scattered epilogue: no scratch, two waves per SIMD (a spill reload waits vmcnt(0) and
    drains the K loop's DMA pipeline).  From hipcc's own resource remarks."""
    from gcd_amd.csrc import build as B
    src = "gemm_p8.hip"
    assert src in B.SOURCES
    pr = subprocess.run([B._hipcc(), *B.FLAGS, *B.EXTRA_FLAGS.get(src, []), "--cuda-device-only", "-S",
                         "-Rpass-analysis=kernel-resource-usage", str(B.CSRC / src), "-o", "/dev/null"],
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert pr.returncode == 0, pr.stdout[-2000:]
    found, cur = {}, None
    for line in pr.stdout.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = found.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs Spill): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    up = {k: v for k, v in found.items() if "gemm_p8_kernelILi4E" in k}
    assert len(up) == 2, sorted(found)
    for name, r in up.items():
        print(name, r)
        assert r["ScratchSize"] == 0 and r["VGPRs"] == 0 and r["Occupancy"] == 2, f"{name}: {r}"
