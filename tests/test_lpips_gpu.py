"""GPU: the LPIPS metric on HIP (gcd_amd/lpips.py, libgcd_amd_lpips.so) and the validation metrics built on it.

Per kernel: the packing against the same fp32 chain in torch rounded to fp16 (equal), ReLU / max-pool bit-equal to torch
on the same fp16 input, the distance against float64 on given fp16 features (lpips_util.DISTANCE_BAR).  End to end: the
three golden cases of the executed reference (tests/golden/lpips_tiny.pt) against its float64 output; the bar of a case is
4 x the recorded error of the reference-side fp16-storage emulation (lpips_util.case_bar), never a figure of the code under
test.  Measured on the MI355X (largest relative error of the non-identical pairs against y64; the emulation's; bar):
  tiny_40x56  8.28e-5   4.22e-5   1.69e-4
  tiny_37x51  2.00e-4   3.12e-4   1.25e-3
  full_64x96  4.80e-5   5.19e-5   2.08e-4
pairs_at_a_time=1 gave bit-identical values in all three.  
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_util as U

pytestmark = pytest.mark.gpu
F16, F32, F64 = torch.float16, torch.float32, torch.float64
CASES = ("tiny_40x56", "tiny_37x51", "full_64x96")
_MODELS = {}


def _model(gpu, name):
    if name not in _MODELS:
        rec, sd, _, _ = U.golden_case(name)
        _MODELS[name] = U.gpu_model(rec["chns"], sd, gpu)
    return _MODELS[name]


def _bits(t):
    return t.cpu().contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------------------ per kernel
@pytest.mark.parametrize("ab", [(1.0, 0.0), (2.0, -1.0)], ids=["signed", "unit"])
def test_pack_equals_the_fp32_chain_rounded_once(gpu, ab):
    from gcd_amd import lpips as L
    n, H, W, cpad = 2, 37, 51, 64
    g = torch.Generator().manual_seed(11)
    x = torch.rand(n, 3, H, W, generator=g)
    x = x if ab == (2.0, -1.0) else x * 2 - 1
    shift, scale = torch.tensor(U.SHIFT), torch.tensor(U.SCALE)
    out = torch.full((n * H * W, cpad), float("nan"), dtype=F16, device=gpu)
    L.pack(x.to(gpu), out, ab, shift.to(gpu), scale.to(gpu))
    t = x * ab[0]                                   # one fp32 operation per line: nothing to fuse
    t = t + ab[1]
    t = t - shift.view(1, 3, 1, 1)
    t = t / scale.view(1, 3, 1, 1)
    want = torch.zeros(n * H * W, cpad, dtype=F16)
    want[:, :3] = t.permute(0, 2, 3, 1).reshape(-1, 3).half()
    assert torch.equal(_bits(out), _bits(want))
    assert bool((out[:, 3:] == 0).all())


@pytest.mark.parametrize("C", [32, 512])
@pytest.mark.parametrize("H,W", [(5, 7), (6, 8)])
def test_relu_pool_is_bit_equal_to_torch(gpu, C, H, W):
    from gcd_amd import lpips as L
    n = 2
    g = torch.Generator().manual_seed(C + H)
    src = (2.0 * torch.randn(n * H * W, C, generator=g)).half()
    nchw = src.float().reshape(n, H, W, C).permute(0, 3, 1, 2)
    want_full = torch.relu(src.float()).half()
    want_pool = F.max_pool2d(torch.relu(nchw), 2, 2).permute(0, 2, 3, 1).reshape(-1, C).half()
    assert bool((src < 0).any()) and want_pool.shape[0] == n * (H // 2) * (W // 2)
    s = src.to(gpu)
    nan = lambda rows: torch.full((rows, C), float("nan"), dtype=F16, device=gpu)
    full, pooled = nan(n * H * W), nan(want_pool.shape[0])
    L.relu_pool(s, full, pooled, n, H, W)
    assert torch.equal(_bits(full), _bits(want_full)) and torch.equal(_bits(pooled), _bits(want_pool))
    full2, pooled2 = nan(n * H * W), nan(want_pool.shape[0])
    L.relu_pool(s, full2, None, n, H, W)            # either destination may be null
    L.relu_pool(s, None, pooled2, n, H, W)
    assert torch.equal(_bits(full2), _bits(want_full)) and torch.equal(_bits(pooled2), _bits(want_pool))
    assert torch.equal(_bits(s), _bits(src))
    pooled3 = nan(want_pool.shape[0])
    L.relu_pool(s, s, pooled3, n, H, W)             # in place, as the tower runs it
    assert torch.equal(_bits(s), _bits(want_full)) and torch.equal(_bits(pooled3), _bits(want_pool))


def _distance(gpu, f0, f1, w, n, HW, blocks=None):
    from gcd_amd import lpips as L
    tm = torch.full((1, n), float("nan"), dtype=F64, device=gpu)
    out = torch.full((n,), float("nan"), dtype=F32, device=gpu)
    L.distance(f0.to(gpu), f1.to(gpu), w.to(gpu), n, HW, tm, 0, 1, out, blocks=blocks)
    return tm.cpu()[0], out.cpu()


@pytest.mark.parametrize("C,HW,blocks", [(64, 203, None), (64, 203, 3), (512, 77, None), (512, 77, 5), (96, 45, None)],
                         ids=["C64", "C64_3blocks", "C512", "C512_5blocks", "C96"])
def test_distance_against_float64(gpu, C, HW, blocks):
    n = 3
    f0, f1, w = U.seeded_features(n, HW, C, 1000 + C)
    f0[5] = 0                                       # a dead pixel on one side
    f0[9] = 0                                       # ... and on both
    f1[9] = 0
    f1[2 * HW:] = f0[2 * HW:]                       # image 2: identical tensors
    want = U.distance_ref(f0, f1, w, n, HW)
    tm, out = _distance(gpu, f0, f1, w, n, HW, blocks)
    tm2, out2 = _distance(gpu, f0, f1, w, n, HW, blocks)
    assert torch.equal(tm.view(torch.int64), tm2.view(torch.int64)) and torch.equal(out.view(torch.int32), out2.view(torch.int32))
    assert float(tm[2]) == 0.0 == float(out[2]) and float(want[2]) == 0.0
    err = float(((tm[:2] - want[:2]).abs() / want[:2]).max())
    print(f"distance C={C} HW={HW} blocks={blocks}: rel err of the tap mean vs float64 {err:.3e} (bar {U.DISTANCE_BAR:.1e})")
    assert torch.equal(out, tm.float())             # one tap: out is its mean rounded to fp32
    assert err <= U.DISTANCE_BAR


def test_distance_of_all_zero_features_is_exactly_zero_and_taps_add_in_order(gpu):
    from gcd_amd import lpips as L
    n, HW, C = 2, 10, 64
    z = torch.zeros(n * HW, C, dtype=F16, device=gpu)
    f0, f1, w = U.seeded_features(n, HW, C, 5)
    tm = torch.tensor([[0.25, 0.5], [float("nan")] * 2, [1e-9, 2.0]], dtype=F64, device=gpu)
    out = torch.full((n,), float("nan"), dtype=F32, device=gpu)
    L.distance(z, z, w.to(gpu), n, HW, tm, 1, 3, out)
    assert tm.cpu().tolist() == [[0.25, 0.5], [0.0, 0.0], [1e-9, 2.0]]
    assert out.cpu().tolist() == torch.tensor([0.25 + 1e-9, 2.5], dtype=F64).float().tolist()
    L.distance(f0.to(gpu), z, w.to(gpu), n, HW, tm, 1, 3, None)          # unit rows against zero rows: sum_c n0^2 w
    want = U.distance_ref(f0, torch.zeros_like(f0), w, n, HW)
    assert float(((tm.cpu()[1] - want).abs() / want).max()) <= U.DISTANCE_BAR


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("name", CASES)
def test_golden_cases_against_the_reference_float64(gpu, name):
    rec, sd, x0, x1 = U.golden_case(name)
    m, bar = _model(gpu, name), U.case_bar(rec)
    y = m(x0.to(gpu), x1.to(gpu))
    assert y.shape == (rec["n"], 1, 1, 1) and y.dtype == F32 and y.device.type == "cuda"
    y, y64 = y.cpu().double().reshape(-1), rec["y64"].reshape(-1)
    err = float(((y[1:] - y64[1:]).abs() / y64[1:]).max())
    emu = float(((rec["y16emu"].reshape(-1)[1:] - y64[1:]).abs() / y64[1:]).max())
    print(f"{name}: GPU vs y64 {err:.3e}; reference-side fp16 emulation vs y64 {emu:.3e}; bar {bar:.3e}")
    assert float(y[0]) == 0.0, "an identical pair scores exactly 0"
    y1 = m(x0.to(gpu), x1.to(gpu), pairs_at_a_time=1).cpu().double().reshape(-1)
    gap = float(((y1[1:] - y[1:]).abs() / y64[1:]).max())
    print(f"{name}: pairs_at_a_time=1 vs the default {gap:.3e}")
    assert float(y1[0]) == 0.0
    assert torch.equal(m(x0.to(gpu), x1.to(gpu)).cpu().double().reshape(-1), y), "two calls must be bit-identical"
    assert err <= bar, (err, bar)
    assert gap <= bar, (gap, bar)


def test_unit_range_and_repacking_when_a_parameter_moves(gpu):
    name = "tiny_40x56"
    rec, sd, x0, x1 = U.golden_case(name)
    m, bar = U.gpu_model(rec["chns"], sd, gpu), U.case_bar(rec)
    y64 = rec["y64"].reshape(-1)
    u0, u1 = ((x0 + 1) / 2).to(gpu), ((x1 + 1) / 2).to(gpu)
    yu = m(u0, u1, value_range="unit").cpu().double().reshape(-1)
    # (x + 1) / 2 * 2 - 1 is x up to an ulp of fp32: far inside the fp16 rounding the bar is made of
    assert float(yu[0]) == 0.0 and float(((yu[1:] - y64[1:]).abs() / y64[1:]).max()) <= bar
    packs = m._packs
    assert m(x0.to(gpu), x1.to(gpu)) is not None and m._packs is packs          # cached
    with torch.no_grad():
        m.lin0.model[1].weight.mul_(2.0)
    y2 = m(x0.to(gpu), x1.to(gpu)).cpu().double().reshape(-1)
    assert m._packs is not packs
    sd2 = dict(sd)
    sd2["lin0.model.1.weight"] = sd["lin0.model.1.weight"] * 2.0
    want = U.lpips_oracle(sd2, x0, x1).reshape(-1)
    assert float(((y2[1:] - want[1:]).abs() / want[1:]).max()) <= bar


def test_operands_the_tower_cannot_take_raise_and_a_later_call_works(gpu):
    from gcd_amd._lib import GcdError
    name = "tiny_40x56"
    rec, sd, x0, x1 = U.golden_case(name)
    m = _model(gpu, name)
    a, b = x0.to(gpu), x1.to(gpu)
    for bad in ((a.double(), b.double()), (a, b[:, :, :-1]), (a[:, :, :15].contiguous(), b[:, :, :15].contiguous()),
                (a, b.cpu()), (a[:, :, :, ::2], b[:, :, :, ::2]), (a[:, :2], b[:, :2])):
        with pytest.raises(GcdError):
            m(*bad)
    with pytest.raises(GcdError):
        U.gpu_model(rec["chns"], sd, "cpu")(a, b)          # parameters left on the CPU
    assert float(m(a, b).reshape(-1)[0]) == 0.0


def test_validation_metrics_against_the_host_metrics_and_the_oracle(gpu):
    """A seeded 4-frame clip at 40 x 56: PSNR / SSIM against gcd_amd.metrics on float64 copies at the tolerances of
    test_metrics_device_gpu.py (1e-9 relative / absolute), LPIPS against the float64 oracle within 4 x the error of the
    oracle's own fp16-storage emulation on this clip."""
    from gcd_amd import metrics as M
    from gcd_amd.validation import validation_metrics
    rec, sd, _, _ = U.golden_case("tiny_40x56")
    x0, x1 = U.seeded_images(5, 40, 56, 77)
    gt, pred = ((x0[1:] + 1) / 2).contiguous(), ((x1[1:] + 1) / 2).contiguous()          # [0, 1]; no identical frame
    md = validation_metrics(gt.to(gpu), pred.to(gpu), _model(gpu, "tiny_40x56"))
    assert sorted(md) == ["lpips", "psnr", "ssim"] and all(type(v) is float for v in md.values())
    host, _ = M.calculate_metrics(gt.numpy().astype(np.float64), None, [{"sampled_rgb": pred.numpy().astype(np.float64)}])
    psnr, ssim = float(np.mean(host["frame_psnr"])), float(np.mean(host["frame_ssim"]))
    s0, s1 = gt * 2.0 - 1.0, pred * 2.0 - 1.0                # the fp32 values the packing kernel forms
    y64 = U.lpips_oracle(sd, s0, s1).reshape(-1)
    emu = U.lpips_oracle(sd, s0, s1, round16=True).reshape(-1)
    bar = 4.0 * float(((emu - y64).abs() / y64).max())
    err = abs(md["lpips"] - float(y64.mean())) / float(y64.mean())
    print(f"validation: lpips {md['lpips']:.6f} (oracle {float(y64.mean()):.6f}, rel {err:.3e}, bar {bar:.3e}), "
          f"psnr rel {abs(md['psnr'] - psnr) / psnr:.3e}, ssim abs {abs(md['ssim'] - ssim):.3e}")
    assert abs(md["psnr"] - psnr) <= 1e-9 * psnr and abs(md["ssim"] - ssim) <= 1e-9
    assert err <= bar
