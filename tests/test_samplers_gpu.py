"""GPU: the sampler family on the fused stage loop — gcd_sampler_stage_f32 against fp64 on every kind of table row, its
unused operands untouched and unread, and Heun / Euler with churn / Euler ancestral / DPM++ 2S ancestral / DPM++ 2M
through the plugin stack (generic, fused eager, fused graph, closure route) against the reference's goldens
(tools/make_golden_samplers.py).

Bars.  Kernel: |out - ref| <= 16 * 2^-24 * S + 2^-126 with S the sum of the absolute values of every product entering
the output (one rounding per product and per add, fewer than 16 operations deep), ref in fp64 on the float32 row and
operands the kernel reads.  Loop: the golden's bars[case] = 1.5 * TOL_LOOP * max(1, sens[case] / sens["euler"]): the
project's bar for plain Euler on this very loop (test_unet_gpu.py::test_sampler_vs_reference_golden), scaled by how much
more the sampler amplifies fp16 operand rounding than Euler does, measured on the reference alone.
"""
import pytest
import torch

from conftest import rel_l2
from oracle import svd_unet_ref as O, weights
import sampler_cases as sc

pytestmark = pytest.mark.gpu
F32 = torch.float32
POISON = 0x7FC5A5A5
ROWS = sc.row_kinds()
GRID_CAP_ELEMS = 4096 * 256 * 4          # blocks x threads x floats per thread of the vector path


# ------------------------------------------------------------------------------------------------------------- the kernel
def _operands(nx, chw, seed, device, misalign=False):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
    ops = dict(cur=r(nx, chw) * 3.0 + 0.5, net=r(2 * nx, chw), h0=r(nx, chw) * 2.0, h1=r(nx, chw), noise=r(nx, chw))
    ops = {k: v.to(device) for k, v in ops.items()}
    if misalign:                                         # every base 4 bytes past a 16-byte boundary
        for k, v in ops.items():
            buf = torch.empty(v.numel() + 1, device=device, dtype=F32)
            buf[1:].copy_(v.reshape(-1))
            ops[k] = buf[1:].view(v.shape)
            assert ops[k].data_ptr() % 16 == 4
    return ops


def _reference(row, o, scale, T):
    """fp64 on the float32 row and operands: {name: (value, S)} for cur and for each buffer the row stores."""
    r = row.double()
    d = {k: v.double() for k, v in o.items()}
    nx = d["cur"].shape[0]
    sigma = r[0]
    s2 = sigma * sigma + 1.0
    c_skip, c_out = 1.0 / s2, -sigma / s2.sqrt()
    sc_ = scale.double()[torch.arange(nx, device=scale.device) % T].reshape(nx, 1)
    pu, pc, qx = d["net"][:nx] * c_out, d["net"][nx:] * c_out, d["cur"] * c_skip
    du, dc = pu + qx, pc + qx
    D = du + sc_ * (dc - du)
    S_D = pu.abs() + qx.abs() + sc_.abs() * (pc.abs() + pu.abs() + 2.0 * qx.abs())
    zero = torch.zeros_like(d["cur"])

    def comb(terms):
        val, S = zero.clone(), zero.clone()
        for coef, t, St in terms:
            if float(coef) != 0.0:                       # a term that is switched off is not read: it may hold NaN
                val, S = val + coef * t, S + coef.abs() * St
        return val, S

    out = {"cur": comb([(r[1], d["cur"], d["cur"].abs()), (r[2], D, S_D), (r[3], d["h0"], d["h0"].abs()),
                        (r[4], d["h1"], d["h1"].abs()), (r[5], d["noise"], d["noise"].abs())])}
    if float(r[6]) != 0.0 or float(r[7]) != 0.0:
        out["h0"] = comb([(r[6], d["cur"], d["cur"].abs()), (r[7], D, S_D)])
    if float(r[8]) != 0.0 or float(r[9]) != 0.0:
        out["h1"] = comb([(r[8], d["cur"], d["cur"].abs()), (r[9], D, S_D)])
    return out


def _launch(row, o, scale, T):
    from gcd_amd import sampler_ops
    coef = row.to(o["cur"].device)
    sampler_ops.sampler_stage(o["cur"], o["net"], scale, coef, T, o["h0"], o["h1"], o["noise"])
    torch.cuda.synchronize()


def _check_against_fp64(name, row, nx, chw, T, gpu, misalign=False):
    o = _operands(nx, chw, 11, gpu, misalign)
    scale = torch.linspace(1.0, 1.5, T, device=gpu)
    ref = _reference(row.to(gpu), o, scale, T)
    before = {k: v.clone() for k, v in o.items()}
    _launch(row, o, scale, T)
    for k in ("cur", "h0", "h1"):
        if k in ref:
            val, S = ref[k]
            err = (o[k].double() - val).abs()
            bound = 16.0 * 2.0 ** -24 * S + 2.0 ** -126
            worst = float((err / bound).max())
            print(f"{name} nx={nx} chw={chw} misalign={misalign}: {k} worst error / bound {worst:.3f}")
            assert bool((err <= bound).all()), f"{name}: {k} off by up to {worst:.2f} x the bound"
        else:
            assert torch.equal(o[k], before[k]), f"{name}: {k} written although its store pair is (0, 0)"
    assert torch.equal(o["net"], before["net"]) and torch.equal(o["noise"], before["noise"])


@pytest.mark.parametrize("name", list(ROWS))
def test_stage_kernel_vs_fp64_on_every_row_kind(gpu, name):
    """Two clips of T = 3 frames (n % T matters): the vector path (chw = 36), the scalar path (chw = 15) and the vector
    shape through bases 4 bytes off alignment (scalar path); `cur` is updated in place."""
    for chw, misalign in [(36, False), (15, False), (36, True)]:
        _check_against_fp64(name, ROWS[name], 6, chw, 3, gpu, misalign)


def test_stage_kernel_stride_loop_runs_twice(gpu):
    """nx * chw just above the grid cap (4096 blocks) x 256 threads x 4 elements: the last 8 elements belong to the
    second trip of the stride loop."""
    nx, chw = 6, GRID_CAP_ELEMS // 6 + 4 - (GRID_CAP_ELEMS // 6) % 4
    assert chw % 4 == 0 and GRID_CAP_ELEMS < nx * chw <= GRID_CAP_ELEMS + 4 * nx
    _check_against_fp64("all_terms", ROWS["all_terms"], nx, chw, 3, gpu)


@pytest.mark.parametrize("name", list(ROWS))
def test_stage_kernel_leaves_unused_operands_untouched_and_unread(gpu, name):
    """Each row kind twice: zeros, then a NaN bit pattern, in every buffer the row gives a zero coefficient.  The outputs
    are bit-equal, and a buffer whose store pair is (0, 0) still holds its pattern."""
    row, T = ROWS[name], 3
    need_net = any(float(row[i]) != 0.0 for i in (2, 7, 9))
    reads = {"h0": float(row[3]) != 0.0, "h1": float(row[4]) != 0.0, "noise": float(row[5]) != 0.0, "net": need_net}
    stores = {"h0": float(row[6]) != 0.0 or float(row[7]) != 0.0, "h1": float(row[8]) != 0.0 or float(row[9]) != 0.0,
              "noise": False, "net": False}
    for chw in (36, 15):
        results = []
        for pattern in (0, POISON):
            o = _operands(6, chw, 13, gpu)
            for k, read in reads.items():
                if not read:
                    o[k].view(torch.int32).fill_(pattern)
            _launch(row, o, torch.linspace(1.0, 1.5, T, device=gpu), T)
            for k in reads:
                if not reads[k] and not stores[k]:
                    assert bool((o[k].view(torch.int32) == pattern).all()), f"{name}: {k} was written"
            results.append([o["cur"]] + [o[k] for k in ("h0", "h1") if stores[k]])
        for a, b in zip(*results):
            assert not bool(torch.isnan(b).any()), f"{name}: NaN from an operand whose coefficient is zero"
            assert torch.equal(a, b), name


def test_stage_kernel_accepts_null_optional_operands(gpu):
    """h0, h1 and noise may be null when the row does not use them (plain Euler row)."""
    from gcd_amd import sampler_ops
    row = ROWS["euler_stage0"]
    assert not bool((row[3:10] != 0).any())
    o = _operands(6, 36, 17, gpu)
    scale = torch.linspace(1.0, 1.5, 3, device=gpu)
    ref, _ = _reference(row.to(gpu), o, scale, 3)["cur"]
    full = o["cur"].clone()
    sampler_ops.sampler_stage(full, o["net"], scale, row.to(gpu), 3, o["h0"], o["h1"], o["noise"])
    sampler_ops.sampler_stage(o["cur"], o["net"], scale, row.to(gpu), 3)
    torch.cuda.synchronize()
    assert torch.equal(full, o["cur"]) and rel_l2(o["cur"], ref) < 1e-6


# ------------------------------------------------------------------------------------------------------- the plugin stack
def _build(cfg, gpu):
    from gcd_amd.video_model import VideoUNet
    with torch.device("meta"):
        net = VideoUNet(**cfg.as_reference_kwargs())
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net = net.to_empty(device=gpu)
    net.load_state_dict(weights.synth_state_dict(shapes))
    return net.eval()


@pytest.fixture(scope="module")
def tiny(gpu):
    return _build(O.TINY, gpu)


def _stack(net, T, gpu, clips=1):
    from gcd_amd.denoiser import Denoiser
    from gcd_amd.sampling import FusedDenoiser
    from gcd_amd.wrappers import OpenAIWrapper
    den = Denoiser({"target": "gcd_amd.denoiser_scaling.VScalingWithEDMcNoise"})
    model = OpenAIWrapper(net)
    extra = {"num_video_frames": T, "image_only_indicator": torch.zeros(2 * clips, T, device=gpu)}
    return den, model, extra, FusedDenoiser(den, model, **extra)


def _inputs(g, gpu, clips=1, seed=None):
    noise, c, uc = weights.synth_inputs(clips, g["T"], g["h"], g["w"], O.TINY.context_dim,
                                        O.TINY.adm_in_channels + O.TINY.aux_emb_dim, g["input_seed"] if seed is None else seed)
    return noise, {k: v.to(gpu) for k, v in c.items()}, {k: v.to(gpu) for k, v in uc.items()}


def _run(sampler, denoiser, noise, c, uc, gpu, drawn=None, use_graph=True):
    replay = sc.Replay(drawn) if drawn is not None else None
    if drawn is not None:
        sampler.noise_sampler = replay if drawn or hasattr(sampler, "eta") else None
    sampler.use_graph = use_graph
    out = sampler(denoiser, noise.clone().to(gpu), cond=c, uc=uc)
    torch.cuda.synchronize()
    assert replay is None or replay.left == 0, "the path drew fewer noise tensors than the reference"
    return out


@pytest.mark.parametrize("name", sc.CASES)
def test_sampler_family_vs_reference_golden(gpu, tiny, name):
    from gcd_amd import sampling
    g = sc.golden()
    case, bar = g["cases"][name], g["bars"][name]
    T = g["T"]
    noise, c, uc = _inputs(g, gpu)
    den, model, extra, fused = _stack(tiny, T, gpu)
    sampler = sc.make_sampler(g["specs"][name], g["steps"], "cuda")
    assert sampler._fused_loop_class() is sampling.FusedStageLoop

    def closure(inp, sigma, cc):           # what DiffusionEngine.sample_video builds
        return den(model, inp, sigma, cc, **extra)

    class Opaque:                          # a callable the sampler cannot see into: generic path
        def __call__(self, inp, sigma, cc):
            return den(model, inp, sigma, cc, **extra)

    out_generic = _run(sampler, Opaque(), noise, c, uc, gpu, case["noise"])
    assert sampler.last_path == "generic"
    out_closure = _run(sampler, closure, noise, c, uc, gpu, case["noise"])
    assert sampler.last_path == "fused", "the sample_video-style closure must reach the fused loop"
    out_eager = _run(sampler, fused, noise, c, uc, gpu, case["noise"], use_graph=False)
    assert sampler.last_path == "fused"
    out_graph = _run(sampler, fused, noise, c, uc, gpu, case["noise"])
    assert sampler.last_path == "fused"
    for kind, o in [("generic", out_generic), ("fused eager", out_eager), ("fused graph", out_graph)]:
        e = rel_l2(o, case["final"])
        print(f"{name} {kind}: rel-L2 vs reference golden {e:.3e} (bar {bar:.3e})")
    e_fg = rel_l2(out_eager, out_generic)
    print(f"{name} fused vs generic: rel-L2 {e_fg:.3e} (bar {bar:.3e})")
    for kind, o in [("generic", out_generic), ("fused eager", out_eager), ("fused graph", out_graph)]:
        assert rel_l2(o, case["final"]) < bar, f"{name} {kind}: {rel_l2(o, case['final']):.3e}"
    assert torch.equal(out_eager, out_graph), "hipGraph replay differs from eager launches"
    assert torch.equal(out_closure, out_graph), "closure-recovered fused path differs from FusedDenoiser"
    assert e_fg < bar


@pytest.mark.parametrize("name", ["heun", "dpmpp2m"])
def test_two_clips_equal_their_single_clip_results(gpu, tiny, name):
    g = sc.golden()
    T, bar = g["T"], g["bars"][name]
    noise, c, uc = _inputs(g, gpu, clips=2, seed=29)
    sampler = sc.make_sampler(g["specs"][name], g["steps"], "cuda")
    joint = _run(sampler, _stack(tiny, T, gpu, clips=2)[3], noise, c, uc, gpu)
    assert sampler.last_path == "fused" and joint.shape[0] == 2 * T
    for b in range(2):
        sl = slice(b * T, (b + 1) * T)
        single = _run(sampler, _stack(tiny, T, gpu)[3], noise[sl], {k: v[sl] for k, v in c.items()},
                      {k: v[sl] for k, v in uc.items()}, gpu)
        e = rel_l2(joint[sl], single)
        print(f"{name} clip {b}: joint vs single rel-L2 {e:.3e} (bar {bar:.3e})")
        assert sampler.last_path == "fused" and e < bar


def test_fused_and_generic_paths_consume_the_same_random_stream(gpu, tiny):
    """noise_sampler = None: torch.randn_like on both paths, so one seed gives one trajectory."""
    g = sc.golden()
    T, bar = g["T"], g["bars"]["euler_ancestral"]
    noise, c, uc = _inputs(g, gpu)
    den, model, extra, fused = _stack(tiny, T, gpu)
    sampler = sc.make_sampler(g["specs"]["euler_ancestral"], g["steps"], "cuda")
    sampler.noise_sampler = None
    torch.manual_seed(77)
    out_fused = _run(sampler, fused, noise, c, uc, gpu)
    assert sampler.last_path == "fused"
    torch.manual_seed(77)
    class Opaque:                          # a callable the sampler cannot see into: generic path
        def __call__(self, inp, sigma, cc):
            return den(model, inp, sigma, cc, **extra)

    out_generic = _run(sampler, Opaque(), noise, c, uc, gpu)
    assert sampler.last_path == "generic"
    torch.manual_seed(78)
    out_other = _run(sampler, fused, noise, c, uc, gpu)
    e = rel_l2(out_fused, out_generic)
    print(f"euler_ancestral, seeded: fused vs generic rel-L2 {e:.3e} (bar {bar:.3e}); other seed "
          f"{rel_l2(out_other, out_generic):.3e}")
    assert e < bar and rel_l2(out_other, out_generic) > 10 * bar


def test_second_call_on_the_same_sampler_recaptures_its_graph(gpu, tiny):
    g = sc.golden()
    T = g["T"]
    noise, c, uc = _inputs(g, gpu)
    fused = _stack(tiny, T, gpu)[3]
    sampler = sc.make_sampler(g["specs"]["dpmpp2m"], g["steps"], "cuda")
    first = _run(sampler, fused, noise, c, uc, gpu)
    second = _run(sampler, fused, noise, c, uc, gpu)
    assert sampler.last_path == "fused" and torch.equal(first, second)
    assert rel_l2(second, g["cases"]["dpmpp2m"]["final"]) < g["bars"]["dpmpp2m"]
