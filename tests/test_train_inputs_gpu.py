"""GPU: input gradients of the planned fine-tune engine (train_plan.set_input_grads / GCD_TRAIN_INPUT_GRADS /
unet_forward_planned(input_grads=True)): d y, d context and d x of the TINY network against the golden made by the
unmodified reference (tests/golden/train_inputs_tiny.pt, tools/make_golden_train_inputs.py) and against the operator-level
tape engine (training.unet_forward_train), which is what such a step runs on with the switch off.

Bars.  BAR = 5e-3 is what test_train_plan_gpu.py::test_planned_engine_matches_autograd_engine holds the parameter gradients
(all of them, as one vector) to; an input gradient is one tensor and is held to it by its own relative L2.  The golden is
fp32 CPU autograd, both engines round every GEMM operand to 16 bits: where the distance to the golden needs more than BAR
the bar is twice what the TAPE engine measures against the same golden (GOLDEN_MEASURED below, both numbers next to it).
"""
from pathlib import Path

import pytest
import torch

import test_train_plan_gpu as TPT
from conftest import rel_l2

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden" / "train_inputs_tiny.pt"
SCALE = 64.0            # static loss scale of every step here (16-bit gradient operands); divided out of what is compared
BAR = 5e-3
INPUTS = ("x", "context", "y")
# against the reference's fp32 golden, per operand type: {output or input: (tape engine measured, planned engine measured)}
# on an MI355X; the same with and without checkpointing.  The bar is max(BAR, 2 x tape): BAR itself for fp16 (every
# figure is under half of it), 2 x tape for bf16 (8 significant bits per GEMM operand against the golden's 24).
GOLDEN_MEASURED = {
    "fp16": {"out": (1.33e-3, 1.26e-3), "x": (2.17e-3, 1.99e-3), "context": (2.25e-3, 1.82e-3), "y": (2.24e-3, 1.98e-3)},
    "bf16": {"out": (1.06e-2, 1.01e-2), "x": (1.66e-2, 1.62e-2), "context": (1.75e-2, 1.52e-2), "y": (1.72e-2, 1.58e-2)},
}


def golden_bar(dtype, k):
    return max(BAR, 2.0 * GOLDEN_MEASURED[dtype][k][0])


@pytest.fixture(scope="module")
def gold():
    return torch.load(GOLDEN, map_location="cpu", weights_only=True)


@pytest.fixture
def dtype(request):
    from gcd_amd import autograd_ops as A
    A.set_train_dtype(request.param)
    A.PACK.clear()
    yield request.param
    A.set_train_dtype("fp16")
    A.PACK.clear()


@pytest.fixture
def det():
    from gcd_amd import autograd_ops as A
    old = A.DETERMINISTIC
    A.set_deterministic(True)
    yield
    A.set_deterministic(old)


def _inputs(gpu, gold):
    s = {k: v.to(gpu) for k, v in gold["inputs"].items()}
    s["T"] = gold["T"]
    return s


def _random_inputs(gpu, seed, clips, T, H=8, W=8):
    from oracle import svd_unet_ref as O
    cfg = O.TINY
    g = torch.Generator().manual_seed(seed)
    n = clips * T
    return dict(x=torch.randn(n, 8, H, W, generator=g).to(gpu), ts=torch.linspace(-1.0, 1.5, n).to(gpu),
                context=torch.randn(n, 1, cfg.context_dim, generator=g).to(gpu),
                y=torch.randn(n, cfg.adm_in_channels + cfg.aux_emb_dim, generator=g).clamp(-1, 1).to(gpu),
                ioi=torch.zeros(clips, T, device=gpu), target=torch.randn(n, 4, H, W, generator=g).to(gpu), T=T)


def _engine(name):
    from gcd_amd import training as TR
    from gcd_amd.train_plan import unet_forward_planned
    if name == "planned":
        return lambda *a, **kw: unet_forward_planned(*a, input_grads=True, **kw)
    return TR.unet_forward_train


def _step(net, s, engine="planned", need=INPUTS, ckpt=False):
    """One forward + backward with the inputs named in `need` requiring grad -> (out, {input: grad | None},
    {parameter: grad}), the loss scale divided out."""
    for p in net.parameters():
        p.grad = None
    t = {k: s[k].clone().requires_grad_(k in need) for k in INPUTS}
    out = _engine(engine)(net, t["x"], s["ts"], t["context"], t["y"], s["T"], s["ioi"], use_checkpoint=ckpt)
    ((out - s["target"]) ** 2).mean().mul(SCALE).backward()
    torch.cuda.synchronize()
    ig = {k: (None if t[k].grad is None else t[k].grad.clone() / SCALE) for k in INPUTS}
    pg = {n: p.grad.clone() / SCALE for n, p in net.named_parameters() if p.grad is not None}
    return out.detach().clone(), ig, pg


class _Spy:
    """Counts the calls of training.unet_forward_train while active (the fallback the switch replaces)."""

    def __enter__(self):
        from gcd_amd import training as TR
        self.TR, self.engine, self.calls = TR, TR.unet_forward_train, 0

        def spy(*a, **kw):
            self.calls += 1
            return self.engine(*a, **kw)
        TR.unet_forward_train = spy
        return self

    def __exit__(self, *exc):
        self.TR.unet_forward_train = self.engine


@pytest.mark.parametrize("ckpt", [False, True], ids=["plain", "ckpt"])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"], indirect=True)
def test_input_gradients_match_the_reference_golden(gpu, gold, dtype, ckpt):
    """Switch on: the step stays on the planned pass (no call of the tape engine: fails without the feature), and d y,
    d context, d x equal the unmodified reference's fp32 autograd within golden_bar; so does the output."""
    net = TPT._tiny(gpu, salt=0)
    s = _inputs(gpu, gold)
    with _Spy() as spy:
        out, ig, pg = _step(net, s, "planned", ckpt=ckpt)
    assert spy.calls == 0, "the planned entry handed the step to the operator-level engine"
    e_out = rel_l2(out, gold["out"])
    errs = {k: rel_l2(ig[k], gold[k + "_grad"]) for k in INPUTS}
    print(f"{dtype} ckpt={ckpt}: planned vs golden: out {e_out:.2e}  " + "  ".join(f"d{k} {v:.2e}" for k, v in errs.items()))
    for k in INPUTS:
        assert ig[k].shape == gold[k + "_grad"].shape and ig[k].dtype == torch.float32
    assert e_out < golden_bar(dtype, "out"), (e_out, golden_bar(dtype, "out"))
    for k in INPUTS:
        assert errs[k] < golden_bar(dtype, k), (k, errs[k], golden_bar(dtype, k))


def test_each_input_alone_equals_all_three_together(gpu, gold):
    net = TPT._tiny(gpu, salt=0)
    s = _inputs(gpu, gold)
    _, all3, _ = _step(net, s, "planned")
    for k in INPUTS:
        with _Spy() as spy:
            _, ig, _ = _step(net, s, "planned", need=(k,))
        assert spy.calls == 0
        assert all(ig[o] is None for o in INPUTS if o != k), k
        e = rel_l2(ig[k], all3[k])
        print(f"d{k} alone vs with the other two: {e:.2e}")
        assert e < BAR


def test_two_chunks_of_rows_and_the_long_temporal_kernel_match_the_tape_engine(gpu):
    """2 clips x 17 frames = 34 rows: two 32-row chunks per few-row problem (the second one 2 rows), the first clip length
    on the long temporal attention kernel.  Planned (switch on) against the tape engine; row 17 of d context — the second
    clip's first frame, the one the temporal cross-attention reads — carries the per-clip term."""
    net = TPT._tiny(gpu, salt=3)
    T = 17
    s = _random_inputs(gpu, 91, 2, T)
    from gcd_amd import autograd_ops as A
    A.PACK.clear()
    _, tape, tpg = _step(net, s, "tape")
    A.PACK.clear()
    with _Spy() as spy:
        _, plan, ppg = _step(net, s, "planned")
    assert spy.calls == 0
    for k in INPUTS:
        e = rel_l2(plan[k], tape[k])
        print(f"34 rows: d{k} planned vs tape {e:.2e}")
        assert e < BAR
    # d context = the per-frame (spatial) destination + on each clip's first frame the per-clip (temporal) one.  The two
    # destinations are arena views that hold this step's sums until the next forward zeroes them: the result's row T is
    # their sum with a non-zero per-clip row, row T + 1 is the per-frame row alone.
    p = net.__dict__["_gcd_train_plan"]
    dc = plan["context"].reshape(2 * T, -1) * SCALE
    per_frame, per_clip = p._d_ctx2d.clone(), p._d_ctx_clip.clone()
    assert per_clip.shape[0] == 2 and float(per_clip[1].abs().max()) > 0 and float(dc[T].abs().max()) > 0
    print(f"34 rows: row {T} of d context: |per-clip term| / |row| = {float(per_clip[1].norm() / dc[T].norm()):.2f}")
    assert torch.equal(dc[T], per_frame[T] + per_clip[1]) and torch.equal(dc[0], per_frame[0] + per_clip[0])
    assert torch.equal(dc[T + 1], per_frame[T + 1]) and torch.equal(dc[2 * T - 1], per_frame[2 * T - 1])
    num = sum(float((ppg[n].double() - v.double()).pow(2).sum()) for n, v in tpg.items())
    den = sum(float(v.double().pow(2).sum()) for v in tpg.values())
    assert (num / den) ** 0.5 < BAR


def test_deterministic_mode_is_bit_identical_and_default_mode_within_spread(gpu, gold):
    from gcd_amd import autograd_ops as A, training as TR
    net = TPT._tiny(gpu, salt=0)
    s = _inputs(gpu, gold)
    TR.set_deterministic(True)
    try:
        a, b = _step(net, s, "planned"), _step(net, s, "planned")
    finally:
        TR.set_deterministic(False)
    for k in INPUTS:
        assert torch.equal(a[1][k], b[1][k]), f"d{k}: {rel_l2(b[1][k], a[1][k]):.2e}"
    assert a[2].keys() == b[2].keys() and len(a[2]) > 100
    bad = [n for n in a[2] if not torch.equal(a[2][n], b[2][n])]
    assert not bad, bad[:4]
    # default mode: fp32 atomics order the sums differently run to run — the spread bar of the suite (1e-3), never equality
    a, b = _step(net, s, "planned"), _step(net, s, "planned")
    for k in INPUTS:
        e = rel_l2(b[1][k], a[1][k])
        print(f"default mode, two runs: d{k} {e:.2e}")
        assert e < 1e-3


def test_parameter_gradients_do_not_change_with_the_switch(gpu, gold, det):
    """Deterministic mode: the parameter gradients of a step that also computes the three input gradients are, bit for bit,
    those of the step with every input detached (the old path)."""
    net = TPT._tiny(gpu, salt=0)
    s = _inputs(gpu, gold)
    o0, _, g0 = _step(net, s, "planned", need=())
    o1, ig, g1 = _step(net, s, "planned")
    assert all(ig[k] is not None for k in INPUTS)
    assert torch.equal(o0, o1) and g0.keys() == g1.keys() and len(g0) > 100
    bad = [n for n in g0 if not torch.equal(g0[n], g1[n])]
    assert not bad, bad[:4]


def test_under_hipgraph_mode_the_call_runs_eager_and_equals_eager(gpu, gold, det):
    """GCD_TRAIN_GRAPH=1 (set_use_graph): a call that needs input gradients is the eager planned pass — GraphedPlan.mode ==
    "eager" for it, also after the graphs of the plain calls have been captured — and gives the eager result (bit for bit
    in deterministic mode); the replays around it are not disturbed."""
    from gcd_amd import autograd_ops as A, train_plan as TP
    net = TPT._tiny(gpu, salt=0)
    s = _inputs(gpu, gold)
    A.PACK.clear()
    eager = _step(net, s, "planned")
    plain = _step(net, s, "planned", need=())
    TP.set_use_graph(True)
    try:
        gp = TP.plan_for(net).graphed
        first = _step(net, s, "planned")
        assert gp.mode == "eager"
        for _ in range(4):                               # warm-up, capture, replay
            rep = _step(net, s, "planned", need=())
        assert gp.mode == "graph"
        after = _step(net, s, "planned")
        assert gp.mode == "eager"
        rep2 = _step(net, s, "planned", need=())
        assert gp.mode == "graph"
    finally:
        TP.set_use_graph(False)
    for run in (first, after):
        assert torch.equal(run[0], eager[0])
        for k in INPUTS:
            assert torch.equal(run[1][k], eager[1][k]), k
        assert all(torch.equal(run[2][n], eager[2][n]) for n in eager[2])
    for run in (rep, rep2):
        assert torch.equal(run[0], plain[0]) and all(torch.equal(run[2][n], plain[2][n]) for n in plain[2])


def test_trainable_pose_embedder_end_to_end(gpu):
    """cfg4's step at the tiny width: GeneralConditioner with a trainable SphericalEmbedder (-> the aux columns of `vector`),
    TrainDenoiser, StandardDiffusionLoss, one AdamHIP step over the UNet's and the embedder's parameters together.  With the
    switch on the step never visits the tape engine, proj.weight.grad / proj.bias.grad are the tape-engine fallback's within
    BAR, and both parameter sets move."""
    from gcd_amd import autograd_ops as A, training as TR
    from gcd_amd.conditioning import GeneralConditioner
    from oracle import svd_unet_ref as O
    cfg = O.TINY
    clips, T, H, W = 2, 3, 8, 8
    n = clips * T
    g = torch.Generator().manual_seed(17)
    batch = {"base": torch.randn(n, cfg.adm_in_channels, generator=g).clamp(-1, 1).to(gpu),
             "pose": (torch.rand(n, 3, generator=g) * 2 - 1).to(gpu),
             "ctx": torch.randn(n, 1, cfg.context_dim, generator=g).to(gpu),
             "cat": (torch.randn(n, 4, H, W, generator=g) * 0.8).to(gpu),
             "global_step": 10, "num_video_frames": T, "image_only_indicator": torch.zeros(clips, T, device=gpu)}
    x0 = torch.randn(n, 4, H, W, generator=g).to(gpu)
    ident = "gcd_amd.conditioning.IdentityEncoder"
    res = {}
    for mode in ("fallback", "switch"):
        net = TPT._tiny(gpu, salt=0)
        torch.manual_seed(5)
        cond = GeneralConditioner([
            {"target": ident, "input_key": "base"},
            {"target": "gcd_amd.conditioning.SphericalEmbedder", "is_trainable": True, "input_key": "pose",
             "params": {"embed_dim": cfg.aux_emb_dim}},
            {"target": ident, "input_key": "ctx"}, {"target": ident, "input_key": "cat"}]).to(gpu).train()
        proj = cond.embedders[1].proj
        den = TR.TrainDenoiser({"target": "gcd_amd.denoiser_scaling.VScalingWithEDMcNoise"}, use_checkpoint=True,
                               engine="planned", input_grads=(mode == "switch"))
        loss_fn = TR.StandardDiffusionLoss(
            sigma_sampler_config={"target": "gcd_amd.training.EDMSampling", "params": {"p_mean": 1.0, "p_std": 1.6}},
            loss_weighting_config={"target": "gcd_amd.training.EDMWeighting", "params": {"sigma_data": 1.0}},
            batch2model_keys=["image_only_indicator", "num_video_frames"])
        params = list(net.parameters()) + list(cond.parameters())
        assert any(p is proj.weight for p in params)
        opt = TR.AdamHIP(params, lr=1e-3)
        before = [p.detach().clone() for p in params]
        A.PACK.clear()
        torch.manual_seed(23)                            # the sigma sampler's and the noise's draws
        import warnings
        with _Spy() as spy, warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            loss = loss_fn(net, den, cond, x0, batch).mean()
        assert spy.calls == (1 if mode == "fallback" else 0), (mode, spy.calls)
        opt.zero_grad()
        (loss * SCALE).backward()
        torch.cuda.synchronize()
        res[mode] = (proj.weight.grad.clone() / SCALE, proj.bias.grad.clone() / SCALE, float(loss.detach()))
        opt.step(grad_scale=1.0 / SCALE)
        torch.cuda.synchronize()
        moved_unet = sum(not torch.equal(p, b) for p, b in zip(params[:-2], before[:-2]))
        assert moved_unet > 100, moved_unet
        assert not torch.equal(proj.weight, before[-2]) and not torch.equal(proj.bias, before[-1])
    (wf, bf, lf), (ws, bs, ls) = res["fallback"], res["switch"]
    ew, eb = rel_l2(ws, wf), rel_l2(bs, bf)
    print(f"end to end: loss {ls:.5f} vs {lf:.5f}; proj.weight.grad planned vs tape {ew:.2e}, proj.bias.grad {eb:.2e}")
    assert float(wf.abs().max()) > 0 and ew < BAR and eb < BAR
