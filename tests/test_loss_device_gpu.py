"""GPU: the fine-tune loss on the device (gcd_amd/loss_device.py, libgcd_amd_loss.so) and the `hip` loss engine of
gcd_amd/training.py: the reference's known answers at the bars the torch path is held to, the class weight map against
the torch map, the gradient against torch.autograd of the fp64 oracle, the tie rule, non-finite isolation, and one
planned fine-tune step under each loss engine.

The focal kernels have one size at which their path changes: a workgroup has 1024 threads (BLOCK), so a frame of up to 1024
elements gives every thread at most one element and the backward one chunk; 1025 is the first frame with a second round."""
import contextlib
from pathlib import Path

import pytest
import torch

from oracle import loss_ref as R
from oracle.make_golden_loss import pd_semantic_frames

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
BLOCK = 1024
CFG = dict(
    harmonize_sigmas=True, focus_top=0.1, focus_steps=5000,
    batch2model_keys=["image_only_indicator", "num_video_frames"],
    loss_weighting_config={"target": "gcd_amd.training.EDMWeighting", "params": {"sigma_data": 1.0}},
    sigma_sampler_config={"target": "gcd_amd.training.EDMSampling", "params": {"p_mean": 1.0, "p_std": 1.6}})
PERSON, VEHICLE = 7.0, 3.0


@contextlib.contextmanager
def loss_engine(name):
    from gcd_amd import training as TR
    old = TR.LOSS_ENGINE
    TR.set_loss_engine(name)
    try:
        yield
    finally:
        TR.set_loss_engine(old)


def _loss(**kw):
    from gcd_amd.training import StandardDiffusionLoss
    return StandardDiffusionLoss(**dict(CFG, **kw))


def _assert_clear_of_the_threshold(jpg, margin=1e-6):
    """The colour match compares a mean with 0.02 and can fall either way within an ulp of it: no pixel of a test's
    frames may sit that close (then every evaluation order gives the same mask)."""
    worst = 1.0
    for rgb in R.PD_PERSON + R.PD_VEHICLE:
        col = (torch.tensor(rgb, dtype=torch.float32) / 127.5 - 1.0)[None, :, None, None]
        worst = min(worst, float(((jpg - col).abs().double().mean(dim=1) - 0.02).abs().min()))
    assert worst >= margin, worst
    return worst


# ------------------------------------------------------------------------------------------- reference known answers
def test_known_answers_plain(gpu):
    g = torch.load(GOLD / "loss_kat.pt")
    out, tgt, w = g["out"].to(gpu), g["tgt"].to(gpu), g["weights"][:, None, None, None].to(gpu)
    assert len(g["cases"]) == 12
    with loss_engine("hip"):
        for case in g["cases"]:
            loss = _loss(loss_type=case["loss_type"])
            got = loss.get_loss(out, tgt, w, {"global_step": case["step"]})
            again = loss.get_loss(out, tgt, w, {"global_step": case["step"]})
            err = float(((got.cpu() - case["loss"]).abs() / case["loss"].abs()).max())
            print(f"plain {case['loss_type']} step {case['step']}: max rel {err:.2e}")
            assert torch.allclose(got.cpu(), case["loss"], rtol=1e-6, atol=0), case
            assert torch.equal(got, again)                          # bit-identical from call to call, no mode switch


def test_known_answers_class_weights(gpu):
    g = torch.load(GOLD / "loss_pd_kat.pt")
    jpg = pd_semantic_frames(g["out"].shape[0], *g["jpg_hw"], seed=g["jpg_seed"])
    print(f"distance of the fixture from the matching threshold: {_assert_clear_of_the_threshold(jpg):.2e}")
    out, tgt, w, jpg = g["out"].to(gpu), g["tgt"].to(gpu), g["weights"][:, None, None, None].to(gpu), jpg.to(gpu)
    assert len(g["cases"]) == 18
    with loss_engine("hip"):
        for case in g["cases"]:
            loss = _loss(loss_type=case["loss_type"], pd_person_weight=case["person"], pd_vehicle_weight=case["vehicle"])
            got = loss.get_loss(out, tgt, w, {"global_step": case["step"], "jpg": jpg})
            again = loss.get_loss(out, tgt, w, {"global_step": case["step"], "jpg": jpg})
            err = float(((got.cpu() - case["loss"]).abs() / case["loss"].abs()).max())
            print(f"pd {case['loss_type']} step {case['step']} person {case['person']} vehicle {case['vehicle']}: max rel {err:.2e}")
            assert torch.allclose(got.cpu(), case["loss"], rtol=2e-6, atol=0), case
            assert torch.equal(got, again)


# --------------------------------------------------------------------------------------------------- class map alone
@pytest.mark.parametrize("BT,hw,latent", [(6, (48, 80), (6, 10)), (3, (50, 83), (6, 10)), (1, (256, 384), (32, 48))],
                         ids=["48x80_to_6x10", "50x83_to_6x10_overlapping_bins", "256x384_to_32x48"])
@pytest.mark.parametrize("person,vehicle", [(PERSON, VEHICLE), (1.0, VEHICLE)], ids=["person_vehicle", "vehicle"])
def test_class_map_vs_torch(gpu, BT, hw, latent, person, vehicle):
    from gcd_amd import loss_device
    jpg = pd_semantic_frames(BT, *hw, seed=43)
    _assert_clear_of_the_threshold(jpg)
    loss = _loss(pd_person_weight=person, pd_vehicle_weight=vehicle)
    want = loss._pd_class_weight_map(jpg, latent)
    got = loss_device.class_weight_map(jpg.to(gpu), latent, loss._pd_classes())
    assert got.shape == want.shape == (BT, 1, *latent) and got.dtype == torch.float32
    err = float((got.cpu() - want).abs().max())
    print(f"class map {hw} -> {latent}: max abs {err:.2e}, map max {float(want.max()):.3f}, non-zero {int((want > 0).sum())}")
    assert float(want.max()) > 1.0 and int((want > 0).sum()) >= 10          # the fixture paints classes into every frame
    assert err <= 1e-6


# -------------------------------------------------------------------------------------------------------- the gradient
SHAPES = {140: (4, 5, 7), 240: (4, 6, 10), 6144: (4, 32, 48),                       # a tail in every vector width; cfg4's frame
          BLOCK - 1: (1, 3, 341), BLOCK: (4, 8, 32), BLOCK + 1: (1, 5, 205)}        # either side of the one path change


@pytest.fixture(scope="module")
def problems():
    """Per n: seeded Gaussian operands, the frames of the class weights, and the checks that no tie and no near-tie decides
    a comparison — made once, on the CPU, and left unchanged."""
    made = {}
    for n, (C_, H, W) in SHAPES.items():
        assert C_ * H * W == n
        g = torch.Generator().manual_seed(1000 + n)
        out, tgt = torch.randn(3, C_, H, W, generator=g), torch.randn(3, C_, H, W, generator=g)
        w = torch.rand(3, generator=g) + 0.5
        up = torch.randn(3, generator=g)
        jpg = pd_semantic_frames(3, 8 * H, 8 * W, seed=50 + n)
        _assert_clear_of_the_threshold(jpg)
        wmap = _loss(pd_person_weight=PERSON, pd_vehicle_weight=VEHICLE)._pd_class_weight_map(jpg, (H, W))
        made[n] = p = dict(out=out, tgt=tgt, w=w, up=up, jpg=jpg, wmap=wmap)
        # 6144 Gaussians do collide in fp32 now and then: an element whose loss equals another's is drawn again
        for _ in range(8):
            dup = torch.zeros(3, n, dtype=torch.bool)
            for loss_type in ("l2", "l1"):
                for with_map in (False, True):
                    flat = _all_fp32(p, loss_type, with_map)
                    for f in range(3):
                        _, inverse, counts = flat[f].unique(return_inverse=True, return_counts=True)
                        dup[f] |= counts[inverse] > 1
            if not bool(dup.any()):
                break
            out[dup.reshape(out.shape)] = torch.randn(int(dup.sum()), generator=g)
    return made


def _all_fp32(p, loss_type, with_map):
    """`all` per element as torch forms it in fp32, [3, n]."""
    diff = p["out"] - p["tgt"]
    raw = diff ** 2 if loss_type == "l2" else diff.abs()
    if with_map:
        raw = raw + raw * p["wmap"] * 0.5
    return raw.reshape(3, -1)


def _keeps(n):
    return [1, n - 1, int(n * 0.1), 0]


def _oracle(p, keep, loss_type, with_map):
    """fp64 loss and torch.autograd gradients of the oracle for .mean() and for the upstream vector; (keep + 0.5) / n as
    focus_top at the end of a one-step annealing makes int(n * cur_top) == keep."""
    n = p["out"][0].numel()
    kw = dict(loss_type=loss_type, focus_top=(keep + 0.5) / n, focus_steps=1) if keep else dict(loss_type=loss_type)
    out = p["out"].double().requires_grad_(True)
    w = p["w"].double()[:, None, None, None]
    if with_map:
        loss = R.get_loss_pd(out, p["tgt"].double(), w, 1, p["jpg"], PERSON, VEHICLE, **kw)
    else:
        loss = R.get_loss(out, p["tgt"].double(), w, 1, **kw)
    g_mean, = torch.autograd.grad(loss.mean(), out, retain_graph=True)
    g_up, = torch.autograd.grad((loss * p["up"].double()).sum(), out)
    return loss.detach(), g_mean, g_up


def _assert_no_tie_decides(p, keep, loss_type, with_map):
    """`all` has n distinct fp32 values per frame, and the keep-th and (keep + 1)-th largest are further apart than the
    rounding of fp32 can move them (8 ulp), so the fp64 oracle and the kernel select the same elements."""
    flat = _all_fp32(p, loss_type, with_map)
    n = flat.shape[1]
    for f in range(3):
        assert flat[f].unique().numel() == n
        if 0 < keep < n:
            s = flat[f].double().sort(descending=True)[0]
            assert float((s[keep - 1] - s[keep]) / s[keep - 1]) > 8 * 2.0 ** -24, (f, keep)


@pytest.mark.parametrize("with_map", [False, True], ids=["plain", "wmap"])
@pytest.mark.parametrize("loss_type", ["l2", "l1"])
@pytest.mark.parametrize("n", list(SHAPES))
def test_gradient_vs_fp64_oracle(gpu, problems, n, loss_type, with_map):
    p = problems[n]
    kw = dict(pd_person_weight=PERSON, pd_vehicle_weight=VEHICLE) if with_map else {}
    tgt, w, up = p["tgt"].to(gpu), p["w"].to(gpu)[:, None, None, None], p["up"].to(gpu)
    batch = {"global_step": 1, "jpg": p["jpg"].to(gpu)}
    with loss_engine("hip"):
        for keep in _keeps(n):
            _assert_no_tie_decides(p, keep, loss_type, with_map)
            want, want_mean, want_up = _oracle(p, keep, loss_type, with_map)
            loss_fn = _loss(loss_type=loss_type, focus_top=(keep + 0.5) / n, focus_steps=1, **kw) if keep else \
                _loss(loss_type=loss_type, focus_top=1.0, focus_steps=-1, **kw)
            out = p["out"].to(gpu).requires_grad_(True)
            got = loss_fn.get_loss(out, tgt, w, batch)
            g_mean, = torch.autograd.grad(got.mean(), out, retain_graph=True)
            g_up, = torch.autograd.grad((got * up).sum(), out)
            e_loss = float(((got.detach().cpu().double() - want).abs() / want.abs()).max())
            e_mean = float(((g_mean.cpu().double() - want_mean).abs() / want_mean.abs()).max())
            e_up = float(((g_up.cpu().double() - want_up).abs() / want_up.abs()).max())
            print(f"n {n} {loss_type} map {with_map} keep {keep}: loss {e_loss:.2e}, d mean {e_mean:.2e}, d upstream {e_up:.2e}")
            assert got.shape == (3,) and g_mean.shape == out.shape and g_mean.dtype == torch.float32
            assert torch.allclose(got.detach().cpu().double(), want, rtol=2e-6, atol=0), keep
            assert torch.allclose(g_mean.cpu().double(), want_mean, rtol=2e-6, atol=0), keep
            assert torch.allclose(g_up.cpu().double(), want_up, rtol=2e-6, atol=0), keep


def test_casts_and_layouts_go_through_autograd(gpu, problems):
    """A model output that is not contiguous fp32 is made so by torch ops: the gradient arrives in the leaf's own dtype and
    layout; target and w get none."""
    from gcd_amd import loss_device
    p = problems[240]
    tgt, w = p["tgt"].to(gpu).requires_grad_(True), p["w"].to(gpu).requires_grad_(True)
    base = p["out"].to(gpu).requires_grad_(True)
    want, d_tgt, d_w = torch.autograd.grad(loss_device.focal_loss(base, tgt, w, 24).sum(), [base, tgt, w], allow_unused=True)
    assert d_tgt is None and d_w is None
    leaf = p["out"].to(gpu).permute(0, 2, 3, 1).contiguous().requires_grad_(True)            # channels-last storage
    got, = torch.autograd.grad(loss_device.focal_loss(leaf.permute(0, 3, 1, 2), tgt, w, 24).sum(), leaf)
    assert torch.equal(got.permute(0, 3, 1, 2), want)
    half = p["out"].to(gpu).half().requires_grad_(True)
    got16, = torch.autograd.grad(loss_device.focal_loss(half, tgt, w[:, None, None, None], 24).sum(), half)
    assert got16.dtype == torch.float16 and got16.shape == half.shape and bool(torch.isfinite(got16).all())
    f32 = half.detach().float().requires_grad_(True)
    want16, = torch.autograd.grad(loss_device.focal_loss(f32, tgt, w, 24).sum(), f32)
    assert torch.equal(got16, want16.half())
    with torch.no_grad():                                                                    # no tape: forward only
        assert torch.equal(loss_device.focal_loss(base, tgt, w, 24), loss_device.focal_loss(base.detach(), tgt, w, 24))


# -------------------------------------------------------------------------------------------------------------- ties
@pytest.mark.parametrize("loss_type", ["l2", "l1"])
@pytest.mark.parametrize("n,shape", [(140, (4, 5, 7)), (2500, (4, 25, 25))], ids=["one_chunk", "three_chunks"])
def test_ties_select_the_lowest_flat_indices(gpu, n, shape, loss_type):
    """diff from {0.5, 1, 2}: tau sits inside the group of ones.  The loss is the oracle's; exactly `keep` elements carry the
    selected coefficient; among the tied ones they are the lowest flat indices; untied elements have the oracle's gradient."""
    from gcd_amd import loss_device
    g = torch.Generator().manual_seed(n)
    diff = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (3, *shape), generator=g)]
    diff = diff * (torch.randint(0, 2, diff.shape, generator=g) * 2 - 1)                 # either sign
    tgt = torch.zeros_like(diff)
    w = torch.tensor([0.75, 1.5, 2.25])
    flat = diff.abs().reshape(3, n)
    twos, ones = (flat == 2.0).sum(1), (flat == 1.0).sum(1)
    quota = 7
    keep = int(twos.max()) + quota
    assert bool((twos + ones > keep).all()) and bool((keep - twos >= 1).all())          # tau == 1 in every frame, ties left over
    out = diff.clone().double().requires_grad_(True)
    want = R.get_loss(out, tgt.double(), w.double()[:, None, None, None], 1, loss_type, (keep + 0.5) / n, 1)
    want_grad, = torch.autograd.grad(want.sum(), out)
    leaf = diff.to(gpu).requires_grad_(True)
    got = loss_device.focal_loss(leaf, tgt.to(gpu), w.to(gpu), keep, loss_type)
    grad, = torch.autograd.grad(got.sum(), leaf)
    assert torch.allclose(got.detach().cpu().double(), want.detach(), rtol=2e-6, atol=0)
    draw = 2.0 * diff.double() if loss_type == "l2" else diff.sign().double()
    coef = (grad.cpu().double() / draw / w.double()[:, None, None, None]).reshape(3, n)
    c_sel, c_rest = 0.9 / keep + 0.1 / n, 0.1 / n
    selected = coef > 0.5 * (c_sel + c_rest)
    assert torch.allclose(coef[selected], torch.full_like(coef[selected], c_sel), rtol=2e-6, atol=0)
    assert torch.allclose(coef[~selected], torch.full_like(coef[~selected], c_rest), rtol=2e-6, atol=0)
    assert selected.sum(1).tolist() == [keep] * 3
    for f in range(3):
        tied = (flat[f] == 1.0).nonzero().reshape(-1)
        q = keep - int(twos[f])
        assert bool(selected[f][flat[f] == 2.0].all()) and not bool(selected[f][flat[f] == 0.5].any())
        assert selected[f][tied].nonzero().reshape(-1).tolist() == list(range(q)), f      # the q lowest flat indices
    untied = (flat != 1.0).reshape(diff.shape)
    assert torch.allclose(grad.cpu().double()[untied], want_grad[untied], rtol=2e-6, atol=0)


# ------------------------------------------------------------------------------------------------- non-finite values
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("keep", [24, 0])
def test_non_finite_value_stays_inside_its_frame(gpu, problems, bad, keep):
    from gcd_amd import loss_device
    p = problems[240]
    tgt, w = p["tgt"].to(gpu), p["w"].to(gpu)
    wmap = loss_device.class_weight_map(p["jpg"].to(gpu), (6, 10), _loss(pd_person_weight=PERSON, pd_vehicle_weight=VEHICLE)._pd_classes())

    def run(out):
        leaf = out.to(gpu).requires_grad_(True)
        loss = loss_device.focal_loss(leaf, tgt, w, keep, "l2", wmap)
        grad, = torch.autograd.grad(loss.sum(), leaf)
        return loss.detach(), grad
    clean_loss, clean_grad = run(p["out"])
    dirty = p["out"].clone()
    dirty[1, 2, 3, 4] = bad
    loss, grad = run(dirty)
    assert bool(torch.isnan(loss[1])) if bad != bad else not bool(torch.isfinite(loss[1]))
    assert bool(torch.isfinite(clean_loss).all())
    for f in (0, 2):
        assert torch.equal(loss[f].view(torch.int32), clean_loss[f].view(torch.int32))
        assert torch.equal(grad[f].view(torch.int32), clean_grad[f].view(torch.int32))


# --------------------------------------------------------------------------------------------------------- integration
def test_planned_step_under_each_loss_engine(gpu):
    """The tiny network and fine-tune step of tests/test_optim_gpu.py (deterministic mode, dynamic loss scale): the torch and
    the hip loss engine, same seed.  The loss scalars agree to 2e-6 and the worst parameter gradient to rel-L2 2e-3, the
    bar of two runs that differ only in rounding (tests/test_train_plan_gpu.py)."""
    import test_backward_gpu as TB
    import test_optim_gpu as TO
    import test_train_plan_gpu as TPT
    from conftest import rel_l2
    from gcd_amd import autograd_ops as A, training as TR
    from oracle import svd_unet_ref as O
    assert TO.HYPER["lr"] > 0                       # (the step below is that module's tiny fine-tune step)
    cfg = O.TINY
    T, H, W, B = 4, 16, 16, 2
    BT = B * T
    g0 = TB._gen(12)
    x0 = torch.randn(BT, 4, H, W, generator=g0).to(gpu)
    cond = {"crossattn": torch.randn(BT, 1, cfg.context_dim, generator=g0).to(gpu),
            "concat": (torch.randn(BT, 4, H, W, generator=g0) * 0.8).to(gpu),
            "vector": torch.randn(BT, cfg.adm_in_channels + cfg.aux_emb_dim, generator=g0).clamp(-1, 1).to(gpu)}
    ioi = torch.zeros(B, T, device=gpu)
    g = torch.Generator().manual_seed(7)
    rand, noise = torch.randn(BT, generator=g), torch.randn(BT, 4, H, W, generator=g).to(gpu)
    den = TR.TrainDenoiser({"target": "gcd_amd.denoiser_scaling.VScalingWithEDMcNoise"}, engine="planned", deterministic=True)
    loss_fn = _loss()

    def step(engine):
        A.PACK.clear()
        net = TPT._tiny(gpu, salt=3)
        opt = TR.AdamHIP(net.parameters(), lr=1e-4, max_grad_norm=1.0, loss_scale="dynamic", init_scale=256.0)
        sig = loss_fn.sigma_sampler(BT, rand=rand).reshape(B, T)[:, :1].expand(B, T).reshape(-1).to(gpu)
        with loss_engine(engine):
            out = den(net, x0 + noise * sig[:, None, None, None], sig, cond, num_video_frames=T, image_only_indicator=ioi)
            loss = loss_fn.get_loss(out, x0, loss_fn.loss_weighting(sig)[:, None, None, None], {"global_step": 2500}).mean()
            opt.scale(loss).backward()
        torch.cuda.synchronize()
        return float(loss.detach()), {k: v.grad.detach().clone() for k, v in net.named_parameters() if v.grad is not None}

    old = A.DETERMINISTIC
    try:
        loss_t, grads_t = step("torch")
        loss_h, grads_h = step("hip")
    finally:
        A.set_deterministic(old)
    assert set(grads_t) == set(grads_h) and len(grads_t) > 100
    worst = max(((rel_l2(grads_h[k], grads_t[k]), k) for k in grads_t if float(grads_t[k].abs().max()) > 0), default=(0.0, ""))
    print(f"loss torch {loss_t:.9g} hip {loss_h:.9g} (rel {abs(loss_h / loss_t - 1):.2e}); worst gradient rel-L2 {worst[0]:.2e} ({worst[1]})")
    assert abs(loss_h / loss_t - 1.0) <= 2e-6
    assert worst[0] < 2e-3
