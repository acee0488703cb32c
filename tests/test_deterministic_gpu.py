"""GPU: the deterministic reduction mode at the level of a fine-tune step (DESIGN.md "Deterministic reductions").

With `training.set_deterministic(True)` a step is a function of (inputs, shapes, dtype): repeated steps are bit-equal on
both engines, both operand types, with and without activation checkpointing, under hipGraph replay, with two plans
interleaved and under gradient accumulation; a seeded three-step Adam run ends in the same weights twice.  And it is the
same answer as the default mode's: against the default mode, against the CPU oracle (tiny width) and against the
reference's fp32 golden (full width), at the bars the default mode's tests use.
Every test restores the default mode (`det` fixture), so the rest of the suite runs on the default path.
"""
import math
from pathlib import Path

import pytest
import torch

import test_backward_gpu as TB
import test_train_plan_gpu as TPT
from conftest import rel_l2
from oracle import svd_unet_ref as O, weights

pytestmark = pytest.mark.gpu


@pytest.fixture
def det():
    from gcd_amd import autograd_ops as A
    old = A.DETERMINISTIC
    A.set_deterministic(True)
    yield
    A.set_deterministic(old)


@pytest.fixture
def dtype(request):
    from gcd_amd import autograd_ops as A
    A.set_train_dtype(request.param)
    A.PACK.clear()
    yield request.param
    A.set_train_dtype("fp16")
    A.PACK.clear()


def _fwd(engine):
    from gcd_amd import training as TR
    from gcd_amd.train_plan import unet_forward_planned
    return unet_forward_planned if engine == "planned" else TR.unet_forward_train


def _step(net, s, engine="planned", ckpt=False, keep_grad=False):
    """One forward + backward on the inputs `s` (TPT._tiny_step_inputs): (output, {name: gradient}) as clones."""
    if not keep_grad:
        for p in net.parameters():
            p.grad = None
    out = _fwd(engine)(net, s["x"], s["ts"], s["ctx"], s["y"], s["T"], s["ioi"], use_checkpoint=ckpt)
    ((out - s["tgt"]) ** 2).mean().mul(64.0).backward()
    torch.cuda.synchronize()
    return out.detach().clone(), {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}


def _assert_equal(a, b, what):
    """Every tensor of both steps, none left out."""
    (oa, ga), (ob, gb) = a, b
    assert torch.equal(oa, ob), f"{what}: output differs, rel-L2 {rel_l2(ob, oa):.2e}"
    assert ga.keys() == gb.keys() and len(ga) > 100
    bad = [(n, rel_l2(gb[n], ga[n])) for n in ga if not torch.equal(ga[n], gb[n])]
    assert not bad, f"{what}: {len(bad)} of {len(ga)} gradients differ; first: {bad[:4]}"


@pytest.mark.parametrize("ckpt", [False, True], ids=["plain", "ckpt"])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"], indirect=True)
@pytest.mark.parametrize("engine", ["planned", "autograd"])
def test_three_steps_are_bit_equal(gpu, det, engine, dtype, ckpt):
    net = TPT._tiny(gpu, salt=5)
    s = TPT._tiny_step_inputs(gpu, 41)
    runs = [_step(net, s, engine, ckpt) for _ in range(3)]
    _assert_equal(runs[0], runs[1], f"{engine}/{dtype}/ckpt={ckpt} step 2 vs 1")
    _assert_equal(runs[0], runs[2], f"{engine}/{dtype}/ckpt={ckpt} step 3 vs 1")


def test_default_mode_calls_no_deterministic_entry_and_modes_agree(gpu):
    """Mode off: zero calls to the new entries (every call goes where it went before).  Mode on: all five are called, and
    the gradients are the default mode's but for the order of its sums: rel-L2 < 1e-3 per tensor of >= 64 elements (the bar
    of test_activation_checkpointing_matches)."""
    from gcd_amd import autograd_ops as A
    assert A.DETERMINISTIC is False, "the suite runs in the default mode"
    net = TPT._tiny(gpu, salt=5)
    s = TPT._tiny_step_inputs(gpu, 41)
    seen = set()
    for engine in ("planned", "autograd"):
        A.DET_CALLS.clear()
        off = _step(net, s, engine)
        assert not A.DET_CALLS, A.DET_CALLS
        A.set_deterministic(True)
        try:
            on = _step(net, s, engine)
        finally:
            A.set_deterministic(False)
        calls = dict(A.DET_CALLS)
        print(f"{engine}: deterministic entries called: {calls}")
        want = {"gcd_layernorm_bwd_det", "gcd_cast_colsum_det_f32"}
        if engine == "planned":
            want |= {"gcd_blend_bwd_det_f32", "gcd_smallm_dgrad_det"}
        assert want <= set(calls), set(calls)
        seen |= set(calls)
        assert torch.equal(on[0], off[0])                  # the forward pass has no order-dependent sum
        assert on[1].keys() == off[1].keys()
        worst = max(((rel_l2(on[1][n], off[1][n]), n) for n in off[1] if off[1][n].numel() >= 64))
        print(f"{engine}: mode on vs off, worst tensor {worst[1]} rel-L2 {worst[0]:.2e}")
        assert worst[0] < 1e-3, worst
    A.DET_CALLS.clear()
    assert seen == {"gcd_rowblock_sum_det_f32", "gcd_layernorm_bwd_det", "gcd_cast_colsum_det_f32", "gcd_blend_bwd_det_f32",
                    "gcd_smallm_dgrad_det"}, seen


def test_checkpointed_vs_plain_measured(gpu, det):
    """Not required to be bit-equal (the two paths fuse differently): measured and printed; the bar is the default mode's."""
    net = TPT._tiny(gpu, salt=5)
    s = TPT._tiny_step_inputs(gpu, 41)
    for engine in ("planned", "autograd"):
        plain, ck = _step(net, s, engine, False), _step(net, s, engine, True)
        same = sum(torch.equal(plain[1][n], ck[1][n]) for n in plain[1])
        worst = max(rel_l2(ck[1][n], plain[1][n]) for n in plain[1] if plain[1][n].numel() >= 64)
        print(f"{engine}: checkpointed vs plain: output equal {torch.equal(plain[0], ck[0])}, {same} of {len(plain[1])} "
              f"gradients bit-equal, worst rel-L2 {worst:.2e}")
        assert worst < 1e-3


def test_graph_warmup_and_replays_are_bit_equal(gpu, det):
    from gcd_amd import autograd_ops as A, train_plan as TP
    net = TPT._tiny(gpu, salt=7)
    s = TPT._tiny_step_inputs(gpu, 43)
    A.PACK.clear()
    eager = _step(net, s, "planned", True)
    TP.set_use_graph(True)
    try:
        runs = [_step(net, s, "planned", True) for _ in range(5)]
        assert TP.plan_for(net).graphed.mode == "graph", "the steps after the warm-up must have been replays"
        # flipping the switch is part of the signature: the next call warms up again instead of replaying the other mode
        A.set_deterministic(False)
        _step(net, s, "planned", True)
        assert TP.plan_for(net).graphed.mode == "eager"
    finally:
        TP.set_use_graph(False)
        A.set_deterministic(True)
    for i, r in enumerate(runs):
        _assert_equal(eager, r, f"graph mode step {i} vs an eager step")


def test_two_plans_alternating_are_bit_equal(gpu, det):
    """test_two_plans_alternating_in_one_process_do_not_interfere with hard equality: no spread branch."""
    from gcd_amd import autograd_ops as A, train_plan as TP
    na, nb = TPT._tiny(gpu, salt=5), TPT._tiny(gpu, salt=6)
    ia, ib = TPT._tiny_step_inputs(gpu, 41), TPT._tiny_step_inputs(gpu, 42)
    oa, ga = _step(na, ia)
    ob, gb = _step(nb, ib)
    heard = []
    TP.add_grad_listener(list(na.parameters()), heard.append)
    try:
        for net in (na, nb):
            for p in net.parameters():
                p.grad = None
        fwd = _fwd("planned")
        out_a = fwd(na, ia["x"], ia["ts"], ia["ctx"], ia["y"], ia["T"], ia["ioi"], use_checkpoint=False)
        out_b = fwd(nb, ib["x"], ib["ts"], ib["ctx"], ib["y"], ib["T"], ib["ioi"], use_checkpoint=False)
        ((out_a - ia["tgt"]) ** 2).mean().mul(64.0).backward()
        ((out_b - ib["tgt"]) ** 2).mean().mul(64.0).backward()
        torch.cuda.synchronize()
    finally:
        TP.remove_grad_listener(list(na.parameters()), heard.append)
    assert torch.equal(out_a, oa) and torch.equal(out_b, ob)
    for net, ref in ((na, ga), (nb, gb)):
        got = {n: p.grad for n, p in net.named_parameters() if p.grad is not None}
        assert got.keys() == ref.keys()
        for n in ref:
            assert torch.equal(got[n], ref[n]), n
    ids_a, ids_b = {id(p) for p in na.parameters()}, {id(p) for p in nb.parameters()}
    assert heard and all(id(p) in ids_a for p in heard) and not any(id(p) in ids_b for p in heard)
    assert not hasattr(A._SCOPE, "sink")


@pytest.mark.parametrize("engine", ["planned", "autograd"])
def test_gradient_accumulation_is_bit_equal(gpu, det, engine):
    """Two backward passes onto live .grad (the second ADDS), the pair repeated."""
    net = TPT._tiny(gpu, salt=5)
    s1, s2 = TPT._tiny_step_inputs(gpu, 41), TPT._tiny_step_inputs(gpu, 42)
    pairs = []
    for _ in range(2):
        first = _step(net, s1, engine)
        second = _step(net, s2, engine, keep_grad=True)
        pairs.append(second)
        worst = max(rel_l2(second[1][n], first[1][n]) for n in first[1] if first[1][n].numel() >= 64)
        assert worst > 1e-2, "the second pass must have added something"
    _assert_equal(pairs[0], pairs[1], f"{engine}: accumulated gradients")


def test_seeded_three_step_run_twice_ends_in_the_same_weights(gpu, det):
    """The promise to the user: a fine-tune re-run from a seed (sigma and noise from seeded generators, AdamHIP) gives
    the same weights, bit for bit."""
    from gcd_amd import autograd_ops as A, training as TR
    cfg = O.TINY
    T, H, W, B = 4, 16, 16, 2
    BT = B * T
    net = TPT._tiny(gpu, salt=3)
    sd0 = {k: v.detach().clone() for k, v in net.state_dict().items()}
    g0 = TB._gen(12)
    x0 = torch.randn(BT, 4, H, W, generator=g0).to(gpu)
    cond = {"crossattn": torch.randn(BT, 1, cfg.context_dim, generator=g0).to(gpu),
            "concat": (torch.randn(BT, 4, H, W, generator=g0) * 0.8).to(gpu),
            "vector": torch.randn(BT, cfg.adm_in_channels + cfg.aux_emb_dim, generator=g0).clamp(-1, 1).to(gpu)}
    ioi = torch.zeros(B, T, device=gpu)
    loss_scale = 256.0

    def run(seed):
        net.load_state_dict(sd0)
        A.PACK.clear()
        den = TR.TrainDenoiser({"target": "gcd_amd.denoiser_scaling.VScalingWithEDMcNoise"}, deterministic=True)
        loss_fn = TR.StandardDiffusionLoss(
            sigma_sampler_config={"target": "gcd_amd.training.EDMSampling", "params": {"p_mean": 1.0, "p_std": 1.6}},
            loss_weighting_config={"target": "gcd_amd.training.EDMWeighting", "params": {"sigma_data": 1.0}},
            focus_top=0.1, focus_steps=5000, batch2model_keys=["image_only_indicator", "num_video_frames"])
        opt = TR.AdamHIP(net.parameters(), lr=1e-4)
        g = torch.Generator().manual_seed(seed)
        losses = []
        for step in range(3):
            opt.zero_grad()
            sig = loss_fn.sigma_sampler(BT, rand=torch.randn(BT, generator=g)).reshape(B, T)[:, :1].expand(B, T).reshape(-1).to(gpu)
            noise = torch.randn(BT, 4, H, W, generator=g).to(gpu)
            out = den(net, x0 + noise * sig[:, None, None, None], sig, cond, num_video_frames=T, image_only_indicator=ioi)
            # global_step 2500 + step: the focal top-k of the loss is active
            loss = loss_fn.get_loss(out, x0, loss_fn.loss_weighting(sig)[:, None, None, None], {"global_step": 2500 + step}).mean()
            (loss * loss_scale).backward()
            opt.step(grad_scale=1.0 / loss_scale)
            losses.append(float(loss.detach()))
        torch.cuda.synchronize()
        return losses, {k: v.detach().clone() for k, v in net.state_dict().items()}
    l1, w1 = run(7)
    l2, w2 = run(7)
    l3, w3 = run(8)
    print(f"losses {l1} / {l2}; another seed: {l3}")
    assert l1 == l2
    moved = sum(not torch.equal(w1[k], sd0[k]) for k in w1)
    assert moved > 100, moved
    bad = [k for k in w1 if not torch.equal(w1[k], w2[k])]
    assert not bad, f"{len(bad)} of {len(w1)} tensors differ between two runs from seed 7: {bad[:4]}"
    assert any(not torch.equal(w1[k], w3[k]) for k in w1), "another seed gives another run"


def test_tiny_step_vs_oracle_in_deterministic_mode(gpu, det):
    """The body of test_unet_training_step_vs_oracle (step 0, planned engine) with the mode on, at its TOL_NET bars."""
    from gcd_amd import training as TR
    from oracle import loss_ref as LR
    net, sd = TB._tiny_unet(gpu, salt=3)
    T, H, W, B = 4, 16, 16, 2
    BT = B * T
    cfg = O.TINY
    g = TB._gen(12)
    x0 = torch.randn(BT, 4, H, W, generator=g)
    noise = torch.randn(BT, 4, H, W, generator=g)
    cond = {"crossattn": torch.randn(BT, 1, cfg.context_dim, generator=g),
            "concat": torch.randn(BT, 4, H, W, generator=g) * 0.8,
            "vector": torch.randn(BT, cfg.adm_in_channels + cfg.aux_emb_dim, generator=g).clamp(-1, 1)}
    sig = LR.harmonize(LR.edm_sigmas(torch.randn(BT, generator=g), 1.0, 1.6), T)
    ioi = torch.zeros(B, T)
    loss_scale = 256.0
    sdr = {k: TB._leaf(v) for k, v in sd.items()}
    noised = x0 + noise * sig[:, None, None, None]
    out_r = O.denoise(sdr, cfg, noised, sig, cond, T, ioi)
    loss_r = LR.get_loss(out_r, x0, LR.edm_weighting(sig, 1.0)[:, None, None, None], 0, "l2", 0.1, 5000).mean()
    loss_r.backward()
    den = TR.TrainDenoiser({"target": "gcd_amd.denoiser_scaling.VScalingWithEDMcNoise"}, engine="planned")
    loss_fn = TR.StandardDiffusionLoss(
        sigma_sampler_config={"target": "gcd_amd.training.EDMSampling", "params": {"p_mean": 1.0, "p_std": 1.6}},
        loss_weighting_config={"target": "gcd_amd.training.EDMWeighting", "params": {"sigma_data": 1.0}},
        focus_top=0.1, focus_steps=5000, batch2model_keys=["image_only_indicator", "num_video_frames"])
    cg = {k: v.to(gpu) for k, v in cond.items()}
    sg = sig.to(gpu)
    out = den(net, noised.to(gpu), sg, cg, num_video_frames=T, image_only_indicator=ioi.to(gpu))
    w = loss_fn.loss_weighting(sg)[:, None, None, None]
    loss = loss_fn.get_loss(out, x0.to(gpu), w, {"global_step": 0}).mean()
    (loss * loss_scale).backward()
    torch.cuda.synchronize()
    assert abs(float(loss) / float(loss_r) - 1.0) < 2e-3
    TB._check("denoiser output", out, out_r, 2e-3)
    num = den_ = 0.0
    worst = ("", 0.0)
    for name, prm in net.named_parameters():
        ref = sdr[name].grad
        if ref is None or float(ref.abs().max()) == 0.0:
            assert prm.grad is None or float(prm.grad.abs().max()) == 0.0, name
            continue
        got = prm.grad.double().cpu() / loss_scale
        num += float((got - ref.double()).pow(2).sum())
        den_ += float(ref.double().pow(2).sum())
        if ref.numel() >= 64:
            e = rel_l2(got, ref)
            if e > worst[1]:
                worst = (name, e)
    total = math.sqrt(num / den_)
    print(f"deterministic mode vs oracle: global rel-L2 {total:.3e}; worst tensor {worst[0]} {worst[1]:.2e}")
    assert total < TB.TOL_NET and worst[1] < 4 * TB.TOL_NET


# ------------------------------------------------------------------------------------------------------ full width (cfg4)
@pytest.fixture(scope="module")
def full_net(gpu):
    """The 1.53 B-parameter Kubric VideoUNet with the golden's synthetic weights, built once for this module."""
    from gcd_amd.video_model import VideoUNet
    gold = Path(__file__).resolve().parent / "golden" / "train_kubric_32x48.pt"
    G = torch.load(gold)
    with torch.device("meta"):
        net = VideoUNet(**O.KUBRIC.as_reference_kwargs())
    sd = weights.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, G["salt"])
    net = net.to_empty(device=gpu)
    net.load_state_dict(sd)
    del sd
    net.train()
    yield net, G
    del net
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", ["fp16", "bf16"], indirect=True)
def test_full_width_cfg4_vs_reference_golden_and_repeat(gpu, det, full_net, dtype):
    """The body of test_training_step_full_width_cfg4_vs_reference_golden (planned engine, train_kubric_32x48.pt) with the
    mode on, at that test's bars (fp16 2e-3 / 5e-3, bf16 7e-3 / 7.5e-3) against the unmodified reference's fp32 autograd;
    then the same step again: every gradient bit-equal."""
    from gcd_amd import training as TR
    from oracle.make_golden_cfg4 import inputs
    from oracle.make_golden_fullres import sample
    net, G = full_net
    x0, noise, cond, sig = inputs()
    B, T = G["B"], G["T"]
    loss_scale = 1024.0
    den = TR.TrainDenoiser({"target": "gcd_amd.denoiser_scaling.VScalingWithEDMcNoise"}, use_checkpoint=True, engine="planned")
    loss_fn = TR.StandardDiffusionLoss(
        sigma_sampler_config={"target": "gcd_amd.training.EDMSampling", "params": {"p_mean": 1.0, "p_std": 1.6}},
        loss_weighting_config={"target": "gcd_amd.training.EDMWeighting", "params": {"sigma_data": 1.0}},
        focus_top=0.1, focus_steps=5000, batch2model_keys=["image_only_indicator", "num_video_frames"])
    noised = (x0 + noise * sig[:, None, None, None]).to(gpu)
    sg = sig.to(gpu)
    cg = {k: v.to(gpu) for k, v in cond.items()}
    ioi = torch.zeros(B, T, device=gpu)

    def step():
        for p in net.parameters():
            p.grad = None
        out = den(net, noised, sg, cg, num_video_frames=T, image_only_indicator=ioi)
        w = loss_fn.loss_weighting(sg)[:, None, None, None]
        loss = loss_fn.get_loss(out, x0.to(gpu), w, {"global_step": G["step"]}).mean()
        (loss * loss_scale).backward()
        torch.cuda.synchronize()
        return out.detach(), loss.detach()
    out, loss = step()
    tol_out, tol_g = (2e-3, 5e-3) if dtype == "fp16" else (7e-3, 7.5e-3)
    e_out = rel_l2(sample(out.cpu(), 65536), G["out_samples"])
    print(f"[{dtype}, deterministic] loss {float(loss):.6f} vs reference {G['loss']:.6f}; denoiser output rel-L2 {e_out:.2e}")
    assert abs(float(loss) / G["loss"] - 1.0) < (2e-3 if dtype == "fp16" else 1e-2)
    assert e_out < tol_out
    num = den_ = 0.0
    worst_norm = ("", 0.0)
    seen = n_dead = 0
    total_ref = sum(v * v for v in G["grad_norms"].values()) ** 0.5
    first = {}
    for name, prm in net.named_parameters():
        if name in G["dead"] or G["grad_norms"][name] < 1e-7 * total_ref:
            assert prm.grad is None or float(prm.grad.double().norm()) / loss_scale < 1e-7 * total_ref, name
            n_dead += 1
            if prm.grad is not None:
                first[name] = prm.grad.clone()
            continue
        first[name] = prm.grad.clone()
        got = prm.grad.detach().float().cpu() / loss_scale
        ref_s = G["grad_samples"][name].double()
        got_s = sample(got, 128).double()
        num += float((got_s - ref_s).pow(2).sum())
        den_ += float(ref_s.pow(2).sum())
        seen += 1
        rn = abs(float(got.double().norm()) / G["grad_norms"][name] - 1.0)
        if got.numel() >= 64 and rn > worst_norm[1]:
            worst_norm = (name, rn)
    g_err = (num / den_) ** 0.5
    print(f"[{dtype}, deterministic] {seen} parameter gradients: sampled global rel-L2 {g_err:.2e}; worst norm ratio off by "
          f"{worst_norm[1]:.2e} ({worst_norm[0]})")
    assert seen + n_dead == len(G["grad_norms"]) + len(G["dead"]) and n_dead >= 128
    assert g_err < tol_g, f"global gradient rel-L2 {g_err:.3e}"
    assert worst_norm[1] < 4 * tol_g, f"gradient norm of {worst_norm[0]} off by {worst_norm[1]:.3e}"
    # ---- the same step a second time: every gradient, bit for bit ----
    out2, loss2 = step()
    assert torch.equal(out2, out) and torch.equal(loss2, loss)
    again = {n: p.grad for n, p in net.named_parameters() if p.grad is not None}
    assert again.keys() == first.keys()
    bad = [n for n in first if not torch.equal(first[n], again[n])]
    assert not bad, f"{len(bad)} of {len(first)} gradients differ between two identical steps: {bad[:4]}"
