"""GPU: the device-resident optimizer step (include/gcd_amd_train_optim.h; training.AdamHIP with clipping, loss scaling,
decoupled decay, EMA; gcd_amd.ema.LitEma).

Every reference is torch on the CPU with the arithmetic in fp64 (torch.optim.Adam / AdamW, clip_grad_norm_, the three-line
EMA recurrence); results are compared in fp32 at rel-L2 < 1e-6, the bar of test_adam_step_vs_torch.  The tensor set covers
the kernels' branches: sizes 1, 5, 16383, 16384, 16385, 3 * 16384 + 7 and 2 000 000, a view offset by one element (its base
is not 16-byte aligned: the scalar path), more than 48 tensors and more than 256 chunks."""
import io
import math

import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

BAR = 1e-6
CHUNK = 16384
SIZES = [1, 5, 16383, 16384, 16385, 3 * 16384 + 7, 2_000_000, 2_500_000] + [3 + 7 * k for k in range(44)]
OFFSET_VIEW = len(SIZES)            # index of the view offset by one element (16385 elements)
LAST = OFFSET_VIEW                  # the last tensor of the set


class Bag(torch.nn.Module):
    """The tensor set as a module (LitEma wants named parameters)."""

    def __init__(self, tensors):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(t) for t in tensors])


def _values(seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) * scale for n in SIZES + [16385]]


def _bag(values, device):
    """Parameters holding `values` on `device`; the last one is a view one element into a larger allocation."""
    ts = [v.clone().to(device) for v in values[:-1]]
    base = torch.zeros(values[-1].numel() + 1, device=device)
    base[1:].copy_(values[-1])
    ts.append(base[1:])
    bag = Bag(ts)
    assert bag.ps[OFFSET_VIEW].data_ptr() % 16 == 4 or device.type == "cpu"
    assert len(bag.ps) > 48 and sum(-(-p.numel() // CHUNK) for p in bag.ps) > 256
    return bag


def _set_grads(bag, grads, scale=1.0):
    """Gradients into STATIC buffers (allocated once): the table is built once."""
    for p, g in zip(bag.ps, grads):
        if p.grad is None:
            p.grad = torch.empty_like(p)
        p.grad.copy_((g.double() * scale).float())


def _ref_setup(values, cls, **kw):
    ps = [torch.nn.Parameter(v.double().clone()) for v in values]
    return ps, cls(ps, **kw)


def _ema_ref_update(shadows, ps, n, decay32, use_num):
    """LitEma.forward in fp64; `decay32` is the decay as LitEma holds it (an fp32 buffer)."""
    d = decay32
    if use_num:
        n += 1
        d = min(decay32, (1 + n) / (10 + n))
    for s, p in zip(shadows, ps):
        s.sub_((1.0 - d) * (s - p.detach()))
    return n


def _check_all(what, got, want):
    worst = max(rel_l2(a, b.float()) for a, b in zip(got, want))
    print(f"{what}: worst rel-L2 {worst:.3e} (bar {BAR:.0e})")
    assert worst < BAR, what
    return worst


def _moments(opt, k):
    return [s[k] for s in opt.state]


HYPER = dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8)


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_parity_adam_adamw_four_steps(gpu, decoupled, wd):
    """Every option off but the decay kind (Adam with device_state=True IS the new path with every option off), and a
    grad_scale that undoes a static loss scale, as in test_adam_step_vs_torch."""
    from gcd_amd.training import AdamHIP
    vals = _values(1)
    bag = _bag(vals, gpu)
    ref, opt_r = _ref_setup(vals, torch.optim.AdamW if decoupled else torch.optim.Adam, weight_decay=wd, **HYPER)
    opt = AdamHIP(bag.parameters(), weight_decay=wd, decoupled_weight_decay=decoupled, device_state=True, **HYPER)
    for step in range(4):
        grads = _values(100 + step)
        for p, g in zip(ref, grads):
            p.grad = g.double()
        _set_grads(bag, grads, 64.0)
        opt_r.step()
        opt.step(grad_scale=1.0 / 64.0)
    assert opt._table.rebuilds == 1 and opt.launches_per_step == 2
    st = opt.stats()
    assert st["step"] == 4 and st["found_inf"] is False and st["grad_norm"] == -1.0 and st["clip_coef"] == 1.0
    _check_all("p", list(bag.ps), ref)
    _check_all("m", _moments(opt, 0), [opt_r.state[p]["exp_avg"] for p in ref])
    _check_all("v", _moments(opt, 1), [opt_r.state[p]["exp_avg_sq"] for p in ref])


@pytest.mark.parametrize("gscale,clipped", [(1.0, True), (1e-4, False)], ids=["clipped", "not-clipped"])
def test_parity_clipping_and_grad_norm(gpu, gscale, clipped):
    from gcd_amd.training import AdamHIP
    vals = _values(2)
    bag = _bag(vals, gpu)
    max_norm = 1.0
    ref, opt_r = _ref_setup(vals, torch.optim.Adam, **HYPER)
    opt = AdamHIP(bag.parameters(), max_grad_norm=max_norm, **HYPER)
    for step in range(4):
        grads = [g * gscale for g in _values(200 + step)]
        for p, g in zip(ref, grads):
            p.grad = g.double()
        norm_r = float(torch.nn.utils.clip_grad_norm_(ref, max_norm))
        assert (norm_r > max_norm) == clipped
        _set_grads(bag, grads)
        opt_r.step()
        opt.step()
        st = opt.stats()
        print(f"step {step}: grad_norm {st['grad_norm']:.9g} vs fp64 {norm_r:.9g}, clip_coef {st['clip_coef']:.9g}")
        assert abs(st["grad_norm"] / norm_r - 1.0) < BAR
        want_coef = min(1.0, max_norm / (norm_r + 1e-6))
        assert abs(st["clip_coef"] / want_coef - 1.0) < BAR and (st["clip_coef"] < 1.0) == clipped
    assert opt.launches_per_step == 3 and opt._table.rebuilds == 1
    _check_all("p", list(bag.ps), ref)
    _check_all("m", _moments(opt, 0), [opt_r.state[p]["exp_avg"] for p in ref])
    _check_all("v", _moments(opt, 1), [opt_r.state[p]["exp_avg_sq"] for p in ref])


@pytest.mark.parametrize("use_num", [True, False], ids=["num_updates", "fixed-decay"])
def test_parity_ema(gpu, use_num):
    """The fused pass's EMA against the recurrence, and LitEma.forward (gcd_ema_update) on its own against the same."""
    from gcd_amd.ema import LitEma
    from gcd_amd.training import AdamHIP
    vals = _values(3)
    bag = _bag(vals, gpu)
    decay = 0.99
    decay32 = float(torch.tensor(decay, dtype=torch.float32))
    ema = LitEma(bag, decay=decay, use_num_upates=use_num)
    alone = LitEma(bag, decay=decay, use_num_upates=use_num)
    ref, opt_r = _ref_setup(vals, torch.optim.Adam, **HYPER)
    shadows = [v.double().clone() for v in vals]
    n = 0
    opt = AdamHIP(bag.parameters(), ema=ema, **HYPER)
    for step in range(4):
        grads = _values(300 + step)
        for p, g in zip(ref, grads):
            p.grad = g.double()
        _set_grads(bag, grads)
        opt_r.step()
        n = _ema_ref_update(shadows, ref, n, decay32, use_num)
        opt.step()
        alone(bag)
    names = [ema.m_name2s_name[f"ps.{i}"] for i in range(len(bag.ps))]
    _check_all("p", list(bag.ps), ref)
    _check_all("ema (fused pass)", [ema._buffers[s] for s in names], shadows)
    _check_all("ema (gcd_ema_update)", [alone._buffers[s] for s in names], shadows)
    for e in (ema, alone):
        assert all(torch.equal(ema._buffers[s], e._buffers[s]) for s in names)      # the two entries share the arithmetic
        assert int(e.num_updates) == (4 if use_num else -1)
    assert opt.stats()["ema_num_updates"] == (4 if use_num else -1)
    # a parameter whose gradient is None gets the EMA part only
    before = [p.detach().clone() for p in bag.ps]
    bag.ps[3].grad = None
    sh3 = ema._buffers[names[3]].clone()
    opt.step()
    assert torch.equal(bag.ps[3].detach(), before[3]) and not torch.equal(ema._buffers[names[3]], sh3)
    assert not torch.equal(bag.ps[4].detach(), before[4])


def _snapshot(bag, opt, ema=None):
    torch.cuda.synchronize()
    out = {"p": [p.detach().clone() for p in bag.ps], "m": [m.clone() for m in _moments(opt, 0)],
           "v": [v.clone() for v in _moments(opt, 1)], "state": opt._state_block.clone()}
    if ema is not None:
        out["ema"] = [b.clone() for _, b in sorted(ema.named_buffers())]
    return out


def _assert_snap_equal(a, b, what, skip=()):
    for k in a:
        if k in skip:
            continue
        xs, ys = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        bad = [i for i, (x, y) in enumerate(zip(xs, ys)) if not torch.equal(x, y)]
        assert not bad, f"{what}: {k} differs at {bad[:5]}"


_POS = {"first": (0, 0), "last": (LAST, 16384), "scalar-tail": (4, 16384)}      # (tensor, element)


@pytest.mark.parametrize("where", list(_POS))
@pytest.mark.parametrize("bad", [math.inf, -math.inf, math.nan], ids=["+inf", "-inf", "nan"])
def test_overflow_skips_the_step(gpu, bad, where):
    """One non-finite value among the gradients (a float in an input): p, m, v keep their bits, the step count stays, the
    loss scale halves, the EMA moves; the next finite step equals the reference that skipped the same step."""
    from gcd_amd.ema import LitEma
    from gcd_amd.training import AdamHIP
    vals = _values(4)
    bag = _bag(vals, gpu)
    decay32 = float(torch.tensor(0.9999, dtype=torch.float32))
    ema = LitEma(bag)
    ref, opt_r = _ref_setup(vals, torch.optim.Adam, **HYPER)
    shadows = [v.double().clone() for v in vals]
    n = 0
    opt = AdamHIP(bag.parameters(), loss_scale="dynamic", init_scale=1024.0, ema=ema, **HYPER)
    scale = 1024.0
    for step in range(3):
        grads = _values(400 + step)
        overflow = step == 1
        _set_grads(bag, grads, scale)
        if overflow:
            t, i = _POS[where]
            assert i == bag.ps[t].numel() - 1 or (t, i) == (0, 0)
            bag.ps[t].grad[i] = bad
            before = _snapshot(bag, opt, ema)
        else:
            for p, g in zip(ref, grads):
                p.grad = g.double()
            opt_r.step()
        n = _ema_ref_update(shadows, ref, n, decay32, True)
        opt.step()
        st = opt.stats()
        if overflow:
            after = _snapshot(bag, opt, ema)
            _assert_snap_equal(before, after, "skipped step", skip=("state", "ema"))
            assert st["found_inf"] is True and st["step"] == 1 and st["skipped_steps"] == 1
            assert st["loss_scale"] == 512.0 and st["growth_tracker"] == 0
            moved = sum(not torch.equal(x, y) for x, y in zip(before["ema"], after["ema"]))
            assert moved >= len(bag.ps), "the EMA moves on a skipped step"
            scale = 512.0
        else:
            assert st["found_inf"] is False and st["loss_scale"] == scale
    assert opt.stats()["step"] == 2 and opt.stats()["skipped_steps"] == 1 and int(ema.num_updates) == 3
    names = [ema.m_name2s_name[f"ps.{i}"] for i in range(len(bag.ps))]
    _check_all("p", list(bag.ps), ref)
    _check_all("m", _moments(opt, 0), [opt_r.state[p]["exp_avg"] for p in ref])
    _check_all("v", _moments(opt, 1), [opt_r.state[p]["exp_avg_sq"] for p in ref])
    _check_all("ema", [ema._buffers[s] for s in names], shadows)


def test_loss_scale_grows_after_growth_interval(gpu):
    from gcd_amd.training import AdamHIP
    bag = _bag(_values(5), gpu)
    opt = AdamHIP(bag.parameters(), loss_scale="dynamic", init_scale=8.0, growth_interval=3, **HYPER)
    seen = []
    for step in range(7):
        _set_grads(bag, _values(500 + step), opt.stats()["loss_scale"])
        loss = opt.scale(torch.ones((), device=gpu))
        opt.step()
        st = opt.stats()
        seen.append((float(loss), st["loss_scale"], st["growth_tracker"]))
    print(seen)
    assert [s[1] for s in seen] == [8.0, 8.0, 16.0, 16.0, 16.0, 32.0, 32.0]
    assert [s[2] for s in seen] == [1, 2, 0, 1, 2, 0, 1]
    assert [s[0] for s in seen] == [8.0, 8.0, 8.0, 16.0, 16.0, 16.0, 32.0]       # scale(): the scale of THIS step
    assert opt.stats()["step"] == 7


def _full_options(bag, **kw):
    from gcd_amd.ema import LitEma
    from gcd_amd.training import AdamHIP
    ema = LitEma(bag, decay=0.999)
    opt = AdamHIP(bag.parameters(), weight_decay=0.01, decoupled_weight_decay=True, max_grad_norm=1.0,
                  loss_scale="dynamic", init_scale=64.0, growth_interval=2, ema=ema, **HYPER, **kw)
    return opt, ema


def _run_steps(bag, opt, first, count):
    for step in range(first, first + count):
        _set_grads(bag, _values(600 + step), 64.0)
        opt.step(grad_scale=1.0 if step % 2 else 0.5)


def test_same_three_steps_twice_are_bit_equal(gpu):
    snaps = []
    for _ in range(2):
        bag = _bag(_values(6), gpu)
        opt, ema = _full_options(bag)
        _run_steps(bag, opt, 0, 3)
        snaps.append(_snapshot(bag, opt, ema))
    _assert_snap_equal(snaps[0], snaps[1], "two runs")
    assert opt.stats()["step"] == 3


def test_resume_is_bit_equal(gpu):
    """4 steps straight == 2 steps, state_dict -> torch.save -> fresh parameters, optimizer and EMA -> load -> 2 steps."""
    bag = _bag(_values(7), gpu)
    opt, ema = _full_options(bag)
    _run_steps(bag, opt, 0, 4)
    straight = _snapshot(bag, opt, ema)

    bag = _bag(_values(7), gpu)
    opt, ema = _full_options(bag)
    _run_steps(bag, opt, 0, 2)
    buf = io.BytesIO()
    torch.save({"model": bag.state_dict(), "opt": opt.state_dict(), "ema": ema.state_dict()}, buf)
    del bag, opt, ema
    buf.seek(0)
    ck = torch.load(buf)
    bag = _bag(_values(99), gpu)                 # other values: everything must come from the checkpoint
    bag.load_state_dict(ck["model"])
    opt, ema = _full_options(bag)
    ema.load_state_dict(ck["ema"])
    opt.load_state_dict(ck["opt"])
    assert opt.stats()["step"] == 2
    _run_steps(bag, opt, 2, 2)
    resumed = _snapshot(bag, opt, ema)
    _assert_snap_equal(straight, resumed, "resumed run")
    assert opt.stats()["step"] == 4 and opt.stats()["loss_scale"] == 256.0


def test_interop_with_torch_adam_both_ways(gpu):
    from gcd_amd.training import AdamHIP
    vals = _values(8)
    # ours for two steps, then torch continues from our state
    bag = _bag(vals, gpu)
    opt = AdamHIP(bag.parameters(), weight_decay=0.01, device_state=True, **HYPER)
    for step in range(2):
        _set_grads(bag, _values(700 + step))
        opt.step()
    ref = [torch.nn.Parameter(p.detach().double().cpu()) for p in bag.ps]
    opt_r = torch.optim.Adam(ref, lr=0.5)
    buf = io.BytesIO()
    torch.save(opt.state_dict(), buf)
    buf.seek(0)
    opt_r.load_state_dict(torch.load(buf))
    assert opt_r.param_groups[0]["lr"] == HYPER["lr"] and float(opt_r.state[ref[0]]["step"]) == 2.0
    for step in range(2, 4):
        grads = _values(700 + step)
        for p, g in zip(ref, grads):
            p.grad = g.double()
        _set_grads(bag, grads)
        opt_r.step()
        opt.step()
    _check_all("torch continues from ours: p", list(bag.ps), ref)
    _check_all("torch continues from ours: v", _moments(opt, 1), [opt_r.state[p]["exp_avg_sq"] for p in ref])
    # torch for two steps, then ours continues from torch's state (both modes of AdamHIP)
    ref, opt_r = _ref_setup(vals, torch.optim.Adam, weight_decay=0.01, **HYPER)
    for step in range(2):
        for p, g in zip(ref, _values(800 + step)):
            p.grad = g.double()
        opt_r.step()
    mine = []
    for device_state in (True, False):
        bag = _bag([p.detach().float() for p in ref], gpu)
        opt = AdamHIP(bag.parameters(), lr=0.5, device_state=device_state)
        opt.load_state_dict(opt_r.state_dict())
        assert opt.stats()["step"] == 2 and opt.weight_decay == 0.01
        mine.append((bag, opt))
    for step in range(2, 4):
        grads = _values(800 + step)
        for p, g in zip(ref, grads):
            p.grad = g.double()
        opt_r.step()
        for bag, opt in mine:
            _set_grads(bag, grads)
            opt.step()
    for (bag, opt), mode in zip(mine, ("device state", "default path")):
        _check_all(f"ours ({mode}) continues from torch: p", list(bag.ps), ref)
        _check_all(f"ours ({mode}) continues from torch: m", _moments(opt, 0), [opt_r.state[p]["exp_avg"] for p in ref])


def test_captured_step_replays_equal_eager(gpu):
    """gradstat + apply captured on one stream after one eager step, replayed for 3 steps with gradients copied into the
    static buffers and set_lr between the replays: equal to the eager run — the step neither synchronises nor rebuilds."""
    bag_e = _bag(_values(9), gpu)
    opt_e, ema_e = _full_options(bag_e)
    _set_grads(bag_e, _values(900), 64.0)
    opt_e.step(grad_scale=0.5)
    for step in range(1, 4):
        opt_e.set_lr(HYPER["lr"] * (1.0 - 0.1 * step))
        _set_grads(bag_e, _values(900 + step), 64.0)
        opt_e.step(grad_scale=0.5)
    eager = _snapshot(bag_e, opt_e, ema_e)
    # captured: step 1 runs as the first replay, with the lr of step 1
    bag = _bag(_values(9), gpu)
    opt, ema = _full_options(bag)
    _set_grads(bag, _values(900), 64.0)
    opt.step(grad_scale=0.5)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step(grad_scale=0.5)
    assert opt._table.rebuilds == 1
    for step in range(1, 4):
        opt.set_lr(HYPER["lr"] * (1.0 - 0.1 * step))
        _set_grads(bag, _values(900 + step), 64.0)
        graph.replay()
    captured = _snapshot(bag, opt, ema)
    _assert_snap_equal(eager, captured, "captured vs eager")
    assert opt.stats()["step"] + opt.stats()["skipped_steps"] == 4
    # a table that would change inside a capture is refused
    bag.ps[2].grad = torch.zeros_like(bag.ps[2])
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2):
        bag.ps[0].grad.mul_(1.0)             # (the capture holds one node whatever happens next)
        with pytest.raises(RuntimeError, match="inside a stream capture"):
            opt.step()


# ----------------------------------------------------------------------------------------------------- the tiny VideoUNet
def _tiny_sampler_out(net, gpu, steps=3):
    from gcd_amd.denoiser import Denoiser
    from gcd_amd.sampling import EulerEDMSampler, FusedDenoiser
    from gcd_amd.wrappers import OpenAIWrapper
    from oracle import svd_unet_ref as O, weights
    cfg = O.TINY
    T, h, w = 14, 16, 16
    noise, c, uc = weights.synth_inputs(1, T, h, w, cfg.context_dim, cfg.adm_in_channels + cfg.aux_emb_dim, seed=61)
    sampler = EulerEDMSampler(
        discretization_config={"target": "gcd_amd.discretizer.EDMDiscretization", "params": {"sigma_max": 700.0}},
        num_steps=steps,
        guider_config={"target": "gcd_amd.guiders.LinearPredictionGuider",
                       "params": {"num_frames": T, "max_scale": 1.5, "min_scale": 1.0}},
        device="cuda")
    fd = FusedDenoiser(Denoiser({"target": "gcd_amd.denoiser_scaling.VScalingWithEDMcNoise"}), OpenAIWrapper(net),
                       num_video_frames=T, image_only_indicator=torch.zeros(2, T, device=gpu))
    out = sampler(fd, noise.clone().to(gpu), cond={k: v.to(gpu) for k, v in c.items()},
                  uc={k: v.to(gpu) for k, v in uc.items()})
    torch.cuda.synchronize()
    return out.detach().clone()


def _tiny_planned_out(net, s):
    from gcd_amd.train_plan import unet_forward_planned
    out = unet_forward_planned(net, s["x"], s["ts"], s["ctx"], s["y"], s["T"], s["ioi"], use_checkpoint=False)
    torch.cuda.synchronize()
    return out.detach().clone()


def test_ema_scope_switches_the_weights_every_engine_sees(gpu):
    """Inside the scope the sampler and the planned engine compute what a network holding the EMA weights as parameters
    computes; after it, what the training weights give.  Fails when copy_to / restore forget invalidate() / PACK.clear()."""
    import test_train_plan_gpu as TPT
    from gcd_amd.ema import LitEma, ema_scope
    net = TPT._tiny(gpu, salt=5)
    ema = LitEma(net)
    g = torch.Generator().manual_seed(77)
    with torch.no_grad():
        for name, p in net.named_parameters():           # EMA weights that differ from the training weights
            s = ema._buffers[ema.m_name2s_name[name]]
            s.mul_(0.9).add_((torch.randn(p.shape, generator=g) * 0.01).to(gpu))
    net_ema = TPT._tiny(gpu, salt=5)
    with torch.no_grad():
        for name, p in net_ema.named_parameters():
            p.copy_(ema._buffers[ema.m_name2s_name[name]])
    s = TPT._tiny_step_inputs(gpu, 41)
    train_out = (_tiny_sampler_out(net, gpu), _tiny_planned_out(net, s))        # (warms every packed-weight cache)
    ema_out = (_tiny_sampler_out(net_ema, gpu), _tiny_planned_out(net_ema, s))
    assert not torch.equal(train_out[0], ema_out[0]) and not torch.equal(train_out[1], ema_out[1])
    with ema_scope(net, ema):
        inside = (_tiny_sampler_out(net, gpu), _tiny_planned_out(net, s))
    after = (_tiny_sampler_out(net, gpu), _tiny_planned_out(net, s))
    for k, what in enumerate(("sampler", "planned engine")):
        assert torch.equal(inside[k], ema_out[k]), f"{what}: inside the scope, rel-L2 {rel_l2(inside[k], ema_out[k]):.2e}"
        assert torch.equal(after[k], train_out[k]), f"{what}: after the scope, rel-L2 {rel_l2(after[k], train_out[k]):.2e}"


def test_tiny_finetune_run_resumed_after_step_one_is_bit_equal(gpu):
    """Three fine-tune steps of the tiny network with GCD_TRAIN_DETERMINISTIC semantics, dynamic loss scaling, clipping and
    EMA; saved after step 1 and resumed in fresh objects: bit-equal to the uninterrupted run."""
    import test_backward_gpu as TB
    import test_train_plan_gpu as TPT
    from gcd_amd import autograd_ops as A, training as TR
    from gcd_amd.ema import LitEma
    from oracle import svd_unet_ref as O
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
    draws = [(torch.randn(BT, generator=g), torch.randn(BT, 4, H, W, generator=g)) for _ in range(3)]
    den = TR.TrainDenoiser({"target": "gcd_amd.denoiser_scaling.VScalingWithEDMcNoise"}, deterministic=True)
    loss_fn = TR.StandardDiffusionLoss(
        sigma_sampler_config={"target": "gcd_amd.training.EDMSampling", "params": {"p_mean": 1.0, "p_std": 1.6}},
        loss_weighting_config={"target": "gcd_amd.training.EDMWeighting", "params": {"sigma_data": 1.0}},
        focus_top=0.1, focus_steps=5000, batch2model_keys=["image_only_indicator", "num_video_frames"])

    def make(salt):
        net = TPT._tiny(gpu, salt=salt)
        ema = LitEma(net, decay=0.999)
        opt = TR.AdamHIP(net.parameters(), lr=1e-4, max_grad_norm=1.0, loss_scale="dynamic", init_scale=256.0,
                         growth_interval=2, ema=ema)
        return net, ema, opt

    def steps(net, opt, which):
        for k in which:
            opt.zero_grad()
            sig = loss_fn.sigma_sampler(BT, rand=draws[k][0]).reshape(B, T)[:, :1].expand(B, T).reshape(-1).to(gpu)
            noise = draws[k][1].to(gpu)
            out = den(net, x0 + noise * sig[:, None, None, None], sig, cond, num_video_frames=T, image_only_indicator=ioi)
            loss = loss_fn.get_loss(out, x0, loss_fn.loss_weighting(sig)[:, None, None, None], {"global_step": 2500 + k}).mean()
            opt.scale(loss).backward()
            opt.step()

    def snap(net, ema, opt):
        torch.cuda.synchronize()
        return {"w": [v.detach().clone() for _, v in sorted(net.state_dict().items())],
                "ema": [v.clone() for _, v in sorted(ema.state_dict().items())],
                "m": [m.clone() for m, _ in opt.state], "v": [v.clone() for _, v in opt.state],
                "state": opt._state_block.clone()}

    old = A.DETERMINISTIC
    try:
        A.PACK.clear()
        net, ema, opt = make(3)
        w0 = [v.detach().clone() for _, v in sorted(net.state_dict().items())]
        steps(net, opt, [0, 1, 2])
        straight = snap(net, ema, opt)
        st = opt.stats()
        print(f"uninterrupted run: {st}")
        assert st["step"] + st["skipped_steps"] == 3 and st["step"] >= 2 and st["ema_num_updates"] == 3
        assert math.isfinite(st["grad_norm"]) and st["grad_norm"] > 0.0
        assert sum(not torch.equal(a, b) for a, b in zip(w0, straight["w"])) > 100

        A.PACK.clear()
        net, ema, opt = make(3)
        steps(net, opt, [0])
        buf = io.BytesIO()
        torch.save({"model": net.state_dict(), "opt": opt.state_dict(), "ema": ema.state_dict()}, buf)
        del net, ema, opt
        buf.seek(0)
        ck = torch.load(buf)
        A.PACK.clear()
        net, ema, opt = make(4)                   # other weights: everything must come from the checkpoint
        net.load_state_dict(ck["model"])
        ema.load_state_dict(ck["ema"])
        opt.load_state_dict(ck["opt"])
        steps(net, opt, [1, 2])
        resumed = snap(net, ema, opt)
    finally:
        A.set_deterministic(old)
    for k in straight:
        bad = [i for i, (a, b) in enumerate(zip(straight[k], resumed[k])) if not torch.equal(a, b)] \
            if isinstance(straight[k], list) else ([] if torch.equal(straight[k], resumed[k]) else [0])
        assert not bad, f"{k}: {len(bad)} tensors differ between the uninterrupted and the resumed run: {bad[:5]}"
