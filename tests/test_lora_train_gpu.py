"""GPU: ft_strategy `time_lora` end to end (gcd_amd/lora.py) on the TINY VideoUNet, 2 clips x 4 frames of 16 x 16 latents,
loss scale 64: both training engines and the inference engine run on the MERGED weights, the adapter gradients are the
projections of the engines' own dW.  The reference is the CPU oracle (oracle.svd_unet_ref.unet_forward) with
sd[name] = W0 + s B @ A built from leaf A, B, so torch.autograd gives the reference dA, dB (and dW of the merged weights).

GOLDEN_MEASURED (MI355X; relative L2 against the oracle, adapter gradients as ONE vector, beside the bar each is held to):
the table in the docstring of test_adapter_gradients_vs_oracle.  8 Adam steps on a fixed batch: loss 1.46685 -> 1.34479.
Accumulation, projected once, against the sum of two projections: worst tensor 5.6e-7.  Graph mode against eager over five
steps: outputs bit-identical, worst adapter gradient below 1e-6."""
import math

import pytest
import torch

from conftest import rel_l2
from oracle import svd_unet_ref as O, weights

pytestmark = pytest.mark.gpu

T, H, W, CLIPS = 4, 16, 16, 2
LOSS_SCALE = 64.0
U = 2.0 ** -24
_REF = {}


def _tiny(gpu, salt):
    from gcd_amd.video_model import VideoUNet
    with torch.device("meta"):
        net = VideoUNet(**O.TINY.as_reference_kwargs())
    sd = weights.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, salt)
    net = net.to_empty(device=gpu)
    net.load_state_dict(sd)
    return net.train(), sd


def _batch(seed, h=H, w=W):
    cfg = O.TINY
    g = torch.Generator().manual_seed(seed)
    n = CLIPS * T
    ioi = torch.zeros(CLIPS, T)
    ioi[1, 2] = 1.0
    return dict(x=torch.randn(n, 8, h, w, generator=g), ts=torch.linspace(-1.0, 1.5, n),
                ctx=torch.randn(n, 1, cfg.context_dim, generator=g),
                y=torch.randn(n, cfg.adm_in_channels + cfg.aux_emb_dim, generator=g).clamp(-1, 1), ioi=ioi,
                tgt=torch.randn(n, 4, h, w, generator=g))


def _to(b, gpu):
    return {k: v.to(gpu) for k, v in b.items()}


def _seed_b(lora, seed):
    """B away from zero (after the initialisation every dA would be zero), then the merge that has to follow."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for b in lora.lora_B:
            b.copy_((torch.randn(b.shape, generator=g) * 0.3).to(b.device))
    lora.merge()


def _forward(engine, net, b, ckpt=True):
    from gcd_amd import training as TR
    from gcd_amd.train_plan import unet_forward_planned
    fn = unet_forward_planned if engine == "planned" else TR.unet_forward_train
    return fn(net, b["x"], b["ts"], b["ctx"], b["y"], T, b["ioi"], use_checkpoint=ckpt)


def _backward(engine, net, b):
    out = _forward(engine, net, b)
    loss = ((out - b["tgt"]) ** 2).mean()
    (loss * LOSS_SCALE).backward()
    return out.detach(), float(loss.detach())


def _infer(net, b):
    with torch.no_grad():
        return net(b["x"], b["ts"], b["ctx"], b["y"], num_video_frames=T, image_only_indicator=b["ioi"]).clone()


def _setup(gpu, salt=11, seed_a=4, seed_b=6):
    from gcd_amd import autograd_ops as A, lora as L
    A.PACK.clear()
    net, sd = _tiny(gpu, salt)
    lora = L.TimeLora(net, generator=torch.Generator().manual_seed(seed_a))
    _seed_b(lora, seed_b)
    return net, sd, lora


def _reference(salt=11, seed_a=4, seed_b=6, batch_seed=21):
    """The oracle's output and dA, dB, dW for the adapters that _setup seeds; computed once."""
    key = (salt, seed_a, seed_b, batch_seed)
    if key in _REF:
        return _REF[key]
    from gcd_amd import lora as L
    from gcd_amd.video_model import VideoUNet
    with torch.device("meta"):
        meta = VideoUNet(**O.TINY.as_reference_kwargs())
    sd = weights.synth_state_dict({k: tuple(v.shape) for k, v in meta.state_dict().items()}, salt)
    names = [n for n, _ in L.adaptable_layers(meta)]
    ga, gb = torch.Generator().manual_seed(seed_a), torch.Generator().manual_seed(seed_b)
    As, Bs, Ws = [], [], []
    sdr = dict(sd)
    for n in names:                 # the same draws, in the same order, as TimeLora.__init__ and _seed_b
        N, K = sd[n + ".weight"].shape
        bound = 1.0 / math.sqrt(K)
        As.append(torch.empty(16, K).uniform_(-bound, bound, generator=ga).requires_grad_(True))
    for n in names:
        N, K = sd[n + ".weight"].shape
        Bs.append((torch.randn(N, 16, generator=gb) * 0.3).requires_grad_(True))
    for n, a, bb in zip(names, As, Bs):
        wm = sd[n + ".weight"] + (1.0 / 16) * (bb @ a)
        wm.retain_grad()
        Ws.append(wm)
        sdr[n + ".weight"] = wm
    b = _batch(batch_seed)
    out = O.unet_forward(sdr, O.TINY, b["x"], b["ts"], b["ctx"], b["y"], T, b["ioi"])
    ((out - b["tgt"]) ** 2).mean().backward()
    _REF[key] = dict(names=names, out=out.detach(), dA=[a.grad for a in As], dB=[x.grad for x in Bs], dW=[w.grad for w in Ws],
                     A=[a.detach() for a in As], B=[x.detach() for x in Bs])
    return _REF[key]


def _cat(ts):
    return torch.cat([t.detach().double().cpu().reshape(-1) for t in ts])


def test_attach_is_a_no_op_and_unmerge_restores(gpu):
    """B = 0: the planned forward and the inference forward are bit-identical to the un-attached network's; after adapters
    with B != 0 were merged, unmerge() brings the original output back bit for bit."""
    from gcd_amd import autograd_ops as A, lora as L
    A.PACK.clear()
    net, sd = _tiny(gpu, 11)
    b = _to(_batch(21), gpu)
    with torch.no_grad():
        plan0 = _forward("planned", net, b).clone()
    inf0 = _infer(net, b)
    lora = L.TimeLora(net, generator=torch.Generator().manual_seed(4))
    for n, p in net.state_dict().items():
        assert torch.equal(p.cpu().view(torch.int32) if p.dtype == torch.float32 else p.cpu(),
                           sd[n].view(torch.int32) if p.dtype == torch.float32 else sd[n]), n
    with torch.no_grad():
        plan1 = _forward("planned", net, b).clone()
    assert torch.equal(plan1, plan0) and torch.equal(_infer(net, b), inf0)
    _seed_b(lora, 6)
    inf2 = _infer(net, b)
    assert rel_l2(inf2, inf0) > 1e-3, "the merged adapters must be visible to the inference engine"
    lora.unmerge()
    assert torch.equal(_infer(net, b), inf0)
    with torch.no_grad():
        assert torch.equal(_forward("planned", net, b), plan0)
    assert all(p.requires_grad for p in net.parameters())


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("engine", ["planned", "autograd"])
def test_adapter_gradients_vs_oracle(gpu, engine, dtype):
    """Output: 5e-3 with fp16 operands, the planned-engine tests' bar.  With bf16 operands the output is printed, not
    held to a bar: the issue asks for bf16 on the adapter-gradient rule only, and the output's distance from the fp32 oracle
    is the engines' operand rounding (bf16 keeps 8 significant bits where fp16 keeps 11), whatever the adapters do.
    Adapter gradients, all of dA and dB as one vector, for both operand types:
    max(5e-3, 2 x the relative L2 that THIS run's dW of the adapted layers has against the oracle's dW) — dW is the
    engines' existing code, and the projection is exact in fp32 up to summation rounding.  Adapters of layers the backward
    pass never reaches (attn2.to_q / to_k of every temporal block, behind the one-key cross-attention) get exactly zero,
    as the oracle's do.  Every frozen parameter keeps grad None.

    GOLDEN_MEASURED   engine    dtype   output (bar)       dW        dA|dB as one vector (bar)
                      planned   fp16    1.25e-3 (5e-3)     1.47e-3   1.44e-3 (5.00e-3)
                      autograd  fp16    1.33e-3 (5e-3)     1.59e-3   1.56e-3 (5.00e-3)
                      planned   bf16    1.01e-2 (none)     1.19e-2   1.16e-2 (2.39e-2)
                      autograd  bf16    1.07e-2 (none)     1.34e-2   1.31e-2 (2.68e-2)
    (bf16 / fp16 = 8.1 on the output: the ratio of the formats' roundoff.)"""
    from gcd_amd import autograd_ops as A
    ref = _reference()
    A.set_train_dtype(dtype)
    try:
        net, _, lora = _setup(gpu)
        assert lora.names == ref["names"]
        for a, ar, bb, br in zip(lora.lora_A, ref["A"], lora.lora_B, ref["B"]):
            assert torch.equal(a.detach().cpu(), ar) and torch.equal(bb.detach().cpu(), br)
        b = _to(_batch(21), gpu)
        out, _ = _backward(engine, net, b)
        lora.project_grads()
        torch.cuda.synchronize()
    finally:
        A.set_train_dtype("fp16")
        A.PACK.clear()
    adapted = {id(w) for w in lora.weights()}
    for n, p in net.named_parameters():
        assert (id(p) in adapted) == p.requires_grad, n
        if id(p) not in adapted:
            assert p.grad is None, n
    e_out = rel_l2(out, ref["out"])
    live = [i for i, g in enumerate(ref["dW"]) if float(g.abs().max()) > 0]
    dead = [i for i in range(len(ref["names"])) if i not in live]
    got_dw = [lora.weights()[i].grad / LOSS_SCALE for i in live]
    e_dw = float((_cat(got_dw) - _cat([ref["dW"][i] for i in live])).norm() / _cat([ref["dW"][i] for i in live]).norm())
    got = _cat([a.grad / LOSS_SCALE for a in lora.lora_A] + [x.grad / LOSS_SCALE for x in lora.lora_B])
    want = _cat(ref["dA"] + ref["dB"])
    e_ad = float((got - want).norm() / want.norm())
    bar = max(5e-3, 2 * e_dw)
    print(f"[{engine}, {dtype}] output {e_out:.2e} (bar {'5e-3' if dtype == 'fp16' else 'none'}); dW of {len(live)} adapted layers {e_dw:.2e}; "
          f"dA|dB as one vector {e_ad:.2e} (bar {bar:.2e}); {len(dead)} layers unreached")
    assert dtype != "fp16" or e_out < 5e-3
    assert e_ad <= bar
    # the layers the graph never reaches: to_q / to_k of the temporal blocks' attn2, nothing else, zeros on both sides
    assert dead and all(ref["names"][i].endswith(("attn2.to_q", "attn2.to_k")) for i in dead)
    assert sorted(ref["names"][i] for i in dead) == sorted(n for n in ref["names"] if n.endswith(("attn2.to_q", "attn2.to_k")))
    for i in dead:
        assert float(ref["dA"][i].abs().max()) == 0.0 and float(ref["dB"][i].abs().max()) == 0.0
        assert float(lora.lora_A[i].grad.abs().max()) == 0.0 and float(lora.lora_B[i].grad.abs().max()) == 0.0, ref["names"][i]


def test_eight_adam_steps_train_only_the_adapters(gpu):
    """8 AdamHIP steps on a fixed batch: the loss goes down; every tensor of the network outside the adapted weights and
    every W0 keep their bits; the live weights are W0 + s B A within the summation bound ((r + 3) u / (1 - (r + 3) u) of
    |W0| + s |B| |A|, elementwise); a fresh VideoUNet loaded with the merged weights read back from the device gives the
    bit-identical inference output — the inference engine had packed the old weights before the first step."""
    from gcd_amd import training as TR
    from gcd_amd.ema import LitEma
    from gcd_amd.video_model import VideoUNet
    net, sd, lora = _setup(gpu)
    b = _to(_batch(21), gpu)
    stale = _infer(net, b)                       # the inference engine packs the weights of before the training
    w0_before = [w.clone() for w in lora.w0()]
    adapted = {n + ".weight" for n in lora.names}
    ema = LitEma(lora)
    assert len(ema.m_name2s_name) == 2 * len(lora.names)
    opt = TR.AdamHIP(lora.parameters(), lr=1e-3)
    assert len(opt.params) == 2 * len(lora.names)
    losses = []
    for _ in range(8):
        opt.zero_grad()
        _, loss = _backward("planned", net, b)
        losses.append(loss)
        for n, p in net.named_parameters():
            assert n in adapted or p.grad is None, n
        lora.step(opt, grad_scale=1.0 / LOSS_SCALE)
        assert all(w.grad is None for w in lora.weights())
    with torch.no_grad():
        final = float(((_forward("planned", net, b) - b["tgt"]) ** 2).mean())
    torch.cuda.synchronize()
    print("losses", " ".join(f"{v:.5f}" for v in losses), f"-> {final:.5f}")
    assert final < losses[0]
    live = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    for k, v in live.items():
        if k not in adapted:
            assert torch.equal(v, sd[k]), k
    gam = (16 + 3) * U / (1 - (16 + 3) * U)
    moved = 0
    for n, w0, w0b, a, bb in zip(lora.names, lora.w0(), w0_before, lora.lora_A, lora.lora_B):
        assert torch.equal(w0, w0b) and torch.equal(w0.cpu(), sd[n + ".weight"]), n
        w0d, ad, bd = w0.double().cpu(), a.detach().double().cpu(), bb.detach().double().cpu()
        want = w0d + (1.0 / 16) * (bd @ ad)
        bound = gam * (w0d.abs() + (1.0 / 16) * (bd.abs() @ ad.abs()))
        assert bool(((live[n + ".weight"].double() - want).abs() <= bound).all()), n
        moved += int((live[n + ".weight"] != sd[n + ".weight"]).any())
    assert moved == len(lora.names)
    after = _infer(net, b)
    assert rel_l2(after, stale) > 1e-4, "8 steps must have changed the output"
    with torch.device("meta"):
        fresh = VideoUNet(**O.TINY.as_reference_kwargs())
    fresh = fresh.to_empty(device=gpu)
    fresh.load_state_dict(live)
    assert torch.equal(_infer(fresh.train(), b), after)
    ema(lora)                                     # the reference's EMA call over the adapters alone


def test_gradient_accumulation_projected_once(gpu):
    """Two micro-batches without a zero_grad in between, one projection: the sum of the two batches' own projections, at
    the existing accumulation test's bar (1e-3 per tensor)."""
    net, _, lora = _setup(gpu, salt=13)
    b1, b2 = _to(_batch(51, 8, 8), gpu), _to(_batch(52, 8, 8), gpu)
    sep = []
    for b in (b1, b2):
        lora.zero_grad()
        _backward("planned", net, b)
        lora.project_grads()
        sep.append([p.grad.clone() for p in lora.parameters()])
    lora.zero_grad()
    assert all(w.grad is None for w in lora.weights())
    _backward("planned", net, b1)
    _backward("planned", net, b2)
    lora.project_grads()
    torch.cuda.synchronize()
    worst, n = 0.0, 0
    for p, g1, g2 in zip(lora.parameters(), *sep):
        want = g1 + g2
        if float(want.abs().max()) > 0:
            worst = max(worst, rel_l2(p.grad, want))
            n += 1
    print(f"accumulated, projected once vs the sum of two projections: worst of {n} tensors {worst:.1e}")
    assert n > 400 and worst < 1e-3


def test_project_refuses_adapters_that_were_not_merged(gpu):
    from gcd_amd._lib import GcdError
    net, _, lora = _setup(gpu)
    b = _to(_batch(21), gpu)
    _backward("planned", net, b)
    with torch.no_grad():
        lora.lora_B[3].mul_(1.5)
    with pytest.raises(GcdError):
        lora.project_grads()
    lora.merge()
    lora.project_grads()
    torch.cuda.synchronize()


class _Nudge:
    """A stand-in optimizer with a fixed trajectory (Adam's first steps are lr * sign(g): a last-bit difference of a
    gradient becomes a different trajectory, which is not what the comparison below is about)."""

    def __init__(self, params, gpu):
        self.params, self.g = list(params), torch.Generator(device=gpu).manual_seed(5)

    def step(self):
        with torch.no_grad():
            for p in self.params:
                p.data.view(-1).add_(torch.randn(p.numel(), generator=self.g, device=p.device) * 0.02 * float(p.data.std()))


def test_lora_step_under_hipgraphs_matches_eager(gpu):
    """GCD_TRAIN_GRAPH=1: five LoRA steps with fresh inputs.  The merge writes the weights through raw pointers between
    replays; the captured forward re-packs them, the captured backward writes dW where project_grads reads it.  Outputs
    and adapter gradients equal the eager run's at the bars of test_planned_engine_under_hipgraphs_matches_eager."""
    from gcd_amd import train_plan as TP
    batches = [_to(_batch(60 + i), gpu) for i in range(5)]
    for bt in batches:
        bt["ioi"] = torch.zeros(CLIPS, T, device=gpu)
    runs = {}
    for graph in (False, True):
        TP.set_use_graph(graph)
        try:
            net, _, lora = _setup(gpu, salt=7)
            opt = _Nudge(lora.parameters(), gpu)
            outs = []
            for bt in batches:
                lora.zero_grad()
                out, _ = _backward("planned", net, bt)
                lora.project_grads()
                outs.append((out.clone(), [p.grad.clone() for p in lora.parameters()]))
                lora.step(opt)
            torch.cuda.synchronize()
            if graph:
                assert TP.plan_for(net).graphed.mode == "graph", "the steps after the warm-up must have been replays"
            runs[graph] = outs
        finally:
            TP.set_use_graph(False)
    for i, ((oe, ge), (og, gg)) in enumerate(zip(runs[False], runs[True])):
        e = rel_l2(og, oe)
        worst = max(rel_l2(a, b_) for a, b_ in zip(gg, ge) if float(b_.abs().max()) > 0)
        print(f"step {i}: graph vs eager output {e:.1e}, worst adapter gradient {worst:.1e}")
        assert e < 1e-4 and worst < 2e-3
