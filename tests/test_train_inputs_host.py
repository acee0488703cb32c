"""Host: the input-gradient switch of the planned fine-tune engine (train_plan.set_input_grads, GCD_TRAIN_INPUT_GRADS, the
`input_grads` keyword), the golden the GPU tests compare with (tests/golden/train_inputs_tiny.pt), and GradBucketer with
parameters outside the UNet (a trainable conditioner's).  The gradients themselves: tests/test_train_inputs_gpu.py."""
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.distributed as dist

import gloo_util

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "train_inputs_tiny.pt"


def test_switch_setter_and_keyword_precedence():
    from gcd_amd import train_plan as TP
    old = TP.INPUT_GRADS
    try:
        TP.set_input_grads(False)
        assert TP.INPUT_GRADS is False
        assert TP.input_grads_on() is False and TP.input_grads_on(None) is False
        assert TP.input_grads_on(True) is True            # the keyword wins over the module setting ...
        TP.set_input_grads(True)
        assert TP.INPUT_GRADS is True and TP.input_grads_on() is True
        assert TP.input_grads_on(False) is False          # ... in both directions
        TP.set_input_grads(0)
        assert TP.INPUT_GRADS is False
    finally:
        TP.set_input_grads(old)


@pytest.mark.parametrize("value,want", [(None, False), ("1", True), ("0", False)])
def test_switch_environment_variable(value, want):
    """Read once, at import: GCD_TRAIN_INPUT_GRADS=1 turns the switch on, 0 or nothing leaves it off."""
    env = {k: v for k, v in os.environ.items() if k != "GCD_TRAIN_INPUT_GRADS"}
    if value is not None:
        env["GCD_TRAIN_INPUT_GRADS"] = value
    out = subprocess.run([sys.executable, "-c", "from gcd_amd import train_plan as TP; print(TP.INPUT_GRADS)"],
                         cwd=ROOT, env=env, capture_output=True, text=True, check=True).stdout.strip()
    assert out == str(want)


def test_switch_is_off_by_default_and_threaded_through_the_denoiser():
    import inspect
    from gcd_amd import train_plan as TP, training as TR
    if "GCD_TRAIN_INPUT_GRADS" not in os.environ:
        assert TP.INPUT_GRADS is False
    sig = inspect.signature(TP.unet_forward_planned)
    assert sig.parameters["input_grads"].default is None and sig.parameters["use_checkpoint"].default is None
    scaling = {"target": "gcd_amd.denoiser_scaling.VScalingWithEDMcNoise"}
    assert TR.TrainDenoiser(scaling).input_grads is None
    assert TR.TrainDenoiser(scaling, input_grads=True).input_grads is True
    with pytest.raises(ValueError):
        TR.TrainDenoiser(scaling, input_grads="on")
    # the denoiser hands its setting to the planned entry (and only to it: the tape engine has no such keyword)
    seen = {}

    def fake(unet, x, ts, ctx, y, T, ioi, **kw):
        seen.update(kw)
        return x[:, :4]
    old = TP.unet_forward_planned
    TP.unet_forward_planned = fake
    try:
        den = TR.TrainDenoiser(scaling, use_checkpoint=True, engine="planned", input_grads=True)
        x = torch.randn(2, 4, 4, 4)
        den(torch.nn.Identity(), x, torch.ones(2), {"crossattn": None, "vector": None}, num_video_frames=2,
            image_only_indicator=None)
    finally:
        TP.unet_forward_planned = old
    assert seen == {"use_checkpoint": True, "input_grads": True}


def test_golden_keys_and_shapes():
    from oracle import svd_unet_ref as O
    from gcd_amd.video_model import VideoUNet
    cfg = O.TINY
    g = torch.load(GOLDEN, map_location="cpu", weights_only=True)
    assert GOLDEN.stat().st_size < (1 << 20) // 2
    clips, T, h, w = g["clips"], g["T"], g["h"], g["w"]
    assert (g["config"], clips, T, h, w) == ("TINY", 2, 3, 8, 8) and isinstance(g["input_seed"], int)
    n = clips * T
    vec = cfg.adm_in_channels + cfg.aux_emb_dim
    assert cfg.aux_emb_dim > 0
    want = {"x": (n, 8, h, w), "ts": (n,), "context": (n, 1, cfg.context_dim), "y": (n, vec), "ioi": (clips, T),
            "target": (n, 4, h, w)}
    assert {k: tuple(v.shape) for k, v in g["inputs"].items()} == want
    assert tuple(g["out"].shape) == (n, 4, h, w)
    for k in ("x", "context", "y"):
        gr = g[k + "_grad"]
        assert tuple(gr.shape) == want[k] and gr.dtype == torch.float32
        assert bool(torch.isfinite(gr).all()) and float(gr.abs().max()) > 0
    # every frame's context row has a gradient; each clip's first frame carries the temporal cross-attention's too
    assert all(float(r.norm()) > 0 for r in g["context_grad"].reshape(n, -1))
    # one row of samples and one norm per parameter of the network, in registration order
    with torch.device("meta"):
        net = VideoUNet(**cfg.as_reference_kwargs())
    names = [k for k, _ in net.named_parameters()]
    assert g["param_names"] == names
    assert tuple(g["param_grad_samples"].shape) == (len(names), 32) and tuple(g["param_grad_norms"].shape) == (len(names),)
    # behind the one-key cross-attention (softmax over one key = 1) the gradients of to_q / to_k / norm2 are zero: the
    # reference's autograd reaches them with rounding noise, ten orders below the others
    norms = dict(zip(names, g["param_grad_norms"].tolist()))
    dead = [k for k in names if ".attn2.to_q." in k or ".attn2.to_k." in k or ".norm2." in k]
    assert dead and all(0 <= norms[k] < 1e-7 for k in dead)
    # (so are, at 8 x 8 latents, the middle block's spatial attn1.to_q / to_k: one token per frame there)
    live = [k for k in names if k not in set(dead) and not (k.startswith("middle_block.1.transformer_blocks.") and ".attn1.to_" in k)]
    assert all(norms[k] > 1e-6 for k in live)
    assert float(g["loss"]) > 0


class _ListenerNet(torch.autograd.Function):
    """What `_PlannedUNet` is to autograd and to GradBucketer: one node that writes its parameters' .grad ITSELF and tells
    their listeners inside backward(), and returns a gradient for its input — which the parameters upstream (the
    conditioner's) then receive from torch, after this backward has returned."""
    params = ()          # (w1, w2) as the Parameter objects the listeners hang on

    @staticmethod
    def forward(ctx, x, w1, w2):
        ctx.save_for_backward(x, w1, w2)
        return torch.tanh(x @ w1.t()) @ w2.t()

    @staticmethod
    def backward(ctx, dy):
        x, w1, w2 = ctx.saved_tensors
        h = torch.tanh(x @ w1.t())
        dh = (dy @ w2) * (1 - h * h)
        for p, g in ((_ListenerNet.params[1], dy.t() @ h), (_ListenerNet.params[0], dh.t() @ x)):
            p.grad = g
            for fn in tuple(p.__dict__.get("_gcd_grad_listeners", ())):
                fn(p)
        return dh @ w1, None, None


def _outside_worker(rank, world, store, q):
    from gcd_amd.training import GradBucketer, allreduce_gradients
    gloo_util.init(rank, world, store)
    try:
        torch.manual_seed(0)
        emb = torch.nn.Linear(13, 16)                               # the trainable embedder: ordinary autograd leaves
        w1 = torch.nn.Parameter(torch.randn(64, 16) * 0.2)          # the "UNet": gradients through the listener interface
        w2 = torch.nn.Parameter(torch.randn(4, 64) * 0.2)
        unet_params, params = [w1, w2], [w1, w2] + list(emb.parameters())
        g = torch.Generator().manual_seed(100 + rank)
        feats, tgt = torch.randn(32, 13, generator=g), torch.randn(32, 4, generator=g)

        def backward(listen: bool):
            x = emb(feats)
            if listen:
                _ListenerNet.params = unet_params
                out = _ListenerNet.apply(x, w1.detach(), w2.detach())
            else:
                out = torch.tanh(x @ w1.t()) @ w2.t()
            ((out - tgt) ** 2).mean().backward()
        backward(False)
        allreduce_gradients(params, dist, bucket_bytes=2048)
        want = [p.grad.clone() for p in params]
        for p in params:
            p.grad = None
        b = GradBucketer(params, dist, bucket_bytes=2048, late=list(emb.parameters()))
        ok = all(p is e for p, e in zip(b.buckets[-1], list(emb.parameters())[::-1]))      # the embedder's own last bucket
        backward(True)
        ok = ok and b.launched_during_backward == len(b.buckets)      # hooks + listeners together completed every bucket
        nb = b.finish()
        ok = ok and nb == len(b.buckets)
        ok = ok and all(torch.allclose(p.grad, w, rtol=1e-5, atol=1e-7) for p, w in zip(params, want))
        ok = ok and all(float(p.grad.abs().max()) > 0 for p in emb.parameters())
        b.close()
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


def test_grad_bucketer_with_parameters_outside_the_unet_gloo_world2():
    """The UNet's gradients reach the bucketer through the planned engine's listeners, inside the node's backward; a
    trainable conditioner's through torch's post-accumulate hooks, after it.  One bucketer over both sets, the conditioner's
    named `late`: every bucket is launched by the end of backward() and the result is the mean over ranks."""
    assert gloo_util.run_world(_outside_worker, 2) == {0: True, 1: True}
