"""Generate tests/golden/train_inputs_tiny.pt: the UNMODIFIED reference VideoUNet (through oracle/ref_shim.py) at the TINY
configuration and the procedural weights of oracle/make_golden.py's unet_tiny fixture, forward + backward in fp32 CPU
autograd with x, context AND y requiring grad — what a trainable conditioner (cfg4: SphericalEmbedder, is_trainable) sees
through cond["vector"] / cond["crossattn"], and what OpenAIWrapper's cat hands on through x.  Needs the reference tree; run
with:  python -m tools.make_golden_train_inputs

Shape: 2 clips x 3 frames at 8 x 8 latents, aux_emb_dim > 0.  Loss: mean squared error against a seeded target.  Recorded:
the inputs' seed and the inputs `inputs(seed)` makes from it, `out`, the whole `y_grad`,
`context_grad`, `x_grad`, and for every parameter gradient its norm and 32 strided samples (`param_names` gives the rows).
"""
from __future__ import annotations

import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from oracle import svd_unet_ref as O  # noqa: E402
from oracle.make_golden import build_reference_unet, sample  # noqa: E402

OUT = ROOT / "tests" / "golden" / "train_inputs_tiny.pt"
CLIPS, T, H, W, INPUT_SEED = 2, 3, 8, 8, 77


def inputs(seed: int = INPUT_SEED, clips: int = CLIPS, T: int = T, h: int = H, w: int = W, cfg=O.TINY) -> dict:
    """x (latents | concat), c_noise-like timesteps, one-token context per frame, vector, image-only mask, loss target."""
    g = torch.Generator().manual_seed(seed)
    n = clips * T
    return dict(x=torch.randn(n, 8, h, w, generator=g), ts=torch.linspace(-1.0, 1.5, n),
                context=torch.randn(n, 1, cfg.context_dim, generator=g),
                y=torch.randn(n, cfg.adm_in_channels + cfg.aux_emb_dim, generator=g).clamp(-1, 1),
                ioi=torch.zeros(clips, T), target=torch.randn(n, 4, h, w, generator=g))


def main():
    cfg = O.TINY
    assert cfg.aux_emb_dim > 0
    net, _ = build_reference_unet(cfg)
    net.train()
    s = inputs()
    x, ctx, y = (s[k].clone().requires_grad_() for k in ("x", "context", "y"))
    out = net(x, s["ts"], context=ctx, y=y, num_video_frames=T, image_only_indicator=s["ioi"])
    loss = ((out - s["target"]) ** 2).mean()
    loss.backward()
    # parameter gradients: names in registration order, one row of 32 strided samples each (fewer elements: zero-padded;
    # a parameter the graph does not reach: norm -1 and a row of zeros) — one tensor, not two thousand small ones
    names = [n for n, _ in net.named_parameters()]
    norms = torch.full((len(names),), -1.0, dtype=torch.float64)
    samples = torch.zeros(len(names), 32)
    for i, (n, p) in enumerate(net.named_parameters()):
        if p.grad is not None:
            norms[i] = p.grad.double().norm()
            v = sample(p.grad, 32)
            samples[i, :v.numel()] = v
    torch.save({
        "config": "TINY", "clips": CLIPS, "T": T, "h": H, "w": W, "input_seed": INPUT_SEED, "loss": float(loss.detach()),
        "out": out.detach(), "x_grad": x.grad, "context_grad": ctx.grad, "y_grad": y.grad,
        "inputs": {k: v.clone() for k, v in s.items()},       # (what `inputs(input_seed)` gives: the tests read these)
        "param_names": names, "param_grad_norms": norms, "param_grad_samples": samples,
    }, OUT)
    print(f"train_inputs_tiny: loss {float(loss):.4f}  |dx| {float(x.grad.norm()):.3e}  |dcontext| "
          f"{float(ctx.grad.norm()):.3e}  |dy| {float(y.grad.norm()):.3e}  {OUT.stat().st_size} bytes")
    # the temporal cross-attention reads each clip's FIRST frame's context: those rows carry the extra term
    per_row = ctx.grad.reshape(CLIPS * T, -1).norm(dim=1)
    print("  |dcontext| per frame:", [f"{float(v):.2e}" for v in per_row])


if __name__ == "__main__":
    main()
