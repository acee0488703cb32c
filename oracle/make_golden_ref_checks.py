"""ORACLE support (build container only): generate tests/golden/ref_checks_tiny.pt by running the
UNMODIFIED reference VideoUNet / OpenAIWrapper / Denoiser (via oracle/ref_shim.py) on procedural weights and
inputs.  The fixture lets tests/test_oracle.py hold the oracle restatement (oracle/svd_unet_ref.py) to the
reference without the reference tree.  Inputs are not stored: `embedders_inputs` / `gradients_inputs` below
rebuild them from oracle/weights.py and seeded CPU generators.
  embedders  one VideoUNet.forward (TINY, weight salt 1, 2 frames of 8x16, image_only_indicator set on one
             frame: the AlphaBlender path) -> its output in full;
  gradients  denoiser + L2 loss, forward and torch.autograd backward (TINY in train mode, weight salt 7,
             2 clips x 2 frames of 8x8, sigma 2.5 / 0.3) -> output and input gradient in full, and every
             parameter gradient packed by `pack()`: its max |g|, its norm, SAMPLES strided samples (all of it
             when smaller) and PROJ seeded Gaussian projections of the whole tensor.
Re-run with:  python -m oracle.make_golden_ref_checks
"""
from __future__ import annotations

import math
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from oracle import svd_unet_ref as O, weights  # noqa: E402

OUT = ROOT / "tests" / "golden" / "ref_checks_tiny.pt"
SAMPLES = 32
PROJ = 4


def _idx(n: int) -> torch.Tensor:
    return torch.linspace(0, n - 1, min(n, SAMPLES)).long()


def _proj(f: torch.Tensor) -> torch.Tensor:
    """PROJ projections <r_k, f> with r_k ~ N(0, I) drawn from a generator seeded by f's size."""
    g = torch.Generator().manual_seed(f.numel())
    return torch.randn(PROJ, f.numel(), generator=g).double() @ f.double()


def pack(grads: dict) -> dict:
    """{name: gradient or None} -> flat tensors, one record per parameter in state-dict order (the names and
    shapes are the architecture's: `unpack` takes them from the caller)."""
    amax, norms, counts, samples, projs = [], [], [], [], []
    for t in grads.values():
        if t is None:
            amax.append(-1.0), norms.append(0.0), counts.append(0), projs.append(torch.zeros(PROJ))
            continue
        f = t.detach().float().reshape(-1)
        s = f[_idx(f.numel())]
        amax.append(float(f.abs().max())), norms.append(float(f.double().norm())), counts.append(s.numel())
        samples.append(s), projs.append(_proj(f).float())
    return dict(has_grad=torch.tensor([t is not None for t in grads.values()]), amax=torch.tensor(amax), norms=torch.tensor(norms, dtype=torch.float64),
                counts=torch.tensor(counts, dtype=torch.int32), samples=torch.cat(samples), proj=torch.stack(projs))


def unpack(pk: dict, shapes: dict) -> dict:
    """`pack`'s records against {name: shape} of the same architecture -> {name: None | dict(shape, amax, norm,
    sample, proj)}"""
    assert len(shapes) == len(pk["has_grad"])
    out, at = {}, 0
    for i, (n, shape) in enumerate(shapes.items()):
        c = int(pk["counts"][i])
        if not bool(pk["has_grad"][i]):
            out[n] = None
            continue
        out[n] = dict(shape=tuple(shape), amax=float(pk["amax"][i]), norm=float(pk["norms"][i]),
                      sample=pk["samples"][at:at + c], proj=pk["proj"][i])
        at += c
    return out


def rel_err(got: torch.Tensor, rec: dict) -> float:
    """rel-L2 of `got` against a record: exact where the samples are the whole tensor, else the largest of three
    estimates of it, each scaled by the reference's norm (a tensor that is mostly ~0, such as a 3x3 kernel's border
    taps, would make a rel-L2 of the samples alone meaningless): the samples' difference over the norm of as many
    average elements, the norm ratio's distance from 1, and rms(projection difference) / ||reference||."""
    def rel(a, b):
        a, b = a.double(), b.double()
        return float((a - b).norm() / b.norm().clamp_min(1e-30))
    assert tuple(got.shape) == tuple(rec["shape"])
    f = got.detach().float().reshape(-1).cpu()
    if f.numel() <= SAMPLES:
        return rel(f, rec["sample"])
    nr = max(rec["norm"], 1e-30)
    pd = (_proj(f) - rec["proj"].double()).norm() / math.sqrt(PROJ)
    k = rec["sample"].numel()
    sd = (f[_idx(f.numel())].double() - rec["sample"].double()).norm() / math.sqrt(k / f.numel())
    return max(float(sd) / nr, abs(float(f.double().norm()) / nr - 1.0), float(pd) / nr)


def unet_inputs(cfg, T, h, w, seed):
    noise, c, uc = weights.synth_inputs(1, T, h, w, cfg.context_dim, cfg.adm_in_channels + cfg.aux_emb_dim, seed)
    x = torch.cat([torch.cat([noise, uc["concat"]], 1), torch.cat([noise, c["concat"]], 1)])
    ts = torch.linspace(-1.5, 1.63, 2 * T)
    return (x, ts, torch.cat([uc["crossattn"], c["crossattn"]]),
            torch.cat([uc["vector"], c["vector"]]), torch.zeros(2, T))


def embedders_inputs():
    x, ts, ctx, y, ioi = unet_inputs(O.TINY, 2, 8, 16, 9)
    ioi[1, 0] = 1.0     # image_only_indicator path of AlphaBlender
    return x, ts, ctx, y, ioi


def gradients_inputs():
    """noise, c, target, sigma, image_only_indicator of the gradient check (T = 2, 2 clips, 8x8)"""
    cfg = O.TINY
    noise, c, _ = weights.synth_inputs(2, 2, 8, 8, cfg.context_dim, cfg.adm_in_channels + cfg.aux_emb_dim, 13)
    target = torch.randn(noise.shape, generator=torch.Generator().manual_seed(14))
    return noise, c, target, torch.tensor([2.5, 2.5, 0.3, 0.3]), torch.zeros(2, 2)


def embedders(VideoUNet) -> dict:
    cfg = O.TINY
    net = VideoUNet(**cfg.as_reference_kwargs()).eval()
    sd = weights.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, salt=1)
    net.load_state_dict(sd)
    x, ts, ctx, y, ioi = embedders_inputs()
    with torch.no_grad():
        out = net(x, ts, context=ctx, y=y, num_video_frames=2, image_only_indicator=ioi)
    return dict(salt=1, T=2, out=out)


def gradients(VideoUNet, OpenAIWrapper, Denoiser, denoiser_cfg) -> dict:
    cfg = O.TINY
    net = VideoUNet(**cfg.as_reference_kwargs()).train()
    sd = weights.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, salt=7)
    net.load_state_dict(sd)
    noise, c, target, sigma, ioi = gradients_inputs()
    x = noise.clone().requires_grad_(True)
    out = Denoiser(denoiser_cfg)(OpenAIWrapper(net), x, sigma, c, num_video_frames=2, image_only_indicator=ioi)
    ((out - target) ** 2).mean().backward()
    return dict(salt=7, T=2, out=out.detach(), x_grad=x.grad.detach(),
                param_grads=pack({n: p.grad for n, p in net.named_parameters()}))


def main():
    from oracle import ref_shim
    torch.manual_seed(0)
    VideoUNet, OpenAIWrapper, Denoiser, _ = ref_shim.reference_classes()
    fx = dict(embedders=embedders(VideoUNet),
              gradients=gradients(VideoUNet, OpenAIWrapper, Denoiser, ref_shim.DENOISER_CFG))
    torch.save(fx, OUT)
    print(f"wrote {OUT} ({OUT.stat().st_size / 2**20:.1f} MiB)")


if __name__ == "__main__":
    main()
