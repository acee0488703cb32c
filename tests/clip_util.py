"""Shared by the CLIP image tower tests and tools/make_golden_clip.py (a helper module like render_util.py, not a conftest):
the seeded inputs, the golden file, and the embedder built on a golden case's regenerated weights."""
from __future__ import annotations

from pathlib import Path

import torch

GOLDEN = Path(__file__).resolve().parent / "golden" / "clip_vision_tiny.pt"
_CACHE = {}


def seeded_image(n: int, H: int, W: int, seed: int) -> torch.Tensor:
    """fp32 [n, 3, H, W] in [-1, 1]: a smooth part (low-resolution noise, upsampled) plus white noise."""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(n, 3, max(H // 8, 2), max(W // 8, 2), generator=g) * 2 - 1
    smooth = torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear", align_corners=False)
    return (0.7 * smooth + 0.3 * (torch.rand(n, 3, H, W, generator=g) * 2 - 1)).clamp(-1, 1).float()


def checksum(t: torch.Tensor):
    return float(t.double().sum()), float(t.double().abs().sum())


def close(a, b, rel=1e-9) -> bool:
    return all(abs(x - y) <= rel * max(abs(y), 1.0) for x, y in zip(a, b))


def load_golden() -> dict:
    if "gold" not in _CACHE:
        _CACHE["gold"] = torch.load(GOLDEN, map_location="cpu", weights_only=True)
    return _CACHE["gold"]


def tower_case(name: str):
    """(record, state dict, raw images) of a tower case: weights and images regenerated from the recorded seeds, once per
    process, and held to the recorded checksums (a torch whose generator drifted must not pass for a kernel error)."""
    if name not in _CACHE:
        from gcd_amd import clip_vision as cv
        rec = load_golden()["tower"][name]
        sd = cv.seeded_state_dict(rec["cfg"], rec["weight_seed"])
        assert list(sd) == list(rec["checksums"])
        for k, v in sd.items():
            assert close(checksum(v), rec["checksums"][k]), f"{name}: regenerated {k} does not match the recorded checksum"
        raw = seeded_image(rec["n"], rec["cfg"]["image_size"], rec["cfg"]["image_size"], rec["image_seed"])
        assert close(checksum(raw), rec["image_checksum"]), f"{name}: regenerated images do not match the recorded checksum"
        _CACHE[name] = (rec, sd, raw)
    return _CACHE[name]


def preprocess_case(name: str):
    rec = load_golden()["preprocess"][name]
    raw = seeded_image(rec["n"], rec["H"], rec["W"], rec["image_seed"])
    assert close(checksum(raw), rec["image_checksum"]), f"{name}: regenerated image does not match the recorded checksum"
    return rec, raw


def embedder(cfg: dict, sd: dict, device="cpu", **kw):
    """FrozenOpenCLIPImageEmbedder over `cfg` with the tower's weights `sd` (open_clip names), frozen, on `device`."""
    from gcd_amd import clip_vision as cv
    emb = cv.FrozenOpenCLIPImageEmbedder(vision_cfg=dict(cfg), **kw)
    emb.model.visual.load_state_dict(sd)
    return emb.to(device)
