"""CPU: the ParallelDomain colours (gcd_amd/geometry.py: semantic_palette, pardom_frame_mode, class_colours,
synth_rgb_pardom) and their library (libgcd_amd_pardom.so; gcd_amd.csrc.build.LIBRARIES, gcd_amd/_lib_pardom.py).  The
library's defines are what the callers count on, it leaves the renderer's library as it was and it refuses bad arguments
(the rules every library is held to are tests/test_libraries_host.py's).  The palette, the mode rule and the header's
formula are held to tests/golden/render_pardom_tiny.pt, which tools/make_golden_render_pardom.py recorded from the
reference's own method."""
import ctypes
from pathlib import Path

import numpy as np
import pytest
import torch

from gcd_amd import _lib, _lib_pardom, geometry as G
from gcd_amd._lib import GcdError
from gcd_amd.csrc import build as b

GOLDEN = Path(__file__).resolve().parent / "golden" / "render_pardom_tiny.pt"
RGB, BLEND, PALETTE = _lib_pardom.PARDOM_RGB, _lib_pardom.PARDOM_BLEND, _lib_pardom.PARDOM_PALETTE
_GOLD = None


def gold():
    global _GOLD
    if _GOLD is None:
        _GOLD = torch.load(GOLDEN, map_location="cpu", weights_only=False)
    return _GOLD


# ----------------------------------------------------------------------------------------------------------- the library
def test_defines_are_what_the_callers_count_on():
    assert _lib_pardom.PARDOM_PALETTE_ROWS == 256 and len({RGB, BLEND, PALETTE}) == 3
    # the largest stride keeps every byte offset of the largest cloud inside int64
    assert (2 ** 31) * _lib_pardom.PARDOM_MAX_LD * 8 < 2 ** 63
    # the renderer's library is what it was: the colours reach the splat as an operand, not as a field of its descriptor
    assert b.LIBRARIES["gcd_amd_render"].sources == ["render.hip"] and _lib.RENDER_ABI_VERSION == 1


def test_bad_arguments_return_a_status_and_a_message():
    """Every argument is checked before anything is launched (no device is needed to be refused)."""
    b.build(verbose=False)
    lib = _lib_pardom.load()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(20)        # never dereferenced: every call below fails its checks first
    ld = _lib_pardom.PARDOM_MAX_LD

    def call(ids=one, ids_ld=1, rgb=one, rgb_ld=3, N=8, palette=one, n_classes=12, alpha=0.5, mode=BLEND, out=one, out_ld=3,
             status=one):
        return lib.gcd_pardom_colours(ids, ids_ld, rgb, rgb_ld, N, palette, n_classes, alpha, mode, out, out_ld, status, None)
    bad = [dict(ids=None), dict(ids=None, mode=PALETTE), dict(rgb=None), dict(rgb=None, mode=RGB), dict(palette=None),
           dict(out=None), dict(status=None), dict(status=None, N=0),
           dict(mode=3), dict(mode=-1), dict(n_classes=0), dict(n_classes=257), dict(n_classes=-4),
           dict(ids_ld=0), dict(rgb_ld=2), dict(out_ld=2), dict(out_ld=0), dict(rgb_ld=-3),
           dict(ids_ld=ld + 1), dict(rgb_ld=ld + 1), dict(out_ld=ld + 1),
           dict(N=-1), dict(N=2 ** 31), dict(palette=odd), dict(out=odd), dict(status=odd), dict(status=odd, N=0),
           dict(alpha=-0.25), dict(alpha=1.5), dict(alpha=float("nan"))]
    for k, kw in enumerate(bad):
        assert call(**kw) == 2, (k, kw)
        assert lib.gcd_pardom_last_error().decode().startswith("gcd_pardom_colours"), (k, kw)
    with pytest.raises(GcdError):
        _lib_pardom.check(2, "gcd_pardom_colours")
    _lib_pardom.check(0)


def test_operands_that_are_not_on_the_gpu_are_refused():
    g = gold()
    ids, rgb = g["clouds"]["near_24x40"]["segm"][0], g["clouds"]["near_24x40"]["rgb"][0]
    with pytest.raises(GcdError):
        G.class_colours(ids, rgb, g["palette"], 0.5, "blend")
    with pytest.raises(GcdError):
        G.class_colours(ids.numpy(), rgb.numpy(), g["palette"], 0.5, "blend")
    with pytest.raises(ValueError):
        G.class_colours(ids, rgb, g["palette"], 0.5, "depth")
    c = g["cases"][0]
    kw = dict(model_frames=1, render_height=24, render_width=40, frame_height=16, frame_width=24, spread_radius=1)
    with pytest.raises(GcdError):
        G.synth_rgb_pardom(g["clouds"][c["cloud"]], "rgb", c["extrinsics"], c["intrinsics"], **kw)
    with pytest.raises(ValueError, match="Unknown selected modality"):          # as the reference does, before any work
        G.synth_rgb_pardom(g["clouds"][c["cloud"]], "depth", c["extrinsics"], c["intrinsics"], **kw)


# ------------------------------------------------------------------------------------------------ palette, modes, formula
def test_semantic_palette_is_the_reference_table():
    g = gold()
    table, n = G.semantic_palette(g["items"])
    assert n == g["n_classes"] == 12 and table.dtype == torch.float64 and tuple(table.shape) == (256, 3)
    assert torch.equal(table, g["palette"])
    assert not bool(table[n:].any()) and not bool(table[5].any()) and not bool(table[3].any())      # unnamed, and black
    assert bool(table[0].any()) and bool(table[n - 1].any())
    # float64 of the exact quotient, not a float32 widened
    item = next(x for x in g["items"] if x["id"] == 7)
    assert table[7].tolist() == [item["color"][k] / 255.0 for k in "rgb"]
    for items in ([], [dict(id=256, color=dict(r=1, g=2, b=3))], [dict(id=-1, color=dict(r=1, g=2, b=3))]):
        with pytest.raises(ValueError):
            G.semantic_palette(items)
    table, n = G.semantic_palette([dict(id=255, color=dict(r=255, g=0, b=51))])
    assert n == 256 and table[255].tolist() == [1.0, 0.0, 0.2] and not bool(table[:255].any())


def _reference_mode(t, modal_time):
    """The branches of the reference's loop body, restated."""
    if 0 < t < modal_time:
        return BLEND, t / modal_time
    if t == 0 and 0 < modal_time:
        return RGB, 0.0
    return PALETTE, 1.0


def test_mode_rule_per_frame():
    for modal_time in (0, 1, 2, 3, 7, 13, 14, 20):
        for t in range(16):
            assert G.pardom_frame_mode(t, modal_time, "rgb") == (None, 0.0)
            assert G.pardom_frame_mode(t, modal_time, "segm") == _reference_mode(t, modal_time)
    assert [G.pardom_frame_mode(t, 3, "segm") for t in range(3)] == [(RGB, 0.0), (BLEND, 1 / 3), (BLEND, 2 / 3)]
    assert [G.pardom_frame_mode(t, 2, "segm") for t in range(4)] == [(RGB, 0.0), (BLEND, 0.5), (PALETTE, 1.0), (PALETTE, 1.0)]
    assert [G.pardom_frame_mode(t, 0, "segm")[0] for t in range(3)] == [PALETTE] * 3
    assert G.pardom_frame_mode(1, 1, "segm")[0] == PALETTE and G.pardom_frame_mode(0, 1, "segm")[0] == RGB
    with pytest.raises(ValueError, match="Unknown selected modality"):
        G.pardom_frame_mode(0, 0, "depth")
    # the golden clips took these modes (the colours of a frame tell: a PALETTE frame holds table rows only)
    g = gold()
    rows = {tuple(r) for r in g["palette"].tolist()}
    for c in g["cases"]:
        for t, fr in enumerate(c["frames"]):
            mode, _ = G.pardom_frame_mode(t, c["modal_time"], c["modality"])
            assert ({tuple(r) for r in fr["colours"].tolist()} <= rows) == (mode == PALETTE), fr["name"]


def header_formula(ids, rgb, palette, alpha, mode):
    """include/gcd_amd_pardom.h's formula in numpy, one rounding per operation."""
    c32 = rgb.numpy().astype(np.float32) / np.float32(255.0)
    P = palette.numpy()[ids.numpy().reshape(-1).astype(np.int64)].reshape(rgb.shape)
    if mode == RGB or mode is None:
        return torch.from_numpy(c32.astype(np.float64))
    if mode == PALETTE:
        return torch.from_numpy(P.copy())
    first = (c32 * np.float32(1.0 - alpha)).astype(np.float32)
    return torch.from_numpy(first.astype(np.float64) + np.float64(alpha) * P)


def test_header_formula_gives_the_reference_colours_and_a_fused_one_does_not():
    """The bar of the GPU test (float64 equality) is the formula's own: on the golden's clouds it reproduces every colour the
    reference built.  A fused multiply-add would not, at alpha = 1/3 and 2/3 (and would at 1/2, which is why the clip
    with modal_time 3 is there)."""
    g = gold()
    seen = set()
    for c in g["cases"]:
        pcl = g["clouds"][c["cloud"]]
        for t, fr in enumerate(c["frames"]):
            mode, alpha = G.pardom_frame_mode(t, c["modal_time"], c["modality"])
            want = header_formula(pcl["segm"][t], pcl["rgb"][t], g["palette"], alpha, mode).reshape(-1, 3)
            assert fr["colours"].dtype == torch.float64 and torch.equal(want, fr["colours"]), fr["name"]
            seen.add((mode, alpha))
            if mode == BLEND:
                c32 = (pcl["rgb"][t].numpy().astype(np.float32) / np.float32(255.0)).reshape(-1, 3)
                P = g["palette"].numpy()[pcl["segm"][t].numpy().reshape(-1).astype(np.int64)]
                first = (c32 * np.float32(1.0 - alpha)).astype(np.float64)
                # a * P + first in one rounding, through exact rational arithmetic
                from fractions import Fraction
                fused = np.array([[float(Fraction(alpha) * Fraction(p) + Fraction(f)) for p, f in zip(pr, fr_)]
                                  for pr, fr_ in zip(P.tolist(), first.tolist())])
                differ = int((fused != fr["colours"].numpy()).sum())
                assert (differ == 0) == (alpha == 0.5), (fr["name"], alpha, differ)
    assert seen == {(None, 0.0), (RGB, 0.0), (BLEND, 1 / 3), (BLEND, 2 / 3), (BLEND, 0.5), (PALETTE, 1.0)}


def test_golden_fixtures_cover_what_they_are_there_for():
    g = gold()
    assert GOLDEN.stat().st_size < 1024 * 1024 and g["src_view"] == G.PARDOM_SRC_VIEW == 16
    by = {c["name"]: c for c in g["cases"]}
    assert [(c["modality"], c["modal_time"], c["T"], c["radius"]) for c in (by["rgb"], by["segm_m0"], by["segm_m3"], by["segm_m2"])] == \
        [("rgb", 0, 1, 1), ("segm", 0, 2, 1), ("segm", 3, 3, 1), ("segm", 2, 4, 2)]
    assert {tuple(c["render_hw"]) for c in g["cases"]} == {(24, 40), (24, 28), (24, 32)}
    assert by["rgb"]["reproject"] and by["segm_m3"]["reproject"] and not by["segm_m0"]["reproject"]
    for pcl in g["clouds"].values():
        for xyz, rgb, ids in zip(pcl["xyz"], pcl["rgb"], pcl["segm"]):
            assert xyz.dtype == torch.float16 and tuple(xyz.shape) == (17, 40, 3) and rgb.dtype == ids.dtype == torch.uint8
            assert tuple(rgb.shape) == (17, 40, 3) and tuple(ids.shape) == (17, 40, 1) and int(ids.max()) < g["n_classes"]
            bad = ~torch.isfinite(xyz).all(dim=-1) | (xyz.abs().max(dim=-1).values == 65504.0)
            assert bool((bad.sum(dim=1) >= 4).all())
    ids = torch.cat([i.reshape(-1) for i in g["clouds"]["near_24x40"]["segm"]])
    assert {0, 3, 5, g["n_classes"] - 1} <= set(ids.tolist())
    far = by["segm_m0_far"]["frames"][0]
    assert float(far["depth"].max()) > 64.0 and all(float(f["depth"].max()) < 64.0 for f in by["segm_m3"]["frames"])
    # the used intrinsics took the three branches of the aspect-ratio correction
    for name in ("segm_m0", "segm_m0_24x28", "segm_m0_24x32"):
        c = by[name]
        H, W = c["render_hw"]
        K, Kn = c["frames"][0]["K"], c["intrinsics"][0]
        scaled_fx, scaled_fy = Kn[0, 0] * W, Kn[1, 1] * H
        if W / H > 640.0 / 480.0 + 1e-3:
            assert K[1, 1] == K[0, 0] == scaled_fx != scaled_fy
        elif W / H < 640.0 / 480.0 - 1e-3:
            assert K[0, 0] == K[1, 1] == scaled_fy != scaled_fx
        else:
            assert K[0, 0] == scaled_fx and K[1, 1] == scaled_fy
