"""GPU: gcd_amd.metrics_device (libgcd_amd_metrics.so) against its oracle, the host gcd_amd.metrics.

The reference value of every case is the host function run on float64 copies of the float32 inputs, with the mask taken
from the float32 `reproject`: the kernels work in fp64, so they compute the same thing and the bars are those of fp64
sums of 49 terms over a denominator >= C2 = 9e-4 — 1e-9 absolute on SSIM and diversity values and on the uncertainty
map, 1e-9 relative on PSNR; NaN and inf positions must be the same.  The device must also be within 1e-6 (the bar of
tests/test_metrics.py) of the host function on the float32 inputs themselves.

The uncertainty map is float32: a value u carries a rounding error of up to ulp(u) / 2, which is below 1e-9 only for
u < 2^-5.  The diversity cases therefore use samples that differ by about 0.01 (as samples of one scene do) for the
1e-9 bar on the map, and a second case with wide spread holds the map to "the float64 reference rounded to float32,
give or take one ulp" instead.
"""
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
NAMES = ("psnr", "ssim", "psnr_vis", "ssim_vis", "psnr_occ", "ssim_occ")
TILE_H, TILE_W = 16, 32                    # the frame kernel's output tile (gcd_amd/csrc/metrics.hip)
ABS64, REL64_PSNR, ABS32 = 1e-9, 1e-9, 1e-6


# --------------------------------------------------------------------------------------------------------- inputs
def _smooth(g, *shape):
    b = torch.rand(*shape, generator=g)
    return (b + b.roll(1, -1) + b.roll(1, -2) + b.roll(2, -1)) / 4.0


def _images(S, T, H, W, seed, noise=0.05):
    g = torch.Generator().manual_seed(seed)
    gt = _smooth(g, T, 3, H, W)
    pred = (gt[None] + noise * torch.randn(S, T, 3, H, W, generator=g)).clamp(0.0, 1.0)
    return pred.float().contiguous(), gt.float().contiguous()


def _bands(T, H, W):
    """Diagonal bands wide enough for an L1 ball of radius 3: both eroded masks are non-empty from about 20 pixels on;
    True = occluded."""
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return torch.stack([(((x + 2 * y + 5 * t) // 20) % 2 == 0) for t in range(T)])


def _reproject(occluded, seed=0):
    """[T, H, W] bool -> [T, 3, H, W] float32: zeros where occluded, values in [0.1, 1] elsewhere."""
    g = torch.Generator().manual_seed(1000 + seed)
    r = 0.1 + 0.9 * torch.rand(occluded.shape[0], 3, *occluded.shape[1:], generator=g)
    return (r * (~occluded)[:, None]).float().contiguous()


# ------------------------------------------------------------------------------------------------------ reference
def _host(pred, gt, rep, dtype):
    from gcd_amd import metrics as M
    p, g_ = pred.numpy().astype(dtype), gt.numpy().astype(dtype)
    return M.calculate_metrics(g_, None if rep is None else rep.numpy(), [{"sampled_rgb": x} for x in p])


def _device(gpu, pred, gt, rep, signed=False):
    from gcd_amd import metrics_device as D
    dev = lambda t: None if t is None else t.to(gpu)      # noqa: E731
    p, g_, r = dev(pred), dev(gt), dev(rep)
    fm = D.frame_metrics(p, g_, r, signed=signed)
    unc, dv = D.diversity(p, r, signed=signed)
    torch.cuda.synchronize()
    return fm.cpu().numpy(), unc.cpu().numpy(), dv.cpu().numpy()


def _same_special(got, want, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN positions differ:\n{got}\n{want}"
    assert np.array_equal(np.isposinf(got), np.isposinf(want)) and np.array_equal(np.isneginf(got), np.isneginf(want)), \
        f"{what}: inf positions differ:\n{got}\n{want}"
    return np.isfinite(want)


def _check(fm, unc, dv, pred, gt, rep, host_pred=None, tag="", host32=True):
    """Device values against the host function on float64 copies (tight) and on the float32 inputs (1e-6; `host32=False`
    leaves that second comparison out, for the one place where the host's own float32 rounding exceeds it)."""
    hp = pred if host_pred is None else host_pred
    md64, unc64 = _host(hp, gt, rep, np.float64)
    md32, unc32 = _host(hp, gt, rep, np.float32)
    names = NAMES if rep is not None else NAMES[:2]
    for i, n in enumerate(NAMES):
        got = fm[:, :, i]
        if n not in names:
            assert (got == 0.0).all(), f"{tag}{n}: without reproject the masked values are stored as 0"
            continue
        want, want32 = md64["frame_" + n], md32["frame_" + n]
        fin = _same_special(got, want, tag + n)
        if host32:
            _same_special(got, want32, tag + n + " (host fp32)")
        err = np.abs(got[fin] - want[fin])
        if n.startswith("psnr"):
            err = err / np.abs(want[fin])
        e64 = float(err.max()) if err.size else 0.0
        e32 = float(np.abs(got[fin] - want32[fin]).max()) if err.size else 0.0
        print(f"{tag}{n}: vs fp64 host {e64:.3e} ({'rel' if n.startswith('psnr') else 'abs'}), vs fp32 host {e32:.3e}")
        assert e64 <= (REL64_PSNR if n.startswith("psnr") else ABS64), (tag, n, e64)
        assert e32 <= ABS32 or not host32, (tag, n, e32)
    cols = [("frame_diversity", 0)] + ([("frame_diversity_vis", 1), ("frame_diversity_occ", 2)] if rep is not None else [])
    for key, c in cols:
        got, want, want32 = dv[:, c], np.asarray(md64[key], np.float64), np.asarray(md32[key], np.float64)
        fin = _same_special(got, want, tag + key)
        e64 = float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0
        e32 = float(np.abs(got[fin] - want32[fin]).max()) if fin.any() else 0.0
        print(f"{tag}{key}: vs fp64 host {e64:.3e}, vs fp32 host {e32:.3e}")
        assert e64 <= ABS64 and e32 <= ABS32, (tag, key, e64, e32)
    if rep is None:
        assert (dv[:, 1:] == 0.0).all()
    assert unc.dtype == np.float32 and unc.shape == unc64.shape
    e32 = float(np.abs(unc.astype(np.float64) - unc32.astype(np.float64)).max())
    assert e32 <= ABS32, (tag, "uncertainty vs fp32 host", e32)
    return md64, unc64


# ------------------------------------------------------------------------------------------------ tile boundaries
SIZES = [(7, 7), (7, 64), (9, 8), (33, 47), (40, 56), (64, 64), (70, 131),
         (TILE_H - 1, TILE_W - 1), (TILE_H + 1, TILE_W + 1), (2 * TILE_H - 1, 2 * TILE_W + 1), (2 * TILE_H + 1, 2 * TILE_W - 1)]


@pytest.mark.parametrize("S,T", [(1, 1), (3, 1), (1, 3), (3, 3)], ids=lambda v: str(v))
@pytest.mark.parametrize("H,W", SIZES, ids=lambda v: str(v))
def test_tile_boundaries(gpu, H, W, S, T):
    pred, gt = _images(S, T, H, W, seed=H * 1000 + W + S * 7 + T, noise=0.01)
    rep = _reproject(_bands(T, H, W), seed=H + W)
    fm, unc, dv = _device(gpu, pred, gt, rep)
    _, unc64 = _check(fm, unc, dv, pred, gt, rep, tag=f"[{H}x{W} S{S} T{T}] ")
    e = float(np.abs(unc.astype(np.float64) - unc64).max())
    print(f"[{H}x{W} S{S} T{T}] uncertainty map vs fp64 host {e:.3e}")
    assert float(unc64.max()) < 2.0 ** -5, "the case is meant to stay where a float32 holds 1e-9"
    assert e <= ABS64
    if S == 1:
        assert (unc == 0.0).all() and (dv[:, 0] == 0.0).all()


# ---------------------------------------------------------------------------------------------------- golden cases
def test_golden_cases_of_the_reference_ssim_code(gpu):
    from oracle.make_golden_metrics import cases
    g = torch.load(Path(__file__).resolve().parent / "golden" / "metrics_kat.pt")["values"]
    seen = 0
    for name, a, b, m, kw in cases():
        if a.dtype != np.float32 or a.ndim != 3 or a.shape[0] != 3 or kw:
            continue                                   # the float32, three-channel, window-7 cases
        seen += 1
        pred, gt = torch.from_numpy(a)[None, None].contiguous(), torch.from_numpy(b)[None].contiguous()
        vis = torch.from_numpy(m)
        rep = vis[None, None].expand(1, 3, *vis.shape).float().contiguous()      # visible where the golden mask is set
        fm, _, _ = _device(gpu, pred, gt, rep)
        want = g[name].numpy()
        print(f"{name}: ssim {fm[0, 0, 1]:.12f} (golden {want[0]:.12f}), ssim_vis {fm[0, 0, 3]:.12f} (golden {want[1]:.12f})")
        assert abs(fm[0, 0, 1] - want[0]) <= 1e-6 and abs(fm[0, 0, 3] - want[1]) <= 1e-6, name
    assert seen == 4


# --------------------------------------------------------------------------------------------------- image content
def _content(kind, T=2, H=24, W=40):
    g = torch.Generator().manual_seed(77)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    if kind == "identical":
        gt = _smooth(g, T, 3, H, W)
        pred = gt.clone()
    elif kind == "constant":
        gt = torch.full((T, 3, H, W), 0.25)
        pred = torch.full((T, 3, H, W), 0.75)
    elif kind == "constant_equal":
        gt = torch.full((T, 3, H, W), 0.5)
        pred = gt.clone()
    elif kind == "gradient":
        gt = ((x / (W - 1)) * 0.6 + (y / (H - 1)) * 0.3).expand(T, 3, H, W).clone()
        pred = (gt + 0.01 * torch.randn(T, 3, H, W, generator=g)).clamp(0, 1)
    elif kind == "edge":
        gt = torch.where(x < W // 2, torch.tensor(0.2), torch.tensor(0.8)).expand(T, 3, H, W).clone()
        pred = (gt + 1e-3 * torch.randn(T, 3, H, W, generator=g)).clamp(0, 1)
    elif kind == "near_saturated":
        gt = torch.ones(T, 3, H, W)
        pred = torch.full((T, 3, H, W), 0.999)
    return pred[None].float().contiguous(), gt.float().contiguous()


@pytest.mark.parametrize("kind", ["identical", "constant", "constant_equal", "gradient", "edge", "near_saturated"])
def test_image_content(gpu, kind):
    """Whole-image values at both bars.  The same images are then run with a mask, against the float64 host only: on
    nearly flat images the host function's OWN float32 SSIM map is 1e-6 .. 3e-6 away from its float64 one over a small
    eroded mask (measured on the two-level image: ssim_vis / ssim_occ 0.9e-6 .. 2.6e-6 for levels 0.2 | 0.8, 0.2 | 0.6,
    0.25 | 0.5 at 24 x 40 and 40 x 64; whole image 0.4e-6 .. 0.9e-6), so a 1e-6 comparison with it would measure the
    oracle's rounding, not the kernel."""
    pred, gt = _content(kind)
    fm, unc, dv = _device(gpu, pred, gt, None)
    _check(fm, unc, dv, pred, gt, None, tag=f"[{kind}] ")
    if kind in ("identical", "constant_equal"):
        assert np.isposinf(fm[:, :, 0]).all() and np.abs(fm[:, :, 1] - 1.0).max() <= ABS64
    rep = _reproject(_bands(gt.shape[0], gt.shape[2], gt.shape[3]))
    fm, unc, dv = _device(gpu, pred, gt, rep)
    _check(fm, unc, dv, pred, gt, rep, tag=f"[{kind}, masked] ", host32=False)
    if kind in ("identical", "constant_equal"):
        assert np.isposinf(fm[:, :, [0, 2, 4]]).all()
        assert np.abs(fm[:, :, [1, 3, 5]] - 1.0).max() <= ABS64


# ----------------------------------------------------------------------------------------------------------- masks
def _mask(kind, T, H, W):
    occ = torch.zeros(T, H, W, dtype=torch.bool)
    if kind == "all_visible":
        pass
    elif kind == "all_occluded":
        occ[:] = True
    elif kind == "one_frame_occluded":
        occ[:] = _bands(T, H, W)
        occ[1] = True
    elif kind == "touching_borders":          # the occluded set is a frame along all four borders, 5 thick
        occ[:] = True
        occ[:, 5:H - 5, 5:W - 5] = False
    elif kind == "one_pixel_hole":            # one visible pixel in an occluded image and the other way round
        occ[0] = True
        occ[0, H // 2, W // 2] = False
        occ[1:, H // 2, W // 2] = True
    elif kind == "stripe6":                   # erodes to nothing: NaN for SSIM, a finite PSNR
        occ[:, :, 17:23] = True
    elif kind == "stripe7":                   # erodes to a line one pixel wide
        occ[:, :, 17:24] = True
    return occ


MASKS = ["none", "all_visible", "all_occluded", "one_frame_occluded", "touching_borders", "one_pixel_hole", "stripe6",
         "stripe7", "threshold"]


@pytest.mark.parametrize("kind", MASKS)
def test_masks(gpu, kind):
    S, T, H, W = 2, 3, 26, 45
    pred, gt = _images(S, T, H, W, seed=5, noise=0.01)
    if kind == "none":
        rep = None
    elif kind == "threshold":
        # 3e-8 per channel sums to 9e-8 <= 1e-7 (occluded), 4e-8 per channel to 1.2e-7 (visible), side by side in columns
        # of 8; negative values count by their magnitude
        x = torch.arange(W)
        val = torch.where((x // 8) % 2 == 0, torch.tensor(3e-8), torch.tensor(4e-8))
        rep = val.expand(T, 3, H, W).clone().float()
        rep[:, 1] = -rep[:, 1]
        rep = rep.contiguous()
    else:
        rep = _reproject(_mask(kind, T, H, W))
    fm, unc, dv = _device(gpu, pred, gt, rep)
    _check(fm, unc, dv, pred, gt, rep, tag=f"[{kind}] ")
    if kind == "stripe6":
        assert np.isnan(fm[:, :, 5]).all() and np.isfinite(fm[:, :, 4]).all() and np.isfinite(fm[:, :, 3]).all()
    if kind == "stripe7":
        assert np.isfinite(fm[:, :, 5]).all()
    if kind == "all_occluded":
        assert np.isnan(fm[:, :, 2:4]).all() and np.isnan(dv[:, 1]).all() and np.isfinite(fm[:, :, 4:6]).all()
    if kind == "all_visible":
        assert np.isnan(fm[:, :, 4:6]).all() and np.isnan(dv[:, 2]).all()
        assert np.array_equal(fm[:, :, 3], fm[:, :, 1]) and np.array_equal(fm[:, :, 2], fm[:, :, 0])
    if kind == "one_frame_occluded":
        assert np.isnan(fm[:, 1, 2:4]).all() and np.isfinite(fm[:, 0, :]).all() and np.isfinite(fm[:, 2, :]).all()
    if kind == "threshold":
        assert np.isfinite(fm).all(), "both kinds of column are 8 wide: both eroded masks are non-empty"


# ---------------------------------------------------------------------------------------------------------- signed
def test_signed_input_is_mapped_and_clamped_on_load(gpu):
    S, T, H, W = 2, 2, 19, 37
    g = torch.Generator().manual_seed(11)
    gt = _smooth(g, T, 3, H, W).float().contiguous()
    raw = ((gt[None] * 2.0 - 1.0) + 0.02 * torch.randn(S, T, 3, H, W, generator=g)).float()
    raw[:, :, :, ::5, ::7] = 1.3                    # outside [-1, 1] on both sides
    raw[:, :, :, 2::5, 3::7] = -1.7
    raw = raw.contiguous()
    mapped = torch.clamp((raw + 1.0) / 2.0, 0.0, 1.0)
    assert float(raw.max()) > 1.0 and float(raw.min()) < -1.0 and mapped.dtype == torch.float32
    rep = _reproject(_bands(T, H, W))
    fm, unc, dv = _device(gpu, raw, gt, rep, signed=True)
    _check(fm, unc, dv, raw, gt, rep, host_pred=mapped, tag="[signed] ")
    fm2, unc2, dv2 = _device(gpu, mapped.contiguous(), gt, rep, signed=False)
    assert np.array_equal(fm, fm2, equal_nan=True) and np.array_equal(unc, unc2) and np.array_equal(dv, dv2, equal_nan=True)


# ------------------------------------------------------------------------------------------------------- diversity
def test_diversity(gpu):
    T, H, W = 3, 21, 50
    pred, gt = _images(3, T, H, W, seed=3, noise=0.01)
    occ = _bands(T, H, W)
    occ[2] = False                                  # frame 2: nothing occluded -> NaN for its occluded mean
    rep = _reproject(occ)
    fm, unc, dv = _device(gpu, pred, gt, rep)
    _, unc64 = _check(fm, unc, dv, pred, gt, rep, tag="[diversity S3] ")
    e = float(np.abs(unc.astype(np.float64) - unc64).max())
    print(f"[diversity S3] uncertainty map vs fp64 host {e:.3e} (map max {unc64.max():.3e})")
    assert float(unc64.max()) < 2.0 ** -5 and e <= ABS64
    assert np.isnan(dv[2, 2]) and np.isfinite(dv[:2]).all() and np.isfinite(dv[2, :2]).all()
    # S = 1: no spread
    fm1, unc1, dv1 = _device(gpu, pred[:1].contiguous(), gt, rep)
    assert (unc1 == 0.0).all() and (dv1[:, 0] == 0.0).all() and np.isnan(dv1[2, 2]) and (dv1[:2, 1:] == 0.0).all()
    # wide spread: the float32 map is the float64 reference rounded once (one ulp for a reference that sits on a tie)
    wide = torch.rand(3, T, 3, H, W, generator=torch.Generator().manual_seed(4)).float().contiguous()
    _, uncw, dvw = _device(gpu, wide, gt, rep)
    md64, unc64w = _host(wide, gt, rep, np.float64)
    r32 = unc64w.astype(np.float32)
    ulp = np.spacing(r32)
    assert float(unc64w.max()) > 0.1 and (np.abs(uncw - r32) <= ulp).all() and (uncw == r32).mean() > 0.999
    for key, c in (("frame_diversity", 0), ("frame_diversity_vis", 1), ("frame_diversity_occ", 2)):
        fin = _same_special(dvw[:, c], md64[key], key)
        assert np.abs(dvw[fin, c] - md64[key][fin]).max() <= ABS64


# ----------------------------------------------------------------------------------------------------- determinism
def test_two_calls_give_identical_raw_outputs(gpu):
    from gcd_amd import metrics_device as D
    pred, gt = _images(3, 3, 70, 131, seed=9)
    rep = _reproject(_bands(3, 70, 131))
    p, g_, r = pred.to(gpu), gt.to(gpu), rep.to(gpu)
    a, (ua, da) = D.frame_metrics(p, g_, r), D.diversity(p, r)
    junk = torch.full((1 << 16,), float("nan"), device=gpu)      # noqa: F841  (other memory in between)
    b, (ub, db) = D.frame_metrics(p, g_, r), D.diversity(p, r)
    # torch.equal is false for NaN: there is none here (both eroded masks are non-empty at this size)
    assert torch.isfinite(a).all() and torch.isfinite(da).all()
    assert torch.equal(a, b) and torch.equal(ua, ub) and torch.equal(da, db)


# ------------------------------------------------------------------------------------------------ past 2^31 elements
def test_offsets_past_two_to_the_31_elements(gpu):
    """pred of 4 x 2 x 3 x 10400 x 10000 floats (10 GB): the last (sample, frame) starts past element 2^31.  Every
    (sample, frame) is computed on its own, tiles folded in the same order, so the values of the last one are bit-identical
    to the same frame handed over alone (which the cases above hold to the host function at small sizes); the same for the
    last frame's diversity.  A 32-bit offset anywhere reads another frame and changes them."""
    from gcd_amd import metrics_device as D
    S, T, H, W = 4, 2, 10400, 10000
    assert (S * T - 1) * 3 * H * W > 2 ** 31
    g = torch.Generator(device=gpu).manual_seed(2)
    pred = torch.rand(S, T, 3, H, W, generator=g, device=gpu)
    gt = torch.rand(T, 3, H, W, generator=g, device=gpu)
    rep = torch.rand(T, 3, H, W, generator=g, device=gpu)
    rep[:, :, :, W // 3:2 * W // 3] = 0.0
    full = D.frame_metrics(pred, gt, rep)
    unc, dv = D.diversity(pred, rep)
    for s, t in ((S - 1, T - 1), (0, 0)):
        alone = D.frame_metrics(pred[s:s + 1, t:t + 1].contiguous(), gt[t:t + 1].contiguous(), rep[t:t + 1].contiguous())
        assert torch.isfinite(alone).all() and torch.equal(full[s, t], alone[0, 0]), (s, t, full[s, t], alone)
    unc1, dv1 = D.diversity(pred[:, T - 1:].contiguous(), rep[T - 1:].contiguous())
    assert torch.isfinite(dv1).all() and torch.equal(dv[T - 1], dv1[0]) and torch.equal(unc[T - 1], unc1[0])
    assert not torch.equal(full[S - 1, T - 1], full[0, 0])
    del pred, gt, rep, unc, unc1, alone
    torch.cuda.empty_cache()                       # 15 GB back to the device


# ---------------------------------------------------------------------------------------------------------- errors
def test_bad_operands_raise_and_a_later_call_works(gpu):
    from gcd_amd import _lib, metrics_device as D
    pred, gt = _images(2, 2, 12, 20, seed=1)
    p, g_ = pred.to(gpu), gt.to(gpu)
    good = D.frame_metrics(p, g_).cpu()
    bad = [
        (p[..., :6, :].contiguous(), g_[..., :6, :].contiguous(), "7 x 7"),                     # H = 6
        (p.half(), g_.half(), "float32"),
        (p.transpose(-1, -2), g_.transpose(-1, -2), "contiguous"),
        (pred, gt, "no CPU"),
        (p, g_[:1].contiguous(), "does not fit"),
        (p, g_[:, :, :, :19].contiguous(), "does not fit"),
    ]
    for a, b, msg in bad:
        with pytest.raises(_lib.GcdError, match=msg):
            D.frame_metrics(a, b)
        with pytest.raises(_lib.GcdError, match=msg):
            D.calculate_metrics(b, None, a)
    with pytest.raises(_lib.GcdError, match="7 x 7"):
        D.diversity(p[..., :6].contiguous())
    with pytest.raises(_lib.GcdError, match="float32"):
        D.diversity(p.double())
    with pytest.raises(_lib.GcdError, match="does not fit"):
        D.frame_metrics(p, g_, g_[:1].contiguous())
    assert torch.equal(D.frame_metrics(p, g_).cpu(), good)
    md, unc = D.calculate_metrics(g_, None, p)
    assert np.isfinite(md["frame_psnr"]).all() and unc.shape == (2, 12, 20)


# ------------------------------------------------------------------------------------------------------ dictionary
@pytest.mark.parametrize("with_mask", [False, True], ids=["no_reproject", "reproject"])
def test_dictionary_matches_the_host_function(gpu, with_mask):
    from gcd_amd import metrics as M, metrics_device as D
    S, T, H, W = 2, 3, 30, 44
    pred, gt = _images(S, T, H, W, seed=21, noise=0.01)
    occ = _bands(T, H, W)
    rep = _reproject(occ) if with_mask else None
    want, want_unc = M.calculate_metrics(gt.numpy(), None if rep is None else rep.numpy(),
                                         [{"sampled_rgb": x} for x in pred.numpy()])
    dev = lambda t: None if t is None else t.to(gpu)      # noqa: E731
    for samples in (dev(pred), [{"sampled_rgb": dev(x)} for x in pred]):
        got, got_unc = D.calculate_metrics(dev(gt), dev(rep), samples)
        assert set(got) == set(want)
        for k in want:
            w, g_ = np.asarray(want[k]), np.asarray(got[k])
            assert g_.shape == w.shape and g_.dtype == w.dtype, (k, g_.shape, w.shape, g_.dtype, w.dtype)
            assert type(got[k]) is type(want[k]), (k, type(got[k]), type(want[k]))
            assert np.allclose(g_, w, rtol=0, atol=ABS32, equal_nan=True), (k, g_, w)
        assert got_unc.shape == want_unc.shape and got_unc.dtype == want_unc.dtype
        assert np.abs(got_unc - want_unc).max() <= ABS32
    assert D.calculate_metrics(dev(gt), dev(rep), dev(pred), return_uncertainty=False)[1] is None
    # an empty frame mask: the host function's values for it are NaN, and so is its dtype rule (float64 then)
    if with_mask:
        occ[1] = True
        rep2 = _reproject(occ)
        want, _ = M.calculate_metrics(gt.numpy(), rep2.numpy(), [{"sampled_rgb": x} for x in pred.numpy()])
        got, _ = D.calculate_metrics(dev(gt), dev(rep2), dev(pred))
        for k in want:
            w, g_ = np.asarray(want[k]), np.asarray(got[k])
            assert g_.shape == w.shape and g_.dtype == w.dtype, (k, g_.dtype, w.dtype)
            assert np.allclose(g_, w, rtol=0, atol=ABS32, equal_nan=True), (k, g_, w)
    # no samples: the host function's answer, without a launch
    if not with_mask:
        try:
            want0 = M.calculate_metrics(gt.numpy(), None, [])
        except Exception as e:                          # whatever the host function does with no samples ...
            with pytest.raises(type(e)):                # ... the device one does too
                D.calculate_metrics(dev(gt), None, [])
        else:
            got0 = D.calculate_metrics(dev(gt), None, [])
            assert set(got0[0]) == set(want0[0]) and got0[1].shape == want0[1].shape
