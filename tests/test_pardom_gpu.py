"""GPU: libgcd_amd_pardom.so and gcd_amd.geometry.synth_rgb_pardom against tests/golden/render_pardom_tiny.pt
(tools/make_golden_render_pardom.py: the reference's own ParallelDomain method, run on the CPU).

Colours: float64-equal to the colours the reference built, every frame of every clip.  The bar is derived, not measured:
every operation of include/gcd_amd_pardom.h's formula is one IEEE rounding of the same operands torch rounds
(tests/test_pardom_host.py checks the formula itself against the golden on the CPU, and that a fused multiply-add would
miss it at alpha 1/3 and 2/3).  Stage 1 on those colours through the existing splat, stage 2 and end to end: the bars of
DESIGN.md §12.2 as they stand there (tests/render_util.check_splat; 2^-22 and 4 x the recorded dtype gap; 2^-20).

Measured on an MI355X: see DESIGN.md §12.2."""
import pytest
import torch

from render_util import check_splat
from test_pardom_host import BLEND, PALETTE, RGB, gold, header_formula

pytestmark = pytest.mark.gpu

CASE_NAMES = ["rgb", "segm_m0", "segm_m3", "segm_m2", "segm_m0_far", "segm_m0_24x28", "segm_m0_24x32"]
_DEV = {}


def case(name):
    return next(c for c in gold()["cases"] if c["name"] == name)


def cloud(gpu, name):
    """The clouds of a case on the device (moved once)."""
    key = case(name)["cloud"]
    if key not in _DEV:
        _DEV[key] = {k: [t.to(gpu) for t in v] for k, v in gold()["clouds"][key].items()}
    return _DEV[key]


def palette(gpu):
    if "palette" not in _DEV:
        _DEV["palette"] = gold()["palette"].to(gpu)
    return _DEV["palette"]


def frame_mode(c, t):
    from gcd_amd import geometry as G
    mode, alpha = G.pardom_frame_mode(t, c["modal_time"], c["modality"])
    return (RGB, 0.0) if mode is None else (mode, alpha)       # the stored colours as they are: what mode RGB writes


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def flat_frame(gpu, name="segm_m3", t=1):
    """(ids (N,), rgb (N, 3), the reference's colours (N, 3), mode, alpha) of one frame: BLEND at 1/3 by default."""
    c, pcl = case(name), cloud(gpu, name)
    return (pcl["segm"][t].reshape(-1), pcl["rgb"][t].reshape(-1, 3), c["frames"][t]["colours"], *frame_mode(c, t))


# ------------------------------------------------------------------------------------------------------------ the colours
@pytest.mark.parametrize("name", CASE_NAMES)
def test_colours_equal_the_reference(gpu, name):
    from gcd_amd import geometry as G
    c, pcl = case(name), cloud(gpu, name)
    for t, fr in enumerate(c["frames"]):
        mode, alpha = frame_mode(c, t)
        out, status = G.class_colours(pcl["segm"][t], pcl["rgb"][t], palette(gpu), alpha, mode, n_classes=gold()["n_classes"])
        assert out.dtype == torch.float64 and tuple(out.shape) == (17 * 40, 3) and out.is_contiguous()
        assert status.dtype == torch.int64 and status.tolist() == [0]
        differ = int((bits(out.cpu()) != bits(fr["colours"])).sum())
        print(f"[{fr['name']}] mode {mode} alpha {alpha:.4f}: {differ} of {out.numel()} values differ")
        assert differ == 0
        again, _ = G.class_colours(pcl["segm"][t], pcl["rgb"][t], palette(gpu), alpha, mode, n_classes=gold()["n_classes"])
        assert torch.equal(bits(out), bits(again)), f"{fr['name']}: two calls differ"
    # the modes by name, and the operands a mode does not read left out
    ids, rgb, want, mode, alpha = flat_frame(gpu, name, 0)
    word = {RGB: "rgb", BLEND: "blend", PALETTE: "palette"}[mode]
    out, _ = G.class_colours(None if mode == RGB else ids, None if mode == PALETTE else rgb, palette(gpu), alpha, word)
    assert torch.equal(bits(out.cpu()), bits(want))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 680, 1023, 1024, 1025, 2720])
def test_colours_at_every_size(gpu, n):
    """Up to 680 points: a part of one workgroup's 1 024; 1 023 .. 1 025: the edge of the first; 2 720: three, the last
    one ragged (the golden's cloud four times over)."""
    from gcd_amd import geometry as G
    ids, rgb, want, mode, alpha = flat_frame(gpu)
    ids, rgb, want = ids.repeat(4)[:n], rgb.repeat(4, 1)[:n], want.repeat(4, 1)[:n]
    for m, a in ((mode, alpha), (PALETTE, 1.0), (RGB, 0.0)):
        out, status = G.class_colours(ids, rgb, palette(gpu), a, m, n_classes=gold()["n_classes"])
        ref = want if m == mode else header_formula(ids.cpu(), rgb.cpu(), gold()["palette"], a, m)
        assert tuple(out.shape) == (n, 3) and status.tolist() == [0]
        assert torch.equal(bits(out.cpu()), bits(ref)), (n, m)


def test_strided_operands_and_an_out_inside_a_guarded_buffer(gpu):
    """(V, N, .) clouds that are slices of wider ones, and out_ld = 5: nothing but the (N, 3) payload is written."""
    from gcd_amd import geometry as G
    c, pcl = case("segm_m3"), cloud(gpu, "segm_m3")
    want = c["frames"][2]["colours"]
    wide_ids = torch.full((17, 40, 4), 255, dtype=torch.uint8, device=gpu)
    wide_rgb = torch.full((17, 40, 6), 77, dtype=torch.uint8, device=gpu)
    wide_ids[:, :, 2:3], wide_rgb[:, :, 1:4] = pcl["segm"][2], pcl["rgb"][2]
    ids, rgb = wide_ids[:, :, 2:3], wide_rgb[:, :, 1:4]
    assert not ids.is_contiguous() and not rgb.is_contiguous()
    n, guard = 680, 64
    poison = 0x7FF8A5A5A5A5A5A5
    buf = torch.full((n + 2 * guard, 5), poison, dtype=torch.int64, device=gpu)
    out = buf.view(torch.float64)[guard:guard + n, :3]
    got, status = G.class_colours(ids, rgb, palette(gpu), 2.0 / 3.0, "blend", out=out, n_classes=gold()["n_classes"])
    assert got.data_ptr() == out.data_ptr() and got.stride(0) == 5 and status.tolist() == [0]
    assert torch.equal(bits(out.cpu()), bits(want))
    assert bool((buf[:guard] == poison).all()) and bool((buf[guard + n:] == poison).all()) and bool((buf[:, 3:] == poison).all())
    # a cloud whose points have no common stride is copied, not misread
    ragged = torch.zeros(17, 41, 3, dtype=torch.uint8, device=gpu)[:, :40]
    ragged.copy_(pcl["rgb"][2])
    got, _ = G.class_colours(pcl["segm"][2], ragged, palette(gpu), 2.0 / 3.0, "blend", n_classes=gold()["n_classes"])
    assert torch.equal(bits(got.cpu()), bits(want))
    with pytest.raises(Exception):
        G.class_colours(ids, rgb, palette(gpu), 0.5, "blend", out=torch.empty(680, 3, device=gpu))          # float32
    with pytest.raises(Exception):
        G.class_colours(ids, rgb, palette(gpu), 0.5, "blend", out=torch.empty(679, 3, dtype=torch.float64, device=gpu))


def test_offsets_past_the_32_bit_marks(gpu):
    """4 100 points whose rows lie 2^20 bytes apart: byte offsets of `out` and of the colours pass 2^31 and 2^32.  The
    allocations are large and almost wholly untouched."""
    from gcd_amd import geometry as G
    ids, rgb, want, mode, alpha = flat_frame(gpu)
    n = 4100
    ids, rgb_small = ids.repeat(7)[:n].contiguous(), rgb.repeat(7, 1)[:n]
    want = want.repeat(7, 1)[:n]
    big_rgb = torch.empty(n, 1 << 20, dtype=torch.uint8, device=gpu)
    big_out = torch.empty(n, 1 << 17, dtype=torch.float64, device=gpu)
    assert big_out.stride(0) * 8 * (n - 1) > 2 ** 32 and big_rgb.stride(0) * (n - 1) > 2 ** 32
    big_rgb[:, :4] = 99
    big_rgb[:, :3] = rgb_small
    big_out[:, :4] = -7.0
    out, status = G.class_colours(ids, big_rgb[:, :3], palette(gpu), alpha, mode, out=big_out[:, :3], n_classes=gold()["n_classes"])
    assert status.tolist() == [0] and torch.equal(bits(out.cpu()), bits(want))
    assert bool((big_out[:, 3] == -7.0).all())
    del big_rgb, big_out, out
    torch.cuda.empty_cache()


def test_ids_out_of_range_give_the_colour_zero_and_are_counted(gpu):
    """The one difference in behaviour: the reference's lookup raises IndexError, a kernel cannot."""
    from gcd_amd import geometry as G
    ids, rgb, _, _, _ = flat_frame(gpu)
    ids, rgb = ids.repeat(2), rgb.repeat(2, 1)            # two workgroups: the counts of both are summed
    n_classes = 5
    expected = int((ids >= n_classes).sum())
    assert 0 < expected < ids.numel()
    clipped = gold()["palette"].clone()
    clipped[n_classes:] = 0.0
    for mode, alpha in ((BLEND, 1.0 / 3.0), (PALETTE, 1.0), (RGB, 0.0)):
        out, status = G.class_colours(ids, rgb, palette(gpu), alpha, mode, n_classes=n_classes)
        assert status.tolist() == [0 if mode == RGB else expected], mode
        assert torch.equal(bits(out.cpu()), bits(header_formula(ids.cpu(), rgb.cpu(), clipped, alpha, mode))), mode
        if mode == PALETTE:
            assert not bool(out[ids >= n_classes].any())
    # every call stores the count: a clean call after a counting one reports 0
    _, status = G.class_colours(ids, rgb, palette(gpu), 0.5, BLEND, n_classes=256)
    assert status.tolist() == [0]
    all_ids = torch.arange(256, dtype=torch.uint8, device=gpu)
    out, status = G.class_colours(all_ids, None, palette(gpu), 1.0, PALETTE, n_classes=1)
    assert status.tolist() == [255] and torch.equal(out[0].cpu(), gold()["palette"][0]) and not bool(out[1:].any())


def test_graph_replay_equals_eager(gpu):
    from gcd_amd import geometry as G
    ids, rgb, want, mode, alpha = flat_frame(gpu)
    ids, rgb = ids.clone(), rgb.clone()
    eager, _ = G.class_colours(ids, rgb, palette(gpu), alpha, mode)
    out = torch.zeros_like(eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        G.class_colours(ids, rgb, palette(gpu), alpha, mode, out=out)                  # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, status = G.class_colours(ids, rgb, palette(gpu), alpha, mode, out=out, n_classes=5)
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    clipped = gold()["palette"].clone()
    clipped[5:] = 0.0
    assert torch.equal(bits(out.cpu()), bits(header_formula(ids.cpu(), rgb.cpu(), clipped, alpha, mode)))
    count = int((ids >= 5).sum())
    assert status.tolist() == [count]
    # a replay reads the operands where they lie and starts its count again
    ids.fill_(0)
    graph.replay()
    torch.cuda.synchronize()
    assert status.tolist() == [0]
    assert torch.equal(bits(out.cpu()), bits(header_formula(ids.cpu(), rgb.cpu(), clipped, alpha, mode)))
    assert torch.equal(bits(eager.cpu()), bits(want))


# ---------------------------------------------------------------------------------------------------- through the renderer
@pytest.mark.parametrize("name", CASE_NAMES)
def test_splat_of_the_recorded_colours(gpu, name):
    """Stage 1: the existing splat on float16 positions and the float64 colours the reference built."""
    from gcd_amd import geometry as G
    c, pcl = case(name), cloud(gpu, name)
    for t, fr in enumerate(c["frames"]):
        got = G.project_points_to_pixels((pcl["xyz"][t].reshape(-1, 3), fr["colours"].to(gpu)), fr["K"], fr["RT"], fr["H"], fr["W"],
                                         fr["radius"])
        check_splat(fr["name"], tuple(x.cpu() for x in got), fr)


def _clip(gpu, name, **kw):
    from gcd_amd import geometry as G
    c = case(name)
    g = gold()
    args = dict(palette=palette(gpu), n_classes=g["n_classes"], modal_time=c["modal_time"], model_frames=c["T"],
                render_height=c["render_hw"][0], render_width=c["render_hw"][1], frame_height=c["frame_hw"][0],
                frame_width=c["frame_hw"][1], spread_radius=c["radius"])
    args.update(kw)
    return G.synth_rgb_pardom(cloud(gpu, name), c["modality"], c["extrinsics"], c["intrinsics"], **args)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_fill_of_the_golden_images_and_the_clip_end_to_end(gpu, name):
    from gcd_amd import geometry as G
    c = case(name)
    T, fhw = c["T"], tuple(c["frame_hw"])
    rgb, reproject = _clip(gpu, name, calc_reproject=c["reproject"], reproject_rgbd=c["reproject"])
    assert rgb.is_cuda and rgb.dtype == torch.float32 and tuple(rgb.shape) == (T, 3, *fhw)
    assert (reproject is not None) == c["reproject"]
    # stage 2 fed the golden's own splat images
    batch = torch.full((T, 3, *fhw), float("nan"), device=gpu)
    for t, fr in enumerate(c["frames"]):
        G.fill_resize(fr["img"].to(gpu), batch[t], 21, 5.25)
    e64 = float((batch.cpu().double() - c["rgb_f64"]).abs().max())
    eref = float((batch.cpu().double() - c["rgb_ref"].double()).abs().max())
    e2e = float((rgb.cpu().double() - c["rgb_f64"]).abs().max())
    print(f"[{name}] fill vs float64 chain {e64:.3e} (bar {2.0 ** -22:.3e}); vs reference dtypes {eref:.3e} (bar 4 x {c['gap']:.3e}); "
          f"end to end {e2e:.3e} (bar {2.0 ** -20:.3e})")
    assert e64 <= 2.0 ** -22
    assert eref <= 4.0 * c["gap"]
    assert e2e <= 2.0 ** -20
    if c["reproject"]:
        assert reproject.dtype == torch.float32 and tuple(reproject.shape) == (T, 3, *fhw)
        for t, fr in enumerate(c["frames"]):
            G.fill_resize(fr["reproject_img"].to(gpu), batch[t], 3, 0.75)
        r64 = float((batch.cpu().double() - c["reproject_f64"]).abs().max())
        rref = float((batch.cpu().double() - c["reproject_ref"].double()).abs().max())
        r2e = float((reproject.cpu().double() - c["reproject_f64"]).abs().max())
        print(f"[{name}] reproject: fill vs float64 chain {r64:.3e}; vs reference dtypes {rref:.3e} (bar 4 x {c['gap_reproject']:.3e}); "
              f"end to end {r2e:.3e}")
        assert r64 <= 2.0 ** -22
        assert rref <= 4.0 * c["gap_reproject"]
        assert r2e <= 2.0 ** -20
        assert not torch.equal(reproject, rgb)


def test_reproject_is_made_when_both_flags_are_set_and_only_then(gpu):
    full = _clip(gpu, "segm_m3", calc_reproject=True, reproject_rgbd=True)
    assert full[1] is not None
    for calc, rgbd in ((False, False), (True, False), (False, True)):
        rgb, reproject = _clip(gpu, "segm_m3", calc_reproject=calc, reproject_rgbd=rgbd)
        assert reproject is None and torch.equal(rgb, full[0])
    rgb, reproject = _clip(gpu, "segm_m3")
    assert reproject is None and torch.equal(rgb, full[0])


def test_rgb_modality_is_render_views_on_the_same_cloud(gpu):
    """The `rgb` modality launches no colour kernel: the stored uint8 colours go to the splat as they are, and frame 0 of a
    `segm` clip with modal_time > 0 (mode RGB: the same values as float64) gives the same frame."""
    from gcd_amd import geometry as G
    c, pcl = case("rgb"), cloud(gpu, "rgb")
    rgb, reproject = _clip(gpu, "rgb", calc_reproject=True, reproject_rgbd=True, palette=None)
    for t, fr in enumerate(c["frames"]):
        want = G.render_views(pcl["xyz"][t].reshape(-1, 3), pcl["rgb"][t].reshape(-1, 3), fr["K"], fr["RT"][None], c["render_hw"],
                              c["frame_hw"], c["radius"], 21, 5.25)
        assert torch.equal(bits(rgb[t]), bits(want[0]))
        want = G.render_views(pcl["xyz"][t][16], pcl["rgb"][t][16], fr["K"], fr["RT"][None], c["render_hw"], c["frame_hw"],
                              c["radius"], 3, 0.75)
        assert torch.equal(bits(reproject[t]), bits(want[0]))
    segm, _ = _clip(gpu, "segm_m3")
    assert torch.equal(bits(segm[0]), bits(rgb[0]))
    with pytest.raises(ValueError):
        _clip(gpu, "segm_m3", palette=None)
