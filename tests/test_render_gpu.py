"""GPU: libgcd_amd_render.so against tests/golden/render_tiny.pt (tools/make_golden_render.py) at the bars of DESIGN.md §12.2.

Splat: img is zero exactly where the reference's is, elsewhere within one fp32 ulp; pixel_weights within 1e-9 relative;
uv and depth within 1e-12 where depth > 0.1.  Stage 2 fed the golden's own splat image: within 2^-22 of the float64 chain
and within 4 x the recorded dtype gap of the chain in the reference's dtypes.  End to end: 2^-20.  Two calls, a call with
two cameras against two calls with one, and a graph replay against eager are bit-identical.

Measured on an MI355X: see DESIGN.md §12.2."""
import pytest
import torch

from render_util import check_float_colours, check_splat, float_colour_cloud, golden_cloud, load_golden

pytestmark = pytest.mark.gpu

_GOLD = None


def gold():
    global _GOLD
    if _GOLD is None:
        _GOLD = load_golden()
    return _GOLD


CASE_NAMES = ["base_r1", "base_r2", "base_r3", "base_r2_cam_b", "past_int32", "far", "ragged_f64", "f16_u8", "one_pixel", "n0", "none_visible",
              "occluder_near", "occluder_far"]
FILLS = [("base_r1", 21), ("base_r1", 3), ("ragged_f64", 21), ("ragged_f64", 3), ("occluder_near", 21), ("occluder_near", 3)]


def case(name):
    return next(c for c in gold()["cases"] if c["name"] == name)


def fill_record(src, k):
    return next(f for f in gold()["fills"] if f["src"] == src and f["k"] == k)


def device_splat(gpu, c):
    from gcd_amd import geometry as G
    xyz, rgb = golden_cloud(gold(), c)
    out = G.project_points_to_pixels((xyz.to(gpu), rgb.to(gpu)), c["K"], c["RT"], c["H"], c["W"], c["radius"])
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", CASE_NAMES)
def test_splat_against_the_reference(gpu, name):
    c = case(name)
    got = device_splat(gpu, c)
    assert got[0].dtype == torch.float32 and tuple(got[0].shape) == (c["H"], c["W"], 3)
    assert got[1].dtype == torch.float64 and tuple(got[1].shape) == (c["H"], c["W"], 1)
    n = golden_cloud(gold(), c)[0].shape[0]
    assert got[2].dtype == torch.float64 and tuple(got[2].shape) == (n, 2) and tuple(got[3].shape) == (n, 1)
    check_splat(name, tuple(t.cpu() for t in got), c)
    again = device_splat(gpu, c)
    for a, b in zip(got[:2], again[:2]):
        assert torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int64),
                           b.view(torch.int32 if b.dtype == torch.float32 else torch.int64)), f"{name}: two calls differ"


def test_float_colours_tiny_and_above_one(gpu):
    """Against the float64 evaluation of the reference's formula: tiny colours under bright ones, colours above 1."""
    from gcd_amd import geometry as G
    xyz, rgb, K, RT, H, W = float_colour_cloud()
    for radius in (0, 2):
        img, pw, _, _ = G.project_points_to_pixels((xyz.to(gpu), rgb.to(gpu)), K, RT, H, W, radius)
        check_float_colours(img.cpu(), pw.cpu(), radius)


def test_visible_count_and_the_empty_set(gpu):
    """A difference from the reference (it raises): no visible point gives a zero image, -1 weights and a count of 0."""
    from gcd_amd import geometry as G
    for name in ("base_r2", "n0", "none_visible"):
        c = case(name)
        xyz, rgb = golden_cloud(gold(), c)
        img, pw, _, _, status = G.splat(xyz.to(gpu), rgb.to(gpu), G.pack_cameras(c["K"], c["RT"], gpu), c["H"], c["W"], c["radius"])
        assert status.dtype == torch.int64 and status.tolist() == [c["visible"]], (name, status.tolist(), c["visible"])
        if c["visible"] == 0:
            assert bool((img == 0).all()) and bool((pw == -1).all())


def test_xyzrgb_tensor_and_pair_are_the_same_call(gpu):
    from gcd_amd import geometry as G
    c = case("ragged_f64")
    xyz, rgb = golden_cloud(gold(), c)
    pair = G.project_points_to_pixels((xyz.to(gpu), rgb.to(gpu)), c["K"], c["RT"], c["H"], c["W"], c["radius"])
    one = G.project_points_to_pixels(torch.cat([xyz, rgb], dim=1).to(gpu), c["K"], c["RT"], c["H"], c["W"], c["radius"])
    for a, b in zip(pair, one):
        assert torch.equal(a, b)


def test_two_cameras_in_one_pass_equal_two_passes_bit_for_bit(gpu):
    from gcd_amd import geometry as G
    a, b = case("base_r2"), case("base_r2_cam_b")
    xyz, rgb = (t.to(gpu) for t in golden_cloud(gold(), a))
    both = G.splat(xyz, rgb, G.pack_cameras(a["K"], torch.stack([a["RT"], b["RT"]]), gpu), a["H"], a["W"], 2, want_uv_depth=True)
    for i, c in enumerate((a, b)):
        single = G.splat(xyz, rgb, G.pack_cameras(c["K"], c["RT"], gpu), c["H"], c["W"], 2, want_uv_depth=True)
        for x, y in zip(both, single):
            assert torch.equal(x[i].reshape(-1).view(torch.uint8), y[0].reshape(-1).view(torch.uint8)), f"camera {i}"
        check_splat(c["name"] + " (nc = 2)", (both[0][i].cpu(), both[1][i].cpu(), both[2][i].cpu(), both[3][i].cpu()), c)


@pytest.mark.parametrize("src,k", FILLS)
def test_fill_and_resize_of_the_golden_image(gpu, src, k):
    from gcd_amd import geometry as G
    f = fill_record(src, k)
    img = case(src)["img"].to(gpu)
    batch = torch.full((3, 3, *f["frame_hw"]), float("nan"), device=gpu)
    G.fill_resize(img, batch[1], k, f["sigma"])                    # a slot of a (T, 3, Hp, Wp) batch
    got = batch[1].cpu().double()
    assert bool(torch.isnan(batch[0]).all()) and bool(torch.isnan(batch[2]).all())
    e64 = float((got - f["frames_f64"]).abs().max())
    eref = float((got - f["frames_ref"].double()).abs().max())
    print(f"[fill {src} k={k}] vs float64 chain {e64:.3e} (bar {2.0 ** -22:.3e}); vs reference dtypes {eref:.3e} "
          f"(bar 4 x {f['gap_frames']:.3e})")
    assert e64 <= 2.0 ** -22
    assert eref <= 4.0 * f["gap_frames"]


def test_blur_into_black_keeps_the_reference_signature(gpu):
    from gcd_amd import geometry as G
    f = fill_record("base_r1", 5)
    img = case("base_r1")["img"].to(gpu)
    out = G.blur_into_black(img)                                   # kernel_size = 5, sigma = 1.5
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(img.shape) and out.is_contiguous()
    e64 = float((out.cpu().double() - f["blur_f64"]).abs().max())
    eref = float((out.cpu().double() - f["blur_ref"].double()).abs().max())
    print(f"[blur_into_black] vs float64 chain {e64:.3e} (bar {2.0 ** -23:.3e}); vs reference dtypes {eref:.3e} (bar 4 x {f['gap_blur']:.3e})")
    assert e64 <= 2.0 ** -23                                       # values in [0, 1]: without the factor 2 of the frames
    assert eref <= 4.0 * f["gap_blur"]


@pytest.mark.parametrize("src,k", [("base_r1", 21), ("ragged_f64", 21), ("base_r1", 3)])
def test_end_to_end_against_the_float64_chain(gpu, src, k):
    from gcd_amd import geometry as G
    c, f = case(src), fill_record(src, k)
    xyz, rgb = (t.to(gpu) for t in golden_cloud(gold(), c))
    out = G.render_views(xyz, rgb, c["K"], c["RT"][None], (c["H"], c["W"]), f["frame_hw"], c["radius"], k, f["sigma"])
    assert tuple(out.shape) == (1, 3, *f["frame_hw"]) and out.dtype == torch.float32
    e = float((out[0].cpu().double() - f["frames_f64"]).abs().max())
    print(f"[end to end {src} k={k}] {e:.3e} (bar {2.0 ** -20:.3e})")
    assert e <= 2.0 ** -20


def _pcl_dict(gpu, frames=3, views=5, n=400):
    g = torch.Generator().manual_seed(7)
    xyz = [(torch.rand(views, n, 3, generator=g) * torch.tensor([3.0, 3.0, 1.5]) - torch.tensor([1.5, 1.5, 0.0])).half().to(gpu)
           for _ in range(frames)]
    rgb = [torch.randint(0, 256, (views, n, 3), generator=g, dtype=torch.uint8).to(gpu) for _ in range(frames)]
    return dict(xyz=xyz, rgb=rgb, segm_rgb=rgb)


def test_synth_src_dst_rgb_gives_the_frames_of_the_single_functions(gpu):
    """The dataset method restated, the fused route and the reference-signature functions chained by hand give the
    same frames, bit for bit: they are the same kernels on the same operands."""
    import numpy as np
    from gcd_amd import geometry as G
    T, rh, rw, fh, fw, radius = 3, 24, 40, 16, 24, 2
    pcl = _pcl_dict(gpu, T)
    look = np.array([0.0, 0.0, 0.5])
    src = torch.tensor(np.stack([G.extrinsics_from_look_at(G.cartesian_from_spherical(np.array([20.0 + 5 * t, 15.0, 6.0]), deg2rad=True),
                                                           look) for t in range(T)]), dtype=torch.float32)
    dst = torch.tensor(np.stack([G.extrinsics_from_look_at(G.cartesian_from_spherical(np.array([60.0 - 9 * t, 30.0, 7.0]), deg2rad=True),
                                                           look) for t in range(T)]), dtype=torch.float32)
    Kn = torch.tensor([[1.2, 0.0, 0.5], [0.0, 1.6, 0.5], [0.0, 0.0, 1.0]]).expand(T, 3, 3)
    rgb_src, rgb_dst, rep = G.synth_src_dst_rgb(pcl, src, dst, Kn, src, model_frames=T, render_height=rh, render_width=rw,
                                                frame_height=fh, frame_width=fw, spread_radius=radius, reproject_rgbd=True)
    for t_ in (rgb_src, rgb_dst, rep):
        assert t_.is_cuda and t_.dtype == torch.float32 and tuple(t_.shape) == (T, 3, fh, fw)
        assert bool(torch.isfinite(t_).all()) and float(t_.min()) >= -1.0 - 1e-6 and float(t_.max()) <= 1.0 + 1e-6
    assert float(rgb_src.max()) > -1.0 and not torch.equal(rgb_src, rgb_dst)
    none = G.synth_src_dst_rgb(pcl, src, dst, Kn, src, model_frames=T, render_height=rh, render_width=rw, frame_height=fh,
                               frame_width=fw, spread_radius=radius)
    assert none[2] is None and torch.equal(none[0], rgb_src) and torch.equal(none[1], rgb_dst)
    # the intrinsics of the method: scaled to pixels in float32; 40 / 24 is wider than 576 / 384, so fy := fx
    K = Kn[0].clone()
    K[0] *= rw
    K[1] *= rh
    K[1, 1] = K[0, 0]
    for t in range(T):
        xyz, rgb = pcl["xyz"][t].reshape(-1, 3), pcl["rgb"][t].reshape(-1, 3)
        fused = G.render_views(xyz, rgb, K, torch.stack([src[t], dst[t]]), (rh, rw), (fh, fw), radius, 21, 5.25)
        assert torch.equal(fused[0], rgb_src[t]) and torch.equal(fused[1], rgb_dst[t])
        # by hand, as the dataset does it: float32 cloud, colours / 255 in float32 on the host (a true division; the
        # device's division by a scalar multiplies by the reciprocal), one (N, 6) tensor
        xyzrgb = torch.cat([xyz.float(), (rgb.cpu() / 255.0).float().to(gpu)], dim=-1)
        for RT, want in ((src[t], rgb_src[t]), (dst[t], rgb_dst[t])):
            img, _, _, _ = G.project_points_to_pixels(xyzrgb, K, RT, rh, rw, spread_radius=radius)
            slot = torch.empty(3, fh, fw, device=gpu)
            G.fill_resize(img, slot, 21, 5.25)
            assert torch.equal(slot, want)
        img, _, _, _ = G.project_points_to_pixels((pcl["xyz"][t][4], pcl["rgb"][t][4]), K, dst[t], rh, rw, spread_radius=radius)
        slot = torch.empty(3, fh, fw, device=gpu)
        G.fill_resize(img, slot, 3, 0.75)
        assert torch.equal(slot, rep[t])


def test_graph_replay_equals_eager(gpu):
    from gcd_amd import geometry as G
    c = case("base_r2")
    xyz, rgb = (t.to(gpu) for t in golden_cloud(gold(), c))
    cams = G.pack_cameras(c["K"], torch.stack([c["RT"], case("base_r2_cam_b")["RT"]]), gpu)
    hw, fhw = (c["H"], c["W"]), (16, 24)
    eager = G.render_views(xyz, rgb, None, None, hw, fhw, 2, 21, 5.25, cams=cams).clone()
    out = torch.zeros(2, 3, *fhw, device=gpu)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        G.render_views(xyz, rgb, None, None, hw, fhw, 2, 21, 5.25, out=out, cams=cams)          # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        G.render_views(xyz, rgb, None, None, hw, fhw, 2, 21, 5.25, out=out, cams=cams)
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    # a replay reads the cameras where they lie: new cameras, same graph
    cams.copy_(G.pack_cameras(c["K"], torch.stack([case("base_r2_cam_b")["RT"], c["RT"]]), gpu))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], eager[1]) and torch.equal(out[1], eager[0])
