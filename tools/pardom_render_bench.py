"""Time the rendering of one ParallelDomain clip on the device (a record, not a gate).

    python tools/pardom_render_bench.py [--views 19] [--points 307200] [--frames 14] [--render 280x420] [--frame 256x384]
                                        [--radius 1] [--modal-times 0,7] [--repeats 5] [--out FILE]

One clip at the shipped configs' shape: `--frames` frames of `--views` stored views x `--points` points (float16 positions,
uint8 colours, uint8 class ids, as the cached clouds are stored), the `segm` modality, rendered at `--render` and resized to
`--frame`.  Two routes in one process, alternated, device events around the whole clip, median of `--repeats`, per
`modal_time`:

  new     gcd_amd.geometry.synth_rgb_pardom: the colour kernel into one reused (N, 3) float64 buffer, then the splat;
  torch   the same stage written with torch ops on the same GPU, in the shape of the original data module: colours / 255 in
          float32, the float64 table indexed by the ids as int64, the blend, a float64 (N, 6) tensor, and the torch view of
          tools/render_bench.py.  (The original itself is not on the GPU machine; this stands in for what it launches.)

Reported per route: ms per clip and per frame and peak device memory; then the colour kernel alone against its torch
expression (colours / 255, the lookup and the blend, nothing of the splat), per mode, per frame of views x points points.
The frames of the two routes are compared so that a timing never stands for a wrong picture.
"""
from __future__ import annotations

import argparse
import importlib.util
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

N_CLASSES = 40


def load_render_bench():
    spec = importlib.util.spec_from_file_location("render_bench", ROOT / "tools" / "render_bench.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def make_frame(V, n, seed, t, dev):
    """A street: a ground plane 240 m long, boxes beside it that move with t, a far backdrop past depth 64; class ids by
    height band.  (V, n, 3) float16, (V, n, 3) uint8, (V, n, 1) uint8, made on the device."""
    g = torch.Generator(device=dev).manual_seed(seed)
    N = V * n
    u = torch.rand(N, 3, generator=g, device=dev)
    kind = torch.rand(N, generator=g, device=dev)
    ground = torch.stack([u[:, 0] * 240.0 - 40.0, u[:, 1] * 40.0 - 20.0, torch.zeros(N, device=dev)], dim=1)
    boxes = torch.stack([u[:, 0] * 120.0 - 10.0 + 0.4 * t, torch.where(u[:, 1] < 0.5, -9.0 - 4.0 * u[:, 1], 7.0 + 4.0 * u[:, 1]),
                         u[:, 2] * 6.0], dim=1)
    far = torch.stack([200.0 + 600.0 * u[:, 0], u[:, 1] * 600.0 - 300.0, u[:, 2] * 60.0], dim=1)
    xyz = torch.where((kind < 0.55)[:, None], ground, torch.where((kind < 0.9)[:, None], boxes, far))
    rgb = ((torch.sin(xyz * torch.tensor([0.13, 0.17, 0.9], device=dev)) * 0.5 + 0.5) * 255.0).to(torch.uint8)
    ids = ((xyz[:, 2] * 3.0).clamp(0, N_CLASSES - 2) + (kind >= 0.9) * 1.0).to(torch.uint8)
    return xyz.half().reshape(V, n, 3), rgb.reshape(V, n, 3), ids.reshape(V, n, 1)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def measure(routes, repeats):
    """Warm-up with peak memory and outputs, then `repeats` alternated rounds: ({name: median ms}, times, peaks, outputs)."""
    times = {n: [] for n in routes}
    peak, outs = {}, {}
    for name, fn in routes.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        _, outs[name] = timed(fn)
        peak[name] = torch.cuda.max_memory_allocated() - base
    for _ in range(repeats):
        for name, fn in routes.items():
            times[name].append(timed(fn)[0])
    return {n: statistics.median(v) for n, v in times.items()}, times, peak, outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=19)
    ap.add_argument("--points", type=int, default=307_200)
    ap.add_argument("--frames", type=int, default=14)
    ap.add_argument("--render", default="280x420")
    ap.add_argument("--frame", default="256x384")
    ap.add_argument("--radius", type=int, default=1)
    ap.add_argument("--modal-times", default="0,7")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from gcd_amd import geometry as G
    assert torch.cuda.is_available(), "pardom_render_bench needs the GPU: there is nothing to time without it"
    RB = load_render_bench()
    dev = torch.device("cuda:0")
    H, W = (int(v) for v in args.render.split("x"))
    fhw = tuple(int(v) for v in args.frame.split("x"))
    T, V, n = args.frames, args.views, args.points
    N = V * n
    pcl = dict(xyz=[], rgb=[], segm=[])
    for t in range(T):
        x, c, s = make_frame(V, n, 300 + t, float(t), dev)
        pcl["xyz"].append(x), pcl["rgb"].append(c), pcl["segm"].append(s)
    g = torch.Generator().manual_seed(5)
    items = [dict(id=k, color=dict(zip("rgb", torch.randint(0, 256, (3,), generator=g).tolist()))) for k in range(N_CLASSES)]
    palette, n_classes = G.semantic_palette(items)
    palette = palette.to(dev)
    # the dataset's default target camera, drifting forward; intrinsics on the unit image, a little different per frame
    rts = torch.tensor(np.stack([G.extrinsics_from_look_at(np.array([-8.0 + 0.5 * t, 0.0, 8.0]), np.array([5.6 + 0.5 * t, 0.0, 1.55]))
                                 for t in range(T)]), dtype=torch.float32)
    Kn = torch.tensor([[0.62, 0.0, 0.5], [0.0, 0.93, 0.5], [0.0, 0.0, 1.0]]).repeat(T, 1, 1)
    Kn[:, 0, 0] += 0.002 * torch.arange(T)
    K = Kn.clone()
    K[:, 0, :] *= W
    K[:, 1, :] *= H
    if W / H > 640.0 / 480.0 + 1e-3:
        K[:, 1, 1] = K[:, 0, 0]
    elif W / H < 640.0 / 480.0 - 1e-3:
        K[:, 0, 0] = K[:, 1, 1]
    Kd, rd = K.to(dev), rts.to(dev)
    k, sigma = 21, 21 / 4.0

    def torch_colours(t, mode, alpha):
        """The colours of frame t with torch ops: float32 stored colours, float64 table rows, the blend promoted by torch."""
        stored = (pcl["rgb"][t] / 255.0).float()
        if mode == G._lib_pardom.PARDOM_RGB:
            return stored
        ids = pcl["segm"][t]
        rows = palette[:n_classes][ids.reshape(-1).long()].reshape(V, n, 3)
        if mode == G._lib_pardom.PARDOM_BLEND:
            return (1.0 - alpha) * stored + alpha * rows
        return rows

    lines = [f"pardom_render_bench: {torch.cuda.get_device_name(0)}; {T} frames of {V} views x {n} points = {N} points per frame "
             f"(float16 + uint8 + uint8 ids), segm, render {H}x{W} -> {fhw[0]}x{fhw[1]}, radius {args.radius}, k {k}; "
             f"median of {args.repeats}, routes alternated"]
    for modal_time in (int(v) for v in args.modal_times.split(",")):
        def new_route():
            return G.synth_rgb_pardom(pcl, "segm", rts, Kn, palette=palette, n_classes=n_classes, modal_time=modal_time,
                                      model_frames=T, render_height=H, render_width=W, frame_height=fhw[0], frame_width=fhw[1],
                                      spread_radius=args.radius)[0]

        def torch_route():
            out = torch.empty(T, 3, *fhw, device=dev)
            for t in range(T):
                mode, alpha = G.pardom_frame_mode(t, modal_time, "segm")
                vis = torch_colours(t, mode, alpha)
                cloud = torch.cat([pcl["xyz"][t].float(), vis], dim=-1).reshape(-1, 6).double()
                out[t] = RB.torch_view(cloud, Kd[t], rd[t], H, W, args.radius, k, sigma, fhw)
            return out

        med, times, peak, outs = measure({"new": new_route, "torch": torch_route}, args.repeats)
        diff = float((outs["new"] - outs["torch"]).abs().max())
        diff_mean = float((outs["new"] - outs["torch"]).abs().mean())
        lines += [
            f"modal_time {modal_time}:",
            f"  new    : {med['new']:9.2f} ms per clip = {med['new'] / T:7.3f} ms per frame  (min {min(times['new']):.2f}, max {max(times['new']):.2f}); "
            f"peak memory {peak['new'] / 2 ** 20:.1f} MiB (the colour buffer is {N * 24 / 2 ** 20:.1f} MiB of it)",
            f"  torch  : {med['torch']:9.2f} ms per clip = {med['torch'] / T:7.3f} ms per frame  (min {min(times['torch']):.2f}, max {max(times['torch']):.2f}); "
            f"peak memory {peak['torch'] / 2 ** 20:.1f} MiB",
            f"  torch / new: {med['torch'] / med['new']:.2f}x; frames of the two routes differ by at most {diff:.3e} (mean {diff_mean:.3e})",
        ]
    # the colour kernel alone
    buf = torch.empty(N, 3, dtype=torch.float64, device=dev)
    P = G._lib_pardom
    for word, mode, alpha in (("PALETTE", P.PARDOM_PALETTE, 1.0), ("BLEND 3/7", P.PARDOM_BLEND, 3.0 / 7.0), ("RGB", P.PARDOM_RGB, 0.0)):
        def kernel():
            for t in range(T):
                G.class_colours(pcl["segm"][t], pcl["rgb"][t], palette, alpha, mode, out=buf, n_classes=n_classes)
            return buf

        def expression():
            for t in range(T):
                out = torch_colours(t, mode, alpha).type(torch.float64)
            return out.reshape(-1, 3)

        med, times, peak, outs = measure({"kernel": kernel, "torch": expression}, args.repeats)
        same = bool(torch.equal(outs["kernel"], outs["torch"]))
        moved = N * (24 + (3 if mode != P.PARDOM_PALETTE else 0) + (1 if mode != P.PARDOM_RGB else 0))
        lines.append(
            f"colours {word:9s}: kernel {med['kernel'] / T * 1e3:8.1f} us per frame ({moved / (med['kernel'] / T) / 1e6:.0f} GB/s of "
            f"{moved / 1e6:.0f} MB; min {min(times['kernel']) / T * 1e3:.1f}, max {max(times['kernel']) / T * 1e3:.1f}), peak {peak['kernel'] / 2 ** 20:.1f} MiB beside the "
            f"buffer; torch expression (to float64) {med['torch'] / T * 1e3:8.1f} us per frame, peak {peak['torch'] / 2 ** 20:.1f} MiB; "
            f"torch / kernel {med['torch'] / med['kernel']:.2f}x; last frame bit-identical: {same}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
