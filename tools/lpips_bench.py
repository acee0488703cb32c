"""Time the LPIPS metric of the validation step on the device (a record, not a gate).

    python tools/lpips_bench.py [--pairs 14] [--sizes 256x384,576x1024] [--repeats 5] [--out profiles/r16_lpips_bench.txt]

Seeded random weights at VGG-16's widths (tests/lpips_util.seeded_state_dict; no checkpoint ships with the project).  Two
routes in one process, alternated, device events around the whole call, one warm-up call each, median of `--repeats`:

  hip     gcd_amd.lpips.LPIPS: gcd_lpips_* kernels + gcd_gemm_f16, pairs chunked as the module chooses;
  torch   the same tower written with torch ops (tests/lpips_util.features / head: F.conv2d, relu, max_pool2d, NCHW) on the
          same GPU under fp16 autocast, all pairs in one batch: what PyTorch-ROCm would run for the reference's module.

Per configuration: ms per call and per pair for both routes, the GEMM share and TFLOP/s of the hip route (per-launch
device events, gcd_amd.ops.start_profile, in a run of its own), peak device memory, both routes against a float32 run of
the torch tower, and gcd_lpips_distance alone on the first and last taps' shapes with its achieved bytes per second
(every byte of f0 and f1 once).
"""
from __future__ import annotations

import argparse
import ctypes as C
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import torch  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def tower_flops(chns, n_images: int, H: int, W: int) -> float:
    """Multiply-adds x 2 of the 13 convolutions (the first at its true 3 input channels)."""
    import lpips_util as U
    total, cin = 0.0, 3
    for k, (convs, c) in enumerate(zip(U.SLICE_CONVS, chns)):
        for _ in convs:
            total += 2.0 * n_images * (H >> k) * (W >> k) * 9 * cin * c
            cin = c
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=14)
    ap.add_argument("--sizes", default="256x384,576x1024")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import lpips_util as U
    from gcd_amd import _lib, lpips as L, ops
    assert torch.cuda.is_available(), "lpips_bench needs the GPU: there is nothing to time without it"
    dev = torch.device("cuda:0")
    sd = U.seeded_state_dict(U.FULL, 3)
    model = U.gpu_model(U.FULL, sd, dev)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    lib = _lib.load()

    def torch_route(a, b, autocast=True):
        with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
            return U.head(sd_dev, U.features(sd_dev, a), U.features(sd_dev, b)).float()

    n = args.pairs
    lines = [f"lpips_bench: {torch.cuda.get_device_name(0)}; LPIPS (VGG-16 widths, seeded random weights), {n} frame pairs; "
             f"median of {args.repeats}, one warm-up call, routes alternated"]
    with torch.no_grad():
        for size in args.sizes.split(","):
            H, W = (int(v) for v in size.split("x"))
            x0, x1 = (t.to(dev) for t in U.seeded_images(n, H, W, 2000 + H))
            routes = {"hip": lambda: model(x0, x1), "torch": lambda: torch_route(x0, x1)}
            times, peak, outs = {k: [] for k in routes}, {}, {}
            for name, fn in routes.items():                # warm-up (packs, code objects, algorithm choice), peak memory
                fn()
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                _, outs[name] = timed(fn)
                peak[name] = torch.cuda.max_memory_allocated() - base
            for _ in range(args.repeats):
                for name, fn in routes.items():
                    times[name].append(timed(fn)[0])
            med = {k: statistics.median(v) for k, v in times.items()}
            prof = ops.start_profile()                     # per-launch events of the hip route's GEMMs, in a run of its own
            model(x0, x1)
            torch.cuda.synchronize()
            ops.stop_profile()
            gemm_ms, ms = 0.0, C.c_float()
            for rec in prof:
                if rec["kind"] == "gemm":
                    _lib.check(lib.gcd_event_elapsed_ms(rec["start"], rec["stop"], C.byref(ms)))
                    gemm_ms += ms.value
                lib.gcd_event_destroy(rec["start"])
                lib.gcd_event_destroy(rec["stop"])
            ref32 = torch.cat([torch_route(x0[i:i + 2], x1[i:i + 2], autocast=False) for i in range(0, n, 2)])
            rel = lambda y: float(((y.double() - ref32.double()).abs().reshape(-1)[1:] / ref32.double().reshape(-1)[1:]).max())
            flops = tower_flops(U.FULL, 2 * n, H, W)
            lines += [
                f"{n} pairs {H}x{W} ({model.pairs_per_chunk(H, W)} pairs per chunk):",
                f"  hip   : {med['hip']:8.2f} ms per call = {med['hip'] / n:6.2f} ms per pair (min {min(times['hip']):.2f}, max {max(times['hip']):.2f}); "
                f"GEMMs {gemm_ms:.2f} ms = {gemm_ms / med['hip']:.2f} of the call, {flops / gemm_ms / 1e9:.0f} TFLOP/s over GEMM time, "
                f"{flops / med['hip'] / 1e9:.0f} TFLOP/s over the call; peak memory {peak['hip'] / 2 ** 20:.0f} MiB",
                f"  torch : {med['torch']:8.2f} ms per call = {med['torch'] / n:6.2f} ms per pair (min {min(times['torch']):.2f}, max {max(times['torch']):.2f}); "
                f"{flops / med['torch'] / 1e9:.0f} TFLOP/s over the call; peak memory {peak['torch'] / 2 ** 20:.0f} MiB",
                f"  torch / hip: {med['torch'] / med['hip']:.2f}x; largest relative gap to the float32 torch tower over the pairs: "
                f"hip {rel(outs['hip']):.3e}, torch-fp16 {rel(outs['torch']):.3e}; identical pair: hip {float(outs['hip'].reshape(-1)[0])!r}, "
                f"torch-fp16 {float(outs['torch'].reshape(-1)[0])!r}",
            ]
            for k in (0, 4):                               # the distance kernel alone, on the first and last taps' shapes
                HW, Ck = (H >> k) * (W >> k), U.FULL[k]
                f0, f1, w = (t.to(dev) for t in U.seeded_features(1, HW, Ck, 7 + k))
                f0, f1 = f0.repeat(n, 1), f1.repeat(n, 1)
                tm = torch.empty(1, n, dtype=torch.float64, device=dev)
                out = torch.empty(n, dtype=torch.float32, device=dev)
                run = lambda: L.distance(f0, f1, w, n, HW, tm, 0, 1, out)
                run()
                t = statistics.median(timed(run)[0] for _ in range(args.repeats + 4))
                nbytes = 2 * n * HW * Ck * 2
                lines.append(f"  gcd_lpips_distance, tap {k} ({n} x {HW} pixels x {Ck} channels, {L.distance_blocks(HW, Ck)} workgroups per image): "
                             f"{t * 1e3:.1f} us, {nbytes / 2 ** 20:.1f} MiB read = {nbytes / t / 1e9:.2f} TB/s")
                del f0, f1
            del x0, x1, outs, ref32
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
