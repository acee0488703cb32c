"""Time the evaluation metrics of one clip on the host and on the device (a record, not a gate).

    python tools/metrics_bench.py [--size 576x1024] [--frames 14] [--samples 2] [--repeats 20] [--out FILE.json]

The frames start where the decoder leaves them: on the GPU.  With and without a re-projection mask, three figures:

  host     gcd_amd.metrics.calculate_metrics, including the device-to-host copy of the frames it needs (wall clock,
           `--host-repeats` runs, the fastest);
  device   gcd_amd.metrics_device.calculate_metrics: device events around its four launches (`kernels_ms`, split into the
           frame and the diversity pair), and wall clock around the whole call with its copies back, uncertainty map
           included (`wall_ms`); median of `--repeats` after a warm-up;
  copy     a device-to-device copy (16-byte accesses) of as many bytes as the kernels' inputs hold, the yardstick for
           the kernels: it reads AND writes that many bytes, a kernel that reads its inputs once moves half as much.

The two paths are also compared value by value (max difference over the dictionary), so a timing never stands for a
wrong result.
"""
from __future__ import annotations

import argparse
import json
import platform
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _cpu_name() -> str:
    try:
        for line in Path("/proc/cpuinfo").read_text().splitlines():
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or "unknown"


def _events(fn, repeats: int, warmup: int = 3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="576x1024")
    ap.add_argument("--frames", type=int, default=14)
    ap.add_argument("--samples", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from gcd_amd import metrics as host, metrics_device as dev_m
    assert torch.cuda.is_available(), "metrics_bench needs the GPU: there is nothing to time without it"
    dev = torch.device("cuda:0")
    H, W = (int(v) for v in args.size.split("x"))
    S, T = args.samples, args.frames
    g = torch.Generator().manual_seed(0)
    base = torch.rand(T, 3, H, W, generator=g)
    gt = ((base + base.roll(1, -1) + base.roll(1, -2) + base.roll(2, -1)) / 4.0).float()
    pred = (gt[None] + 0.05 * torch.randn(S, T, 3, H, W, generator=g)).clamp(0, 1).float()
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    occ = torch.stack([((x + 2 * y + 37 * t) // 160) % 3 == 0 for t in range(T)])          # a third occluded, in bands
    rep = ((0.1 + 0.9 * torch.rand(T, 3, H, W, generator=g)) * (~occ)[:, None]).float()
    pred_d, gt_d, rep_d = pred.to(dev), gt.to(dev), rep.to(dev)
    result = {"gpu": torch.cuda.get_device_name(0), "cpu": _cpu_name(), "S": S, "T": T, "H": H, "W": W,
              "repeats": args.repeats, "host_repeats": args.host_repeats, "cases": {}}
    for tag, r_d in (("reproject", rep_d), ("no_reproject", None)):
        # host: the frames leave the GPU first
        host_s, md_h = [], None
        for _ in range(args.host_repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p_h, g_h = pred_d.cpu().numpy(), gt_d.cpu().numpy()
            r_h = None if r_d is None else r_d.cpu().numpy()
            t1 = time.perf_counter()
            md_h, unc_h = host.calculate_metrics(g_h, r_h, [{"sampled_rgb": p} for p in p_h])
            host_s.append((time.perf_counter() - t0, t1 - t0))
        host_total, host_copy = min(host_s)
        # device
        frames_ms = _events(lambda: dev_m.frame_metrics(pred_d, gt_d, r_d), args.repeats)
        div_ms = _events(lambda: dev_m.diversity(pred_d, r_d), args.repeats)
        both_ms = _events(lambda: (dev_m.frame_metrics(pred_d, gt_d, r_d), dev_m.diversity(pred_d, r_d)), args.repeats)
        walls = []
        for i in range(args.repeats + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            md_d, unc_d = dev_m.calculate_metrics(gt_d, r_d, pred_d)
            if i >= 2:
                walls.append((time.perf_counter() - t0) * 1e3)
        walls_nomap = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dev_m.calculate_metrics(gt_d, r_d, pred_d, return_uncertainty=False)
            walls_nomap.append((time.perf_counter() - t0) * 1e3)
        # yardstick: a copy of the inputs' byte count
        nbytes = 4 * (pred_d.numel() + gt_d.numel() + (0 if r_d is None else r_d.numel()))
        src = torch.empty(nbytes // 4, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        copy_ms = _events(lambda: dst.copy_(src), args.repeats)
        del src, dst
        diff = 0.0
        for k in md_h:
            a, b = np.asarray(md_h[k], np.float64), np.asarray(md_d[k], np.float64)
            assert np.array_equal(np.isnan(a), np.isnan(b)), k
            fin = np.isfinite(a)
            diff = max(diff, float(np.abs(a[fin] - b[fin]).max()) if fin.any() else 0.0)
        diff = max(diff, float(np.abs(unc_h.astype(np.float64) - unc_d.astype(np.float64)).max()))
        result["cases"][tag] = {
            "host_s": host_total, "host_copy_s": host_copy,
            "device_wall_ms": statistics.median(walls), "device_wall_ms_min_max": [min(walls), max(walls)],
            "device_wall_no_map_ms": statistics.median(walls_nomap),
            "device_kernels_ms": both_ms[0], "device_kernels_ms_min_max": list(both_ms[1:]),
            "frames_kernels_ms": frames_ms[0], "diversity_kernels_ms": div_ms[0],
            "copy_ms": copy_ms[0], "copy_ms_min_max": list(copy_ms[1:]), "input_bytes": nbytes,
            "copy_GBps_read_plus_write": 2 * nbytes / copy_ms[0] / 1e6,
            "frames_over_copy": frames_ms[0] / copy_ms[0],
            "host_over_device_wall": host_total * 1e3 / statistics.median(walls),
            "max_abs_diff_host_vs_device": diff,
        }
        c = result["cases"][tag]
        print(f"[{tag}] host {host_total:.2f} s (copy {host_copy:.3f} s) | device wall {c['device_wall_ms']:.2f} ms "
              f"(no map {c['device_wall_no_map_ms']:.2f} ms), kernels {both_ms[0]:.3f} ms = frames {frames_ms[0]:.3f} + "
              f"diversity {div_ms[0]:.3f} | copy of {nbytes / 1e6:.0f} MB {copy_ms[0]:.3f} ms | frames / copy "
              f"{c['frames_over_copy']:.2f} | host / device {c['host_over_device_wall']:.0f}x | max diff {diff:.2e}",
              flush=True)
    print(json.dumps(result))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
