"""tools/temporal_attn_bench.py — the temporal-attention kernels alone, per clip length, in one process.

Forward at the four UNet levels of a 72 x 128 clip under CFG (2 clips: C = 320 / 640 / 1280 / 1280 on
HW = 9216 / 2304 / 576 / 144 pixels); T = 14 runs gcd_attn_temporal_f16 (the old kernel), T = 25 / 32 / 48 / 64
gcd_attn_temporal_long_f16.  Bytes counted: q|k|v read + out written (8 C bytes per row).
Backward at cfg4's shape (2 clips, 32 x 48 latents: HW = 1536 / 384 / 96 / 24), T = 14 (gcd_attn_temporal_bwd) and
25 (gcd_attn_temporal_long_bwd).  Bytes counted: fp16 q|k|v + fp32 dO read, fp32 dq|dk|dv written (22 C per row).

    python tools/temporal_attn_bench.py [--iters 20] [--warmup 3] [--json out.json]

Device events around `iters` back-to-back launches after `warmup` launches; the median of 5 such groups."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

LEVELS = [(320, 9216), (640, 2304), (1280, 576), (1280, 144)]
LEVELS_TRAIN = [(320, 1536), (640, 384), (1280, 96), (1280, 24)]


def _time(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        runs.append(a.elapsed_time(b) * 1e3 / iters)
    return sorted(runs)[2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", type=str, default="")
    a = ap.parse_args()
    from gcd_amd import _lib, ops
    lib = _lib.load()
    dev = torch.device("cuda:0")
    clips = 2
    rows = []
    for T in (14, 25, 32, 48, 64):
        for lvl, (C, HW) in enumerate(LEVELS):
            heads = C // 64
            M = clips * T * HW
            qkv = torch.randn(M, 3 * C, device=dev).half()
            out = torch.empty(M, C, dtype=torch.float16, device=dev)
            us = _time(lambda: ops.attn_temporal(qkv, out, clips, T, HW, heads), a.iters, a.warmup)
            nbytes = 8 * M * C
            rows.append(dict(kind="fwd", T=T, level=lvl, C=C, HW=HW, clips=clips,
                             entry="gcd_attn_temporal_f16" if T <= 16 else "gcd_attn_temporal_long_f16",
                             us=round(us, 1), MB=round(nbytes / 1e6, 1), TBps=round(nbytes / us / 1e6, 2)))
            print(json.dumps(rows[-1]), flush=True)
            del qkv, out
    for T in (14, 25):
        for lvl, (C, HW) in enumerate(LEVELS_TRAIN):
            heads = C // 64
            M = clips * T * HW
            qkv = torch.randn(M, 3 * C, device=dev).half()
            dO = torch.randn(M, C, device=dev)
            dq = torch.empty(M, 3 * C, device=dev)
            name = "gcd_attn_temporal_bwd" if T <= 16 else "gcd_attn_temporal_long_bwd"
            fn = getattr(lib, name)

            def bwd():
                _lib.check(fn(qkv.data_ptr(), 3 * C, dO.data_ptr(), C, dq.data_ptr(), 3 * C, clips, T, HW, heads,
                              ops._stream()), name)
            us = _time(bwd, a.iters, a.warmup)
            nbytes = 22 * M * C
            rows.append(dict(kind="bwd", T=T, level=lvl, C=C, HW=HW, clips=clips, entry=name, us=round(us, 1),
                             MB=round(nbytes / 1e6, 1), TBps=round(nbytes / us / 1e6, 2)))
            print(json.dumps(rows[-1]), flush=True)
            del qkv, dO, dq
    l0 = {r["T"]: r for r in rows if r["kind"] == "fwd" and r["level"] == 0}
    summary = dict(l0_T25_over_T14_rate=round(l0[25]["TBps"] / l0[14]["TBps"], 3),
                   fwd_us_per_level_sum={T: round(sum(r["us"] for r in rows if r["kind"] == "fwd" and r["T"] == T), 1)
                                         for T in (14, 25, 32, 48, 64)},
                   device=torch.cuda.get_device_name(0))
    print(json.dumps(summary))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(dict(rows=rows, summary=summary), indent=1))


if __name__ == "__main__":
    main()
