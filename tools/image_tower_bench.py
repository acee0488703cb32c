"""Time the CLIP ViT-H/14 image tower behind cond["crossattn"] on the device (a record, not a gate).

    python tools/image_tower_bench.py [--layers 32] [--images 14,28] [--sizes 256x384,576x1024] [--repeats 5] [--out FILE]

Seeded random weights (`clip_vision.seeded_state_dict`; no checkpoint ships with the project), the full ViT-H/14 unless
`--layers` says otherwise.  Two routes in one process, alternated, device events around the whole call, median of
`--repeats`:

  hip     gcd_amd.clip_vision.FrozenOpenCLIPImageEmbedder: gcd_clip_* kernels + gcd_gemm_f16 / gcd_layernorm_f16;
  torch   the module's own torch restatement (preprocess_reference + VisionTransformer.forward_torch) on the same GPU under
          fp16 autocast: what PyTorch-ROCm runs for the reference embedder (its forward is decorated with autocast) once
          open_clip and kornia are installed.  (Neither is here; this stands in for what they launch.)

Per configuration: ms per call and per image for both routes, the preprocessing alone, the GEMM share and TFLOP/s of the hip
route (per-launch device events, gcd_amd.ops.start_profile, in a run of its own), peak device memory, the rel-L2 between the
routes and of each against a float32 run of the restatement, and the share of the fine-tune step (0.136 s,
profiles/r06_bench_train.json) and of a 25-step clip (25 x 96.55 ms, profiles/r06_bench.json) the tower takes.
"""
from __future__ import annotations

import argparse
import ctypes as C
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

TRAIN_STEP_S = 0.136            # profiles/r06_bench_train.json (fp16)
CLIP_25_STEPS_S = 25 * 0.09655  # profiles/r06_bench.json: 96.55 ms per 28-frame CFG step


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def rel_l2(a, b) -> float:
    return float((a.double() - b.double()).norm() / b.double().norm())


def tower_flops(cfg: dict, n: int) -> float:
    """Multiply-adds x 2 of the GEMMs of one call (conv1 at its padded K, the blocks, the projection)."""
    W, S = cfg["width"], (cfg["image_size"] // cfg["patch_size"]) ** 2 + 1
    kp = (3 * cfg["patch_size"] ** 2 + 31) // 32 * 32
    per_block = 2.0 * n * S * (4 * W * W + 2 * W * cfg["mlp_width"])
    return 2.0 * n * (S - 1) * kp * W + cfg["layers"] * per_block + 2.0 * n * W * cfg["embed_dim"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--images", default="14,28")
    ap.add_argument("--sizes", default="256x384,576x1024")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from gcd_amd import _lib, clip_vision as cv, ops
    assert torch.cuda.is_available(), "image_tower_bench needs the GPU: there is nothing to time without it"
    dev = torch.device("cuda:0")
    cfg = dict(cv.ARCHS["ViT-H-14"], layers=args.layers)
    emb = cv.FrozenOpenCLIPImageEmbedder(vision_cfg=cfg)
    emb.model.visual.load_state_dict(cv.seeded_state_dict(cfg, 11))
    emb = emb.to(dev)
    vis, lib = emb.model.visual, _lib.load()

    def torch_route(x, autocast=True):
        with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
            return vis.forward_torch(cv.preprocess_reference(x, vis.image_size, emb.antialias, emb.mean, emb.std)).float()

    lines = [f"image_tower_bench: {torch.cuda.get_device_name(0)}; ViT-H/14 image tower, {args.layers} layers, "
             f"{sum(p.numel() for p in vis.parameters()) / 1e6:.0f} M parameters (seeded random); median of {args.repeats}, routes alternated"]
    with torch.no_grad():
        for size in args.sizes.split(","):
            H, Wd = (int(v) for v in size.split("x"))
            for n in (int(v) for v in args.images.split(",")):
                g = torch.Generator().manual_seed(1000 + n + H)
                x = (torch.rand(n, 3, H, Wd, generator=g) * 2 - 1).to(dev)
                routes = {"hip": lambda: emb(x), "torch": lambda: torch_route(x),
                          "hip_pre": lambda: cv.preprocess(x, vis.image_size, vis.patch_size, emb.antialias, emb.mean, emb.std, vis.kp)[0],
                          "torch_pre": lambda: cv.preprocess_reference(x, vis.image_size, emb.antialias, emb.mean, emb.std)}
                times, peak, outs = {k: [] for k in routes}, {}, {}
                for name, fn in routes.items():            # warm-up (packs, code objects, algorithm choice), peak memory
                    fn()
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    _, outs[name] = timed(fn)
                    peak[name] = torch.cuda.max_memory_allocated() - base
                for _ in range(args.repeats):              # alternated
                    for name, fn in routes.items():
                        times[name].append(timed(fn)[0])
                med = {k: statistics.median(v) for k, v in times.items()}
                # per-launch events of the hip route's GEMMs, in a run of its own
                prof = ops.start_profile()
                emb(x)
                torch.cuda.synchronize()
                ops.stop_profile()
                gemm_ms, ms = 0.0, C.c_float()
                for rec in prof:
                    if rec["kind"] == "gemm":
                        _lib.check(lib.gcd_event_elapsed_ms(rec["start"], rec["stop"], C.byref(ms)))
                        gemm_ms += ms.value
                    lib.gcd_event_destroy(rec["start"])
                    lib.gcd_event_destroy(rec["stop"])
                ref32 = torch_route(x, autocast=False)
                flops = tower_flops(cfg, n)
                lines += [
                    f"{n} images {H}x{Wd}:",
                    f"  hip   : {med['hip']:8.2f} ms per call = {med['hip'] / n:6.2f} ms per image (min {min(times['hip']):.2f}, max {max(times['hip']):.2f}); "
                    f"preprocess {med['hip_pre']:.3f} ms; GEMMs {gemm_ms:.2f} ms = {gemm_ms / med['hip']:.2f} of the call, "
                    f"{flops / gemm_ms / 1e9:.0f} TFLOP/s over GEMM time, {flops / med['hip'] / 1e9:.0f} TFLOP/s over the call; "
                    f"peak memory {peak['hip'] / 2 ** 20:.0f} MiB",
                    f"  torch : {med['torch']:8.2f} ms per call = {med['torch'] / n:6.2f} ms per image (min {min(times['torch']):.2f}, max {max(times['torch']):.2f}); "
                    f"preprocess {med['torch_pre']:.3f} ms; {flops / med['torch'] / 1e9:.0f} TFLOP/s over the call; peak memory {peak['torch'] / 2 ** 20:.0f} MiB",
                    f"  torch / hip: {med['torch'] / med['hip']:.2f}x; rel-L2 hip vs torch-fp16 {rel_l2(outs['hip'], outs['torch']):.3e}, "
                    f"hip vs float32 {rel_l2(outs['hip'], ref32):.3e}, torch-fp16 vs float32 {rel_l2(outs['torch'], ref32):.3e}",
                    f"  share of the fine-tune step ({TRAIN_STEP_S * 1e3:.0f} ms): hip {med['hip'] / 1e3 / TRAIN_STEP_S:.3f}, torch {med['torch'] / 1e3 / TRAIN_STEP_S:.3f}; "
                    f"of a 25-step clip ({CLIP_25_STEPS_S:.2f} s): hip {med['hip'] / 1e3 / CLIP_25_STEPS_S:.4f}, torch {med['torch'] / 1e3 / CLIP_25_STEPS_S:.4f}",
                ]
                del x, outs, ref32
                torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
