"""`python -m gcd_amd.infer`: scripts/infer.py of the reference for one process and one GPU — a GCD config, a checkpoint,
an image or a folder of frames in; sampled clips as frame folders and .mp4 out.

    python -m gcd_amd.infer --config configs/infer_kubric.yaml --checkpoint kubric_gradual_max90.ckpt \\
        --input frames_dir --output out --delta_azimuth 30 --delta_elevation 15

The arguments are infer.py's (:45-107) where they apply; `--train_config` names a training YAML whose `data:` section
gives the camera ranges the model was trained with (default: the Kubric training configs' values)."""
from __future__ import annotations

import argparse
import time


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m gcd_amd.infer", description=__doc__.split("\n\n")[0])
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--input", type=str, nargs="+", required=True, help="image files and / or folders of frames")
    p.add_argument("--output", type=str, required=True)
    p.add_argument("--config", "--config_path", dest="config", type=str, required=True)
    p.add_argument("--checkpoint", "--model_path", dest="checkpoint", type=str, required=True)
    p.add_argument("--train_config", type=str, default=None)
    p.add_argument("--use_ema", type=int, default=0)
    p.add_argument("--seed", type=int, default=None)
    p.add_argument("--num_samples", "--samples", dest="num_samples", type=int, default=2)
    p.add_argument("--num_frames", "--frames", dest="num_frames", type=int, default=14)
    p.add_argument("--num_steps", "--steps", dest="num_steps", type=int, default=25)
    p.add_argument("--guider_max_scale", type=float, default=1.5)
    p.add_argument("--guider_min_scale", type=float, default=1.0)
    p.add_argument("--motion_id", type=int, default=127)
    p.add_argument("--force_custom_mbid", type=int, default=0)
    p.add_argument("--cond_aug", type=float, default=0.02)
    p.add_argument("--decoding_t", type=int, default=14)
    p.add_argument("--delta_azimuth", type=float, default=30.0)
    p.add_argument("--delta_elevation", type=float, default=15.0)
    p.add_argument("--delta_radius", type=float, default=0.0)
    p.add_argument("--frame_start", type=int, default=0)
    p.add_argument("--frame_stride", type=int, default=2)
    p.add_argument("--frame_rate", type=int, default=12)
    p.add_argument("--frame_width", type=int, default=384)
    p.add_argument("--frame_height", type=int, default=256)
    p.add_argument("--center_crop", type=int, default=1)
    p.add_argument("--save_images", type=int, default=1)
    p.add_argument("--save_mp4", type=int, default=1)
    p.add_argument("--save_input", type=int, default=1)
    return p.parse_args(argv)


def main(argv=None) -> int:
    args = parse_args(argv)
    import torch
    from . import inference as I
    if args.seed is not None:
        torch.manual_seed(args.seed)
    t0 = time.time()
    model = I.load_model_bundle(args.device, args.config, args.checkpoint, bool(args.use_ema), num_steps=args.num_steps,
                                num_frames=args.num_frames, max_scale=args.guider_max_scale,
                                min_scale=args.guider_min_scale)
    controls = I.camera_controls_from_yaml(args.train_config) if args.train_config else None
    print(f"Loading the model took {time.time() - t0:.2f}s")
    with model.ema_scope("Testing"):
        for i, example in enumerate(args.input):
            t0 = time.time()
            out = I.run_inference(
                model, example, args.output, num_samples=args.num_samples, num_frames=args.num_frames,
                num_steps=args.num_steps, guider_max_scale=args.guider_max_scale, guider_min_scale=args.guider_min_scale,
                motion_id=args.motion_id, force_custom_mbid=bool(args.force_custom_mbid), cond_aug=args.cond_aug,
                decoding_t=args.decoding_t, delta_azimuth=args.delta_azimuth, delta_elevation=args.delta_elevation,
                delta_radius=args.delta_radius, frame_start=args.frame_start, frame_stride=args.frame_stride,
                frame_rate=args.frame_rate, frame_width=args.frame_width, frame_height=args.frame_height,
                center_crop=bool(args.center_crop), save_images=bool(args.save_images), save_mp4=bool(args.save_mp4),
                save_input=bool(args.save_input), controls=controls)
            torch.cuda.synchronize()
            print(f"{i}: {example}: {len(out['samples'])} clip(s) of {out['samples'][0].shape if out['samples'] else ()} "
                  f"(path {model.sampler.last_path}) in {time.time() - t0:.2f}s")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
