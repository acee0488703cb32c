"""The host pieces of the reference's inference script that a user needs to run a clip end to end with this package alone:
`scripts/eval_utils.py` (load_model_bundle :35-92, prepare_model_inference_params :157-188, construct_batch :191-263),
`sgm/data/common.py` (center_crop_numpy :87-118, process_image :133-163) and `scripts/infer.py` (load_input :110-151,
run_inference :154-182).  Input IO and batch assembly on the host, as in the reference; the model is
`gcd_amd.diffusion.DiffusionEngine`, the writer `gcd_amd.eval_io.write_video_and_frames`.

The reference reads the camera ranges a model was trained with from the `data:` section of its training config
(eval_utils.py:95-143).  `load_config` does not read that section: they are a `CameraControls`, whose defaults are the
Kubric training configs' values; `camera_controls_from_yaml` reads them from a training YAML when one is at hand.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from ._lib import GcdError
from .camera import construct_trajectory

IMAGE_EXTENSIONS = [".jpg", ".jpeg", ".png", ".bmp", ".tiff"]
VIDEO_EXTENSIONS = [".mp4", ".avi", ".mov", ".flv", ".mkv", ".webm"]


@dataclass
class CameraControls:
    """What eval_utils.expand_model_bundle appends to the model bundle (:95-143)."""
    delta_azimuth_range: Sequence[float] = (-90.0, 90.0)
    delta_elevation_range: Sequence[float] = (-30.0, 30.0)
    delta_radius_range: Sequence[float] = (-3.0, 3.0)
    trajectory: str = "interpol_linear"
    move_time: int = 13
    camera_control: str = "spherical"
    motion_bucket_range: Sequence[int] = field(default_factory=lambda: [0, 255])


def camera_controls_from_yaml(path) -> CameraControls:
    """The `data.params` of a training config (eval_utils.py:105-138); the reference's fall-backs for a missing key."""
    import yaml
    with open(path) as f:
        doc = yaml.safe_load(f) or {}
    p = ((doc.get("data") or {}).get("params")) or {}
    mbr = p.get("motion_bucket_range", [127, 127])
    if isinstance(mbr, str):
        mbr = [int(v) for v in mbr.split(",")]
    # deliberate, as in the reference (eval_utils.py:106-117): the presence of `azimuth_range` (the absolute range) is what
    # is tested, `delta_azimuth_range` is what is read; likewise for elevation and radius
    return CameraControls(
        delta_azimuth_range=p["delta_azimuth_range"] if "azimuth_range" in p else (0.0, 0.0),
        delta_elevation_range=p["delta_elevation_range"] if "elevation_range" in p else (0.0, 0.0),
        delta_radius_range=p["delta_radius_range"] if "radius_range" in p else (0.0, 0.0),
        trajectory=p.get("trajectory", "interpol_linear"), move_time=int(p.get("move_time", 0)),
        camera_control=p.get("camera_control", "none"), motion_bucket_range=list(mbr))


# ----------------------------------------------------------------------------------------------------------------- model
def load_model_bundle(device: str, config_path, model_path: Optional[str], use_ema: bool = False, num_steps: int = 25,
                      num_frames: int = 14, max_scale: float = 1.5, min_scale: float = 1.0, **overrides):
    """eval_utils.load_model_bundle (:35-61): read the inference config, point it at the checkpoint and the device, build
    the engine on that device in eval mode.  Returns the engine.  `overrides` are written over the engine's keywords."""
    from . import config as C
    cfg = C.load_config(config_path)
    params = cfg.setdefault("params", {})
    for emb in (params.get("conditioner_config") or {}).get("params", {}).get("emb_models", []):
        clip = (emb.get("params") or {}).get("open_clip_embedding_config")
        if clip is not None and "cuda" in str(device):
            clip.setdefault("params", {})["init_device"] = device
    params["ckpt_path"] = model_path
    # NOTE (reference): this decides which keys to load and when
    params["use_ema"] = bool(use_ema)
    params["ckpt_has_ema"] = bool(use_ema)
    sp = params["sampler_config"]["params"]
    sp["num_steps"] = num_steps
    gp = sp["guider_config"]["params"]
    gp["num_frames"], gp["max_scale"], gp["min_scale"] = num_frames, max_scale, min_scale
    sp["device"] = device
    with torch.device(device):
        model = C.instantiate_model(cfg, **overrides).to(device).eval()
    return model


def prepare_model_inference_params(model, device, num_steps, num_frames, max_scale, min_scale, autocast, decoding_t):
    """eval_utils.py:157-188.  As in the reference the guider's per-frame scale was fixed at construction: writing
    `max_scale` / `min_scale` afterwards changes the attributes only (`load_model_bundle` takes them for real).
    `autocast` has no effect on the HIP path; the returned dict is what the reference hands to torch.autocast."""
    model.sampler.num_steps = num_steps
    model.sampler.guider.num_frames = num_frames
    model.sampler.guider.max_scale = max_scale
    model.sampler.guider.min_scale = min_scale
    model.en_and_decode_n_samples_a_time = decoding_t
    for embedder in model.conditioner.embedders:
        if hasattr(embedder, "disable_encoder_autocast"):
            embedder.disable_encoder_autocast = not bool(autocast)
        if hasattr(embedder, "en_and_decode_n_samples_a_time"):
            embedder.en_and_decode_n_samples_a_time = decoding_t
    return {"enabled": bool(autocast), "device_type": str(device).split(":")[0]}


# ----------------------------------------------------------------------------------------------------------------- batch
def motion_value(azimuth_deg: float, elevation_deg: float, controls: CameraControls) -> int:
    """eval_utils.py:253-260: the motion bucket of a model trained with the bucket tied to the camera motion,
    int(round(lo + (hi - lo) * |delta| / |delta max|)) over (azimuth, elevation)."""
    lo, hi = controls.motion_bucket_range
    my_motion = np.linalg.norm(np.array([azimuth_deg, elevation_deg], dtype=np.float32), ord=2)
    max_motion = np.linalg.norm([max(*controls.delta_azimuth_range), max(*controls.delta_elevation_range)], ord=2)
    return int(round(lo + (hi - lo) * (my_motion / max_motion)))


def construct_batch(input_rgb, azimuth_deg, elevation_deg, radius_m, input_frames, frame_rate, motion_bucket, cond_aug,
                    force_custom_mbid, controls: Optional[CameraControls], device) -> Dict:
    """eval_utils.construct_batch (:191-263).  input_rgb: (Tc, 3, Hp, Wp) float32 in [0, 1].  When fewer than Tc input
    frames are given, the last given frame is repeated; `cond_frames` gets its augmentation noise from torch's generator
    of `device`."""
    controls = controls if controls is not None else CameraControls()
    Tc, _, Hp, Wp = input_rgb.shape
    input_rgb_torch = torch.as_tensor(np.asarray(input_rgb), dtype=torch.float32).to(device) * 2.0 - 1.0
    if input_frames < Tc:
        input_rgb_torch[input_frames:] = input_rgb_torch[input_frames - 1:input_frames]

    batch = dict()
    batch["motion_bucket_id"] = torch.ones(Tc, dtype=torch.int32, device=device) * int(motion_bucket)
    batch["fps_id"] = torch.ones(Tc, dtype=torch.int32, device=device) * int(frame_rate)
    batch["cond_aug"] = torch.ones(Tc, dtype=torch.float32, device=device) * cond_aug
    batch["cond_frames_without_noise"] = input_rgb_torch
    batch["cond_frames"] = input_rgb_torch + torch.randn_like(input_rgb_torch) * cond_aug
    batch["jpg"] = torch.zeros_like(input_rgb_torch)
    batch["image_only_indicator"] = torch.zeros(1, Tc, dtype=torch.float32, device=device)
    batch["num_video_frames"] = Tc

    if controls.camera_control == "spherical":
        assert np.isfinite(azimuth_deg) and np.isfinite(elevation_deg) and np.isfinite(radius_m)
        if controls.move_time > Tc:
            raise GcdError(f"construct_batch: the camera moves over {controls.move_time} frames, the clip has {Tc}; pass "
                           "CameraControls(move_time=...) of at most the clip length")
        start = np.array([0.0, 0.0, 0.0], dtype=np.float32)
        end = np.array([azimuth_deg, elevation_deg, radius_m], dtype=np.float32)
        src, dst = construct_trajectory(start, end, controls.trajectory, Tc, controls.move_time)
        rel = dst - src
        rel[:, 0] *= np.pi / 180.0
        rel[:, 1] *= np.pi / 180.0
        batch["scaled_relative_angles"] = torch.tensor(rel, dtype=torch.float32, device=device)
    elif controls.camera_control == "relative_pose":
        batch["scaled_relative_pose"] = torch.zeros((Tc, 3, 4), dtype=torch.float32, device=device)

    # the motion value of a model trained with synchronised values overrides the given one
    motion_range = controls.motion_bucket_range[1] - controls.motion_bucket_range[0]
    if controls.camera_control != "none" and not force_custom_mbid and motion_range > 0:
        batch["motion_bucket_id"] = torch.ones(Tc, dtype=torch.int32, device=device) * \
            motion_value(azimuth_deg, elevation_deg, controls)
    return batch


# -------------------------------------------------------------------------------------------------------------- input IO
def center_crop_box(H: int, W: int, aspect_ratio: float):
    """common.py:92-114: (y1, y2, x1, x2) of the centre crop to `aspect_ratio` = width / height, or None when the image
    already has it (within 2e-3)."""
    video_ar = W / H
    if video_ar > aspect_ratio + 2e-3:
        crop_width, crop_height = int(H * aspect_ratio), H
    elif video_ar < aspect_ratio - 2e-3:
        crop_width, crop_height = W, int(W / aspect_ratio)
    else:
        return None
    y1 = (H - crop_height) // 2
    x1 = (W - crop_width) // 2
    return y1, y1 + crop_height, x1, x1 + crop_width


def center_crop_numpy(image, aspect_ratio: float, warn_spatial: bool = False):
    """common.py:87-118 on a (..., H, W, C) array."""
    H, W = image.shape[-3:-1]
    box = center_crop_box(H, W, aspect_ratio)
    if box is None:
        return image
    y1, y2, x1, x2 = box
    if warn_spatial:
        print(f"Warning: Cropping video from {W} x {H} to {x2 - x1} x {y2 - y1}.")
    return image[..., y1:y2, x1:x2, :]


def resize_bilinear(rgb: np.ndarray, frame_width: int, frame_height: int) -> np.ndarray:
    """(H, W, C) float32 -> (frame_height, frame_width, C): bilinear with half-pixel centres and no antialias — what
    cv2.resize(..., interpolation=cv2.INTER_LINEAR) computes on float32 images — as host torch."""
    x = torch.from_numpy(np.ascontiguousarray(rgb)).permute(2, 0, 1)[None]
    y = torch.nn.functional.interpolate(x, size=(frame_height, frame_width), mode="bilinear", align_corners=False,
                                        antialias=False)
    return y[0].permute(1, 2, 0).contiguous().numpy()


def process_image(rgb, center_crop, frame_width: int, frame_height: int, warn_spatial: bool = False) -> np.ndarray:
    """common.py:133-163: (H, W, 3+) uint8 or float in [0, 1] -> (3, frame_height, frame_width) float32 in [-1, 1]."""
    rgb = np.asarray(rgb)[..., 0:3]
    if rgb.dtype.kind in ["i", "u"]:
        rgb = (rgb / 255.0).astype(np.float32)
    else:
        rgb = rgb.astype(np.float32)
    if center_crop:
        rgb = center_crop_numpy(rgb, frame_width / frame_height, warn_spatial)
    if frame_width > 0 and frame_height > 0 and (rgb.shape[1] != frame_width or rgb.shape[0] != frame_height):
        if warn_spatial:
            print(f"Warning: Resizing image/frame from {rgb.shape[1]} x {rgb.shape[0]} to "
                  f"{frame_width} x {frame_height}.")
        rgb = resize_bilinear(rgb, frame_width, frame_height)
    rgb = rgb * 2.0 - 1.0
    return np.ascontiguousarray(np.transpose(rgb, (2, 0, 1)))


def is_image_file(path) -> bool:
    return os.path.splitext(str(path))[1].lower() in IMAGE_EXTENSIONS


def is_video_file(path) -> bool:
    return os.path.splitext(str(path))[1].lower() in VIDEO_EXTENSIONS


def load_rgb_image(path, center_crop, frame_width, frame_height, warn_spatial=False) -> np.ndarray:
    """common.load_rgb_image (:121-130) through PIL: (3, H, W) float32 in [-1, 1]."""
    from PIL import Image
    with Image.open(path) as im:
        rgb = np.asarray(im.convert("RGB"))
    return process_image(rgb, center_crop, frame_width, frame_height, warn_spatial)


def image_files_in(path) -> List[str]:
    """The sorted names of the image files (not folders) directly in `path`: the frames of a folder input."""
    path = str(path)
    return sorted(f for f in os.listdir(path) if is_image_file(f) and os.path.isfile(os.path.join(path, f)))


def load_image_folder(path, clip_frames, center_crop, frame_width, frame_height, warn_spatial=False) -> np.ndarray:
    """The frames `clip_frames` (indices into the sorted image files of the folder) -> (Tc, 3, H, W) in [-1, 1].  An index
    past the last file takes the last file, so that a short folder still fills a clip."""
    files = image_files_in(path)
    if not files:
        raise GcdError(f"{path}: no image files ({', '.join(IMAGE_EXTENSIONS)})")
    picked = [files[min(int(i), len(files) - 1)] for i in clip_frames]
    return np.stack([load_rgb_image(os.path.join(path, f), center_crop, frame_width, frame_height, warn_spatial)
                     for f in picked], axis=0)


def load_image_or_video(path, clip_frames, center_crop, frame_width, frame_height, warn_spatial=False) -> np.ndarray:
    """eval_utils.load_image_or_video (:435-447): an image file is repeated as a still over the clip, a folder of
    images gives its frames.  Video files need a decoder this package does not have."""
    path = str(path)
    if os.path.isdir(path):
        return load_image_folder(path, clip_frames, center_crop, frame_width, frame_height, warn_spatial)
    if is_image_file(path):
        rgb = load_rgb_image(path, center_crop, frame_width, frame_height, warn_spatial)
        return rgb[None].repeat(len(clip_frames), axis=0)
    if is_video_file(path):
        raise GcdError(f"{path}: video files are not read here (no decoder ships with gcd_amd); extract the frames into a "
                       "folder of images (e.g. ffmpeg -i clip.mp4 frames/%04d.png) and pass the folder")
    raise GcdError(f"{path}: neither an image file nor a folder of images")


def frames_in(path, clip_frames) -> int:
    """How many distinct input frames `load_image_or_video` has for this clip (construct_batch's `input_frames`)."""
    path = str(path)
    if os.path.isdir(path):
        n = len(image_files_in(path))
        return max(1, sum(1 for i in clip_frames if int(i) < n))
    return len(clip_frames)


# ------------------------------------------------------------------------------------------------------------- inference
@torch.no_grad()
def sample_clips(model, batch: Dict, num_samples: int = 1, num_steps: int = 25, num_frames: int = 14,
                 max_scale: float = 1.5, min_scale: float = 1.0, decoding_t: int = 14,
                 device: Optional[str] = None) -> List[Dict[str, np.ndarray]]:
    """infer.run_inference (:154-182): `num_samples` calls of `sample_video` on one batch.  Each entry holds
    cond_rgb / sampled_rgb, (Tc, 3, Hp, Wp) float32 in [0, 1], and sampled_latent, (Tc, 4, Hp / 8, Wp / 8)."""
    prepare_model_inference_params(model, device if device is not None else str(model.device), num_steps, num_frames,
                                   max_scale, min_scale, False, decoding_t)
    pred_samples = []
    for _ in range(num_samples):
        video_dict = model.sample_video(batch, enter_ema=False, limit_batch=False)
        pred_samples.append({"cond_rgb": video_dict["cond_video"].detach().cpu().numpy(),
                             "sampled_rgb": video_dict["sampled_video"].detach().cpu().numpy(),
                             "sampled_latent": video_dict["sampled_z"].detach().cpu().numpy()})
    return pred_samples


def run_inference(model, input_path, output_dir, *, num_samples: int = 1, num_frames: int = 14, num_steps: int = 25,
                  guider_max_scale: float = 1.5, guider_min_scale: float = 1.0, motion_id: int = 127,
                  force_custom_mbid: bool = False, cond_aug: float = 0.02, decoding_t: Optional[int] = None,
                  delta_azimuth: float = 30.0, delta_elevation: float = 15.0, delta_radius: float = 0.0,
                  frame_start: int = 0, frame_stride: int = 2, frame_rate: int = 12, frame_width: int = 384,
                  frame_height: int = 256, center_crop: bool = True, save_images: bool = True, save_mp4: bool = True,
                  save_input: bool = True, controls: Optional[CameraControls] = None, name: Optional[str] = None) -> Dict:
    """One example of scripts/infer.py (load_input :110-151, run_inference :154-182, the plain outputs of save_results
    :438-447): read `input_path` (an image file or a folder of frames), assemble the batch, sample `num_samples` clips
    and write `<output_dir>/<name>_pred_s<k>/0000.png ...` and `<output_dir>/<name>_pred_s<k>.mp4` (and `_input`).
    Returns {"input_rgb", "samples" (list of (Tc, 3, Hp, Wp) arrays in [0, 1]), "latents", "written" (the writer's
    records, outputs first), "batch"}.  The galleries with captions (cv2.putText) are not made."""
    from .eval_io import write_video_and_frames
    if frame_start < 0 or frame_stride < 0 or frame_rate < 0:
        raise GcdError(f"frame_start, frame_stride and frame_rate must not be negative: {frame_start} {frame_stride} "
                       f"{frame_rate}")
    if frame_height % 64 or frame_width % 64:
        raise GcdError(f"Input resolution must be a multiple of 64, but got {frame_height} x {frame_width}")
    device = str(model.device)
    Tc = int(num_frames)
    clip_frames = np.arange(Tc) * int(frame_stride) + int(frame_start)
    input_rgb = load_image_or_video(input_path, clip_frames, center_crop, frame_width, frame_height, True)
    input_rgb = (input_rgb + 1.0) / 2.0
    batch = construct_batch(input_rgb, delta_azimuth, delta_elevation, delta_radius, frames_in(input_path, clip_frames),
                            frame_rate, motion_id, cond_aug, force_custom_mbid, controls, device)
    preds = sample_clips(model, batch, num_samples, num_steps, Tc, guider_max_scale, guider_min_scale,
                         Tc if decoding_t is None else decoding_t, device)
    if name is None:
        name = os.path.splitext(os.path.basename(os.path.normpath(str(input_path))))[0]
    vis_fps = (6 + frame_rate) // 2
    written = []
    if save_images or save_mp4:
        for s, pred in enumerate(preds):
            written.append(write_video_and_frames(np.transpose(pred["sampled_rgb"], (0, 2, 3, 1)),
                                                  dst_dp=os.path.join(str(output_dir), f"{name}_pred_s{s}"), fps=vis_fps,
                                                  save_images=save_images, save_mp4=save_mp4, quality=9))
        if save_input:
            written.append(write_video_and_frames(np.transpose(input_rgb, (0, 2, 3, 1)),
                                                  dst_dp=os.path.join(str(output_dir), f"{name}_input"), fps=vis_fps,
                                                  save_images=save_images, save_mp4=save_mp4, quality=9))
    return {"input_rgb": input_rgb, "samples": [p["sampled_rgb"] for p in preds],
            "latents": [p["sampled_latent"] for p in preds], "written": written, "batch": batch}
