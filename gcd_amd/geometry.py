"""Point clouds to (source, target) frames on the device (libgcd_amd_render.so, include/gcd_amd_render.h).

GCD's data modules do not load videos: for every example they re-render the clip of the source and of the target camera
from cached point clouds.  This module is that stage: `project_points_to_pixels` and `blur_into_black` keep the
signatures, shapes and dtypes of the functions they restate, `render_views` is the fused route (one pass over the cloud for
all cameras of a frame, the filled and resized view stored straight into its slot of a (T, 3, Hp, Wp) batch) and
`synth_src_dst_rgb` restates the dataset method as a free function.  DESIGN.md §12.2 has the semantics, the accumulation
scheme and the bars.  `synth_rgb_pardom` is the ParallelDomain dataset's method: per-frame intrinsics, stored view 16 as the
re-projection, and in the `segm` modality the colours of `class_colours` (libgcd_amd_pardom.so,
include/gcd_amd_pardom.h) handed to the same splat.

Two differences in behaviour.  Where no point passes the mask the original raises (a `.max()` of nothing); a kernel
cannot, so that camera's image is zero, its weights are -1 and `splat` returns the number of visible points per camera
as a device tensor for the caller who wants to look.  And a float colour that is negative, NaN or infinite counts as 0
(the sums are unsigned integers); colours above 1 are summed as they are and only the final image is clamped.

Like gcd_amd.ops: the kernels launch on the current device's current stream and there is no CPU fallback — a cloud or an
image that is not a GPU tensor raises GcdError.  The small camera helpers at the end are host code (numpy).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib, _lib_pardom
from .ops import _need_gpu, _stream

_XYZ_CODES = {torch.float16: _lib.RENDER_F16, torch.float32: _lib.RENDER_F32, torch.float64: _lib.RENDER_F64}
_RGB_CODES = dict(_XYZ_CODES)
_RGB_CODES[torch.uint8] = _lib.RENDER_U8


def pack_cameras(K, RTs, device) -> torch.Tensor:
    """K (3, 3), or (nc, 3, 3) with a matrix per camera, and RTs (nc, 4, 4) or (4, 4), any float dtype, host or device
    -> the (nc, 25) float64 device table the splat reads: K then RT, row-major, each converted to float64 as it is."""
    K = torch.as_tensor(K).to(torch.float64).reshape(-1, 9)
    RTs = torch.as_tensor(RTs).to(torch.float64).reshape(-1, 16)
    if K.shape[0] not in (1, RTs.shape[0]):
        raise _lib.GcdError(f"pack_cameras: {K.shape[0]} intrinsics for {RTs.shape[0]} cameras")
    return torch.cat([K.to(device).expand(RTs.shape[0], 9), RTs.to(device)], dim=1).contiguous()


def _cloud(who: str, xyz, rgb):
    if not (torch.is_tensor(xyz) and torch.is_tensor(rgb)):
        raise _lib.GcdError(f"{who}: the cloud must be torch tensors on the GPU; there is no CPU fallback")
    _need_gpu(xyz, rgb)
    if xyz.dim() != 2 or rgb.dim() != 2 or xyz.shape[1] != 3 or rgb.shape[1] != 3 or xyz.shape[0] != rgb.shape[0]:
        raise _lib.GcdError(f"{who}: xyz and rgb must be (N, 3), got {tuple(xyz.shape)} and {tuple(rgb.shape)}")
    if xyz.dtype not in _XYZ_CODES or rgb.dtype not in _RGB_CODES:
        raise _lib.GcdError(f"{who}: xyz must be float16 / float32 / float64 and rgb those or uint8 "
                            f"(got {xyz.dtype}, {rgb.dtype})")
    if xyz.shape[0] and (xyz.stride(1) != 1 or rgb.stride(1) != 1):
        xyz, rgb = xyz.contiguous(), rgb.contiguous()
    return xyz, rgb


def splat(xyz: torch.Tensor, rgb: torch.Tensor, cams: torch.Tensor, H: int, W: int, spread_radius: int = 2,
          want_uv_depth: bool = False):
    """The splat for the nc cameras of `cams` (see pack_cameras) in one pass over the cloud.  Returns
    (img (nc, H, W, 3) float32, pixel_weights (nc, H, W, 1) float64, uv (nc, N, 2) float64 or None,
    depth (nc, N, 1) float64 or None, visible (nc,) int64), all on the device; nothing synchronises."""
    xyz, rgb = _cloud("splat", xyz, rgb)
    _need_gpu(cams)
    if cams.dtype != torch.float64 or cams.dim() != 2 or cams.shape[1] != _lib.RENDER_CAM_DOUBLES or not cams.is_contiguous():
        raise _lib.GcdError(f"splat: cams must be a contiguous (nc, {_lib.RENDER_CAM_DOUBLES}) float64 tensor (pack_cameras)")
    lib = _lib.load_render()
    nc, N, dev = cams.shape[0], xyz.shape[0], xyz.device
    need = lib.gcd_render_scratch_bytes(nc, H, W)
    if need == 0:
        _lib.check_render(2, "gcd_render_scratch_bytes")
    scratch = torch.empty(need // 8, dtype=torch.int64, device=dev)
    img = torch.empty(nc, H, W, 3, dtype=torch.float32, device=dev)
    weights = torch.empty(nc, H, W, 1, dtype=torch.float64, device=dev)
    uv = torch.empty(nc, N, 2, dtype=torch.float64, device=dev) if want_uv_depth else None
    depth = torch.empty(nc, N, 1, dtype=torch.float64, device=dev) if want_uv_depth else None
    status = torch.empty(nc, dtype=torch.int64, device=dev)
    d = _lib.RenderSplatDesc(
        xyz=xyz.data_ptr() if N else None, rgb=rgb.data_ptr() if N else None,
        xyz_ld=xyz.stride(0) if N else 3, rgb_ld=rgb.stride(0) if N else 3, N=N,
        xyz_dtype=_XYZ_CODES[xyz.dtype], rgb_dtype=_RGB_CODES[rgb.dtype], cams=cams.data_ptr(),
        nc=nc, H=H, W=W, spread_radius=spread_radius,
        img=img.data_ptr(), img_cs=H * W * 3, img_ld=W * 3, weights=weights.data_ptr(), weights_cs=H * W, weights_ld=W,
        uv=uv.data_ptr() if want_uv_depth and N else None, depth=depth.data_ptr() if want_uv_depth and N else None,
        status=status.data_ptr(), scratch=scratch.data_ptr(), scratch_bytes=need)
    _lib.check_render(lib.gcd_render_splat(C.byref(d), _stream()), "gcd_render_splat")
    return img, weights, uv, depth, status


def fill_resize(img: torch.Tensor, out: torch.Tensor, kernel_size: int, sigma: float, scale: float = 2.0,
                offset: float = -1.0) -> torch.Tensor:
    """img (H, W, 3) float32 -> out (3, Hp, Wp) float32 (any strides: a slot of a batch tensor, or a permuted view):
    holes filled from the k x k Gaussian of their surroundings, the 3 x 3 smoothing, the bilinear resize and
    value * scale + offset."""
    if not (torch.is_tensor(img) and torch.is_tensor(out)):
        raise _lib.GcdError("fill_resize: operands must be torch tensors on the GPU; there is no CPU fallback")
    _need_gpu(img, out)
    if img.dtype != torch.float32 or out.dtype != torch.float32:
        raise _lib.GcdError(f"fill_resize: operands must be float32 (got {img.dtype}, {out.dtype})")
    if img.dim() != 3 or img.shape[2] != 3 or out.dim() != 3 or out.shape[0] != 3:
        raise _lib.GcdError(f"fill_resize: img must be (H, W, 3) and out (3, Hp, Wp), got {tuple(img.shape)}, {tuple(out.shape)}")
    if img.stride(2) != 1 or img.stride(1) != 3:
        img = img.contiguous()
    H, W = img.shape[:2]
    lib = _lib.load_render()
    need = lib.gcd_render_fill_scratch_bytes(H, W)
    if need == 0:
        _lib.check_render(2, "gcd_render_fill_scratch_bytes")
    scratch = torch.empty(need // 8, dtype=torch.float64, device=img.device)
    _lib.check_render(lib.gcd_render_fill_resize_f32(
        img.data_ptr(), img.stride(0), H, W, int(kernel_size), float(sigma), out.data_ptr(), out.stride(0), out.stride(1),
        out.stride(2), out.shape[1], out.shape[2], float(scale), float(offset), scratch.data_ptr(), need, _stream()),
        "gcd_render_fill_resize_f32")
    return out


def project_points_to_pixels(xyzrgb: Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]], K, RT, H: int, W: int,
                             spread_radius: int = 2):
    """xyzrgb: an (N, 6) float tensor, or an (xyz, rgb) pair (xyz float16 / 32 / 64, rgb those or uint8 0 .. 255).
    Returns (img (H, W, 3) float32 in [0, 1], pixel_weights (H, W, 1) float64 with -1 where nothing landed,
    uv (N, 2) float64, depth (N, 1) float64)."""
    if isinstance(xyzrgb, (tuple, list)):
        xyz, rgb = xyzrgb
    else:
        if not torch.is_tensor(xyzrgb):
            raise _lib.GcdError("project_points_to_pixels: the cloud must be a torch tensor on the GPU; there is no CPU fallback")
        if xyzrgb.dim() != 2 or xyzrgb.shape[1] != 6:
            raise _lib.GcdError(f"project_points_to_pixels: xyzrgb must be (N, 6), got {tuple(xyzrgb.shape)}")
        xyz, rgb = xyzrgb[:, 0:3], xyzrgb[:, 3:6]          # two strided views: the cloud is not copied
    xyz, rgb = _cloud("project_points_to_pixels", xyz, rgb)
    img, weights, uv, depth, _ = splat(xyz, rgb, pack_cameras(K, RT, xyz.device), H, W, spread_radius, want_uv_depth=True)
    return img[0], weights[0], uv[0], depth[0]


def blur_into_black(img: torch.Tensor, kernel_size: int = 5, sigma: float = 1.5) -> torch.Tensor:
    """img (H, W, 3) float32 -> (H, W, 3) float32: pixels whose three channels sum to 0 take the Gaussian of the valid
    pixels around them, then the 3 x 3 smoothing (sigma 0.6)."""
    if not torch.is_tensor(img):
        raise _lib.GcdError("blur_into_black: img must be a torch tensor on the GPU; there is no CPU fallback")
    _need_gpu(img)
    out = torch.empty(tuple(img.shape), dtype=torch.float32, device=img.device)
    fill_resize(img, out.permute(2, 0, 1), kernel_size, sigma, scale=1.0, offset=0.0)
    return out


def render_views(xyz: torch.Tensor, rgb: torch.Tensor, K, RTs, render_hw: Tuple[int, int], frame_hw: Tuple[int, int],
                 spread_radius: int, kernel_size: int, sigma: float,
                 out: Optional[Sequence[torch.Tensor]] = None, cams: Optional[torch.Tensor] = None):
    """The fused route: the cloud is read once for the nc cameras of RTs (nc, 4, 4), and each view is filled, resized
    to frame_hw and mapped to [-1, 1] into out[i] (3, Hp, Wp), which may be a slot of a batch tensor.  Without `out` a
    (nc, 3, Hp, Wp) tensor is made.  `cams`: a table from pack_cameras in place of K / RTs (nothing is copied to the
    device then, so the call can be captured into a graph)."""
    xyz, rgb = _cloud("render_views", xyz, rgb)
    if cams is None:
        cams = pack_cameras(K, RTs, xyz.device)
    nc = cams.shape[0]
    if out is None:
        out = torch.empty(nc, 3, frame_hw[0], frame_hw[1], dtype=torch.float32, device=xyz.device)
    if len(out) != nc or any(tuple(o.shape) != (3, frame_hw[0], frame_hw[1]) for o in out):
        raise _lib.GcdError(f"render_views: out must hold {nc} tensors of shape {(3, *frame_hw)}")
    img, _, _, _, _ = splat(xyz, rgb, cams, render_hw[0], render_hw[1], spread_radius)
    for i in range(nc):
        fill_resize(img[i], out[i], kernel_size, sigma)
    return out


def synth_src_dst_rgb(pcl_dict, extrinsics_src, extrinsics_dst, avail_intrinsics, avail_extrinsics, *, model_frames: int,
                      render_height: int, render_width: int, frame_height: int, frame_width: int, spread_radius: int,
                      reproject_rgbd: bool = False):
    """pcl_dict['xyz'][t] (V, N, 3) float16 and pcl_dict['rgb'][t] (V, N, 3) uint8 per frame; extrinsics (T, 4, 4) and
    avail_intrinsics (T, 3, 3) float32, normalised to the unit image.  Returns (rgb_src, rgb_dst, reproject or None),
    (T, 3, Hp, Wp) float32 in [-1, 1] on the device.  `reproject` renders the stored viewpoint 4 alone into the target
    camera with a 3 x 3 fill: the baseline that metrics_device.calculate_metrics takes."""
    T = model_frames
    blur, reproject_blur = 21, 3
    K = torch.as_tensor(avail_intrinsics)[0].detach().cpu().to(torch.float32).clone()
    K[0, :] *= render_width
    K[1, :] *= render_height
    old_ar, new_ar = 576.0 / 384.0, render_width / render_height          # the crop of the frame loader, not a stretch
    if new_ar > old_ar + 1e-3:
        K[1, 1] = K[0, 0]
    elif new_ar < old_ar - 1e-3:
        K[0, 0] = K[1, 1]
    first = pcl_dict["xyz"][0]
    if not torch.is_tensor(first):
        raise _lib.GcdError("synth_src_dst_rgb: the clouds must be torch tensors on the GPU; there is no CPU fallback")
    _need_gpu(first)
    dev = first.device
    src, dst = torch.as_tensor(extrinsics_src), torch.as_tensor(extrinsics_dst)
    shape = (T, 3, frame_height, frame_width)
    rgb_src = torch.empty(shape, dtype=torch.float32, device=dev)
    rgb_dst = torch.empty(shape, dtype=torch.float32, device=dev)
    reproject = torch.empty(shape, dtype=torch.float32, device=dev) if reproject_rgbd else None
    hw, fhw = (render_height, render_width), (frame_height, frame_width)
    for t in range(T):
        xyz, rgb = pcl_dict["xyz"][t], pcl_dict["rgb"][t]
        render_views(xyz.reshape(-1, 3), rgb.reshape(-1, 3), K, torch.stack([src[t], dst[t]]), hw, fhw, spread_radius, blur,
                     blur / 4.0, out=[rgb_src[t], rgb_dst[t]])
        if reproject is not None:
            render_views(xyz[4], rgb[4], K, dst[t:t + 1], hw, fhw, spread_radius, reproject_blur, reproject_blur / 4.0,
                         out=[reproject[t]])
    return rgb_src, rgb_dst, reproject


# ---- ParallelDomain: class colours and the modal blend ------------------------------------------------------------------

PARDOM_SRC_VIEW = 16           # the stored forward ego viewpoint: what `reproject` renders
_PARDOM_MODES = {"rgb": _lib_pardom.PARDOM_RGB, "blend": _lib_pardom.PARDOM_BLEND, "palette": _lib_pardom.PARDOM_PALETTE}


def semantic_palette(items) -> Tuple[torch.Tensor, int]:
    """The class colours of an ontology's `items` ({'id': k, 'color': {'r', 'g', 'b'}} each) as the (256, 3) float64
    table `class_colours` reads, with n_classes = the largest id + 1: row k is (r, g, b) / 255.0 in float64, ids that no
    item names and the rows from n_classes on are zero.  Host code."""
    by_id = {int(x["id"]): (x["color"]["r"], x["color"]["g"], x["color"]["b"]) for x in items}
    if not by_id or min(by_id) < 0 or max(by_id) >= _lib_pardom.PARDOM_PALETTE_ROWS:
        raise ValueError(f"semantic_palette: class ids must lie in 0 .. {_lib_pardom.PARDOM_PALETTE_ROWS - 1}")
    table = np.zeros((_lib_pardom.PARDOM_PALETTE_ROWS, 3))
    for k, v in by_id.items():
        table[k] = np.array(v) / 255.0
    return torch.tensor(table), max(by_id) + 1


def pardom_frame_mode(t: int, modal_time: int, modality: str):
    """What frame t of a clip shows: (None, 0.0) for the stored colours as they are (the `rgb` modality: no colour
    kernel), else (mode of `class_colours`, alpha).  In `segm` the clip fades from colour to class colour over the first
    modal_time frames."""
    if modality == "rgb":
        return None, 0.0
    if modality != "segm":
        raise ValueError(f"Unknown selected modality: {modality}")
    if 0 < t < modal_time:
        return _lib_pardom.PARDOM_BLEND, t / modal_time
    if t == 0 and 0 < modal_time:
        return _lib_pardom.PARDOM_RGB, 0.0
    return _lib_pardom.PARDOM_PALETTE, 1.0


def _points(t: torch.Tensor, channels: int) -> torch.Tensor:
    """(..., channels) -> (N, channels) with a unit channel stride: a view where the strides allow one."""
    t = t.reshape(-1, channels)
    unit = channels == 1 or t.stride(1) == 1
    return t if t.shape[0] == 0 or (unit and t.stride(0) >= channels) else t.contiguous()


def class_colours(ids: Optional[torch.Tensor], rgb: Optional[torch.Tensor], palette: torch.Tensor, alpha: float,
                  mode: Union[int, str], out: Optional[torch.Tensor] = None, n_classes: int = _lib_pardom.PARDOM_PALETTE_ROWS):
    """The colours of a cloud's points: ids (N,), (N, 1) or (V, N, 1) uint8 class ids, rgb (N, 3) or (V, N, 3) uint8,
    palette (256, 3) float64 (see semantic_palette), mode 'rgb' | 'blend' | 'palette' (or the PARDOM_* codes).  `ids` may be
    None in mode 'rgb' and `rgb` in mode 'palette'.  Returns (out (N, 3) float64 — `out` itself when given, which may
    have a row stride above 3 — and the number of ids >= n_classes as an int64 device tensor of one element; such a
    point takes the class colour 0).  Nothing synchronises."""
    code = _PARDOM_MODES.get(mode, mode) if isinstance(mode, str) else mode
    if code not in _PARDOM_MODES.values():
        raise ValueError(f"class_colours: mode must be one of {sorted(_PARDOM_MODES)}, got {mode!r}")
    need_ids, need_rgb = code != _lib_pardom.PARDOM_RGB, code != _lib_pardom.PARDOM_PALETTE
    given = [t for t, need in ((ids, need_ids), (rgb, need_rgb)) if need or t is not None]
    if not all(torch.is_tensor(t) for t in (*given, palette)):
        raise _lib.GcdError("class_colours: the operands must be torch tensors on the GPU; there is no CPU fallback")
    _need_gpu(*given, palette)
    if any(t.dtype != torch.uint8 for t in given):
        raise _lib.GcdError("class_colours: ids and rgb must be uint8")
    if palette.dtype != torch.float64 or tuple(palette.shape) != (_lib_pardom.PARDOM_PALETTE_ROWS, 3) or not palette.is_contiguous():
        raise _lib.GcdError(f"class_colours: palette must be a contiguous ({_lib_pardom.PARDOM_PALETTE_ROWS}, 3) float64 tensor")
    ids = _points(ids, 1) if ids is not None else None
    rgb = _points(rgb, 3) if rgb is not None else None
    N = (ids if rgb is None else rgb).shape[0]
    if ids is not None and rgb is not None and ids.shape[0] != rgb.shape[0]:
        raise _lib.GcdError(f"class_colours: {ids.shape[0]} ids for {rgb.shape[0]} colours")
    dev = palette.device
    if out is None:
        out = torch.empty(N, 3, dtype=torch.float64, device=dev)
    else:
        _need_gpu(out)
        if out.dtype != torch.float64 or tuple(out.shape) != (N, 3) or (N and (out.stride(1) != 1 or out.stride(0) < 3)):
            raise _lib.GcdError(f"class_colours: out must be ({N}, 3) float64 with a unit channel stride, got "
                                f"{tuple(out.shape)} {out.dtype} strides {tuple(out.stride())}")
    status = torch.empty(1, dtype=torch.int64, device=dev)
    lib = _lib_pardom.load()
    _lib_pardom.check(lib.gcd_pardom_colours(
        ids.data_ptr() if ids is not None and N else None, ids.stride(0) if ids is not None and N else 1,
        rgb.data_ptr() if rgb is not None and N else None, rgb.stride(0) if rgb is not None and N else 3, N,
        palette.data_ptr(), int(n_classes), float(alpha), code, out.data_ptr() if N else None, out.stride(0) if N else 3,
        status.data_ptr(), _stream()), "gcd_pardom_colours")
    return out, status


def synth_rgb_pardom(pcl_dict, modality: str, extrinsics, intrinsics, *, palette: Optional[torch.Tensor] = None,
                     n_classes: int = _lib_pardom.PARDOM_PALETTE_ROWS, modal_time: int = 0, model_frames: int,
                     render_height: int, render_width: int, frame_height: int, frame_width: int, spread_radius: int,
                     calc_reproject: bool = False, reproject_rgbd: bool = False):
    """The ParallelDomain dataset's synth_rgb.  pcl_dict['xyz'][t] (V, N, 3) float16, pcl_dict['rgb'][t] (V, N, 3) uint8
    and pcl_dict['segm'][t] (V, N, 1) uint8 per frame, on the device; extrinsics (T, 4, 4) and intrinsics (T, 3, 3)
    float32, the latter normalised to the unit image; palette / n_classes from semantic_palette (the `segm` modality
    only).  Returns (rgb, reproject or None), (T, 3, Hp, Wp) float32 in [-1, 1] on the device; `reproject`, made when
    calc_reproject and reproject_rgbd are both set, renders the stored viewpoint 16 alone with a 3 x 3 fill.  An id that
    is not below n_classes shows the class colour 0 (the original raises an IndexError)."""
    T = model_frames
    blur, reproject_blur = 21, 3
    pardom_frame_mode(0, modal_time, modality)                            # an unknown modality raises before any work
    K = torch.as_tensor(intrinsics).detach().cpu().to(torch.float32).clone()
    K[:, 0, :] *= render_width
    K[:, 1, :] *= render_height
    old_ar, new_ar = 640.0 / 480.0, render_width / render_height          # the crop of the frame loader, not a stretch
    if new_ar > old_ar + 1e-3:
        K[:, 1, 1] = K[:, 0, 0]
    elif new_ar < old_ar - 1e-3:
        K[:, 0, 0] = K[:, 1, 1]
    first = pcl_dict["xyz"][0]
    if not torch.is_tensor(first):
        raise _lib.GcdError("synth_rgb_pardom: the clouds must be torch tensors on the GPU; there is no CPU fallback")
    _need_gpu(first)
    dev = first.device
    cams = pack_cameras(K[:T], torch.as_tensor(extrinsics)[:T], dev)      # one copy to the device for the clip
    shape = (T, 3, frame_height, frame_width)
    rgb_out = torch.empty(shape, dtype=torch.float32, device=dev)
    reproject = torch.empty(shape, dtype=torch.float32, device=dev) if calc_reproject and reproject_rgbd else None
    hw, fhw = (render_height, render_width), (frame_height, frame_width)
    colours = None
    if modality == "segm":
        if palette is None:
            raise ValueError("synth_rgb_pardom: the segm modality needs a palette (semantic_palette)")
        palette = palette.to(dev)
        n_points = max(int(x.shape[0] * x.shape[1]) for x in pcl_dict["xyz"][:T])
        colours = torch.empty(n_points, 3, dtype=torch.float64, device=dev)      # reused by every frame
    for t in range(T):
        xyz, rgb = pcl_dict["xyz"][t], pcl_dict["rgb"][t]
        V, N = xyz.shape[0], xyz.shape[1]
        mode, alpha = pardom_frame_mode(t, modal_time, modality)
        if mode is None:
            vis = rgb
        else:
            vis, _ = class_colours(pcl_dict["segm"][t], rgb, palette, alpha, mode, out=colours[:V * N], n_classes=n_classes)
            vis = vis.view(V, N, 3)
        render_views(xyz.reshape(-1, 3), vis.reshape(-1, 3), None, None, hw, fhw, spread_radius, blur, blur / 4.0,
                     out=[rgb_out[t]], cams=cams[t:t + 1])
        if reproject is not None:
            render_views(xyz[PARDOM_SRC_VIEW], vis[PARDOM_SRC_VIEW], None, None, hw, fhw, spread_radius, reproject_blur,
                         reproject_blur / 4.0, out=[reproject[t]], cams=cams[t:t + 1])
    return rgb_out, reproject


# ---- camera helpers (host, numpy) ---------------------------------------------------------------------------------------

def cartesian_from_spherical(spherical, deg2rad: bool = False):
    """(..., 3) (azimuth, elevation, radius) -> (..., 3) (x, y, z), z up."""
    s = np.asarray(spherical)
    az, el, r = s[..., 0], s[..., 1], s[..., 2]
    if deg2rad:
        az, el = np.deg2rad(az), np.deg2rad(el)
    ce = r * np.cos(el)
    return np.stack([ce * np.cos(az), ce * np.sin(az), r * np.sin(el)], axis=-1)


def extrinsics_from_look_at(camera_position, camera_look_at):
    """A (4, 4) camera-to-world matrix whose columns are the camera's right, down and forward axes; the world's down
    direction is -z."""
    pos = np.asarray(camera_position, dtype=np.float64)
    fwd = np.asarray(camera_look_at, dtype=np.float64) - pos
    fwd = fwd / np.linalg.norm(fwd)
    right = np.cross(np.array([0.0, 0.0, -1.0]), fwd)
    right = right / np.linalg.norm(right)
    down = np.cross(fwd, right)
    RT = np.eye(4)
    RT[0:3, 0], RT[0:3, 1], RT[0:3, 2], RT[0:3, 3] = right, down, fwd, pos
    return RT


def camera_to_world(xyz_camera, extrinsics):
    """(..., 3) camera coordinates -> world coordinates: x R^T + t."""
    return xyz_camera @ extrinsics[0:3, 0:3].T + extrinsics[0:3, 3]


def world_to_camera(xyz_world, extrinsics):
    """(..., 3) world coordinates -> camera coordinates: (x - t) R."""
    return (xyz_world - extrinsics[0:3, 3]) @ extrinsics[0:3, 0:3]
