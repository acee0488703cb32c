"""ctypes binding of libgcd_amd.so (the C ABI declared in include/gcd_amd.h).

The library is the product: there is no Python/CPU fallback.  If the shared object is missing or a
call fails, this module raises — loudly — instead of computing the result some other way.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import Callable, NamedTuple

import os

_PKG = Path(__file__).resolve().parent
# GCD_AMD_LIB: another build of the SAME sources (tools/libgcd_amd_*.so: ablation / A-B variants) for the benchmark
# tools; the product is the in-tree library next to this file.
LIB_PATH = Path(os.environ["GCD_AMD_LIB"]).resolve() if os.environ.get("GCD_AMD_LIB") else _PKG / "libgcd_amd.so"

ABI_VERSION = 9

# GEMM modes / output kinds (mirror include/gcd_amd.h)
GEMM_PLAIN, GEMM_CONV3X3, GEMM_TEMPORAL3 = 0, 1, 2
OUT_F32, OUT_F16, OUT_GEGLU = 0, 1, 2


class GcdError(RuntimeError):
    """A libgcd_amd entry point returned a non-zero status."""


class GemmDesc(C.Structure):
    _fields_ = [
        ("A", C.c_void_p), ("W", C.c_void_p), ("out", C.c_void_p),
        ("lda", C.c_int64), ("ldo", C.c_int64),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("mode", C.c_int32),
        ("Cin", C.c_int32), ("Hi", C.c_int32), ("Wi", C.c_int32), ("Ho", C.c_int32),
        ("Wo", C.c_int32), ("stride", C.c_int32), ("upsample", C.c_int32), ("T", C.c_int32),
        ("HW", C.c_int32),
        ("bias", C.c_void_p), ("rowvec", C.c_void_p), ("ld_rowvec", C.c_int64),
        ("rows_per_vec", C.c_int32),
        ("R1", C.c_void_p), ("ldr1", C.c_int64), ("R2", C.c_void_p), ("ldr2", C.c_int64),
        ("s_acc", C.c_float), ("s_r1", C.c_float), ("s_r2", C.c_float),
        ("frame_alpha", C.c_void_p), ("rows_per_alpha", C.c_int32), ("r1_blend", C.c_int32),
        ("out_kind", C.c_int32), ("zero_page", C.c_void_p),
        ("ln_out16", C.c_void_p), ("ld_ln_out", C.c_int64), ("ln_gamma", C.c_void_p),
        ("ln_beta", C.c_void_p), ("ln_eps", C.c_float), ("ln_rows_per_vec", C.c_int32),
        ("ln_addvec", C.c_void_p), ("ld_ln_addvec", C.c_int64), ("ln_sum_out", C.c_void_p),
        ("ld_ln_sum", C.c_int64),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("asym_pad", C.c_int32),
        ("colstats", C.c_void_p), ("out_blocked", C.c_int32), ("a_blocked", C.c_int32),
        ("operand_bf16", C.c_int32), ("sched", C.c_int32),
    ]


class FfDesc(C.Structure):
    """gcd_ff_desc (include/gcd_amd.h): the one-kernel FeedForward of the C = 320 level."""
    _fields_ = [
        ("X", C.c_void_p), ("ldx", C.c_int64), ("wp", C.c_void_p), ("b1", C.c_void_p), ("b2", C.c_void_p),
        ("R1", C.c_void_p), ("ldr1", C.c_int64), ("R2", C.c_void_p), ("ldr2", C.c_int64),
        ("out", C.c_void_p), ("ldo", C.c_int64), ("out_kind", C.c_int32),
        ("frame_alpha", C.c_void_p), ("rows_per_alpha", C.c_int32), ("s_acc", C.c_float), ("s_r2", C.c_float),
        ("M", C.c_int32), ("C", C.c_int32), ("hidden", C.c_int32), ("sched", C.c_int32),
        ("x32", C.c_void_p), ("ldx32", C.c_int64), ("ln_gamma", C.c_void_p), ("ln_beta", C.c_void_p),
        ("ln_eps", C.c_float), ("addvec", C.c_void_p), ("ld_addvec", C.c_int64), ("rows_per_vec", C.c_int32),
    ]


_vp, _i, _i64, _f = C.c_void_p, C.c_int, C.c_int64, C.c_float

# name -> (restype, argtypes); every symbol include/gcd_amd.h declares
SIGNATURES = {
    "gcd_abi_version": (_i, []),
    "gcd_last_error": (C.c_char_p, []),
    "gcd_device_info": (_i, [_i, C.c_char_p, _i, C.POINTER(_i), C.POINTER(C.c_size_t)]),
    "gcd_tune_set": (_i, [_i, _i]),
    "gcd_gemm_f16": (_i, [C.POINTER(GemmDesc), _vp]),
    "gcd_gemm_ln_fusable": (_i, [_i, _i, _i, _i]),
    "gcd_gemm_colstats_supported": (_i, [C.POINTER(GemmDesc)]),
    "gcd_gemm_hidden_blocked_supported": (_i, [_i, _i, _i]),
    "gcd_ff_packed_bytes": (_i64, []),
    "gcd_ff_pack_f16": (_i, [_vp, _vp, _vp, _i, _vp]),
    "gcd_ff_fused_supported": (_i, [_i, _i, _i]),
    "gcd_ff_fused_fits": (_i, [_i64, _i, _i, _i64, _i]),
    "gcd_ff_fused_f16": (_i, [C.POINTER(FfDesc), _vp]),
    "gcd_lnqkv_packed_bytes": (_i64, [_i]),
    "gcd_lnqkv_supported": (_i, [_i, _i]),
    "gcd_lnqkv_fits": (_i, [_i, _i, _i64, _i64]),
    "gcd_lnqkv_pack_f16": (_i, [_vp, _i, _vp, _vp]),
    "gcd_lnqkv_f16": (_i, [_vp, _i64, _vp, _vp, _f, _vp, _vp, _i64, _i, _i, _i, _i, _vp]),
    "gcd_groupnorm_stats_from_colsums": (_i, [_vp, _i, _vp, _i, _i64, _i64, _f, _vp, _vp]),
    "gcd_linear_smallm_f32": (_i, [_vp, _i64, _vp, _vp, _vp, _i64, _i, _i, _i, _i, _vp]),
    "gcd_groupnorm_stats": (_i, [_vp, _i64, _i, _vp, _i64, _i, _i64, _i64, _f, _vp, _i, _vp, _vp]),
    "gcd_groupnorm_apply": (_i, [_vp, _i64, _i, _vp, _i64, _i, _i64, _i64, _vp, _vp, _vp, _i, _vp,
                                 _i64, _vp, _i64, _vp]),
    "gcd_layernorm_f16": (_i, [_vp, _i64, _i64, _i, _vp, _vp, _f, _vp, _i64, _i, _vp, _i64, _vp,
                               _i64, _i, _vp]),
    "gcd_attn_transpose_v": (_i, [_vp, _i64, _i, _i, _i, _vp, _i, _vp]),
    "gcd_attn_spatial_f16": (_i, [_vp, _i64, _vp, _i, _vp, _i64, _i, _i, _i, _i, _vp]),
    "gcd_attn_temporal_f16": (_i, [_vp, _i64, _vp, _i64, _i, _i, _i, _i, _vp]),
    "gcd_attn_temporal_long_f16": (_i, [_vp, _i64, _vp, _i64, _i, _i, _i, _i, _vp]),
    "gcd_softmax_rows_f16": (_i, [_vp, _i64, _vp, _i64, _i64, _i, _vp]),
    "gcd_transpose_f16": (_i, [_vp, _i64, _vp, _i64, _i, _i, _vp]),
    "gcd_time_mix_unpack": (_i, [_vp, _i64, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "gcd_pack_input": (_i, [_vp, _i, _i, _vp, _i, _vp, _i, _i, _vp, _i, _vp]),
    "gcd_unpack_output": (_i, [_vp, _i64, _vp, _i, _i, _i, _vp]),
    "gcd_cast_f32_f16": (_i, [_vp, _i64, _vp, _i64, _i64, _i, _vp]),
    "gcd_cfg_euler_step": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i64, _vp]),
    "gcd_edm_scalings": (_i, [_vp, _vp, _vp, _i, _vp]),
    "gcd_timestep_embedding": (_i, [_vp, _vp, _i, _i, _f, _vp]),
    "gcd_im2col3x3_f16": (_i, [_vp, _i64, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "gcd_col2im3x3_f32": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "gcd_im2col_t3_f16": (_i, [_vp, _i64, _vp, _i64, _i, _i, _i, _vp]),
    "gcd_col2im_t3_f32": (_i, [_vp, _vp, _i64, _i64, _i, _i, _i, _vp]),
    "gcd_rowblock_sum_f32": (_i, [_vp, _i64, _i64, _i, _i64, _vp, _vp]),
    "gcd_groupnorm_bwd_scratch_floats": (_i64, [_i, _i64, _i64]),
    "gcd_groupnorm_bwd": (_i, [_vp, _i64, _vp, _i64, _i, _i64, _i64, _vp, _vp, _vp, _i, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp]),
    "gcd_layernorm_bwd": (_i, [_vp, _i64, _vp, _i64, _i64, _i, _vp, _f, _vp, _i64, _vp, _vp, _vp, _i64, _vp]),
    "gcd_geglu_fwd_f32": (_i, [_vp, _i64, _vp, _i64, _i64, _i, _vp]),
    "gcd_geglu_fwd_f16": (_i, [_vp, _i64, _vp, _i64, _i64, _i, _vp]),
    "gcd_geglu_fwd_bf16": (_i, [_vp, _i64, _vp, _i64, _i64, _i, _vp]),
    "gcd_geglu_bwd_f32": (_i, [_vp, _i64, _vp, _i64, _vp, _i64, _i64, _i, _vp]),
    "gcd_softmax_bwd_rows": (_i, [_vp, _i64, _vp, _i64, _vp, _i64, _i64, _i, _f, _vp]),
    "gcd_attn_spatial_bwd_ws_bytes": (_i64, [_i, _i, _i]),
    "gcd_attn_spatial_bwd": (_i, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i, _i, _i, _f, _vp]),
    "gcd_attn_temporal_bwd": (_i, [_vp, _i64, _vp, _i64, _vp, _i64, _i, _i, _i, _i, _vp]),
    "gcd_attn_temporal_long_bwd": (_i, [_vp, _i64, _vp, _i64, _vp, _i64, _i, _i, _i, _i, _vp]),
    "gcd_cast_scale_f32_f16": (_i, [_vp, _i64, _vp, _i64, _i64, _i, _f, _vp]),
    "gcd_cast_f32_bf16": (_i, [_vp, _i64, _vp, _i64, _i64, _i, _vp]),
    "gcd_cast_colsum_f32": (_i, [_vp, _i64, _vp, _i64, _i64, _i, _i64, _vp, _i, _vp, _vp]),
    "gcd_cast_f16_bf16": (_i, [_vp, _i64, _vp, _i64, _i64, _i, _vp]),
    "gcd_adam_step": (_i, [_vp, _vp, _vp, _vp, _i64, _f, _f, _f, _f, _f, _i, _f, _vp]),
    "gcd_adam_step_multi": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _i, _f, _vp]),
    "gcd_graph_begin_capture": (_i, [_vp]),
    "gcd_graph_end_capture": (_i, [_vp, C.POINTER(_vp)]),
    "gcd_graph_launch": (_i, [_vp, _vp]),
    "gcd_graph_destroy": (_i, [_vp]),
    "gcd_event_create": (_i, [C.POINTER(_vp)]),
    "gcd_event_record": (_i, [_vp, _vp]),
    "gcd_event_sync": (_i, [_vp]),
    "gcd_event_elapsed_ms": (_i, [_vp, _vp, C.POINTER(_f)]),
    "gcd_event_destroy": (_i, [_vp]),
    "gcd_stream_sync": (_i, [_vp]),
}

# libgcd_amd_train.so (include/gcd_amd_train.h): kernels of the fine-tune step only
TRAIN_LIB_PATH = _PKG / "libgcd_amd_train.so"
TRAIN_ABI_VERSION = 3


class PackEntry(C.Structure):
    """gcd_pack_entry (include/gcd_amd_train.h)."""
    _fields_ = [("src", _vp), ("dst_f", _vp), ("dst_t", _vp),
                ("f_ns", _i64), ("f_ts", _i64), ("t_cs", _i64), ("t_ts", _i64),
                ("N", C.c_int32), ("C", C.c_int32), ("taps", C.c_int32), ("mirror", C.c_int32),
                ("tile0", C.c_int32), ("tiles_c", C.c_int32)]


class SmallmProblem(C.Structure):
    """gcd_smallm_problem (include/gcd_amd_train.h)."""
    _fields_ = [("x", _vp), ("W", _vp), ("b", _vp), ("y", _vp), ("dx", _vp), ("dW", _vp), ("db", _vp),
                ("ldx", _i64), ("ldy", _i64), ("lddx", _i64),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("flags", C.c_int32),
                ("block0", C.c_int32), ("reserved", C.c_int32)]


TRAIN_SIGNATURES = {
    "gcd_train_abi_version": (_i, []),
    "gcd_train_last_error": (C.c_char_p, []),
    "gcd_wgrad_tr_scratch_floats": (_i64, [_i64, _i, _i]),
    "gcd_wgrad_tr_f16": (_i, [_vp, _i64, _vp, _i64, _i64, _i, _i, _i, _vp, _i64, _vp, _i64, _vp]),
    "gcd_wgrad_tr_f16_ex": (_i, [_vp, _i64, _vp, _i64, _i64, _i, _i, _i, _vp, _i64, _i, _i, _i, _i, _vp, _i64, _vp]),
    "gcd_wgrad_conv_tr_f16": (_i, [_vp, _i64, _vp, _i64, _i64, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _i, _vp, _i64, _vp]),
    "gcd_train_pack_weights": (_i, [_vp, _i, _i, _i, _vp]),
    "gcd_blend_fwd_f32": (_i, [_vp, _i64, _vp, _i64, _vp, _i64, _i, _i64, _vp, _i64, _vp]),
    "gcd_blend_bwd_f32": (_i, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i, _i64, _vp, _i64, _i, _vp, _i64, _vp, _vp]),
    "gcd_gn_affine_grads": (_i, [_vp, _i, _i, _vp, _vp, _i, _vp]),
    "gcd_smallm_fwd": (_i, [_vp, _i, _i, _vp]),
    "gcd_smallm_dgrad": (_i, [_vp, _i, _i, _vp]),
    "gcd_smallm_wgrad": (_i, [_vp, _i, _i, _vp]),
}

# the deterministic reductions (include/gcd_amd_train_det.h; gcd_amd/csrc/train_det.hip), same shared object
TRAIN_DET_SIGNATURES = {
    "gcd_rowblock_sum_det_scratch_floats": (_i64, [_i64, _i, _i64]),
    "gcd_rowblock_sum_det_f32": (_i, [_vp, _i64, _i64, _i, _i64, _vp, _vp, _i64, _vp]),
    "gcd_layernorm_bwd_det_scratch_floats": (_i64, [_i64, _i]),
    "gcd_layernorm_bwd_det": (_i, [_vp, _i64, _vp, _i64, _i64, _i, _vp, _f, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _vp]),
    "gcd_cast_colsum_det_scratch_floats": (_i64, [_i64, _i, _i64]),
    "gcd_cast_colsum_det_f32": (_i, [_vp, _i64, _vp, _i64, _i64, _i, _i64, _vp, _i, _vp, _vp, _i64, _vp]),
    "gcd_blend_bwd_det_scratch_floats": (_i64, [_i64, _i, _i64]),
    "gcd_blend_bwd_det_f32": (_i, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i, _i64, _vp, _i64, _i, _vp, _i64, _vp,
                                   _vp, _i64, _vp]),
    "gcd_smallm_dgrad_det_scratch_floats": (_i64, [_i]),
    "gcd_smallm_dgrad_det": (_i, [_vp, _i, _i, _vp, _i64, _vp]),
}



# the device-resident optimizer step (include/gcd_amd_train_optim.h; gcd_amd/csrc/train_optim.hip), same shared object
OPTIM_CHUNK = 16384


class OptimState(C.Structure):
    """gcd_optim_state: 64 bytes of device memory (fp32 / int32 only)."""
    _fields_ = [("step", C.c_int32), ("lr", _f), ("loss_scale", _f), ("growth_tracker", C.c_int32),
                ("found_inf", C.c_int32), ("grad_norm", _f), ("clip_coef", _f), ("skipped_total", C.c_int32),
                ("ema_num_updates", C.c_int32), ("gfactor", _f), ("bc1", _f), ("bc2_sqrt", _f), ("ema_omd", _f),
                ("reserved", C.c_int32 * 3)]


class OptimTensor(C.Structure):
    """gcd_optim_tensor: one entry of the device table."""
    _fields_ = [("p", _vp), ("g", _vp), ("m", _vp), ("v", _vp), ("ema", _vp), ("n", _i64),
                ("chunk0", C.c_int32), ("reserved", C.c_int32)]


class OptimConfig(C.Structure):
    """gcd_optim_config: hyper-parameters, host memory."""
    _fields_ = [("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("weight_decay", C.c_double),
                ("grad_scale", _f), ("max_norm", _f), ("growth_factor", _f), ("backoff_factor", _f), ("ema_decay", _f),
                ("growth_interval", C.c_int32), ("dynamic_scale", C.c_int32), ("decoupled", C.c_int32),
                ("use_ema", C.c_int32), ("reserved", C.c_int32), ("ema_count", _vp)]


TRAIN_OPTIM_SIGNATURES = {
    "gcd_optim_gradstat_scratch_floats": (_i64, [_i64]),
    "gcd_optim_gradstat": (_i, [_vp, _i, _i64, C.POINTER(OptimConfig), _vp, _vp, _i64, _vp]),
    "gcd_optim_advance": (_i, [C.POINTER(OptimConfig), _vp, _vp]),
    "gcd_optim_apply": (_i, [_vp, _i, _i64, C.POINTER(OptimConfig), _vp, _vp]),
    "gcd_ema_update": (_i, [_vp, _i, _i64, C.POINTER(OptimConfig), _vp, _vp]),
}

# libgcd_amd_sampler.so (include/gcd_amd_sampler.h; gcd_amd/csrc/sampler_stage.hip): the stage kernel of the sampler family
SAMPLER_LIB_PATH = _PKG / "libgcd_amd_sampler.so"
SAMPLER_ABI_VERSION = 1
SAMPLER_ROW = 12          # floats per row of the coefficient table
SAMPLER_SIGNATURES = {
    "gcd_sampler_abi_version": (_i, []),
    "gcd_sampler_last_error": (C.c_char_p, []),
    "gcd_sampler_stage_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i64, _vp]),
}

# libgcd_amd_metrics.so (include/gcd_amd_metrics.h; gcd_amd/csrc/metrics.hip): the evaluation metrics on the device
METRICS_LIB_PATH = _PKG / "libgcd_amd_metrics.so"
METRICS_ABI_VERSION = 1
METRICS_SIGNED = 1             # flags bit 0: pred is the decoder's raw output in [-1, 1]
METRICS_FRAME_VALUES = 6       # psnr, ssim, psnr_vis, ssim_vis, psnr_occ, ssim_occ
METRICS_DIVERSITY_VALUES = 3   # all, visible, occluded
METRICS_SIGNATURES = {
    "gcd_metrics_abi_version": (_i, []),
    "gcd_metrics_last_error": (C.c_char_p, []),
    "gcd_metrics_frames_scratch_bytes": (_i64, [_i, _i, _i, _i]),
    "gcd_metrics_diversity_scratch_bytes": (_i64, [_i, _i, _i, _i]),
    "gcd_metrics_frames_f32": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _i64, _vp, _vp]),
    "gcd_metrics_diversity_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _i64, _vp, _vp]),
}

# libgcd_amd_render.so (include/gcd_amd_render.h; gcd_amd/csrc/render.hip): point clouds to (source, target) frames
RENDER_LIB_PATH = _PKG / "libgcd_amd_render.so"
RENDER_ABI_VERSION = 1
RENDER_F16, RENDER_F32, RENDER_F64, RENDER_U8 = 0, 1, 2, 3      # element types of the cloud
RENDER_MAX_CAMERAS = 8
RENDER_CAM_DOUBLES = 25        # K (3 x 3) then RT (4 x 4), row-major
RENDER_MAX_KERNEL = 31


class RenderSplatDesc(C.Structure):
    """gcd_render_splat_desc (include/gcd_amd_render.h)."""
    _fields_ = [("xyz", _vp), ("rgb", _vp), ("xyz_ld", _i64), ("rgb_ld", _i64), ("N", _i64),
                ("xyz_dtype", C.c_int32), ("rgb_dtype", C.c_int32), ("cams", _vp),
                ("nc", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("spread_radius", C.c_int32),
                ("img", _vp), ("img_cs", _i64), ("img_ld", _i64),
                ("weights", _vp), ("weights_cs", _i64), ("weights_ld", _i64),
                ("uv", _vp), ("depth", _vp), ("status", _vp), ("scratch", _vp), ("scratch_bytes", _i64)]


_d = C.c_double
RENDER_SIGNATURES = {
    "gcd_render_abi_version": (_i, []),
    "gcd_render_last_error": (C.c_char_p, []),
    "gcd_render_scratch_bytes": (_i64, [_i, _i, _i]),
    "gcd_render_fill_scratch_bytes": (_i64, [_i, _i]),
    "gcd_render_splat": (_i, [C.POINTER(RenderSplatDesc), _vp]),
    "gcd_render_fill_resize_f32": (_i, [_vp, _i64, _i, _i, _i, _d, _vp, _i64, _i64, _i64, _i, _i, _d, _d, _vp, _i64, _vp]),
}


class Binding(NamedTuple):
    """One shared object of the project: where it is, which ABI version it must report, the entries that report the
    version and the last error, the signature table(s) of everything its header(s) declare, and its loader and check."""
    name: str
    path: Path
    abi_version: int
    version_entry: str
    error_entry: str
    tables: tuple
    load: Callable[[], C.CDLL]
    check: Callable[..., None]


def _bind(name: str, path: Path, abi_version: int, version_entry: str, error_entry: str, *tables: dict) -> Binding:
    """`load` and `check` are plain functions over this call's cells: the tape fine-tune engine calls each of them about
    10^4 times per step."""
    cdll = None

    def load() -> C.CDLL:
        """Load the library (once per process).  Raises if it has not been built — never falls back."""
        nonlocal cdll
        if cdll is not None:
            return cdll
        if not path.exists():
            raise GcdError(f"{path} is missing: the HIP library has not been built. "
                           "Run `python -m gcd_amd.csrc.build` (needs hipcc); gcd_amd has no CPU fallback.")
        lib = C.CDLL(str(path))
        for table in tables:
            for entry, (res, args) in table.items():
                fn = getattr(lib, entry)  # AttributeError if the .so does not export a declared symbol
                fn.restype = res
                fn.argtypes = args
        v = getattr(lib, version_entry)()
        if v != abi_version:
            raise GcdError(f"lib{name} ABI version {v} != expected {abi_version}; rebuild the library")
        cdll = lib
        return lib

    def check(rc: int, what: str = "") -> None:
        if rc != 0:
            msg = getattr(load(), error_entry)().decode(errors="replace")
            raise GcdError(f"{what or 'lib' + name + ' call'} failed (status {rc}): {msg}")

    return Binding(name, path, abi_version, version_entry, error_entry, tables, load, check)


BINDINGS = {b.name: b for b in (
    _bind("gcd_amd", LIB_PATH, ABI_VERSION, "gcd_abi_version", "gcd_last_error", SIGNATURES),
    _bind("gcd_amd_train", TRAIN_LIB_PATH, TRAIN_ABI_VERSION, "gcd_train_abi_version", "gcd_train_last_error",
          TRAIN_SIGNATURES, TRAIN_DET_SIGNATURES, TRAIN_OPTIM_SIGNATURES),
    _bind("gcd_amd_sampler", SAMPLER_LIB_PATH, SAMPLER_ABI_VERSION, "gcd_sampler_abi_version", "gcd_sampler_last_error",
          SAMPLER_SIGNATURES),
    _bind("gcd_amd_metrics", METRICS_LIB_PATH, METRICS_ABI_VERSION, "gcd_metrics_abi_version", "gcd_metrics_last_error",
          METRICS_SIGNATURES),
    _bind("gcd_amd_render", RENDER_LIB_PATH, RENDER_ABI_VERSION, "gcd_render_abi_version", "gcd_render_last_error",
          RENDER_SIGNATURES),
)}
load, check = BINDINGS["gcd_amd"].load, BINDINGS["gcd_amd"].check
load_train, check_train = BINDINGS["gcd_amd_train"].load, BINDINGS["gcd_amd_train"].check
load_sampler, check_sampler = BINDINGS["gcd_amd_sampler"].load, BINDINGS["gcd_amd_sampler"].check
load_metrics, check_metrics = BINDINGS["gcd_amd_metrics"].load, BINDINGS["gcd_amd_metrics"].check
load_render, check_render = BINDINGS["gcd_amd_render"].load, BINDINGS["gcd_amd_render"].check
