"""ctypes binding of libldm3d.so (C ABI: include/ldm3d.h).  Fails loudly: there is no fallback path."""
from __future__ import annotations

import ctypes as C
import os
import threading

LDM_MAX_LEVELS = 8
_HERE = os.path.dirname(os.path.abspath(__file__))
# LDM3D_LIB: a diagnostic build of the same sources (tools/kstamps.py: in-kernel stamps); never a different implementation
LIB_PATH = os.environ.get("LDM3D_LIB") or os.path.join(_HERE, "libldm3d.so")


class Measurement(C.Structure):
    """ldm_measurement (include/ldm3d.h): the built-in pooled quadratic measurement of a guided step and its device scratch."""
    _fields_ = [("target", C.c_void_p), ("target_batch", C.c_int), ("weight", C.c_void_p), ("weight_batch", C.c_int),
                ("pool", C.c_int), ("scale", C.c_float), ("normalize", C.c_int),
                ("grad_out", C.c_void_p), ("gx", C.c_void_p), ("dx", C.c_void_p), ("norm2", C.c_void_p), ("norm_table", C.c_void_p)]


class ImageMeasurement(C.Structure):
    """ldm_image_measurement (include/ldm3d.h): the pooled quadratic on the decoded prediction and the device scratch of its step."""
    _fields_ = [("target", C.c_void_p), ("target_batch", C.c_int), ("weight", C.c_void_p), ("weight_batch", C.c_int),
                ("pool", C.c_int), ("scale", C.c_float), ("normalize", C.c_int), ("inv_scale_factor", C.c_float),
                ("z0", C.c_void_p), ("recon", C.c_void_p), ("dz", C.c_void_p), ("grad_out", C.c_void_p), ("gx", C.c_void_p),
                ("dx", C.c_void_p), ("norm2", C.c_void_p), ("norm_table", C.c_void_p), ("partials", C.c_void_p),
                ("vae_workspace", C.c_void_p), ("vae_workspace_bytes", C.c_size_t)]


class UNetCfg(C.Structure):
    _fields_ = [("spatial_dims", C.c_int), ("in_channels", C.c_int), ("out_channels", C.c_int),
                ("num_levels", C.c_int),
                ("channels", C.c_int * LDM_MAX_LEVELS), ("attention_levels", C.c_int * LDM_MAX_LEVELS),
                ("num_head_channels", C.c_int * LDM_MAX_LEVELS), ("num_res_blocks", C.c_int * LDM_MAX_LEVELS),
                ("norm_num_groups", C.c_int), ("norm_eps", C.c_float)]


class VaeCfg(C.Structure):
    _fields_ = [("spatial_dims", C.c_int), ("in_channels", C.c_int), ("out_channels", C.c_int),
                ("latent_channels", C.c_int), ("num_levels", C.c_int),
                ("channels", C.c_int * LDM_MAX_LEVELS), ("num_res_blocks", C.c_int * LDM_MAX_LEVELS),
                ("attention_levels", C.c_int * LDM_MAX_LEVELS),
                ("norm_num_groups", C.c_int), ("norm_eps", C.c_float),
                ("with_encoder_nonlocal_attn", C.c_int), ("with_decoder_nonlocal_attn", C.c_int)]


# name -> (restype, argtypes); mirrors include/ldm3d.h one to one (tests/test_abi.py checks the header against it)
_P = C.c_void_p
_F = C.POINTER(C.c_float)
SIGNATURES = {
    "ldm_version": (C.c_int, []),
    "ldm_last_error": (C.c_char_p, []),
    "ldm_unet_create": (C.c_int, [C.POINTER(UNetCfg), C.POINTER(_P)]),
    "ldm_vae_create": (C.c_int, [C.POINTER(VaeCfg), C.POINTER(_P)]),
    "ldm_model_destroy": (None, [_P]),
    "ldm_model_num_params": (C.c_int, [_P]),
    "ldm_model_param_name": (C.c_char_p, [_P, C.c_int]),
    "ldm_model_param_ndim": (C.c_int, [_P, C.c_int]),
    "ldm_model_param_shape": (C.POINTER(C.c_int64), [_P, C.c_int]),
    "ldm_model_load_param": (C.c_int, [_P, C.c_char_p, _P, C.c_size_t]),
    "ldm_model_param_numel_total": (C.c_int64, [_P]),
    "ldm_unet_workspace_bytes": (C.c_size_t, [_P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ldm_unet_forward": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int,
                                   _P, C.c_size_t, _P]),
    "ldm_model_param_offset": (C.c_int64, [_P, C.c_int]),
    "ldm_model_load_params_device": (C.c_int, [_P, C.POINTER(_P), C.c_int, _P]),
    "ldm_model_load_params_flat": (C.c_int, [_P, _P, _P]),
    "ldm_unet_train_workspace_bytes": (C.c_size_t, [_P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ldm_unet_train_forward": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int,
                                         _P, C.c_size_t, _P]),
    "ldm_unet_train_backward": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "ldm_unet_train_backward_input": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "ldm_unet_train_input_workspace_bytes": (C.c_size_t, [_P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ldm_op_conv3d_dgrad_thin": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P,
                                           C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "ldm_op_conv3d_dgrad_thin_pack": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "ldm_op_conv3d_dgrad_thin_packed": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "ldm_vae_train_workspace_bytes": (C.c_size_t, [_P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ldm_vae_train_forward": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "ldm_vae_train_backward": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "ldm_grad_sq_norm": (C.c_int, [_P, C.c_int64, _P, _P]),
    "ldm_op_mse_loss": (C.c_int, [_P, _P, C.c_int64, _P, _P, _P]),
    "ldm_adam_step": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, _P,
                                C.c_float, _P]),
    "ldm_model_adam_step": (C.c_int, [_P, _P, _P, _P, _P, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, _P,
                                      C.c_float, _P]),
    "ldm_adam_step_ema": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int,
                                    C.c_float, C.c_int, _P, C.c_float, _P]),
    "ldm_model_adam_step_ema": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int,
                                          C.c_float, C.c_int, _P, C.c_float, _P]),
    "ldm_model_set_graph_mode": (C.c_int, [_P, C.c_int]),
    "ldm_model_set_precision": (C.c_int, [_P, C.c_int]),
    "ldm_model_get_precision": (C.c_int, [_P]),
    "ldm_model_tap_count": (C.c_int, [_P, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ldm_model_tap_elems": (C.c_int64, [_P, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ldm_model_tap_info": (C.c_int, [_P, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int,
                                     C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    "ldm_model_taps_workspace_bytes": (C.c_size_t, [_P, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ldm_unet_forward_taps": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P,
                                        _P, C.c_size_t, _P]),
    "ldm_vae_encode_taps": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_size_t, _P]),
    "ldm_vae_decode_taps": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_size_t, _P]),
    "ldm_vae_encode_workspace_bytes": (C.c_size_t, [_P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ldm_vae_decode_workspace_bytes": (C.c_size_t, [_P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ldm_vae_encode": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "ldm_vae_decode": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "ldm_add_noise": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int64, _P]),
    "ldm_scheduler_step": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.c_int, C.c_int, _F, C.c_int, _P]),
    "ldm_add_noise_target": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int64, C.c_int, _P]),
    "ldm_scale": (C.c_int, [_P, _P, C.c_int64, C.c_float, _P]),
    "ldm_latent_batch": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int64, C.POINTER(C.c_int), C.c_int, _P, _P, C.c_float, C.c_int,
                                   _P, _P, _P, C.c_uint64, C.c_uint32, _P, _P, _P, _P, _P]),
    "ldm_rflow_step": (C.c_int, [_P, _P, _P, _P, C.c_int64, _F, _P]),
    "ldm_rflow_noise_target": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int64, _P]),
    "ldm_latent_batch_rflow": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int64, C.POINTER(C.c_int), C.c_int, _P, _P, C.c_float,
                                         _P, _P, _P, C.c_uint64, C.c_uint32, _P, _P, _P, _P, _P]),
    "ldm_rflow_timesteps": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_float, _P,
                                      C.c_uint64, C.c_uint32, _P, _P, _P, _P]),
    "ldm_op_weighted_mse_loss": (C.c_int, [_P, _P, C.c_int, C.c_int64, _P, _P, C.c_int, _P, _P, C.c_int, C.c_float, _P, _P, _P, _P]),
    "ldm_timestep_resample": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_int), C.c_int, C.c_uint64, C.c_uint32,
                                        _P, _P, _P, _P]),
    "ldm_sampler_create_rflow": (C.c_int, [_P, C.c_int, C.POINTER(_P)]),
    "ldm_sampler_create": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.POINTER(_P)]),
    "ldm_sampler_create_pndm": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(_P)]),
    "ldm_sampler_state_bytes": (C.c_size_t, [_P, C.c_int64]),
    "ldm_sampler_bind_state": (C.c_int, [_P, _P, C.c_size_t, C.c_int64]),
    "ldm_pndm_step": (C.c_int, [_P] * 9 + [C.c_int64, C.c_int, _F, _P]),
    "ldm_sampler_create_dpm": (C.c_int, [_P, C.c_int, C.c_int, C.c_uint64, C.POINTER(_P)]),
    "ldm_dpm_step": (C.c_int, [_P] * 7 + [C.c_int64, C.c_int, _F, _P]),
    "ldm_sampler_destroy": (None, [_P]),
    "ldm_sampler_reset": (C.c_int, [_P, _P, C.c_int, _P]),
    "ldm_sampler_step": (C.c_int, [_P, _P, _P, _P, C.c_int64, _P, C.c_int, _P]),
    "ldm_sampler_noise": (C.c_int, [_P, C.c_int, _P, C.c_int64, _P]),
    "ldm_sampler_seek": (C.c_int, [_P, C.c_int, _P, C.c_int, _P]),
    "ldm_sampler_start": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, C.c_int, C.c_int64, C.c_uint64, C.c_uint32, _P]),
    "ldm_sampler_start_noise": (C.c_int, [C.c_uint64, C.c_uint32, _P, C.c_int64, _P]),
    "ldm_sampler_create_repaint": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.POINTER(_P)]),
    "ldm_sampler_bind_known": (C.c_int, [_P, _P, C.c_int, _P, C.c_int64, C.c_int64]),
    "ldm_sampler_repaint_noise": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int64, _P]),
    "ldm_repaint_merge": (C.c_int, [_P, _P, C.c_int, _P, _P, _P, _P, C.c_int, C.c_int64, C.c_int64, _F, C.c_int, _P]),
    "ldm_unet_denoise_step": (C.c_int, [_P, _P, _P, C.c_int, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int,
                                        _P, C.c_size_t, _P]),
    "ldm_unet_denoise_step_measured": (C.c_int, [_P, _P, _P, _P, C.c_int, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int,
                                                 _P, C.c_size_t, _P]),
    "ldm_op_guidance_residual": (C.c_int, [_P, _P, _P, C.c_int, _P, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, _P, _P, _P,
                                           C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "ldm_op_guidance_update": (C.c_int, [_P, _P, _P, _P, C.c_float, C.c_int, C.c_int, C.c_int64, _P]),
    "ldm_vae_decode_grad_workspace_bytes": (C.c_size_t, [_P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ldm_vae_decode_grad_forward": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "ldm_vae_decode_grad_backward": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "ldm_unet_denoise_step_measured_image": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int,
                                                       _P, C.c_size_t, _P]),
    "ldm_image_residual_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ldm_op_guidance_x0": (C.c_int, [_P, _P, C.c_float, C.c_float, C.c_int, C.c_float, _P, C.c_int64, _P]),
    "ldm_op_image_residual": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, _P, _P, _P, C.c_size_t,
                                        C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "ldm_op_guidance_chain": (C.c_int, [_P, C.c_float, C.c_float, C.c_int, C.c_float, _P, _P, C.c_int64, _P]),
    "ldm_likelihood_create": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_float, C.POINTER(_P)]),
    "ldm_likelihood_destroy": (None, [_P]),
    "ldm_likelihood_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int64]),
    "ldm_likelihood_reset": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int64, _P, _P]),
    "ldm_likelihood_noise": (C.c_int, [_P, _P, C.c_int, C.c_int64, _P]),
    "ldm_likelihood_noisy": (C.c_int, [_P, _P, _F, _P, C.c_int, C.c_int64, _P]),
    "ldm_likelihood_term": (C.c_int, [_P, _P, _P, _F, C.c_int, C.c_int, C.c_float, _P, _P, _P, C.c_int, C.c_int64, _P, C.c_size_t, _P]),
    "ldm_unet_likelihood_step": (C.c_int, [_P, _P, _P, _P, C.c_int, _P, C.c_int, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int,
                                           _P, C.c_size_t, _P, C.c_size_t, _P]),
    "ldm_op_resize_nearest": (C.c_int, [_P, _P] + [C.c_int] * 8 + [_P]),
    "ldm_ensemble_update": (C.c_int, [_P, C.c_int, C.c_int64, C.c_int64, _P, _P, C.c_int, _P]),
    "ldm_ensemble_stats_scratch_bytes": (C.c_size_t, [C.c_int64]),
    "ldm_ensemble_finalize": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, _P, C.c_size_t, C.c_int64, _P]),
    "ldm_window_grid_create": (C.c_int, [_P, _P, _P, _P, _P, _P, C.POINTER(_P)]),
    "ldm_window_grid_destroy": (None, [_P]),
    "ldm_window_gather": (C.c_int, [_P, _P, _P, C.c_int, _P]),
    "ldm_window_blend": (C.c_int, [_P, _P, _P, C.c_int, _P]),
    "ldm_unet_denoise_step_windows": (C.c_int, [_P, _P, _P, _P, C.c_int, _P, C.c_int, _P, _P, _P, C.c_int, _P, C.c_size_t, _P]),
    "ldm_guidance_combine": (C.c_int, [_P, _P, C.c_float, _P, C.c_int64, _P]),
    "ldm_unet_guided_workspace_bytes": (C.c_size_t, [_P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ldm_unet_denoise_step_guided": (C.c_int, [_P, _P, _P, C.c_int, _P, C.c_int, C.c_float, C.c_float, _P, _P, C.c_int, C.c_int, C.c_int,
                                               C.c_int, _P, C.c_size_t, _P]),
    "ldm_unet_denoise_step_windows_guided": (C.c_int, [_P, _P, _P, _P, C.c_int, _P, C.c_int, C.c_float, C.c_float, _P, _P, _P, C.c_int,
                                                       _P, C.c_size_t, _P]),
    "ldm_cond_dropout": (C.c_int, [_P, C.c_int, C.c_int64, C.POINTER(C.c_int), C.c_float, C.c_float, C.POINTER(C.c_ubyte),
                                   C.c_uint64, C.c_uint32, C.POINTER(C.c_ubyte), _P]),
    "ldm_op_conv3d": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, _P, C.c_int, _P, C.c_int, _P, _P, _P, C.c_int, _P, _P, _P,
                                C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "ldm_op_weight_flip_transpose": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "ldm_op_conv3d_wgrad": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "ldm_op_group_norm_bwd_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "ldm_op_group_norm_bwd": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, _P, _P, C.c_int, C.c_float, C.c_int, _P, _P, _P, _P, _P, _P,
                                        C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "ldm_op_scale_intensity_percentiles_scratch_bytes": (C.c_size_t, [C.c_int]),
    "ldm_op_scale_intensity_percentiles": (C.c_int, [_P, _P, C.c_int, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, _P, C.c_size_t, _P]),
    "ldm_op_image_metrics_scratch_bytes": (C.c_size_t, [C.c_int] * 6),
    "ldm_op_image_metrics": (C.c_int, [_P, C.POINTER(C.c_int64), _P, C.POINTER(C.c_int64)] + [C.c_int] * 5 + [_F, C.c_int, C.c_float, C.c_float,
                                       C.c_float, _P, _P, _P, C.c_size_t, _P]),
    "ldm_op_im2col": (C.c_int, [_P, _P] + [C.c_int] * 10 + [_P]),
    "ldm_op_col2im": (C.c_int, [_P, _P] + [C.c_int] * 10 + [_P]),
    "ldm_op_leaky_relu": (C.c_int, [_P, _P, C.c_int64, C.c_float, _P]),
    "ldm_op_leaky_relu_bwd": (C.c_int, [_P, _P, _P, C.c_int64, C.c_float, _P]),
    "ldm_op_pack_ncdhw": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int64, _P]),
    "ldm_op_unpack_ndhwc": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int64, _P]),
    "ldm_op_conv3d_gn_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ldm_op_conv3d_gn": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, C.c_int, C.c_float, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "ldm_op_conv3d_fin_gn_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ldm_op_conv3d_fin_gn": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_int, _P, _P, _P, C.c_int, C.c_float, C.c_int, _P, _P,
                                       C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "ldm_op_group_norm_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "ldm_op_group_norm": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, C.c_int, C.c_float, C.c_int, _P, C.c_int, C.c_int,
                                    _P, C.c_size_t, _P]),
    "ldm_op_attention": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "ldm_op_attention_hd": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "ldm_op_attention_bwd_hd": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "ldm_op_attention_train": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "ldm_op_attention_bwd": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "ldm_profile_start": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "ldm_profile_detail": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int]),
    "ldm_profile_stop": (C.c_int, [C.POINTER(C.c_double)]),
    "ldm_set_plan_trace": (C.c_int, [C.c_char_p]),
    "ldm_op_pack_ncdhw_f32": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int64, _P]),
    "ldm_op_unpack_ndhwc_f32": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int64, _P]),
    "ldm_op_im2col_f32": (C.c_int, [_P, _P] + [C.c_int] * 10 + [_P]),
    "ldm_op_col2im_f32": (C.c_int, [_P, _P] + [C.c_int] * 10 + [_P]),
    "ldm_op_leaky_relu_f32": (C.c_int, [_P, _P, C.c_int64, C.c_float, _P]),
    "ldm_op_leaky_relu_bwd_f32": (C.c_int, [_P, _P, _P, C.c_int64, C.c_float, _P]),
    "ldm_op_gemm_f32": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, _P]),
    "ldm_debug_conv_block_slots": (C.c_int, [C.c_int]),
    "ldm_op_conv3d_block_stats_rows": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "ldm_op_conv3d_block": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "ldm_op_conv3d_block128": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "ldm_op_linear_bf16": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, _P, _P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                     _P, C.c_int, C.c_int, _P, _P, C.c_int, C.c_float, C.c_int, _P, _P]),
    "ldm_op_linear_f32x3": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, _P, _P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, _P]),
    "ldm_op_gemm_wgrad_f32": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, C.c_int, C.c_int64, C.c_int, _P]),
    "ldm_op_group_norm_f32_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "ldm_op_group_norm_f32": (C.c_int, [_P, C.c_int, _P, _P, C.c_int, C.c_float, C.c_int, _P, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "ldm_op_group_norm_bwd_f32": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int, C.c_float, C.c_int, _P, _P, _P, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "ldm_op_conv3d_f32_stats_blocks": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "ldm_op_conv3d_f32": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, _P, C.c_int, _P, _P, C.c_int, _P, _P] + [C.c_int] * 13
                          + [_P, C.c_size_t, _P]),
    "ldm_op_weight_flip_transpose_f32_ws_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "ldm_op_weight_flip_transpose_f32": (C.c_int, [_P, _P] + [C.c_int] * 6 + [_P, C.c_size_t, _P]),
    "ldm_op_conv3d_wgrad_f32": (C.c_int, [_P, C.c_int, _P, C.c_int, _P] + [C.c_int] * 13 + [_P]),
    "ldm_op_attention_f32": (C.c_int, [_P, _P, _P] + [C.c_int] * 5 + [_P]),
    "ldm_op_attention_bwd_f32": (C.c_int, [_P] * 6 + [C.c_int] * 4 + [_P]),
    "ldm_op_group_norm_bwd2_f32": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, _P, _P, C.c_int, C.c_float, C.c_int, _P, _P, _P, _P, _P, _P,
                                             C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "ldm_op_upsample_bwd_f32": (C.c_int, [_P, _P] + [C.c_int] * 5 + [_P]),
    "ldm_op_group_norm_bwd_saved_scratch_bytes": (C.c_size_t, [C.c_int] * 4),
    "ldm_op_group_norm_bwd_fold_chunks": (C.c_int, [C.c_int] * 4),
    "ldm_op_group_norm_bwd_saved": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, _P, _P, _P, C.c_int, C.c_int] + [_P] * 7
                                    + [C.c_int] * 3 + [_P, C.c_size_t, _P]),
    "ldm_op_colsum_finalize_ws_bytes": (C.c_size_t, [_P, C.c_int]),
    "ldm_op_colsum_finalize": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "ldm_op_grad_export_ws_bytes": (C.c_size_t, [_P, C.c_int]),
    "ldm_op_grad_export": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "ldm_op_weight_flip_transpose_batched_ws_bytes": (C.c_size_t, [_P, C.c_int]),
    "ldm_op_weight_flip_transpose_batched": (C.c_int, [_P, _P, _P, C.c_int, _P, C.c_size_t, _P]),
    "ldm_op_linear_bwd_nz": (C.c_int, [C.c_int]),
    "ldm_op_linear_bwd": (C.c_int, [_P] * 6 + [C.c_int] * 6 + [_P, C.c_size_t, _P]),
    "ldm_op_upsample_bwd": (C.c_int, [_P, _P] + [C.c_int] * 5 + [_P]),
    "ldm_op_add_bf16": (C.c_int, [_P, _P, _P, C.c_int64, _P]),
    "ldm_op_vae_heads": (C.c_int, [_P] * 5 + [C.c_int] * 3 + [_P]),
    "ldm_op_vae_heads_bwd": (C.c_int, [_P, C.c_int] + [_P] * 5 + [C.c_int] * 5 + [_P]),
    "ldm_debug_kstamps": (C.c_int, [C.POINTER(C.c_uint64), C.c_int, C.c_int]),
    "ldm_model_plan_conv_cfgs": (C.c_int, [_P, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]),
    "ldm_comm_unique_id": (C.c_int, [C.c_char_p]),
    "ldm_comm_init": (C.c_int, [C.c_int, C.c_int, C.c_char_p, C.POINTER(_P)]),
    "ldm_comm_init_custom": (C.c_int, [C.c_int, C.c_int, _P, _P, C.POINTER(_P)]),
    "ldm_comm_allreduce": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, _P]),
    "ldm_comm_broadcast": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, _P]),
    "ldm_comm_barrier": (C.c_int, [_P, _P]),
    "ldm_comm_destroy": (None, [_P]),
    "ldm_comm_rank": (C.c_int, [_P]),
    "ldm_comm_world": (C.c_int, [_P]),
    "ldm_model_set_grad_sync": (C.c_int, [_P, _P]),
    "ldm_model_set_grad_wire": (C.c_int, [_P, C.c_int]),
    "ldm_model_grad_sync_pending": (C.c_int, [_P]),
    "ldm_model_set_grad_accum": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "ldm_op_grad_accumulate": (C.c_int, [_P, _P, C.c_int64, C.c_float, C.c_int, _P]),
    "ldm_comm_stats": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "ldm_comm_is_rccl": (C.c_int, [_P]),
    "ldm_comm_rccl_version": (C.c_int, []),
    "ldm_model_plan_launches": (C.c_int, [_P, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ldm_model_grad_sync_trace": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int]),
    "ldm_model_grad_schedule": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64),
                                          C.POINTER(C.c_int64), C.POINTER(C.c_int), C.c_int]),
    # plan-only operators (tests/test_gpu_plan_only_ops.py)
    "ldm_op_conv3d_thin": (C.c_int, [_P, C.c_int, _P, _P, _P] + [C.c_int] * 6 + [_P]),
    "ldm_op_conv3d_thin_f32_ws_bytes": (C.c_size_t, [C.c_int] * 6),
    "ldm_op_conv3d_thin_f32": (C.c_int, [_P, C.c_int, _P, _P, _P] + [C.c_int] * 6 + [_P, C.c_size_t, _P]),
    "ldm_op_timestep_embedding": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "ldm_op_gemv": (C.c_int, [_P, C.c_int, _P, _P, _P] + [C.c_int] * 6 + [_P]),
    "ldm_op_pack2": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_float, _P]),
    "ldm_op_pack_im2col": (C.c_int, [_P, C.c_int, _P, C.c_int, _P] + [C.c_int] * 6 + [C.c_float, _P]),
    "ldm_op_phase_weights": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "ldm_op_im2col_weights": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "ldm_op_x3_weights": (C.c_int, [_P, _P, C.c_int64, C.c_int, _P]),
    "ldm_op_x3_phase_weights": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "ldm_op_split_f32": (C.c_int, [_P, _P] + [C.c_int] * 6 + [_P]),
}
# ldm_allreduce_fn (include/ldm3d.h): int fn(void* user, void* buf, int64_t count, int dtype, int op, void* stream)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, _P, _P, C.c_int64, C.c_int, C.c_int, _P)

_lib = None
_lock = threading.Lock()


class LdmError(RuntimeError):
    """Raised for every non-zero ldm_status (message from ldm_last_error)."""


def lib() -> C.CDLL:
    """Load libldm3d.so once.  Raises (never degrades) if it has not been built."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise LdmError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; "
                                   f"g.build()'` or `make -C {os.path.join(_HERE, 'csrc')}` (no CPU fallback exists)")
                h = C.CDLL(LIB_PATH)
                for name, (res, args) in SIGNATURES.items():
                    fn = getattr(h, name)            # AttributeError = ABI mismatch: fail loudly
                    fn.restype = res
                    fn.argtypes = args
                _lib = h
    return _lib


def check(status: int) -> None:
    if status != 0:
        msg = lib().ldm_last_error()
        raise LdmError(f"libldm3d status {status}: {msg.decode() if msg else '?'}")


def ptr(t) -> int | None:
    """Device/host address of a torch tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def current_stream() -> int:
    import torch
    return torch.cuda.current_stream().cuda_stream
