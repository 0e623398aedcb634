"""ctypes binding of libpanic3d_hip.so — the C ABI of include/panic3d_hip.h.  No torch types cross this boundary.

The library is the product: if it is missing this module raises (there is NO CPU / PyTorch fallback path).
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.environ.get("P3D_LIB") or os.path.join(HERE, "libpanic3d_hip.so")  # P3D_LIB: development override

P3D_FLAG_CROP, P3D_FLAG_CULL, P3D_FLAG_BINARIZE, P3D_FLAG_FORCE_SIGMOID, P3D_FLAG_WHITE_BACK, P3D_FLAG_NO_EARLY_OUT, P3D_FLAG_SHARED_PLANES, P3D_FLAG_SKIP_CROPPED, P3D_FLAG_NO_PAIR, P3D_FLAG_FAST_COLOR, P3D_FLAG_PER_VIEW_CLAMP, P3D_FLAG_NO_STAGING, P3D_FLAG_FORCE_STAGING = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 8192
P3D_FLAG_DISPARITY = 4096
P3D_FLAG_PAIR16 = 16384
P3D_FLAG_QUAD8 = 32768
P3D_FLAG_WEIGHTS_ONLY = 65536
P3D_FLAG_GENERIC_TAPS = 131072  # test switch: k_render keeps the generic gather set-up (include/panic3d_hip.h)
P3D_FLAG_SERIAL_MERGE = 262144  # test switch: k_render's merge pre-pass by the serial walk (include/panic3d_hip.h)
P3D_MAX_S = 192
P3D_ABI_VERSION = 9  # include/panic3d_hip.h; lib() refuses a library built for another version


class Opts(C.Structure):
    """p3d_opts"""
    _fields_ = [("coord_scale", C.c_float), ("ray_start", C.c_float), ("ray_end", C.c_float),
                ("depth_delta", C.c_float), ("crop_limit", C.c_float), ("cull_thresh", C.c_float),
                ("Sc", C.c_int32), ("Sf", C.c_int32), ("plane_mode", C.c_int32), ("flags", C.c_int32)]


class Dumps(C.Structure):
    """p3d_dumps"""
    _fields_ = [("depths_coarse", C.c_void_p), ("sigma_coarse", C.c_void_p), ("weights_coarse", C.c_void_p),
                ("depths_fine", C.c_void_p), ("inds", C.c_void_p), ("depths_sorted", C.c_void_p),
                ("sigma_sorted", C.c_void_p), ("depth_unclamped", C.c_void_p), ("tminmax", C.c_void_p)]


class PasteArgs(C.Structure):
    """p3d_paste_args"""
    _fields_ = [(n, C.c_void_p) for n in ("weights", "xyz", "occ", "rays_o", "rays_d", "front", "image", "out_image", "out_paste",
                                          "out_mask", "out_mask_weights", "out_mask_edges", "out_mask_occ", "out_mask_dxyz")] + \
               [(n, C.c_int32) for n in ("N", "r", "S", "front_shared", "normalize_images")] + \
               [(n, C.c_float) for n in ("thresh_weight", "thresh_edges", "thresh_occ", "thresh_dxyz", "box_warp")]


class PasteGradArgs(C.Structure):
    """p3d_paste_grad_args (include/p3d_paste_grad.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("g_out", "g_paste", "mask", "xyz", "front", "g_image", "g_xyz", "g_front", "workspace")] + \
               [("workspace_bytes", C.c_size_t)] + \
               [(n, C.c_int32) for n in ("N", "r", "S", "front_shared", "normalize_images", "grad_sample")] + [("box_warp", C.c_float)]


class ConvArgs(C.Structure):
    """p3d_conv_args"""
    _fields_ = [(n, C.c_void_p) for n in ("x", "w", "w_f16", "styles", "demod_coefs", "noise", "bias", "fir", "y", "workspace",
                                          "saturated", "x_img", "y_img", "y_img_styles", "rgb_w", "rgb_styles", "rgb_partial")] + \
               [("workspace_bytes", C.c_size_t)] + \
               [(n, C.c_int32) for n in ("N", "I", "H", "W", "O", "ks", "up", "demodulate", "noise_per_sample", "act", "mma")] + \
               [(n, C.c_float) for n in ("alpha", "gain", "clamp")] + [("rgb_channels", C.c_int32), ("w_f16_layout", C.c_int32)]


class OptimTensor(C.Structure):
    """p3d_optim_tensor (include/p3d_optim.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("p", "m", "v", "ema")] + [("numel", C.c_int64), ("aligned16", C.c_int32), ("reserved", C.c_int32)]


class OptimStep(C.Structure):
    """p3d_optim_step (include/p3d_optim.h)"""
    _fields_ = [("grad", C.c_void_p), ("step_size", C.c_float), ("bc2_sqrt", C.c_float), ("ema_w", C.c_float), ("grad_aligned16", C.c_int32)]


class OptimChunk(C.Structure):
    """p3d_optim_chunk (include/p3d_optim.h)"""
    _fields_ = [("offset", C.c_int64), ("tensor", C.c_int32), ("count", C.c_int32)]


class OptimArgs(C.Structure):
    """p3d_optim_args (include/p3d_optim.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("tensors", "steps", "chunks")] + [("n_chunks", C.c_int64)] + \
               [(n, C.c_int32) for n in ("n_tensors", "mode", "sanitize")] + \
               [(n, C.c_float) for n in ("grad_scale", "nan_v", "posinf_v", "neginf_v", "eps")] + [("beta1", C.c_double), ("beta2", C.c_double)]


class EncLayer(C.Structure):
    """p3d_enc_layer (include/p3d_encoder.h)"""
    _fields_ = [(n, C.c_int32) for n in ("kind", "N", "Ci", "H", "W", "Co", "Ho", "Wo", "k", "stride", "in_", "out", "res", "flags", "plan",
                                         "reserved")] + [("w_off", C.c_int64), ("b_off", C.c_int64)]


class RmlineDog(C.Structure):
    """p3d_rmline_dog (include/p3d_rmline.h)"""
    _fields_ = [(n, C.c_double) for n in ("t", "sigma", "k", "epsilon", "kernel_factor")] + [("d", C.c_int32), ("reserved", C.c_int32)]


class RmlineLayer(C.Structure):
    """p3d_rmline_layer (include/p3d_rmline.h)"""
    _fields_ = [(n, C.c_int32) for n in ("Ci", "Co", "act", "plan")] + [("slope", C.c_float), ("reserved", C.c_int32), ("w_off", C.c_int64),
                                                                          ("b_off", C.c_int64)]


class ClipStep(C.Structure):
    """p3d_clip_step (include/p3d_clip.h)"""
    _fields_ = [(n, C.c_int32) for n in ("kind", "M", "K", "Nout", "N", "T", "heads", "S", "patch", "H", "W", "ld", "in_", "out", "res", "flags",
                                         "plan")] + [("eps", C.c_float), ("reserved", C.c_int32 * 2)] + \
               [(n, C.c_int64) for n in ("w_off", "b_off", "w2_off", "b2_off")]


P3D_CONV_MMA_F32, P3D_CONV_MMA_F16, P3D_CONV_MMA_F16X2 = 0, 1, 2
P3D_WLAYOUT_OIK, P3D_WLAYOUT_PLAIN, P3D_WLAYOUT_UP = 0, 1, 2

# symbol -> (restype, argtypes); every function include/panic3d_hip.h declares
_P, _I, _L, _F, _Z = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t
SIGNATURES = {
    "p3d_planes_to_nhwc_f32": (_I, [_P, _I, _I, _I, _I, _P, _P]),
    "p3d_decode_features_f32": (_I, [_P, _I, _L, _P, _P, _P, _P, _I, _P, _P, _P]),
    "p3d_struct_layout": (_I, [_I, C.POINTER(C.c_size_t), _I]),
    "p3d_triplane_decode_f32": (_I, [_P, _I, _I, _I, _P, _L, _P, _P, _P, _P, C.POINTER(Opts), _P, _P, _P]),
    "p3d_grid_density_f32": (_I, [_P, _I, _I, _I, _L, _L, _F, _F, _F, _F, _P, _P, _P, _P, C.POINTER(Opts), _P, _P, _F, _P]),
    "p3d_render_workspace_bytes": (_Z, [_I, _L, _I, _I]),
    "p3d_render_f32": (_I, [_P, _I, _I, _I, _P, _P, _L, _I, _P, _P, _P, _P, _P, _P, C.POINTER(Opts), _P, _P, _P, _P, _P,
                            _Z, C.POINTER(Dumps), _P]),
    "p3d_render_limits_f32": (_I, [_P, _I, _I, _I, _P, _P, _L, _I, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(Opts), _P, _P, _P, _P, _P,
                                   _Z, C.POINTER(Dumps), _P]),
    "p3d_render_rng_f32": (_I, [_P, _I, _I, _I, _P, _P, _L, _I, C.c_uint64, _P, _P, _P, _P, _P, _P, C.POINTER(Opts), _P, _P, _P, _P, _P,
                                _Z, C.POINTER(Dumps), _P]),
    "p3d_render_plan_info": (_I, [_I, _L, _I, C.POINTER(Opts), _I, _I, C.POINTER(C.c_int64), _I]),
    "p3d_render_taps_info": (_I, [_I, _I, _I, _L, _I, C.POINTER(Opts), _I, _I]),
    "p3d_sample_stratified_f32": (_I, [_F, _F, _F, _I, _P, _L, _P, _P]),
    "p3d_composite_workspace_bytes": (_Z, [_L, _I, _I]),
    "p3d_depth_minmax_f32": (_I, [_P, _L, _P, _P, _Z, _P]),
    "p3d_composite_f32": (_I, [_P, _P, _P, _L, _I, _I, _I, _P, _P, _P, _P, _P]),
    "p3d_importance_f32": (_I, [_P, _P, _L, _I, _I, _P, _P, _P, _P]),
    "p3d_unify_perm_f32": (_I, [_P, _P, _L, _I, _I, _P, _P]),
    "p3d_modconv2d_workspace_bytes": (_Z, [_I, _I, _I, _I, _I, _I]),
    "p3d_modconv2d_f32": (_I, [_P, _I, _I, _I, _I, _P, _I, _I, _P, _I, _P, _P, _I, _P, _I, _I, _F, _F, _F, _P, _P, _P, _Z, _P]),
    "p3d_demod_coefs_f32": (_I, [_P, _P, _P, _I, _I, _I, _P, _P]),
    "p3d_conv_weights_to_f16": (_I, [_P, _I, _I, _I, _P, _P]),
    "p3d_modconv2d_f16mma_f32": (_I, [_P, _I, _I, _I, _I, _P, _P, _I, _I, _P, _I, _P, _P, _I, _P, _I, _I, _F, _F, _F, _P, _P, _P, _Z, _P]),
    "p3d_conv_weights_to_f16x2": (_I, [_P, _I, _I, _I, _P, _P]),
    "p3d_modconv2d_f16x2mma_f32": (_I, [_P, _I, _I, _I, _I, _P, _P, _I, _I, _P, _I, _P, _P, _I, _P, _I, _I, _F, _F, _F, _P, _P, _P, _Z, _P, _P]),
    "p3d_modconv2d_ex_f32": (_I, [C.POINTER(ConvArgs), _P]),
    "p3d_conv_takes_image": (_I, [_I, _I, _I, _I]),
    "p3d_act_image_bytes": (_Z, [_I, _I, _I, _I]),
    "p3d_act_to_image_f32": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "p3d_act_to_image_add_f32": (_I, [_P, _P, _I, _I, _I, _I, _P, _I, _I, _I, _P, _P, _P]),
    "p3d_conv_fuses_torgb": (_I, [_I, _I, _I, _I, _I, _I]),
    "p3d_conv_weight_layout": (_I, [_I, _I, _I, _I]),
    "p3d_conv_weights_to_f16x2_layout": (_I, [_P, _I, _I, _I, _I, _P, _P]),
    "p3d_torgb_partial_bytes": (_Z, [_I, _I, _I, _I, _I]),
    "p3d_torgb_combine_f32": (_I, [_P, _I, _I, _I, _I, _I, _P, _F, _P, _P, _P, _P]),
    "p3d_torgb_weights_f32": (_I, [_P, _I, _I, _P, _P]),
    "p3d_torgb_f32": (_I, [_P, _I, _I, _I, _I, _P, _I, _P, _P, _F, _P, _P, _P, _P]),
    "p3d_upfirdn2d_f32": (_I, [_P, _L, _I, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "p3d_upsample2d_add_f32": (_I, [_P, _L, _I, _I, _P, _P, _P, _P]),
    "p3d_bias_act_f32": (_I, [_P, _P, _L, _I, _L, _I, _F, _F, _F, _P, _P]),
    "p3d_sigma2density_f32": (_I, [_P, _P, _L, _F, _P, _P]),
    "p3d_mc_workspace_bytes": (_Z, [_I]),
    "p3d_mc_count_f32": (_I, [_P, _I, _I, _F, _P, _Z, _P, _P]),
    "p3d_mc_emit_f32": (_I, [_P, _I, _I, _F, _P, _Z, _L, _L, _P, _P, _P, _P, _P]),
    "p3d_paste_front_f32": (_I, [C.POINTER(PasteArgs), _P]),
    "p3d_build_info": (C.c_char_p, []),
    "p3d_abi_version": (_I, []),
}

# symbol -> (restype, argtypes); every function include/p3d_render_grad.h declares (the backward passes).  A table of its own:
# SIGNATURES mirrors include/panic3d_hip.h exactly.
GRAD_SIGNATURES = {
    "p3d_render_backward_workspace_bytes": (_Z, [_I, _L, _I, _I]),
    "p3d_render_backward_f32": (_I, [_P, _I, _I, _I, _P, _P, _L, _P, _P, _P, _P, _P, C.POINTER(Opts), _P, _P, _P, _P, _P, _P, _P,
                                     _P, _P, _P, _Z, _P]),
    "p3d_triplane_decode_backward_workspace_bytes": (_Z, [_I, _L]),
    "p3d_triplane_decode_backward_f32": (_I, [_P, _I, _I, _I, _P, _L, _P, _P, _P, _P, C.POINTER(Opts), _P, _P, _P, _P, _P, _P, _P,
                                              _P, _Z, _P]),
}
# symbol -> (restype, argtypes); every function include/p3d_synthesis_grad.h declares (the synthesis layers' backward).  A third table:
# the two above mirror their headers exactly.
SYN_GRAD_SIGNATURES = {
    "p3d_bias_act_backward_f32": (_I, [_P, _P, _I, _I, _L, _I, _F, _F, _F, _P, _P, _P, _P, _P]),
    "p3d_conv_dgrad_f32": (_I, [_P, _I, _I, _I, _I, _P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "p3d_mod_backward_f32": (_I, [_P, _P, _I, _I, _L, _P, _P, _P]),
    "p3d_conv_wgrad_workspace_bytes": (_Z, [_I, _I, _I, _I, _I, _I]),
    "p3d_conv_wgrad_f32": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _Z, _P]),
    "p3d_torgb_combine_backward_f32": (_I, [_P, _I, _I, _I, _I, _I, _P, _F, _P, _P, _P, _P, _P, _P]),
}
# symbol -> (restype, argtypes); every function include/p3d_paste_grad.h declares (the front-view paste's backward)
PASTE_GRAD_SIGNATURES = {
    "p3d_paste_front_backward_workspace_bytes": (_Z, [_I, _I]),
    "p3d_paste_front_backward_f32": (_I, [C.POINTER(PasteGradArgs), _P]),
}
# symbol -> (restype, argtypes); every function include/p3d_discriminator.h declares (the dual discriminator's layers)
DISC_SIGNATURES = {
    "p3d_conv2d_act_f32": (_I, [_P, _I, _I, _I, _I, _P, _I, _I, _I, _I, _I, _I, _P, _I, _F, _F, _F, _P, _P, _P, _P]),
    "p3d_mbstd_f32": (_I, [_P, _I, _I, _L, _I, _I, _I, _P, _P, _P]),
    "p3d_mbstd_backward_f32": (_I, [_P, _P, _P, _L, _I, _I, _L, _I, _I, _P, _P]),
}
# symbol -> (restype, argtypes); every function include/p3d_loss.h declares (the training loss's blur, L1 and view terms)
LOSS_SIGNATURES = {
    "p3d_blur_f32": (_I, [_P, _L, _I, _I, _P, _I, _P, _P]),
    "p3d_l1_workspace_bytes": (_Z, [_L]),
    "p3d_l1_f32": (_I, [_P, _P, _L, _F, _P, _P, _P, _Z, _P]),
    "p3d_view_terms_workspace_bytes": (_Z, [_I, _I]),
    "p3d_view_terms_f32": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _F, _P, _P, _P, _P, _Z, _P]),
}
# symbol -> (restype, argtypes); every function include/p3d_optim.h declares (the optimiser step: multi-tensor Adam and the G_ema update)
OPTIM_SIGNATURES = {
    "p3d_optim_plan": (_L, [_P, _I, _P, _L]),
    "p3d_optim_aligned16": (_I, [_P, _I]),
    "p3d_optim_step_f32": (_I, [C.POINTER(OptimArgs), _P]),
    "p3d_optim_struct_layout": (_I, [_I, C.POINTER(C.c_size_t), _I]),
}
# symbol -> (restype, argtypes); every function include/p3d_lpips.h declares (LPIPS: the AlexNet trunk's layers, the pool and the head)
LPIPS_SIGNATURES = {
    "p3d_lpips_conv_relu_f32": (_I, [_P, _I, _I, _I, _I, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "p3d_lpips_conv_relu_backward_f32": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    "p3d_lpips_pool_f32": (_I, [_P, _L, _I, _I, _P, _P]),
    "p3d_lpips_pool_backward_f32": (_I, [_P, _P, _L, _I, _I, _P, _P]),
    "p3d_lpips_head_workspace_bytes": (_Z, [_I, _L]),
    "p3d_lpips_head_f32": (_I, [_P, _P, _P, _I, _I, _L, _P, _P, _I, _P, _Z, _P]),
    "p3d_lpips_head_backward_f32": (_I, [_P, _P, _P, _P, _I, _I, _L, _P, _I, _P, _P]),
}
# symbol -> (restype, argtypes); every function include/p3d_encoder.h declares (the conditioning encoder: ResNet layers, front end, the table walk)
ENCODER_SIGNATURES = {
    "p3d_enc_conv_plan": (_I, [_I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(C.c_int)]),
    "p3d_enc_conv_workspace_bytes": (_Z, [_I, _I, _I, _I, _I, _I, _I, _I]),
    "p3d_enc_conv_f32": (_I, [_P, _I, _I, _I, _I, _P, _I, _I, _I, _P, _P, _I, _P, _I, _P, _Z, _P]),
    "p3d_enc_maxpool_f32": (_I, [_P, _L, _I, _I, _P, _P]),
    "p3d_enc_prepare_f32": (_I, [_P, _I, _I, _I, _I, _P, _P, _I, _I, _P, _P]),
    "p3d_enc_struct_layout": (_I, [C.POINTER(C.c_size_t), _I]),
    "p3d_encoder_forward_f32": (_I, [C.POINTER(EncLayer), _I, _P, _L, _P, _L, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _I, _P, _Z, _P]),
    "p3d_encoder_workspace_bytes": (_Z, [C.POINTER(EncLayer), _I]),
}
# symbol -> (restype, argtypes); every function include/p3d_metrics.h declares (the geometry metrics: point-to-mesh distance)
METRICS_SIGNATURES = {
    "p3d_point_mesh_plan": (_I, [_L, _L, _I, C.POINTER(C.c_int64), _I]),
    "p3d_point_mesh_workspace_bytes": (_Z, [_L, _L]),
    "p3d_point_mesh_dist2_f32": (_I, [_P, _L, _P, _L, _P, _L, _I, _F, _P, _P, _P, _P, _Z, _P]),
}
# symbol -> (restype, argtypes); every function include/p3d_rmline.h declares (the illustration-to-render module: line mask, generator layers, the walk)
RMLINE_SIGNATURES = {
    "p3d_rmline_dog_taps": (_I, [C.POINTER(RmlineDog), C.POINTER(C.c_int)]),
    "p3d_rmline_mask_f32": (_I, [_P, _I, _I, _I, _I, _P, C.POINTER(RmlineDog), _P, _P, _P, _P]),
    "p3d_rmline_conv_plan": (_I, [_I, _I, _I, C.POINTER(C.c_int)]),
    "p3d_rmline_conv_f32": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _I, _I, _F, _I, _I, _P, _P]),
    "p3d_rmline_struct_layout": (_I, [_I, C.POINTER(C.c_size_t), _I]),
    "p3d_rmline_forward_f32": (_I, [_P, _I, _I, _I, _I, _P, C.POINTER(RmlineDog), C.POINTER(RmlineLayer), _I, _P, _L, _I, _I, _P, _P, _P, _P, _L, _P,
                                    C.POINTER(C.c_int), _P]),
}
# symbol -> (restype, argtypes); every function include/p3d_rmline_grad.h declares (the module's training operators)
RMLINE_GRAD_SIGNATURES = {
    "p3d_rmline_bn_stats_f32": (_I, [_P, _L, _I, _F, _P, _P, _P, _P, _P, _P, _L, _P]),
    "p3d_rmline_bn_fold_f32": (_I, [_P, _P, _P, _P, _P, _P, _F, _I, _I, _P, _P, _P]),
    "p3d_rmline_conv_dgrad_f32": (_I, [_P, _I, _I, _I, _I, _P, _I, _P, _P, _P, _F, _I, _P, _P]),
    "p3d_rmline_wgrad_plan": (_I, [_I, _I, _I, _I, C.POINTER(C.c_int64)]),
    "p3d_rmline_conv_wgrad_f32": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _I, _I, _I, _P, _P, _P, _L, _P]),
    "p3d_rmline_bn_coef_f32": (_I, [_P, _P, _P, _P, _P, _P, _P, _F, _L, _I, _I, _P, _P, _P, _P, _P, _P]),
    "p3d_rmline_head_f32": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "p3d_rmline_head_grad_f32": (_I, [_P, _P, _P, _P, _P, _P, C.POINTER(C.c_int64), _I, _I, _I, _I, _P, _P]),
}
P3D_RMLINE_SUM_PER_TAP = 32  # include/p3d_rmline.h
P3D_RMLINE_BN_MAX_GROUPS, P3D_RMLINE_BN_ROWS, P3D_RMLINE_WG_MAX_SLICES, P3D_RMLINE_OUT_OIHW = 256, 256, 512, 16    # include/p3d_rmline_grad.h
# symbol -> (restype, argtypes); every function include/p3d_clip.h declares (CLIP's image tower, its front end, the cosine, PSNR's reductions)
CLIP_SIGNATURES = {
    "p3d_clip_resize_plan": (_I, [_I, _I, _I, C.POINTER(C.c_int)]),
    "p3d_clip_resize_table": (_I, [_I, _I, _I, _I, _I, C.POINTER(C.c_int32)]),
    "p3d_clip_prepare_workspace_bytes": (_Z, [_I, _I, _I, _I]),
    "p3d_clip_prepare_f32": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _Z, _P]),
    "p3d_clip_gemm_plan": (_I, [_I, _I, _I, _I, C.POINTER(C.c_int)]),
    "p3d_clip_gemm_workspace_bytes": (_Z, [_I, _I, _I, _I]),
    "p3d_clip_gemm_f32": (_I, [_P, _I, _I, _P, _I, _P, _P, _I, _I, _I, _I, _P, _I, _P, _Z, _P]),
    "p3d_clip_layernorm_f32": (_I, [_P, _I, _I, _L, _P, _P, _F, _P, _P]),
    "p3d_clip_embed_f32": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _F, _P, _P]),
    "p3d_clip_attention_plan": (_I, [_I, _I, _I, C.POINTER(C.c_int)]),
    "p3d_clip_attention_f32": (_I, [_P, _I, _I, _I, _I, _P, _P]),
    "p3d_clip_cosine_f32": (_I, [_P, _P, _I, _I, _P, _P]),
    "p3d_clip_struct_layout": (_I, [C.POINTER(C.c_size_t), _I]),
    "p3d_clip_forward_f32": (_I, [C.POINTER(ClipStep), _I, _P, _L, _P, _L, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _I, _P, _Z, _P]),
    "p3d_clip_workspace_bytes": (_Z, [C.POINTER(ClipStep), _I]),
    "p3d_psnr_workspace_bytes": (_Z, [_L]),
    "p3d_psnr_f32": (_I, [_P, _P, _L, _P, _P, _Z, _P]),
}
# symbol -> (restype, argtypes); every function include/p3d_augment.h declares (the augmentation pipe's operator and its adjoint)
AUGMENT_SIGNATURES = {
    "p3d_augment_filter": (_I, [C.POINTER(C.c_float), C.POINTER(C.c_double)]),
    "p3d_augment_geometry": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "p3d_augment_plan": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(C.c_int), _I]),
    "p3d_augment_workspace_bytes": (_Z, [_I, _I, _I, _I, _I, _I, _I, _I]),
    "p3d_augment_apply_f32": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _Z, _P]),
    "p3d_augment_apply_adjoint_f32": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _Z, _P]),
}
# symbol -> (restype, argtypes); every function include/p3d_r1.h declares (the R1 penalty: tangent layer, mbstd double backward, the penalty's sums)
R1_SIGNATURES = {
    "p3d_conv2d_mask_f32": (_I, [_P, _I, _I, _I, _I, _P, _I, _I, _I, _I, _I, _I, _P, _I, _F, _F, _F, _P, _P]),
    "p3d_mbstd_backward2_f32": (_I, [_P, _P, _L, _P, _I, _I, _L, _I, _I, _P, _P, _P]),
    "p3d_r1_sumsq_f32": (_I, [_P, _L, _P, _L, _I, _P, _P]),
}
# symbol -> (restype, argtypes); every function include/p3d_augment_tail.h declares (the augmentation pipe's filter, noise and cutout, and the adjoint)
AUGMENT_TAIL_SIGNATURES = {
    "p3d_augment_tail_plan": (_I, [_I, C.POINTER(C.c_int), _I]),
    "p3d_augment_tail_f32": (_I, [_P, _P, _I, _P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "p3d_augment_tail_adjoint_f32": (_I, [_P, _P, _I, _P, _I, _I, _I, _I, _P, _P]),
}
P3D_TAIL_MAX_TAPS, P3D_TAIL_TILE_W, P3D_TAIL_MAX_SIDE, P3D_TAIL_LDS_BYTES = 63, 64, 32768, 81920  # include/p3d_augment_tail.h
P3D_AUG_PLAN_AUTO, P3D_AUG_PLAN_TILE, P3D_AUG_PLAN_STAGED, P3D_AUG_TILE, P3D_AUG_LDS_BYTES, P3D_AUG_MAX_SIDE = 0, 1, 2, 16, 65536, 16384  # include/p3d_augment.h
P3D_CLIP_KC, P3D_CLIP_CUS, P3D_CLIP_TILE_64, P3D_CLIP_TILE_32, P3D_CLIP_MAX_SPLIT, P3D_CLIP_XCDS = 64, 256, 1, 2, 255, 8   # include/p3d_clip.h
P3D_CLIP_GELU, P3D_CLIP_PATCH, P3D_CLIP_HEAD_DIM, P3D_CLIP_MAX_T, P3D_CLIP_MAX_SIDE, P3D_CLIP_MAX_S = 1, 2, 64, 64, 16384, 4096  # include/p3d_clip.h
P3D_CLIP_KIND_PREPARE, P3D_CLIP_KIND_GEMM, P3D_CLIP_KIND_LAYERNORM, P3D_CLIP_KIND_EMBED, P3D_CLIP_KIND_ATTENTION = 0, 1, 2, 3, 4  # include/p3d_clip.h
P3D_RMLINE_MAX_TAPS, P3D_RMLINE_MAX_DILATE, P3D_RMLINE_MAX_C = 33, 8, 64                                       # include/p3d_rmline.h
P3D_RMLINE_ACT_NONE, P3D_RMLINE_ACT_LEAKY, P3D_RMLINE_ACT_TANH = 0, 1, 2                                       # include/p3d_rmline.h
P3D_RMLINE_TILE_8, P3D_RMLINE_TILE_4 = 1, 2                                                                    # include/p3d_rmline.h
P3D_RMLINE_IN_STACK, P3D_RMLINE_OUT_PLANAR, P3D_RMLINE_OUT_LERP, P3D_RMLINE_IN_NO_MASK = 1, 2, 4, 8            # include/p3d_rmline.h
P3D_RMLINE_FWD_MASK_INPUT, P3D_RMLINE_FWD_LERP = 1, 2                                                          # include/p3d_rmline.h
P3D_PM_NO_CULL, P3D_PM_SLICES_SHIFT, P3D_PM_MAX_SLICES, P3D_PM_QUERY_BLOCK, P3D_PM_FACE_TILE = 1, 8, 256, 128, 64  # include/p3d_metrics.h
P3D_ENC_KC, P3D_ENC_CUS, P3D_ENC_TILE_64, P3D_ENC_TILE_32, P3D_ENC_MAX_SPLIT, P3D_ENC_RELU = 64, 256, 1, 2, 255, 1  # include/p3d_encoder.h
P3D_ENC_KIND_CONV, P3D_ENC_KIND_MAXPOOL, P3D_ENC_KIND_PREPARE = 0, 1, 2                                           # include/p3d_encoder.h
P3D_LPIPS_MAX_K, P3D_LPIPS_MAX_STRIDE, P3D_LPIPS_BWD_MAX_CI = 11, 4, 4  # include/p3d_lpips.h
P3D_OPTIM_CHUNK = 4096                                              # include/p3d_optim.h
P3D_OPTIM_ADAM, P3D_OPTIM_ADAM_EMA, P3D_OPTIM_EMA = 1, 2, 3         # include/p3d_optim.h
P3D_BLUR_MAX_TAPS = 127                                # include/p3d_loss.h
P3D_DEPTH_Z, P3D_DEPTH_X, P3D_DEPTH_NORM = 0, 1, 2     # include/p3d_loss.h
P3D_GRAD_STATS_BYTES = 256 # include/p3d_render_grad.h: u64 at byte 0 of the workspace = samples that ran the MLP backward

_LIB = None


def lib():
    """Load the shared library (once).  Raises RuntimeError when it has not been built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(SO):
            raise RuntimeError(f"{SO} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(there is no CPU fallback for the HIP path)")
        if "P3D_LIB" not in os.environ:
            from . import _build
            if _build.needs_build():  # compiled from other sources than the ones on disk: never run stale kernels silently
                import sys
                print(f"panic3d_amd: {SO} does not match csrc/ (source hash): rebuilding", file=sys.stderr)
                _build.build()  # (not force: under torch.distributed.run the rank that gets the lock builds, the others find it done)
        L = C.CDLL(SO)
        for name, (res, args) in list(SIGNATURES.items()) + list(GRAD_SIGNATURES.items()) + list(SYN_GRAD_SIGNATURES.items()) \
                + list(PASTE_GRAD_SIGNATURES.items()) + list(DISC_SIGNATURES.items()) + list(LOSS_SIGNATURES.items()) + list(OPTIM_SIGNATURES.items()) \
                + list(LPIPS_SIGNATURES.items()) + list(ENCODER_SIGNATURES.items()) + list(METRICS_SIGNATURES.items()) + list(RMLINE_SIGNATURES.items()) \
                + list(CLIP_SIGNATURES.items()) + list(RMLINE_GRAD_SIGNATURES.items()) + list(AUGMENT_SIGNATURES.items()) + list(R1_SIGNATURES.items()) \
                + list(AUGMENT_TAIL_SIGNATURES.items()):
            fn = getattr(L, name)  # AttributeError if the .so does not export a declared symbol
            fn.restype, fn.argtypes = res, args
        got = L.p3d_abi_version()
        if got != P3D_ABI_VERSION:
            raise RuntimeError(f"{SO} was built for ABI version {got}, this binding is written for {P3D_ABI_VERSION}: rebuild the library")
        check_struct_layouts(L)
        _LIB = L
    return _LIB


OPTIM_STRUCT_MIRRORS = {0: OptimTensor, 1: OptimStep, 2: OptimChunk, 3: OptimArgs}  # P3D_OPTIM_STRUCT_* (p3d_optim_struct_layout)
STRUCT_MIRRORS = {0: Opts, 1: Dumps, 2: PasteArgs, 3: ConvArgs}  # P3D_STRUCT_* -> the ctypes restatement above
RMLINE_STRUCT_MIRRORS = {0: RmlineDog, 1: RmlineLayer}  # p3d_rmline_struct_layout


def check_struct_layouts(L):
    """Compare every ctypes mirror with the layout the library was compiled with (p3d_struct_layout: sizeof + the offset of
    each field in declaration order).  The mirrors are written by hand; p3d_abi_version() alone would not notice a field that
    was added to one side only, or a padding difference."""
    buf = (C.c_size_t * 64)()
    n = L.p3d_enc_struct_layout(buf, 64)
    if n <= 0 or list(buf[:n]) != [C.sizeof(EncLayer)] + [getattr(EncLayer, name).offset for name, _ in EncLayer._fields_]:
        raise RuntimeError(f"EncLayer: the ctypes mirror in _lib.py does not match the struct {SO} was compiled with ({list(buf[:max(n, 0)])}): "
                           "include/p3d_encoder.h and _lib.py have diverged")
    n = L.p3d_clip_struct_layout(buf, 64)
    if n <= 0 or list(buf[:n]) != [C.sizeof(ClipStep)] + [getattr(ClipStep, name).offset for name, _ in ClipStep._fields_]:
        raise RuntimeError(f"ClipStep: the ctypes mirror in _lib.py does not match the struct {SO} was compiled with ({list(buf[:max(n, 0)])}): "
                           "include/p3d_clip.h and _lib.py have diverged")
    for query, which, cls in [("p3d_struct_layout", w, c) for w, c in STRUCT_MIRRORS.items()] + \
            [("p3d_optim_struct_layout", w, c) for w, c in OPTIM_STRUCT_MIRRORS.items()] + \
            [("p3d_rmline_struct_layout", w, c) for w, c in RMLINE_STRUCT_MIRRORS.items()]:
        n = getattr(L, query)(which, buf, 64)
        if n <= 0:
            raise RuntimeError(f"{query}({which}) failed: {n}")
        mine = [C.sizeof(cls)] + [getattr(cls, name).offset for name, _ in cls._fields_]
        theirs = list(buf[:n])
        if mine != theirs:
            raise RuntimeError(f"{cls.__name__}: the ctypes mirror in _lib.py (size, offsets {mine}) does not match the struct "
                               f"{SO} was compiled with ({theirs}): include/ and _lib.py have diverged")


def check(rc, what):
    if rc != 0:
        kind = {-1: "invalid argument", -2: "size out of supported range", -3: "workspace too small"}.get(rc, f"hipError {rc}")
        raise RuntimeError(f"{what} failed: {kind} (code {rc})")
