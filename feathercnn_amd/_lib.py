"""ctypes binding of the C-ABI in include/feather_hip/feather_hip.h (one declaration per exported symbol)."""
from __future__ import annotations

import collections
import ctypes
import functools
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LOADED = {}  # path -> ctypes.CDLL with every symbol of its table typed

STAGE_NAMES = ("wino_input", "wino_gemm", "wino_output", "igemm", "depthwise", "init", "wino_chain")


class fhip_conv_param(ctypes.Structure):
    """fhip_conv_param == booster::ConvParam field for field (reference booster.h:59-77)."""
    _fields_ = [(n, ctypes.c_int) for n in (
        "output_channels", "input_channels", "input_h", "input_w", "kernel_h", "kernel_w", "output_h", "output_w",
        "stride_h", "stride_w", "pad_left", "pad_bottom", "pad_right", "pad_top", "group", "bias_term", "activation")]


class fhip_winograd_plan(ctypes.Structure):
    _fields_ = [("tiles_x", ctypes.c_int), ("tiles_y", ctypes.c_int), ("tiles_per_image", ctypes.c_int),
                ("columns", ctypes.c_int), ("columns_padded", ctypes.c_int), ("column_block", ctypes.c_int), ("frequency_points", ctypes.c_int), ("tile_outputs", ctypes.c_int),
                ("in_channels_padded", ctypes.c_int),
                ("out_channels_padded", ctypes.c_int), ("v_offset_bytes", ctypes.c_size_t), ("v_bytes", ctypes.c_size_t),
                ("m_offset_bytes", ctypes.c_size_t), ("m_bytes", ctypes.c_size_t), ("u_bytes", ctypes.c_size_t)]


class fhip_pool_param(ctypes.Structure):
    """fhip_pool_param (feather_net.h), the fields PoolingLayer::LoadParam reads (reference pooling_layer.h:90-107)."""
    _fields_ = [(n, ctypes.c_int) for n in (
        "channels", "input_h", "input_w", "kernel_h", "kernel_w", "stride_h", "stride_w", "pad_left", "pad_right",
        "pad_top", "pad_bottom", "pooling_type", "global_pooling")]


class fhip_pixel_image(ctypes.Structure):
    """fhip_pixel_image (feather_net.h): one image of a mixed-size batch; stride 0 = w * channels, roi_w = roi_h = 0 = the whole image."""
    _fields_ = [("data", ctypes.c_void_p)] + [(n, ctypes.c_int) for n in ("w", "h", "stride", "roi_x", "roi_y", "roi_w", "roi_h")]


_P = ctypes.POINTER(fhip_conv_param)
_Q = ctypes.POINTER(fhip_pool_param)
_PI = ctypes.POINTER(ctypes.c_int)
_SZ = ctypes.c_size_t
_V = ctypes.c_void_p
_I = ctypes.c_int

# symbol -> (restype, argtypes); tests/test_boundary.py checks this table against the header.
SIGNATURES = {
    "fhip_conv_assign_output_dim": (_I, [_P]),
    "fhip_conv_flops": (ctypes.c_double, [_P]),
    "fhip_conv_select_algo": (_I, [_P, ctypes.POINTER(_I)]),
    "fhip_conv_select_algo_tuned": (_I, [_P, ctypes.POINTER(_I)]),
    "fhip_conv_get_buffer_size": (_I, [_P, _I, _I, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]),
    "fhip_conv_packed_layout": (_I, [_P, _I, ctypes.POINTER(ctypes.c_int)]),
    "fhip_conv_init": (_I, [_P, _I, _V, _V, _V]),
    "fhip_conv_forward": (_I, [_P, _I, _I, _V, _V, _V, _V, _V, _V]),
    "fhip_winograd_f63_plan": (_I, [_P, _I, ctypes.POINTER(fhip_winograd_plan)]),
    "fhip_winograd_f63_plan_canvas": (_I, [_P, _I, _I, ctypes.POINTER(fhip_winograd_plan)]),
    "fhip_winograd_f63_canvas_param": (_I, [_P, _I, _P]),
    "fhip_winograd_f63_transform_kernel": (_I, [_P, _V, _V, _V]),
    "fhip_winograd_f63_input_transform": (_I, [_P, _I, _V, _V, _V]),
    "fhip_winograd_f63_tile_gemm": (_I, [_P, _I, _V, _V, _V, _V]),
    "fhip_winograd_f63_output_transform": (_I, [_P, _I, _V, _V, _V, _V]),
    "fhip_stage_timing_enable": (_I, [_I]),
    "fhip_stage_timing_collect": (_I, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_longlong)]),
    "fhip_last_error": (ctypes.c_char_p, []),
    "fhip_version": (ctypes.c_char_p, []),
    "fhip_device_info": (_I, [ctypes.c_char_p, _I, ctypes.POINTER(_I), ctypes.POINTER(_I)]),
    "fhip_conv_streams_1x1": (_I, [_P, _I, _I]),
    "fhip_calibrate_mfma_f32": (_I, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), _V]),
    # include/feather_hip/feather_net.h -- layers between the convolutions
    "fhip_relu": (_I, [_V, _V, _SZ, _V]),
    "fhip_add": (_I, [_V, _V, _V, _SZ, _I, _V]),
    "fhip_affine": (_I, [_V, _V, _V, _V, _I, _I, _I, _I, _V]),
    "fhip_conv_can_fuse_residual": (_I, [_P, _I]),
    "fhip_conv_forward_residual": (_I, [_P, _I, _I, _V, _V, _V, _V, _V, _V, _V]),
    "fhip_conv_can_fuse_dw_pw": (_I, [_P, _P, _I]),
    "fhip_conv_forward_dw_pw": (_I, [_P, _P, _I, _V, _V, _V, _V, _V, _V, _V]),
    "fhip_conv_can_chain_winograd": (_I, [_P, _I, _P, _I, _I]),
    "fhip_conv_forward_chained": (_I, [_P, _I, _V, _V, _V, _V, _V, _V, _P, _V, _I, _V]),
    "fhip_winograd_f63_output_to_next_input": (_I, [_P, _P, _I, _V, _V, _V, _I, _V]),
    "fhip_conv_can_fuse_siblings": (_I, [_P, _I, _P, _I, _I]),
    "fhip_conv_siblings_geometry": (_I, [_P, _P, _P]),
    "fhip_conv_forward_siblings": (_I, [_P, _P, _I, _V, _V, _V, _V, _V, _V]),
    "fhip_conv_can_fuse_first_winograd": (_I, [_P, _P, _I, _I]),
    "fhip_winograd_f63_input_from_first": (_I, [_P, _P, _I, _V, _V, _V, _V, _V]),
    "fhip_conv_can_fuse_maxpool2": (_I, [_P, _I]),
    "fhip_conv_forward_maxpool2": (_I, [_P, _I, _I, _V, _V, _V, _V, _V, _V]),
    "fhip_pixels_to_float": (_I, [_V, _V, _I, _I, _I, _I, _I, _I, _V, _V, _V]),
    "fhip_yuv420sp_to_float": (_I, [_V, _V, _I, _I, _I, _I, _I, _I, _I, _V, _V, _V]),
    "fhip_pixel_images_plan": (_I, [_V, _I, _I, _I, _I, _V, ctypes.POINTER(_SZ)]),
    "fhip_pixels_to_float_images": (_I, [_V, _V, _V, _V, _V, _V]),
    "fhip_pooling_output_dim": (_I, [_Q, _PI, _PI]),
    "fhip_pooling": (_I, [_Q, _I, _V, _V, _V]),
    "fhip_softmax": (_I, [_V, _V, _I, _I, _V]),
    # include/feather_hip/feather_net.h -- feather::Net on device blobs
    "fhip_net_create": (_I, [ctypes.POINTER(_V)]),
    "fhip_net_destroy": (_I, [_V]),
    "fhip_net_set_stream": (_I, [_V, _V]),
    "fhip_net_get_stream": (_I, [_V, ctypes.POINTER(_V)]),
    "fhip_net_set_fusion": (_I, [_V, _I]),
    "fhip_net_set_graph": (_I, [_V, _I]),
    "fhip_net_set_tuned_selection": (_I, [_V, _I]),
    "fhip_net_set_dilated": (_I, [_V, _I]),
    "fhip_net_set_quantized": (_I, [_V, _I]),
    "fhip_net_set_requantized": (_I, [_V, _I]),
    "fhip_net_set_extended_layers": (_I, [_V, _I]),
    "fhip_net_set_detection": (_I, [_V, _I]),
    "fhip_net_set_colpass": (_I, [_V, _I]),
    "fhip_net_set_yolo": (_I, [_V, _I]),
    "fhip_net_set_roi": (_I, [_V, _I]),
    "fhip_net_set_frame": (_I, [_V, _I]),
    "fhip_net_set_transformer": (_I, [_V, _I]),
    "fhip_net_set_recurrent": (_I, [_V, _I]),
    "fhip_net_set_concurrency": (_I, [_V, _I]),
    "fhip_net_set_sub_batches": (_I, [_V, _I]),
    "fhip_net_load_param": (_I, [_V, ctypes.c_char_p]),
    "fhip_net_load_param_mem": (_I, [_V, ctypes.c_char_p, _SZ]),
    "fhip_net_load_weights": (_I, [_V, ctypes.c_char_p]),
    "fhip_net_load_weights_mem": (_I, [_V, _V, _SZ]),
    "fhip_net_load_weights_device": (_I, [_V, _V, _SZ]),
    "fhip_net_feed_input": (_I, [_V, ctypes.c_char_p, _I, _I, _I, _I, _V, _I]),
    "fhip_net_feed_pixels": (_I, [_V, ctypes.c_char_p, _I, _V, _I, _I, _I, _I, _I, _V, _V, _I]),
    "fhip_net_feed_yuv420sp": (_I, [_V, ctypes.c_char_p, _I, _V, _I, _I, _I, _I, _I, _I, _V, _V, _I]),
    "fhip_net_feed_pixel_images": (_I, [_V, ctypes.c_char_p, _I, _V, _I, _I, _I, _V, _V, _I]),
    "fhip_net_forward": (_I, [_V]),
    "fhip_net_extract": (_I, [_V, ctypes.c_char_p, ctypes.POINTER(_V), _PI, _PI, _PI, _PI]),
    "fhip_net_extract_host": (_I, [_V, ctypes.c_char_p, _V, _SZ]),
    "fhip_net_layer_count": (_I, [_V]),
    "fhip_net_layer_info": (_I, [_V, _I, ctypes.c_char_p, ctypes.c_char_p, _I, _PI]),
    "fhip_net_layer_conv_param": (_I, [_V, _I, _P, _PI]),
    "fhip_net_layer_fused_pointwise": (_I, [_V, _I, _P, _PI]),
    "fhip_net_layer_chain": (_I, [_V, _I, _PI, _PI]),
    "fhip_net_layer_canvas": (_I, [_V, _I, _PI]),
    "fhip_net_layer_colpass": (_I, [_V, _I, _PI]),
    "fhip_net_layer_sibling": (_I, [_V, _I, _PI]),
    "fhip_net_layer_residual": (_I, [_V, _I, _PI]),
    "fhip_net_forward_timed": (_I, [_V, ctypes.POINTER(ctypes.c_float)]),
    "fhip_net_memory": (_I, [_V, ctypes.POINTER(_SZ), ctypes.POINTER(_SZ), ctypes.POINTER(_SZ)]),
}

# include/feather_hip/feather_pixout.h -- libfeather_pixout.so, the image output path (a library of its own)
PIXOUT_SIGNATURES = {
    "fhip_pixout_channels": (_I, [_I]),
    "fhip_float_to_pixels": (_I, [_V, _SZ, _V, _I, _I, _I, _I, _I, _I, _V, _V, _V]),
    "fhip_float_to_pixels_host": (_I, [_V, _SZ, _V, _I, _I, _I, _I, _I, _I, _V, _V, _V]),
    "fhip_pixout_last_error": (ctypes.c_char_p, []),
}

# include/feather_hip/feather_gconv.h -- libfeather_gconv.so, grouped convolution with 1 < group < C (a library of its own)
GCONV_SIGNATURES = {
    "fhip_gconv_supported": (_I, [_P]),
    "fhip_gconv_get_buffer_size": (_I, [_P, _I, ctypes.POINTER(_SZ), ctypes.POINTER(_SZ)]),
    "fhip_gconv_init": (_I, [_P, _V, _V, _V]),
    "fhip_gconv_forward": (_I, [_P, _I, _V, _V, _V, _V, _V, _V]),
    "fhip_gconv_route": (_I, [_P, _V, _V, ctypes.c_char_p, _I]),
    "fhip_gconv_last_error": (ctypes.c_char_p, []),
}

# include/feather_hip/feather_deconv.h -- libfeather_deconv.so, transposed convolution (a library of its own)
class fhip_deconv_param(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("output_channels", "input_channels", "input_h", "input_w", "kernel_h", "kernel_w", "output_h", "output_w",
                                            "stride_h", "stride_w", "pad_left", "pad_bottom", "pad_right", "pad_top", "group", "bias_term",
                                            "activation", "output_pad_right", "output_pad_bottom")]


_DP = ctypes.POINTER(fhip_deconv_param)
DECONV_SIGNATURES = {
    "fhip_deconv_assign_output_dim": (_I, [_DP]),
    "fhip_deconv_supported": (_I, [_DP]),
    "fhip_deconv_get_buffer_size": (_I, [_DP, _I, ctypes.POINTER(_SZ), ctypes.POINTER(_SZ)]),
    "fhip_deconv_init": (_I, [_DP, _V, _V, _V]),
    "fhip_deconv_forward": (_I, [_DP, _I, _V, _V, _V, _V, _V, _V]),
    "fhip_deconv_route": (_I, [_DP, ctypes.c_char_p, _I]),
    "fhip_deconv_last_error": (ctypes.c_char_p, []),
}

# include/feather_hip/feather_inorm.h -- libfeather_inorm.so, InstanceNorm and the activations of generative nets (a library of its own)
_FL = ctypes.c_float
INORM_SIGNATURES = {
    "fhip_instance_norm_get_buffer_size": (_I, [_I, _I, _I, _I, ctypes.POINTER(_SZ)]),
    "fhip_instance_norm_forward": (_I, [_I, _I, _I, _I, _V, _V, _V, _V, _FL, _I, _FL, _V, _V]),
    "fhip_instance_norm_forward_route": (_I, [_I, _I, _I, _I, _I, _V, _V, _V, _V, _FL, _I, _FL, _V, _V]),
    "fhip_instance_norm_route": (_I, [_I, _I, _I, _I, _V, _V, ctypes.c_char_p, _I]),
    "fhip_activation_forward": (_I, [_I, _V, _V, _I, _I, _I, _FL, _FL, _V, _V]),
    "fhip_inorm_last_error": (ctypes.c_char_p, []),
}

# include/feather_hip/feather_shuffle.h -- libfeather_shuffle.so, the channel map: ShuffleChannel, Slice and their chains with Concat
_PP = ctypes.POINTER(ctypes.c_void_p)
_IP = ctypes.POINTER(ctypes.c_int)
SHUFFLE_SIGNATURES = {
    "fhip_channel_map_supported": (_I, [_I, _I, _I, _I]),
    "fhip_channel_slice_resolve": (_I, [_I, _IP, _I, _IP]),
    "fhip_channel_shuffle_forward": (_I, [_V, _V, _I, _I, _I, _I, _I, _I, _V]),
    "fhip_channel_slice_forward": (_I, [_PP, _V, _I, _I, _I, _I, _IP, _I, _V]),
    "fhip_channel_map_create": (_I, [_PP, _IP, _I, _IP, _I, _IP]),
    "fhip_channel_map_destroy": (_I, [_V]),
    "fhip_channel_map_forward": (_I, [_V, _PP, _PP, _I, _I, _I, _V]),
    "fhip_channel_map_forward_route": (_I, [_I, _V, _PP, _PP, _I, _I, _I, _V]),
    "fhip_channel_map_route": (_I, [_I, _I, _I, _PP, _I, ctypes.c_char_p, _I]),
    "fhip_shuffle_last_error": (ctypes.c_char_p, []),
}

# include/feather_hip/feather_canvas.h -- libfeather_canvas.so, the chained Winograd transforms of layers that run on 2x2 image canvases
_PL = ctypes.POINTER(fhip_winograd_plan)
CANVAS_SIGNATURES = {
    "fhip_canvas_output_to_next_input": (_I, [_I, _P, _P, _I, _PL, _PL, _V, _V, _V, _V]),
    "fhip_canvas_output_transform": (_I, [_P, _I, _PL, _V, _V, _V, _I, _V]),
    "fhip_canvas_last_error": (ctypes.c_char_p, []),
}

# include/feather_hip/feather_atrous.h -- libfeather_atrous.so, dilated convolution (a library of its own)
class fhip_atrous_param(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("output_channels", "input_channels", "input_h", "input_w", "kernel_h", "kernel_w", "output_h", "output_w",
                                            "stride_h", "stride_w", "pad_left", "pad_bottom", "pad_right", "pad_top", "group", "bias_term",
                                            "activation", "dilation_h", "dilation_w")]


_AP = ctypes.POINTER(fhip_atrous_param)
ATROUS_SIGNATURES = {
    "fhip_atrous_assign_output_dim": (_I, [_AP]),
    "fhip_atrous_supported": (_I, [_AP]),
    "fhip_atrous_get_buffer_size": (_I, [_AP, _I, ctypes.POINTER(_SZ), ctypes.POINTER(_SZ)]),
    "fhip_atrous_init": (_I, [_AP, _V, _V, _V]),
    "fhip_atrous_forward": (_I, [_AP, _I, _V, _V, _V, _V, _V, _V]),
    "fhip_atrous_route": (_I, [_AP, ctypes.c_char_p, _I]),
    "fhip_atrous_get_buffer_size_route": (_I, [_AP, _I, ctypes.c_char_p, ctypes.POINTER(_SZ), ctypes.POINTER(_SZ)]),
    "fhip_atrous_init_route": (_I, [_AP, _V, _V, _V, ctypes.c_char_p]),
    "fhip_atrous_forward_route": (_I, [_AP, _I, _V, _V, _V, _V, _V, _V, ctypes.c_char_p]),
    "fhip_atrous_last_error": (ctypes.c_char_p, []),
}

# include/feather_hip/feather_gate.h -- libfeather_gate.so, squeeze-and-excitation channel gating, Swish, HardSigmoid (a library of its own)
GATE_SIGNATURES = {
    "fhip_channel_gate_forward": (_I, [_I, _I, _I, _I, _V, _V, _V, _V, _I, _V]),
    "fhip_squeeze_get_buffer_size": (_I, [_I, _I, _I, _I, ctypes.POINTER(_SZ)]),
    "fhip_squeeze_forward": (_I, [_I, _I, _I, _I, _V, _V, _V, _V]),
    "fhip_excite_forward": (_I, [_I, _I, _I, _V, _V, _V, _V, _V, _V, _I, _I, _FL, _FL, _V]),
    "fhip_excite_forward_slices": (_I, [_I, _I, _I, _I, _V, _V, _V, _V, _V, _V, _I, _I, _FL, _FL, _V]),
    "fhip_gate_activation_forward": (_I, [_I, _V, _V, _I, _I, _I, _FL, _FL, _V]),
    "fhip_gate_route": (_I, [_I, _I, _I, _I, _I, _V, _V, _V, ctypes.c_char_p, _I]),
    "fhip_gate_last_error": (ctypes.c_char_p, []),
}

# include/feather_hip/feather_resample.h -- libfeather_resample.so, Interp (nearest / bilinear resize) and HardSwish (a library of its own)
RESAMPLE_SIGNATURES = {
    "fhip_interp_output_dim": (_I, [_I, _I, _FL, _FL, _I, _I, _PI, _PI]),
    "fhip_interp_forward": (_I, [_I, _I, _I, _I, _I, _I, _I, _I, _FL, _FL, _V, _V, _V, _I, _V]),
    "fhip_interp_route": (_I, [_I, _I, _I, _I, _I, _I, _I, _FL, _FL, _V, _V, _V, ctypes.c_char_p, _I]),
    "fhip_hardswish_forward": (_I, [_V, _V, _I, _I, _I, _FL, _FL, _V]),
    "fhip_hardswish_route": (_I, [_V, _V, _I, _I, _I, ctypes.c_char_p, _I]),
    "fhip_resample_last_error": (ctypes.c_char_p, []),
}

# include/feather_hip/feather_lrn.h -- libfeather_lrn.so, local response normalisation alone and with the Pooling layer behind it (a library
# of its own)
LRN_SIGNATURES = {
    "fhip_lrn_forward": (_I, [_I, _I, _FL, _FL, _FL, _I, _I, _I, _I, _V, _V, _V]),
    "fhip_lrn_forward_chunked": (_I, [_I, _FL, _FL, _FL, _I, _I, _I, _I, _I, _V, _V, _V]),
    "fhip_lrn_route": (_I, [_I, _I, _I, _I, _I, _I, _V, _V, ctypes.c_char_p, _I]),
    "fhip_lrn_pool_forward": (_I, [_I, _I, _FL, _FL, _FL, _I, _I, _I, _I, _Q, _V, _V, _V]),
    "fhip_lrn_pool_route": (_I, [_I, _I, _I, _I, _I, _I, _Q, _V, _V, ctypes.c_char_p, _I]),
    "fhip_lrn_last_error": (ctypes.c_char_p, []),
}

# include/feather_hip/feather_qconv.h -- libfeather_qconv.so, ncnn-style int8 convolution with fp32 input and output (a library of its own)
class fhip_qconv_param(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("output_channels", "input_channels", "input_h", "input_w", "kernel_h", "kernel_w", "output_h", "output_w",
                                            "stride_h", "stride_w", "pad_left", "pad_bottom", "pad_right", "pad_top", "group", "bias_term",
                                            "activation", "dilation_h", "dilation_w", "int8_scale_term")]


_QP = ctypes.POINTER(fhip_qconv_param)
QCONV_SIGNATURES = {
    "fhip_qconv_assign_output_dim": (_I, [_QP]),
    "fhip_qconv_supported": (_I, [_QP]),
    "fhip_qconv_get_buffer_size": (_I, [_QP, _I, ctypes.POINTER(_SZ), ctypes.POINTER(_SZ)]),
    "fhip_qconv_init": (_I, [_QP, _V, _V, _V]),
    "fhip_qconv_dequant_scales": (_I, [_V, _V, _I, _FL]),
    "fhip_qconv_forward": (_I, [_QP, _I, _V, _V, _V, _V, _V, _V, _FL, _V]),
    "fhip_quantize_forward": (_I, [_V, _V, _SZ, _FL, _V]),
    "fhip_qconv_route": (_I, [_QP, ctypes.c_char_p, _I]),
    "fhip_qconv_get_buffer_size_route": (_I, [_QP, _I, ctypes.c_char_p, ctypes.POINTER(_SZ), ctypes.POINTER(_SZ)]),
    "fhip_qconv_init_route": (_I, [_QP, _V, _V, _V, ctypes.c_char_p]),
    "fhip_qconv_forward_route": (_I, [_QP, _I, _V, _V, _V, _V, _V, _V, _FL, _V, ctypes.c_char_p]),
    "fhip_qconv_last_error": (ctypes.c_char_p, []),
}


# include/feather_hip/feather_q8.h -- libfeather_q8.so, int8 convolution on q8 tensors: int8 activations between int8 layers (a library of
# its own)
class fhip_q8_param(ctypes.Structure):
    _fields_ = fhip_qconv_param._fields_ + [("input_int8", ctypes.c_int), ("output_int8", ctypes.c_int)]


_8P = ctypes.POINTER(fhip_q8_param)
Q8_SIGNATURES = {
    "fhip_q8_tensor_bytes": (_I, [_I, _I, _I, _I, ctypes.POINTER(_SZ)]),
    "fhip_q8_assign_output_dim": (_I, [_8P]),
    "fhip_q8_supported": (_I, [_8P]),
    "fhip_q8_get_buffer_size": (_I, [_8P, _I, ctypes.POINTER(_SZ), ctypes.POINTER(_SZ)]),
    "fhip_q8_init": (_I, [_8P, _V, _V, _V]),
    "fhip_q8_dequant_scales": (_I, [_V, _V, _I, _FL]),
    "fhip_q8_forward": (_I, [_8P, _I, _V, _V, _V, _V, _V, _V, _FL, _FL, _V]),
    "fhip_q8_route": (_I, [_8P, ctypes.c_char_p, _I]),
    "fhip_q8_get_buffer_size_route": (_I, [_8P, _I, ctypes.c_char_p, ctypes.POINTER(_SZ), ctypes.POINTER(_SZ)]),
    "fhip_q8_init_route": (_I, [_8P, _V, _V, _V, ctypes.c_char_p]),
    "fhip_q8_forward_route": (_I, [_8P, _I, _V, _V, _V, _V, _V, _V, _FL, _FL, _V, ctypes.c_char_p]),
    "fhip_q8_quantize_forward": (_I, [_V, _V, _I, _I, _I, _I, _FL, _V]),
    "fhip_q8_dequantize_forward": (_I, [_V, _V, _I, _I, _I, _I, _FL, _V]),
    "fhip_q8_relu_forward": (_I, [_V, _V, _SZ, _V]),
    "fhip_q8_max_pool_forward": (_I, [_Q, _I, _V, _V, _V]),
    "fhip_q8_last_error": (ctypes.c_char_p, []),
}


# include/feather_hip/feather_detect.h -- libfeather_detect.so, the layers of an SSD detection head: Permute, Normalize, a softmax along any
# axis, PriorBox (a host function) and DetectionOutput (a library of its own)
_FP = ctypes.POINTER(ctypes.c_float)
DETECT_SIGNATURES = {
    "fhip_permute_output_dim": (_I, [_I, _I, _I, _I, _I, _PI, _PI, _PI]),
    "fhip_permute_forward": (_I, [_I, _I, _I, _I, _I, _I, _V, _V, _V]),
    "fhip_permute_concat_forward": (_I, [_I, _PI, _PI, _I, _V, _PP, _V]),
    "fhip_normalize_forward": (_I, [_I, _I, _I, _I, _I, _FL, _V, _V, _V, _V]),
    "fhip_axis_softmax_forward": (_I, [_I, _I, _I, _V, _V, _V]),
    "fhip_priorbox_fill": (_I, [_I, _I, _I, _I, _FP, _I, _FP, _I, _FP, _I, _FP, _I, _I, _FL, _FL, _FL, _PI, _FP, _SZ]),
    "fhip_detection_output_get_buffer_size": (_I, [_I, _I, _I, _I, _I, ctypes.POINTER(_SZ)]),
    "fhip_detection_output_forward": (_I, [_I, _I, _I, _FL, _I, _I, _FL, _I, _V, _V, _V, _V, _V, _V]),
    "fhip_detect_route": (_I, [_I, _I, _I, _I, _I, _I, _V, _V, ctypes.c_char_p, _I]),
    "fhip_detect_last_error": (ctypes.c_char_p, []),
}


# include/feather_hip/feather_colpass.h -- libfeather_colpass.so, the Winograd tile GEMM of 64-input-channel layers that writes the
# column-passed M (48 planes) and the chained transform that reads it (a library of its own)
COLPASS_SIGNATURES = {
    "fhip_colpass_supported": (_I, [_P, _I]),
    "fhip_colpass_tile_gemm": (_I, [_P, _I, _PL, _V, _V, _V, _V]),
    "fhip_colpass_output_to_next_input": (_I, [_P, _P, _I, _PL, _PL, _V, _V, _V, _I, _V]),
    "fhip_colpass_last_error": (ctypes.c_char_p, []),
}


# include/feather_hip/feather_yolo.h -- libfeather_yolo.so, the layers of a YOLO detection head: Reorg, YoloDetectionOutput and
# Yolov3DetectionOutput (a library of its own)
YOLO_SIGNATURES = {
    "fhip_reorg_output_dim": (_I, [_I, _I, _I, _I, _PI, _PI, _PI]),
    "fhip_reorg_forward": (_I, [_I, _I, _I, _I, _I, _I, _V, _V, _V]),
    "fhip_yolo_get_buffer_size": (_I, [_I, _I, _I, _I, _PI, _PI, ctypes.POINTER(_SZ)]),
    "fhip_yolo_detection_forward": (_I, [_I, _I, _I, _I, _I, _PI, _PI, _FL, _FL, _FP, _I, _PI, _FP, _I, _V, _PP, _V, _V]),
    "fhip_yolo_route": (_I, [_I, _I, _I, ctypes.c_char_p, _I]),
    "fhip_yolo_last_error": (ctypes.c_char_p, []),
}


# include/feather_hip/feather_roi.h -- libfeather_roi.so, the layers of a two-stage detector: Proposal, ROIPooling, ROIAlign and PSROIPooling
# (a library of its own)
ROI_SIGNATURES = {
    "fhip_roi_generate_anchors": (_I, [_I, _FP, _I, _FP, _I, _FP]),
    "fhip_proposal_get_buffer_size": (_I, [_I, _I, _I, _I, ctypes.POINTER(_SZ)]),
    "fhip_proposal_forward": (_I, [_I, _I, _I, _I, _I, _I, _I, _FL, _FL, _FP, _V, _V, _V, _V, _V, _V, _V]),
    "fhip_roi_pool_forward": (_I, [_I, _I, _I, _I, _I, _I, _I, _FL, _V, _V, _V, _V]),
    "fhip_roi_align_forward": (_I, [_I, _I, _I, _I, _I, _I, _I, _FL, _I, _I, _I, _V, _V, _V, _V]),
    "fhip_psroi_pool_forward": (_I, [_I, _I, _I, _I, _I, _I, _I, _FL, _I, _V, _V, _V, _V]),
    "fhip_roi_route": (_I, [_I, _I, _I, ctypes.c_char_p, _I]),
    "fhip_roi_last_error": (ctypes.c_char_p, []),
}


# include/feather_hip/feather_frame.h -- libfeather_frame.so, the layers that frame an image-to-image net: Padding, Crop (one window) and
# PixelShuffle (a library of its own)
FRAME_SIGNATURES = {
    "fhip_frame_window_output_dim": (_I, [_I] * 9 + [ctypes.POINTER(_I)] * 3),
    "fhip_frame_window_forward": (_I, [_I, _FL, _V] + [_I] * 10 + [_V, _V, _V]),
    "fhip_pixel_shuffle_output_dim": (_I, [_I] * 4 + [ctypes.POINTER(_I)] * 3),
    "fhip_pixel_shuffle_forward": (_I, [_I, _I, _I, _FL, _I, _I, _I, _I, _V, _V, _V]),
    "fhip_frame_route": (_I, [_I, _I, _I, _I, _I, _I, ctypes.c_char_p, _I]),
    "fhip_frame_last_error": (ctypes.c_char_p, []),
}


# include/feather_hip/feather_attn.h -- libfeather_attn.so, the layers of a Vision Transformer encoder: the attention core, LayerNorm, GELU
# and the element-wise BinaryOp (a library of its own)
ATTN_SIGNATURES = {
    "fhip_attention_forward": (_I, [_I, _I, _I, _I, _I, _V, _I, _V, _I, _V, _I, _V, _V]),
    "fhip_layer_norm_forward": (_I, [_I, _I, _V, _V, _FL, _V, _V, _V]),
    "fhip_add_layer_norm_forward": (_I, [_I, _I, _V, _V, _FL, _V, _V, _V, _V, _V]),
    "fhip_gelu_forward": (_I, [_I, _V, _V, _SZ, _V]),
    "fhip_binary_forward": (_I, [_I, _I, _I, _V, _V, _V, _FL, _SZ, _SZ, _V]),
    "fhip_attn_route": (_I, [_I, _I, _I, ctypes.c_char_p, _I]),
    "fhip_attn_last_error": (ctypes.c_char_p, []),
}


# include/feather_hip/feather_rnn.h -- libfeather_rnn.so, the recurrent core of ncnn's LSTM, GRU and RNN layers (a library of its own)
_RNN_FORWARD = [_I, _I, _I, _I, _I, _V, _I, _V, _V, _V, _V, _V, _I, _V, _V, _V, _V]
RNN_SIGNATURES = {
    "fhip_rnn_sequence_fits": (_I, [_I, _I]),
    "fhip_rnn_forward": (_I, _RNN_FORWARD),
    "fhip_rnn_forward_route": (_I, _RNN_FORWARD + [_I]),
    "fhip_rnn_route": (_I, [_I, _I, _I, _I, _I, ctypes.c_char_p, _I]),
    "fhip_rnn_last_error": (ctypes.c_char_p, []),
}


def _load(path, signatures):
    """Open the library at `path` once and type every symbol of `signatures`.  Fails loudly: there is no fallback implementation."""
    lib = _LOADED.get(path)
    if lib is None:
        # PyTorch bundles its own HIP/HSA runtime; it must be the one already mapped when our library (linked against
        # libamdhip64.so.7 by SONAME) is loaded, or the process ends up with two HSA runtimes and no visible device.
        import torch  # noqa: F401  (device memory + stream provider of this host mirror)
        if not os.path.exists(path):
            raise RuntimeError(f"feathercnn_amd: HIP library {path} is missing -- run `python -c 'import __graft_entry__ as g; "
                               "g.build()'` (or `make -C feathercnn_amd/csrc`). There is no CPU fallback.")
        lib = ctypes.CDLL(path)
        for name, (res, args) in signatures.items():
            fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _LOADED[path] = lib
    return lib


def checker(load, last_error: str):
    """The `_check(rc, what)` of one library: raises FeatherHipError with the text of the library's last-error symbol when a C-ABI call
    returned non-zero.  `load` is the library's load_* function."""
    def _check(rc: int, what: str):
        if rc != 0:
            from .booster import FeatherHipError  # booster imports this module
            msg = getattr(load(), last_error)().decode(errors="replace")
            raise FeatherHipError(f"{what} failed with code {rc}: {msg}")
    return _check


Library = collections.namedtuple("Library", "file headers macro signatures last_error structs route")

# One row per run-time library, in the order of csrc/Makefile (the main library, then SIDE): the file next to this module, the public headers
# under include/feather_hip/, the export macro of those headers, the signature table, the last-error symbol, the ctypes mirrors of the structs
# the headers define, and the name of the ROUTE_* constant of feathercnn_amd/net.py where the Net runtime routes layers to the library.
# tests/test_side_contract_cpu.py holds every row to the contract the libraries share; a new library adds a row here.
LIBRARIES = {
    "hip": Library("libfeather_hip.so", ("feather_hip.h", "feather_net.h"), "FHIP_API", SIGNATURES, "fhip_last_error",
                   (fhip_conv_param, fhip_winograd_plan, fhip_pool_param, fhip_pixel_image), None),
    "pixout": Library("libfeather_pixout.so", ("feather_pixout.h",), "FHIP_PIXOUT_API", PIXOUT_SIGNATURES, "fhip_pixout_last_error", (), None),
    "gconv": Library("libfeather_gconv.so", ("feather_gconv.h",), "FHIP_GCONV_API", GCONV_SIGNATURES, "fhip_gconv_last_error", (), "ROUTE_GCONV"),
    "deconv": Library("libfeather_deconv.so", ("feather_deconv.h",), "FHIP_DECONV_API", DECONV_SIGNATURES, "fhip_deconv_last_error",
                      (fhip_deconv_param,), "ROUTE_DECONV"),
    "inorm": Library("libfeather_inorm.so", ("feather_inorm.h",), "FHIP_INORM_API", INORM_SIGNATURES, "fhip_inorm_last_error", (), "ROUTE_INORM"),
    "shuffle": Library("libfeather_shuffle.so", ("feather_shuffle.h",), "FHIP_SHUFFLE_API", SHUFFLE_SIGNATURES, "fhip_shuffle_last_error", (),
                       "ROUTE_SHUFFLE"),
    "canvas": Library("libfeather_canvas.so", ("feather_canvas.h",), "FHIP_CANVAS_API", CANVAS_SIGNATURES, "fhip_canvas_last_error", (), None),
    "atrous": Library("libfeather_atrous.so", ("feather_atrous.h",), "FHIP_ATROUS_API", ATROUS_SIGNATURES, "fhip_atrous_last_error",
                      (fhip_atrous_param,), "ROUTE_ATROUS"),
    "gate": Library("libfeather_gate.so", ("feather_gate.h",), "FHIP_GATE_API", GATE_SIGNATURES, "fhip_gate_last_error", (), "ROUTE_GATE"),
    "resample": Library("libfeather_resample.so", ("feather_resample.h",), "FHIP_RESAMPLE_API", RESAMPLE_SIGNATURES, "fhip_resample_last_error", (),
                        "ROUTE_RESAMPLE"),
    "lrn": Library("libfeather_lrn.so", ("feather_lrn.h",), "FHIP_LRN_API", LRN_SIGNATURES, "fhip_lrn_last_error", (), "ROUTE_LRN"),
    "qconv": Library("libfeather_qconv.so", ("feather_qconv.h",), "FHIP_QCONV_API", QCONV_SIGNATURES, "fhip_qconv_last_error",
                     (fhip_qconv_param,), "ROUTE_QCONV"),
}
MAIN = "hip"
# The rows of SIDE_MORE of csrc/Makefile, the same tuple: libraries added where the tables the contract tests hold over LIBRARIES could not be
# edited; tests/test_q8_contract_cpu.py restates the contract for them.  A change that may touch those tables folds the rows
# into LIBRARIES.
MORE_LIBRARIES = {
    "q8": Library("libfeather_q8.so", ("feather_q8.h",), "FHIP_Q8_API", Q8_SIGNATURES, "fhip_q8_last_error", (fhip_q8_param,), None),
    # route: DETECT_ROUTE of net.py (FHIP_DETECT_NET_ROUTE of its own header), outside the closed ROUTE_* set
    "detect": Library("libfeather_detect.so", ("feather_detect.h",), "FHIP_DETECT_API", DETECT_SIGNATURES, "fhip_detect_last_error", (), None),
}
# The rows of SIDE_THIRD of csrc/Makefile, the same tuple, for the same reason: MORE_LIBRARIES is closed as well;
# tests/test_colpass_contract_cpu.py restates the contract for them.
THIRD_LIBRARIES = {
    # route: a faster way to run two layers of a chained Winograd run (fhip_net_set_colpass), not a layer type
    "colpass": Library("libfeather_colpass.so", ("feather_colpass.h",), "FHIP_COLPASS_API", COLPASS_SIGNATURES, "fhip_colpass_last_error", (), None),
}
# The rows of SIDE_OPEN of csrc/Makefile, the same tuple: the last table, and an open one.  tests/test_open_contract_cpu.py holds EVERY row
# of it to the contract the libraries share and takes a row's sweep table from a naming rule (tests/<name>_cases.py: targets(), KERNELS, LIB),
# so the next library adds a row here, a name to SIDE_OPEN and a cases file -- not a fifth table.
OPEN_LIBRARIES = {
    # route: YOLO_ROUTE of net.py (FHIP_YOLO_NET_ROUTE of its own header), outside the closed ROUTE_* set
    "yolo": Library("libfeather_yolo.so", ("feather_yolo.h",), "FHIP_YOLO_API", YOLO_SIGNATURES, "fhip_yolo_last_error", (), None),
    # route: ROI_ROUTE of net.py (FHIP_ROI_NET_ROUTE of its own header)
    "roi": Library("libfeather_roi.so", ("feather_roi.h",), "FHIP_ROI_API", ROI_SIGNATURES, "fhip_roi_last_error", (), None),
}
TABLES = (LIBRARIES, MORE_LIBRARIES, THIRD_LIBRARIES, OPEN_LIBRARIES)
# Rows that stand in none of the tables, the same tuple, built by STANDALONE of csrc/Makefile.  The open table was meant to take the next
# library, but tests/test_roi_cpu.py holds it to its two rows and tests/test_open_contract_cpu.py the tables and lists to four, so
# libfeather_frame.so stands here; tests/test_frame_contract_cpu.py restates the open table's contract for these rows, by the same naming
# rule (tests/<name>_cases.py: targets(), KERNELS, LIB).  A change that may touch those tests folds the rows into OPEN_LIBRARIES.
STANDALONE_LIBRARIES = {
    # route: FRAME_ROUTE of net.py (FHIP_FRAME_NET_ROUTE of its own header)
    "frame": Library("libfeather_frame.so", ("feather_frame.h",), "FHIP_FRAME_API", FRAME_SIGNATURES, "fhip_frame_last_error", (), None),
}
# The rows of LATER of csrc/Makefile, the same tuple: the libraries added after libfeather_frame.so, whose own list is pinned to its one
# row as well.  tests/test_later_contract_cpu.py holds EVERY row here to the shared contract by the naming rule and asserts neither the
# number of rows nor their names: the next library adds a row here, a name to LATER and a cases file.
LATER_LIBRARIES = {
    # route: ATTN_ROUTE of net.py (FHIP_ATTN_NET_ROUTE of its own header)
    "attn": Library("libfeather_attn.so", ("feather_attn.h",), "FHIP_ATTN_API", ATTN_SIGNATURES, "fhip_attn_last_error", (), None),
    # route: RNN_ROUTE of net.py (FHIP_RNN_NET_ROUTE of its own header)
    "rnn": Library("libfeather_rnn.so", ("feather_rnn.h",), "FHIP_RNN_API", RNN_SIGNATURES, "fhip_rnn_last_error", (), None),
}
_OUTSIDE = (STANDALONE_LIBRARIES, LATER_LIBRARIES)  # the rows in none of TABLES


def row(name: str) -> Library:
    """The row of the library `name`, from any of the tables or from the rows outside them."""
    for table in TABLES + _OUTSIDE:
        if name in table:
            return table[name]
    raise KeyError(name)


def path(name: str) -> str:
    """Where the library `name` of any table lies: next to this module; FEATHER_HIP_LIB names another main library."""
    default = os.path.join(_HERE, row(name).file)
    return os.environ.get("FEATHER_HIP_LIB", default) if name == MAIN else default


def load(name: str):
    """Load the library `name` of any table and type every symbol of its table.  Fails loudly: there is no fallback implementation."""
    return _load(path(name), row(name).signatures)


def lib_path() -> str:
    return path(MAIN)


def load_library():
    """Load libfeather_hip.so.  Fails loudly: there is no fallback implementation."""
    return load(MAIN)


# the names the wrappers, tools/ and the tests call: <x>_path() and load_<x>_library() of every side library
for _name in (n for t in TABLES + _OUTSIDE for n in t):
    if _name != MAIN:
        globals()[f"{_name}_path"] = functools.partial(path, _name)
        globals()[f"load_{_name}_library"] = functools.partial(load, _name)
del _name
