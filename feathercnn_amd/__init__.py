"""feathercnn_amd -- MI355X (gfx950) native convolution hot path behind FeatherCNN's booster operator API.

The product is the C-ABI shared library ``libfeather_hip.so`` (declared in ``include/feather_hip/feather_hip.h``,
C++ host class in ``include/booster/booster.h``).  This package is the Python host-side mirror of that same
interface (``ConvParam`` / ``ConvBooster`` with the reference's method names) used by the tests and the bench;
PyTorch only provides device memory, streams and ``torch.distributed`` plumbing.

There is NO CPU fallback: importing works anywhere, but every compute call requires the HIP library and a GPU
and fails loudly otherwise.
"""
from .booster import (ALGO_NAMES, DEPTHWISE, IM2COL, NAIVE, SGECONV, WINOGRADF23, WINOGRADF63, WINOGRADF63FUSED,
                      ConvBooster, ConvLayer, ConvParam, FeatherHipError, None_, ReLU)
from ._lib import lib_path, load_library
from .atrous import AtrousConv, AtrousLayer, AtrousParam
from .deconv import Deconv, DeconvLayer, DeconvParam
from .detect import axis_softmax, detect_route, detection_output, normalize, permute, permute_concat, priorbox
from .gate import channel_gate, excite, gate_activation, squeeze
from .gconv import GroupedConv, GroupedConvLayer
from .inorm import activation, instance_norm, instance_norm_route
from .qconv import QuantConv, QuantParam, dequant_scales, qconv_route, quantize
from .q8 import Q8Conv, Q8Param, q8_max_pool, q8_pack, q8_relu, q8_route, q8_unpack
from .lrn import lrn, lrn_pool, lrn_pool_route, lrn_route
from .resample import hard_swish, interp, interp_output_dim, interp_route
from .shuffle import ChannelMap, channel_map, channel_shuffle, channel_slice
from .yolo import reorg, reorg_output_dim, yolo_detection, yolo_route
from .yolo import (CHUNK as YOLO_CHUNK, MAX_BOXES as YOLO_MAX_BOXES, MAX_CELLS as YOLO_MAX_CELLS, MAX_CLASSES as YOLO_MAX_CLASSES,
                   MAX_ROWS as YOLO_MAX_ROWS, MAX_SCALES as YOLO_MAX_SCALES, NET_ROUTE as YOLO_NET_ROUTE)
from .roi import generate_anchors, proposal, psroi_pool, roi_align, roi_pool, roi_route
from .roi import NET_ROUTE as ROI_NET_ROUTE
from .frame import crop, frame_route, pad, pixel_shuffle, pixel_shuffle_output_dim, window, window_output_dim
from .frame import NET_ROUTE as FRAME_NET_ROUTE
from .attn import add_layer_norm, attention, attn_route, binary, gelu, layer_norm
from .attn import NET_ROUTE as ATTN_NET_ROUTE
from .rnn import GRU, LSTM, RNN, recurrent, rnn_route
from .rnn import NET_ROUTE as RNN_NET_ROUTE
from .pixels import (PIXEL_BGR, PIXEL_BGR2GRAY, PIXEL_BGR2RGB, PIXEL_GRAY, PIXEL_GRAY2BGR, PIXEL_GRAY2RGB, PIXEL_RGB, PIXEL_RGB2BGR,
                     PIXEL_RGB2GRAY, PIXEL_RGBA, PIXEL_RGBA2BGR, PIXEL_RGBA2GRAY, PIXEL_RGBA2RGB, float_to_pixels, pixels_images_to_float,
                     pixels_to_float, yuv420sp_to_float)

__all__ = ["recurrent", "rnn_route", "LSTM", "GRU", "RNN", "RNN_NET_ROUTE", "attention", "layer_norm", "add_layer_norm", "gelu", "binary", "attn_route", "ATTN_NET_ROUTE", "pad", "crop", "window", "window_output_dim", "pixel_shuffle", "pixel_shuffle_output_dim", "frame_route", "FRAME_NET_ROUTE", "generate_anchors", "proposal", "roi_pool", "roi_align", "psroi_pool", "roi_route", "ROI_NET_ROUTE", "reorg", "reorg_output_dim", "yolo_detection", "yolo_route", "YOLO_NET_ROUTE", "YOLO_MAX_SCALES", "YOLO_MAX_BOXES", "YOLO_MAX_CLASSES",
           "YOLO_MAX_CELLS", "YOLO_MAX_ROWS", "YOLO_CHUNK", "permute", "permute_concat", "normalize", "priorbox", "axis_softmax", "detection_output", "detect_route", "Q8Conv", "Q8Param", "q8_pack", "q8_unpack", "q8_relu", "q8_max_pool", "q8_route", "QuantConv", "QuantParam", "quantize", "qconv_route", "dequant_scales", "ConvParam", "ConvBooster", "ConvLayer", "GroupedConv", "GroupedConvLayer", "Deconv", "DeconvLayer", "DeconvParam", "AtrousConv", "AtrousLayer", "AtrousParam", "instance_norm", "instance_norm_route", "activation", "channel_gate", "squeeze", "excite", "gate_activation", "interp", "interp_output_dim", "interp_route", "hard_swish", "lrn", "lrn_pool", "lrn_route", "lrn_pool_route", "channel_shuffle", "channel_slice", "channel_map", "ChannelMap", "FeatherHipError", "load_library", "lib_path", "NAIVE", "IM2COL",
           "SGECONV", "DEPTHWISE", "WINOGRADF63", "WINOGRADF63FUSED", "WINOGRADF23", "None_", "ReLU", "ALGO_NAMES", "pixels_to_float", "pixels_images_to_float", "float_to_pixels", "yuv420sp_to_float", "PIXEL_RGB", "PIXEL_BGR", "PIXEL_GRAY", "PIXEL_RGBA",
           "PIXEL_RGB2BGR", "PIXEL_RGB2GRAY", "PIXEL_BGR2RGB", "PIXEL_BGR2GRAY", "PIXEL_GRAY2RGB", "PIXEL_GRAY2BGR", "PIXEL_RGBA2RGB",
           "PIXEL_RGBA2BGR", "PIXEL_RGBA2GRAY"]
