"""Python host-side mirror of ``feather::Net`` (reference src/net.h:30-70, src/net.cpp) over the C-ABI in
``include/feather_hip/feather_net.h``: ``LoadParam`` / ``LoadWeights`` / ``FeedInput`` / ``Forward`` / ``Extract`` with the
reference's names, plus the batch dimension.  Blobs live in HBM; the wrapper only moves pointers.  No fallback path."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .booster import ALGO_NAMES, FeatherHipError, _check, _stream


# fhip_net_layer_info's route codes: booster::ConvAlgo, plus FHIP_NET_ROUTE_GCONV (feather_net.h) for a layer with 1 < group < C
ROUTE_GCONV = 100
ROUTE_NAMES = dict(ALGO_NAMES)
ROUTE_NAMES[ROUTE_GCONV] = "GCONV"
ROUTE_DECONV = 101  # FHIP_NET_ROUTE_DECONV: a Deconvolution / DeconvolutionDepthWise layer (libfeather_deconv.so)
ROUTE_NAMES[ROUTE_DECONV] = "DECONV"
ROUTE_INORM = 102  # FHIP_NET_ROUTE_INORM: an InstanceNorm layer (libfeather_inorm.so)
ROUTE_NAMES[ROUTE_INORM] = "INORM"
ROUTE_SHUFFLE = 103  # FHIP_NET_ROUTE_SHUFFLE: a ShuffleChannel / Slice layer or a collapsed run of them with Concat (libfeather_shuffle.so)
ROUTE_NAMES[ROUTE_SHUFFLE] = "SHUFFLE"
ROUTE_ATROUS = 104  # FHIP_NET_ROUTE_ATROUS: a Convolution layer with dilation > 1, after SetDilated(True) (libfeather_atrous.so)
ROUTE_NAMES[ROUTE_ATROUS] = "ATROUS"
ROUTE_GATE = 105  # FHIP_NET_ROUTE_GATE: a two-bottom BinaryOp mul / Scale -233, Swish, HardSigmoid, or a collapsed SE block (libfeather_gate.so)
ROUTE_NAMES[ROUTE_GATE] = "GATE"
ROUTE_RESAMPLE = 106  # FHIP_NET_ROUTE_RESAMPLE: an Interp or HardSwish layer, after SetExtendedLayers(True) (libfeather_resample.so)
ROUTE_NAMES[ROUTE_RESAMPLE] = "RESAMPLE"
ROUTE_LRN = 107  # FHIP_NET_ROUTE_LRN: an LRN layer, alone or with the Pooling layer behind it, after SetExtendedLayers(True) (libfeather_lrn.so)
ROUTE_NAMES[ROUTE_LRN] = "LRN"
ROUTE_QCONV = 108  # FHIP_NET_ROUTE_QCONV: a Convolution / InnerProduct layer with int8 weights, after SetQuantized(True) (libfeather_qconv.so)
ROUTE_NAMES[ROUTE_QCONV] = "QCONV"
DETECT_ROUTE = 109  # FHIP_DETECT_NET_ROUTE (feather_detect.h): a layer of an SSD detection head, after SetDetection(True) (libfeather_detect.so)
ROUTE_NAMES[DETECT_ROUTE] = "DETECT"
YOLO_ROUTE = 110  # FHIP_YOLO_NET_ROUTE (feather_yolo.h): a layer of a YOLO head, after SetYolo() (libfeather_yolo.so)
ROUTE_NAMES[YOLO_ROUTE] = "YOLO"
ROI_ROUTE = 111  # FHIP_ROI_NET_ROUTE (feather_roi.h): Proposal, ROIPooling, ROIAlign or PSROIPooling, after SetRoi() (libfeather_roi.so)
ROUTE_NAMES[ROI_ROUTE] = "ROI"
FRAME_ROUTE = 112  # FHIP_FRAME_NET_ROUTE (feather_frame.h): Padding, Crop or PixelShuffle, after SetFrame() (libfeather_frame.so)
ROUTE_NAMES[FRAME_ROUTE] = "FRAME"
ATTN_ROUTE = 113  # FHIP_ATTN_NET_ROUTE (feather_attn.h): MemoryData, LayerNorm, GELU, MultiHeadAttention or an element-wise BinaryOp, after SetTransformer() (libfeather_attn.so)
ROUTE_NAMES[ATTN_ROUTE] = "ATTN"
RNN_ROUTE = 114  # FHIP_RNN_NET_ROUTE (feather_rnn.h): LSTM, GRU or RNN, after SetRecurrent() (libfeather_rnn.so)
ROUTE_NAMES[RNN_ROUTE] = "RNN"

class Net:
    def __init__(self, fusion: int = 1, graph: bool = False, stream=None, tuned: bool = False, concurrency: bool = False,
                 sub_batches: int = 1):
        self._lib = _lib.load_library()
        h = ctypes.c_void_p()
        _check(self._lib.fhip_net_create(ctypes.byref(h)), "fhip_net_create")
        self._h = h
        _check(self._lib.fhip_net_set_fusion(h, int(fusion)), "fhip_net_set_fusion")
        _check(self._lib.fhip_net_set_graph(h, int(bool(graph))), "fhip_net_set_graph")
        _check(self._lib.fhip_net_set_tuned_selection(h, int(bool(tuned))), "fhip_net_set_tuned_selection")
        _check(self._lib.fhip_net_set_concurrency(h, int(bool(concurrency))), "fhip_net_set_concurrency")
        if stream is not None:
            _check(self._lib.fhip_net_set_stream(h, ctypes.c_void_p(stream)), "fhip_net_set_stream")
        if sub_batches != 1:  # replicas of the net on streams of their own, each taking a share of every batch (feather_net.h)
            _check(self._lib.fhip_net_set_sub_batches(h, int(sub_batches)), "fhip_net_set_sub_batches")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.fhip_net_destroy(self._h)
            self._h = None

    __del__ = close

    def SetDilated(self, on: bool = True):
        """feather::Net::SetDilated: accept Convolution layers with dilation > 1 (routed to libfeather_atrous.so) instead of refusing them
        at LoadParam.  Call before LoadParam."""
        _check(self._lib.fhip_net_set_dilated(self._h, int(bool(on))), "fhip_net_set_dilated")

    def SetQuantized(self, on: bool = True):
        """feather::Net::SetQuantized: accept Convolution, ConvolutionDepthWise and InnerProduct layers with int8 weights (ncnn's
        int8_scale_term; routed to libfeather_qconv.so) instead of refusing them at LoadParam.  Call before LoadParam."""
        _check(self._lib.fhip_net_set_quantized(self._h, int(bool(on))), "fhip_net_set_quantized")

    def SetRequantized(self, on: bool = True):
        """feather::Net::SetRequantized: with SetQuantized, accept int8 Convolution / ConvolutionDepthWise layers with a requantised int8
        output (int8_scale_term 101 .. 200) instead of refusing them at LoadParam; the activation between two int8 layers then stays int8
        on the device (routed to libfeather_q8.so, reported as QCONV).  Call before LoadParam."""
        _check(self._lib.fhip_net_set_requantized(self._h, int(bool(on))), "fhip_net_set_requantized")

    def SetExtendedLayers(self, on: bool = True):
        """feather::Net::SetExtendedLayers: accept Interp and HardSwish layers (routed to libfeather_resample.so) and LRN layers
        (libfeather_lrn.so) instead of refusing them
        at LoadParam.  Call before LoadParam."""
        _check(self._lib.fhip_net_set_extended_layers(self._h, int(bool(on))), "fhip_net_set_extended_layers")

    def SetDetection(self, on: bool = True):
        """feather::Net::SetDetection: accept the layers of ncnn's SSD detection head -- Permute, Flatten, Reshape, Normalize, PriorBox,
        DetectionOutput, and Concat / Softmax along any axis of a blob's rank (routed to libfeather_detect.so) -- instead of refusing them at
        LoadParam.  Call before LoadParam."""
        _check(self._lib.fhip_net_set_detection(self._h, int(bool(on))), "fhip_net_set_detection")

    def SetYolo(self, rows: int = 256):
        """feather::Net::SetYolo: accept the layers of ncnn's YOLO heads -- Reorg, YoloDetectionOutput and Yolov3DetectionOutput (routed to
        libfeather_yolo.so) -- instead of refusing them at LoadParam.  `rows` (1 .. 1024) is the height of the detection top: the first `rows`
        detections of every image, read by ExtractDetections; 0 switches the layers off again.  Call before LoadParam."""
        _check(self._lib.fhip_net_set_yolo(self._h, int(rows)), "fhip_net_set_yolo")

    def SetRoi(self, on: bool = True):
        """feather::Net::SetRoi: accept the layers of ncnn's two-stage detectors -- Proposal, ROIPooling, ROIAlign and PSROIPooling (routed to
        libfeather_roi.so) -- instead of refusing them at LoadParam.  im_info is a second Input: FeedInput(name, [N][1][1][3]) with (height,
        width, scale) per image.  Call before LoadParam."""
        _check(self._lib.fhip_net_set_roi(self._h, int(bool(on))), "fhip_net_set_roi")

    def SetFrame(self, on: bool = True):
        """feather::Net::SetFrame: accept ncnn's Padding, Crop and PixelShuffle (routed to libfeather_frame.so) instead of refusing them at
        LoadParam.  Call before LoadParam."""
        _check(self._lib.fhip_net_set_frame(self._h, int(bool(on))), "fhip_net_set_frame")

    def SetTransformer(self, on: bool = True):
        """feather::Net::SetTransformer: accept ncnn's MemoryData, LayerNorm, GELU, MultiHeadAttention and the element-wise BinaryOp (routed to
        libfeather_attn.so) and run an InnerProduct on a [T][F] blob once per token, instead of refusing them at LoadParam.  Needs
        SetDetection() too (blob ranks).  Call before LoadParam."""
        _check(self._lib.fhip_net_set_transformer(self._h, int(bool(on))), "fhip_net_set_transformer")

    def SetRecurrent(self, on: bool = True):
        """feather::Net::SetRecurrent: accept ncnn's LSTM, GRU and RNN (routed to libfeather_rnn.so) instead of refusing them at LoadParam.
        Needs SetDetection() too (blob ranks).  Call before LoadParam."""
        _check(self._lib.fhip_net_set_recurrent(self._h, int(bool(on))), "fhip_net_set_recurrent")

    def set_graph(self, on: bool):
        _check(self._lib.fhip_net_set_graph(self._h, int(bool(on))), "fhip_net_set_graph")

    def set_tuned(self, on: bool):
        """fhip_net_set_tuned_selection, legal between Forwards: the routes are chosen again at the next Forward."""
        _check(self._lib.fhip_net_set_tuned_selection(self._h, int(bool(on))), "fhip_net_set_tuned_selection")

    def SetColpass(self, mode: int = 1):
        """feather::Net::SetColpass (fhip_net_set_colpass), legal between Forwards: how chained Winograd layers with 64 input channels run their
        tile GEMM and boundary -- 0 on the main route, 1 through libfeather_colpass.so where M is HBM-bound (default), 2 wherever the library
        accepts the layer.  Planned again (and a captured graph dropped) at the next Forward."""
        _check(self._lib.fhip_net_set_colpass(self._h, int(mode)), "fhip_net_set_colpass")

    def set_concurrency(self, on: bool):
        """fhip_net_set_concurrency, legal between Forwards: the side stream is planned again (and a captured graph dropped) at the next Forward."""
        _check(self._lib.fhip_net_set_concurrency(self._h, int(bool(on))), "fhip_net_set_concurrency")

    def use_current_stream(self):
        """Enqueue on torch's current stream (so torch events and tensors order against the net's work)."""
        _check(self._lib.fhip_net_set_stream(self._h, _stream()), "fhip_net_set_stream")

    # -- reference API ------------------------------------------------------------------------------------------
    def LoadParam(self, param) -> int:
        """Net::LoadParam (net.cpp:54-170): a path, or the .param text itself as bytes."""
        if isinstance(param, bytes):
            _check(self._lib.fhip_net_load_param_mem(self._h, param, len(param)), "fhip_net_load_param_mem")
        else:
            _check(self._lib.fhip_net_load_param(self._h, str(param).encode()), "fhip_net_load_param")
        return 0

    def LoadWeights(self, weights) -> int:
        """Net::LoadWeights (net.cpp:172-233): a path, or the .bin image as bytes."""
        if isinstance(weights, (bytes, bytearray, memoryview)):
            buf = (ctypes.c_char * len(weights)).from_buffer_copy(weights)
            _check(self._lib.fhip_net_load_weights_mem(self._h, buf, len(weights)), "fhip_net_load_weights_mem")
        else:
            _check(self._lib.fhip_net_load_weights(self._h, str(weights).encode()), "fhip_net_load_weights")
        return 0

    def FeedInput(self, input_name: str, data) -> int:
        """Net::FeedInput (net.cpp:235-246) with a batch: `data` is [N][C][H][W] (or [C][H][W]) fp32, a numpy array
        (host) or a torch CUDA tensor (device, copied device-to-device)."""
        import torch
        if isinstance(data, torch.Tensor) and data.is_cuda:
            t = data.contiguous().float()
            torch.cuda.current_stream().synchronize()  # the net's stream may differ from the producer's
            shape, ptr, dev = tuple(t.shape), ctypes.c_void_p(t.data_ptr()), 1
            keep = t
        else:
            a = np.ascontiguousarray(np.asarray(data, dtype=np.float32))
            shape, ptr, dev = a.shape, a.ctypes.data_as(ctypes.c_void_p), 0
            keep = a
        if len(shape) == 3:
            shape = (1,) + tuple(shape)
        if len(shape) != 4:
            raise FeatherHipError("FeedInput wants [N][C][H][W] or [C][H][W]")
        n, c, h, w = (int(v) for v in shape)
        _check(self._lib.fhip_net_feed_input(self._h, input_name.encode(), n, c, h, w, ptr, dev), "fhip_net_feed_input")
        self.synchronize()  # the host array / device tensor may be freed or overwritten by the caller
        del keep
        return 0

    def FeedPixels(self, input_name: str, pixels, ptype: int, target=None, mean=None, norm=None) -> int:
        """ncnn's Mat::from_pixels_resize (+ substract_mean_normalize) straight into the input blob, on the device
        (fhip_net_feed_pixels): `pixels` is uint8 [N][H][W][C] (or [H][W][C]), a numpy array (uploaded once as uint8) or a CUDA
        tensor; ptype a PIXEL_* code; target = (w, h), default the source size; mean / norm: one value per output channel, or None."""
        from .pixels import _images, _per_channel, pixel_channels
        import torch
        n, h, w, ptr, dev, keep = _images(pixels, ptype)
        tw, th = (w, h) if target is None else (int(target[0]), int(target[1]))
        _, cout = pixel_channels(ptype)
        m, mp = _per_channel(mean, cout, "mean")
        s, sp = _per_channel(norm, cout, "norm")
        if dev:
            torch.cuda.current_stream().synchronize()  # the net's stream may differ from the producer's
        _check(self._lib.fhip_net_feed_pixels(self._h, input_name.encode(), n, ptr, int(ptype), w, h, tw, th, mp, sp, dev),
               "fhip_net_feed_pixels")
        self.synchronize()  # the host array / device tensor may be freed or overwritten by the caller
        del keep, m, s
        return 0

    def FeedPixelImages(self, input_name: str, images, ptype: int, target, rois=None, mean=None, norm=None) -> int:
        """A mixed-size batch straight into the input blob, on the device (fhip_net_feed_pixel_images): `images` a list of uint8 [H][W][C]
        numpy arrays (each ROI's rows uploaded) or CUDA tensors, all of one kind; row-strided views are read in place.  rois: None or one
        (x, y, w, h) / None per image; target = (w, h); mean / norm: one value per output channel, or None.  Image i becomes
        from_pixels_resize of a dense copy of its ROI."""
        from .pixels import _image_descs, _per_channel, pixel_channels
        import torch
        descs, dev, keep = _image_descs(images, ptype, rois)
        tw, th = int(target[0]), int(target[1])
        _, cout = pixel_channels(ptype)
        m, mp = _per_channel(mean, cout, "mean")
        s, sp = _per_channel(norm, cout, "norm")
        if dev:
            torch.cuda.current_stream().synchronize()  # the net's stream may differ from the producer's
        _check(self._lib.fhip_net_feed_pixel_images(self._h, input_name.encode(), len(descs), descs, int(ptype), tw, th, mp, sp, dev),
               "fhip_net_feed_pixel_images")
        self.synchronize()  # the host arrays / device tensors may be freed or overwritten by the caller
        del keep, m, s
        return 0

    def FeedYUV420sp(self, input_name: str, frames, ptype: int = 1, target=None, resize_first: bool = True, mean=None, norm=None) -> int:
        """NV21 camera frames straight into the input blob, on the device (fhip_net_feed_yuv420sp): `frames` is uint8 [N][h*3/2][w] (or
        [h*3/2][w]), a numpy array (uploaded once as uint8) or a CUDA tensor; ptype PIXEL_RGB (1), PIXEL_RGB2BGR or PIXEL_RGB2GRAY;
        target = (w, h), default the frame size; resize_first picks the reference's chain (resize_bilinear_yuv420sp before
        yuv420sp2rgb, or from_pixels_resize after it); mean / norm: one value per output channel, or None."""
        from .pixels import _frames, _per_channel
        import torch
        n, w, h, cout, ptr, dev, keep = _frames(frames, ptype)
        tw, th = (w, h) if target is None else (int(target[0]), int(target[1]))
        m, mp = _per_channel(mean, cout, "mean")
        s, sp = _per_channel(norm, cout, "norm")
        if dev:
            torch.cuda.current_stream().synchronize()  # the net's stream may differ from the producer's
        _check(self._lib.fhip_net_feed_yuv420sp(self._h, input_name.encode(), n, ptr, w, h, tw, th, int(ptype), int(bool(resize_first)), mp,
                                                sp, dev), "fhip_net_feed_yuv420sp")
        self.synchronize()  # the host array / device tensor may be freed or overwritten by the caller
        del keep, m, s
        return 0

    def Forward(self) -> int:
        _check(self._lib.fhip_net_forward(self._h), "fhip_net_forward")
        return 0

    def Extract(self, blob_name: str) -> np.ndarray:
        """Net::Extract (net.cpp:263-296): the blob as a host [N][C][H][W] array (synchronises the stream)."""
        ptr, shape = self.ExtractDevice(blob_name)
        out = np.empty(shape, dtype=np.float32)
        _check(self._lib.fhip_net_extract_host(self._h, blob_name.encode(), out.ctypes.data_as(ctypes.c_void_p), out.size),
               "fhip_net_extract_host")
        return out

    def ExtractDetections(self, blob_name: str):
        """The top of a DetectionOutput layer as one (count_i, 6) array per image, rows (label, score, xmin, ymin, xmax, ymax): Extract, with
        the zero rows past every image's count trimmed on the host."""
        out = self.Extract(blob_name)
        if out.shape[1] != 1 or out.shape[3] != 6:
            raise FeatherHipError(f"blob {blob_name} of shape {out.shape} is not a DetectionOutput top [n][1][keep_top_k][6]")
        return [img[0][:int((img[0][:, 0] > 0).sum())].copy() for img in out]

    def ExtractProposals(self, rois_blob: str, scores_blob: str = None):
        """The top of a Proposal layer as one (count_i, 4) array per image, rows (x1, y1, x2, y2): Extract, with the sentinel rows (0, 0, -1, -1)
        past every image's count trimmed on the host.  With `scores_blob` (the layer's second top): (rois, scores), the scores one (count_i,)
        array per image."""
        out = self.Extract(rois_blob)
        if out.shape[2] != 1 or out.shape[3] != 4:
            raise FeatherHipError(f"blob {rois_blob} of shape {out.shape} is not a Proposal top [n][R][1][4]")
        rows = out[:, :, 0]
        counts = [int((img[:, 2] >= img[:, 0]).sum()) for img in rows]
        rois = [img[:k].copy() for img, k in zip(rows, counts)]
        if scores_blob is None:
            return rois
        s = self.Extract(scores_blob)
        if s.shape != out.shape[:2] + (1, 1):
            raise FeatherHipError(f"blob {scores_blob} of shape {s.shape} is not the score top [n][R][1][1] of {rois_blob}")
        return rois, [img[:k, 0, 0].copy() for img, k in zip(s, counts)]

    def ExtractPixels(self, blob_name: str, ptype: int, target=None, mean=None, norm=None) -> np.ndarray:
        """The blob as uint8 images, converted on the device (fhip_float_to_pixels on the net's stream, after Forward): ncnn's
        substract_mean_normalize (when mean / norm are given, one value per channel) + Mat::to_pixels_resize of every image ->
        np.uint8 [N][target_h][target_w][C].  ptype: PIXEL_RGB, PIXEL_BGR, PIXEL_GRAY, PIXEL_RGBA, PIXEL_RGB2BGR or PIXEL_BGR2RGB, whose
        channels must be the blob's C; target = (w, h), default the blob's size.  Only the bytes cross the bus."""
        from .pixels import _check_pixout, _per_channel, output_channels
        cn = output_channels(ptype)
        ptr, (n, c, h, w) = self.ExtractDevice(blob_name)
        if c != cn:
            raise FeatherHipError(f"blob {blob_name} has {c} channels, pixel type {ptype:#x} needs {cn}")
        if not ptr:
            raise FeatherHipError(f"blob {blob_name} has no data yet (run Forward first)")
        tw, th = (w, h) if target is None else (int(target[0]), int(target[1]))
        m, mp = _per_channel(mean, cn, "mean")
        s, sp = _per_channel(norm, cn, "norm")
        stream = ctypes.c_void_p()
        _check(self._lib.fhip_net_get_stream(self._h, ctypes.byref(stream)), "fhip_net_get_stream")
        out = np.empty((n, th, tw, cn), dtype=np.uint8)
        _check_pixout(_lib.load_pixout_library().fhip_float_to_pixels_host(out.ctypes.data_as(ctypes.c_void_p), 0, ctypes.c_void_p(ptr), n,
                                                                           int(ptype), w, h, tw, th, mp, sp, stream),
                      "fhip_float_to_pixels_host")
        del m, s
        return out

    def ExtractDevice(self, blob_name: str):
        """(device pointer, (n, c, h, w)) of a blob -- the float** form of Net::Extract."""
        p = ctypes.c_void_p()
        dims = [ctypes.c_int() for _ in range(4)]
        _check(self._lib.fhip_net_extract(self._h, blob_name.encode(), ctypes.byref(p), *[ctypes.byref(d) for d in dims]),
               "fhip_net_extract")
        return p.value, tuple(d.value for d in dims)

    # -- introspection ------------------------------------------------------------------------------------------
    def synchronize(self):
        import torch
        torch.cuda.synchronize()  # device-wide: covers the net's own stream too

    def layers(self):
        out = []
        n = self._lib.fhip_net_layer_count(self._h)
        for i in range(n):
            t, nm, algo = ctypes.create_string_buffer(64), ctypes.create_string_buffer(256), ctypes.c_int()
            _check(self._lib.fhip_net_layer_info(self._h, i, t, nm, 64, ctypes.byref(algo)), "fhip_net_layer_info")
            out.append((t.value.decode(), nm.value.decode(), ROUTE_NAMES.get(algo.value)))
        return out

    def conv_params(self):
        """{layer index: (fhip_conv_param, batch)} for the convolution layers as they run (after Reshape)."""
        out = {}
        for i in range(self._lib.fhip_net_layer_count(self._h)):
            p, b = _lib.fhip_conv_param(), ctypes.c_int()
            if self._lib.fhip_net_layer_conv_param(self._h, i, ctypes.byref(p), ctypes.byref(b)) == 0:
                out[i] = (p, b.value)
        return out

    def fused_pointwise(self):
        """{layer index: (fhip_conv_param of the 1x1 convolution a depthwise layer absorbed, runs_as_one_kernel)} (fusion level 2)."""
        out = {}
        for i in range(self._lib.fhip_net_layer_count(self._h)):
            p, one = _lib.fhip_conv_param(), ctypes.c_int()
            if self._lib.fhip_net_layer_fused_pointwise(self._h, i, ctypes.byref(p), ctypes.byref(one)) == 0:
                out[i] = (p, bool(one.value))
        return out

    def siblings(self):
        """{layer index: 1 | 2} -- 1: this 1x1 convolution's launch also computes the next layer (fhip_conv_forward_siblings), 2: that next layer."""
        out = {}
        for i in range(self._lib.fhip_net_layer_count(self._h)):
            st = ctypes.c_int()
            if self._lib.fhip_net_layer_sibling(self._h, i, ctypes.byref(st)) == 0 and st.value:
                out[i] = st.value
        return out

    def residuals(self):
        """{layer index: 1 | 2} -- 1: the absorbed Eltwise SUM operand is added in this convolution's GEMM epilogue (one more output-sized read by
        the same launch, fhip_conv_forward_residual), 2: absorbed but added by a launch of its own (fhip_net_layer_residual)."""
        out = {}
        for i in range(self._lib.fhip_net_layer_count(self._h)):
            st = ctypes.c_int()
            if self._lib.fhip_net_layer_residual(self._h, i, ctypes.byref(st)) == 0 and st.value:
                out[i] = st.value
        return out

    def chains(self, raw=False):
        """{layer index: (v_from_previous, writes_next_v)} for the convolutions that are part of a chained Winograd run (fusion level 3).
        raw=True keeps the library's values: 2 marks the pair "first layer computed inside the next layer's input transform" -- (0, 2) on the
        first layer, which is not a Winograd layer and launches nothing, (2, x) on its consumer.  The boolean view (raw=False) is about chained
        Winograd layers only: the first layer is left out of it and the consumer's V is not "from the previous layer's chained transform"."""
        out = {}
        for i in range(self._lib.fhip_net_layer_count(self._h)):
            a, b = ctypes.c_int(), ctypes.c_int()
            if self._lib.fhip_net_layer_chain(self._h, i, ctypes.byref(a), ctypes.byref(b)) == 0 and (a.value or b.value):
                if raw:
                    out[i] = (a.value, b.value)
                elif a.value == 1 or b.value == 1:
                    out[i] = (a.value == 1, b.value == 1)
        return out

    def canvases(self):
        """[layer index] of the chained Winograd layers that run on 2x2 image canvases (fhip_net_layer_canvas; fusion level 3)."""
        out = []
        for i in range(self._lib.fhip_net_layer_count(self._h)):
            c = ctypes.c_int()
            if self._lib.fhip_net_layer_canvas(self._h, i, ctypes.byref(c)) == 0 and c.value:
                out.append(i)
        return out

    def colpasses(self):
        """[layer index] of the chained Winograd layers that run through libfeather_colpass.so (fhip_net_layer_colpass; fusion level 3)."""
        out = []
        for i in range(self._lib.fhip_net_layer_count(self._h)):
            c = ctypes.c_int()
            if self._lib.fhip_net_layer_colpass(self._h, i, ctypes.byref(c)) == 0 and c.value:
                out.append(i)
        return out

    def forward_timed(self):
        """One eager forward with HIP events around every layer: [(type, name, algo, ms)]."""
        n = self._lib.fhip_net_layer_count(self._h)
        ms = (ctypes.c_float * max(n, 1))()
        _check(self._lib.fhip_net_forward_timed(self._h, ms), "fhip_net_forward_timed")
        info = self.layers()  # fusion may have shrunk the list during the first forward
        return [(t, nm, a, ms[i]) for i, (t, nm, a) in enumerate(info)]

    def memory(self):
        v = [ctypes.c_size_t() for _ in range(3)]
        _check(self._lib.fhip_net_memory(self._h, *[ctypes.byref(x) for x in v]), "fhip_net_memory")
        return {"blob_bytes": v[0].value, "weight_bytes": v[1].value, "arena_bytes": v[2].value}


# ---- the layer kernels on torch CUDA tensors (tests and ad-hoc use) ---------------------------------------------
def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def relu(x):
    import torch
    y = torch.empty_like(x)
    _check(_lib.load_library().fhip_relu(_p(y), _p(x), x.numel(), _stream()), "fhip_relu")
    return y


def add(a, b, relu: bool = False):
    import torch
    y = torch.empty_like(a)
    _check(_lib.load_library().fhip_add(_p(y), _p(a), _p(b), a.numel(), int(relu), _stream()), "fhip_add")
    return y


def affine(x, mul, add_=None, relu: bool = False):
    import torch
    y = torch.empty_like(x)
    n, c, h, w = x.shape
    _check(_lib.load_library().fhip_affine(_p(y), _p(x), _p(mul), _p(add_), n, c, h * w, int(relu), _stream()),
           "fhip_affine")
    return y


def pool_param(c, h, w, kernel, stride=1, pad=(0, 0, 0, 0), pooling_type=0, global_pooling=False):
    """pad = (left, right, top, bottom) as PoolingLayer::LoadParam names them."""
    kh, kw = (kernel, kernel) if isinstance(kernel, int) else kernel
    sh, sw = (stride, stride) if isinstance(stride, int) else stride
    return _lib.fhip_pool_param(c, h, w, kh, kw, sh, sw, pad[0], pad[1], pad[2], pad[3], pooling_type, int(global_pooling))


def pooling(x, q):
    import torch
    oh, ow = ctypes.c_int(), ctypes.c_int()
    lib = _lib.load_library()
    _check(lib.fhip_pooling_output_dim(ctypes.byref(q), ctypes.byref(oh), ctypes.byref(ow)), "fhip_pooling_output_dim")
    y = torch.empty((x.shape[0], x.shape[1], oh.value, ow.value), device=x.device, dtype=torch.float32)
    _check(lib.fhip_pooling(ctypes.byref(q), x.shape[0], _p(y), _p(x), _stream()), "fhip_pooling")
    return y


def softmax(x):
    import torch
    y = torch.empty_like(x)
    _check(_lib.load_library().fhip_softmax(_p(y), _p(x), x.shape[0], x[0].numel(), _stream()), "fhip_softmax")
    return y
