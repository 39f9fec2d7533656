"""Synthetic ncnn-format models (``.param`` text + ``.bin`` weights) of the benchmark networks.

The reference ships no model files and there is no network, so whole-net runs use the standard public architectures
with seeded random weights written in the format ``feather::Net`` loads (reference
src/net.cpp:67-170, src/ncnn/paramdict.cpp:92-174, src/ncnn/modelbin.cpp:47-197).  The same files feed the reference
``feather::Net`` (the CPU checker of the tests) and this package's ``Net``.

Weight distribution: He-uniform ``U(-1,1)*sqrt(6/fan_in)`` so activations keep O(1) magnitude through 50 layers;
bias ``U(-0.1,0.1)``; BatchNorm slope/var ``U(0.5,1.5)``, mean/bias ``U(-0.1,0.1)``.
"""
from __future__ import annotations

import struct

import numpy as np


INT8_TAG = 0x000D4B38           # ncnn's tag of int8 weights (modelbin.cpp)
QUANT_DEFAULT_SCALE = 32.0      # input scale of a quantised layer that has no calibrated one: activations of order 1 use a quarter of the q range


def _round_half_away(t):
    a = np.abs(t)
    f = np.floor(a)
    return np.where(np.signbit(t), -1, 1) * np.where(a - f >= 0.5, f + 1, f)


def quantize_weights(w, cout):
    """fp32 weights [cout][...] -> (int8 weights, per-channel scales 127 / absmax(w[k]); 0 for an all-zero filter): ncnn's rule."""
    w = np.asarray(w, np.float32).reshape(cout, -1)
    amax = np.abs(w).max(axis=1)
    with np.errstate(divide="ignore"):
        s_w = np.where(amax == 0, np.float32(0), np.float32(127) / amax).astype(np.float32)
    q = np.clip(_round_half_away(w * s_w[:, None]), -127, 127).astype(np.int8)
    return q, s_w


class GraphBuilder:
    def __init__(self, seed: int = 1234, dry: bool = False, quant=None, requant=None):
        """dry=True: build the .param only and count the .bin bytes (``nbytes``) without drawing any weights.
        quant: None writes fp32 layers; a dict {layer name: input scale} makes conv() and fc() write int8 layers (param 8=1: int8-tagged
        weights quantised per output channel, the bias, the weight scales, one input scale; a name the dict lacks gets QUANT_DEFAULT_SCALE).
        The weights drawn are those of the fp32 build with the same seed.  A net that holds such a layer needs Net.SetQuantized(True).
        conv(), fc() and se_block() take a `quant=` of their own for ONE layer of an otherwise fp32 (or int8) net: None keeps the build's
        setting, False writes fp32, True int8 at QUANT_DEFAULT_SCALE, a number int8 at that input scale."""
        self.quant = quant
        self.requant = requant  # {layer name: output scale}: conv() writes those layers of an int8 build with a requantised int8 output
        self.trace = None  # a list: conv / fc / relu / bn / scale / pool record themselves for numpy_forward (input_scales)
        self.rng = np.random.default_rng(seed)
        self.lines: list[str] = []
        self.bin = bytearray()
        self.blob_count = 0
        self.dry = dry
        self.nbytes = 0

    # -- low level ----------------------------------------------------------------------------------------------
    def layer(self, type_, name, bottoms, tops, params=None):
        kv = " ".join(f"{k}={v}" for k, v in (params or {}).items())
        self.lines.append(f"{type_} {name} {len(bottoms)} {len(tops)} {' '.join(list(bottoms) + list(tops))} {kv}".rstrip())
        self.blob_count += len(tops)
        return tops[0] if tops else None

    def _tagged(self, a):  # mb.load(n, 0): 4-byte zero tag + raw fp32
        self.nbytes += 4
        if not self.dry:
            self.bin += struct.pack("<I", 0)
        self._raw(a)

    def _raw(self, a):  # mb.load(n, 1)
        if self.dry:
            self.nbytes += 4 * a
        else:
            self.bin += np.ascontiguousarray(a, dtype="<f4").tobytes()
            self.nbytes += 4 * a.size

    def _note(self, *op):
        if self.trace is not None:
            self.trace.append(op)

    def _scale_of(self, name, quant):
        """The int8 input scale of layer `name`, or None for a fp32 layer: the layer's own `quant=` where it gives one, else the build's."""
        if quant is None:
            return None if self.quant is None else self.quant.get(name, QUANT_DEFAULT_SCALE)
        if quant is False:
            return None
        return QUANT_DEFAULT_SCALE if quant is True else float(quant)

    def _weights(self, name, w, cout, b, s_in=None, s_out=None):
        """The .bin of a conv / fc layer: tagged fp32 weights and the raw bias, or (with an input scale `s_in`) the int8 form (see __init__);
        with `s_out` one more raw fp32 behind it, the output scale of a requantised layer."""
        if s_in is None:
            self._tagged(w)
            if b is not None:
                self._raw(b)
            return
        wsize = w if self.dry else w.size
        self.nbytes += 4 + (wsize + 3) // 4 * 4
        s_w = cout
        if not self.dry:
            q, s_w = quantize_weights(w, cout)
            self.bin += struct.pack("<I", INT8_TAG) + q.tobytes() + bytes(-wsize % 4)
        if b is not None:
            self._raw(b)
        self._raw(s_w)
        self._raw(1 if self.dry else np.array([s_in], np.float32))
        if s_out is not None:
            self._raw(1 if self.dry else np.array([s_out], np.float32))

    def _uniform(self, n, lo, hi, scale=None):
        if self.dry:
            return n
        a = self.rng.uniform(lo, hi, size=n).astype(np.float32)
        return a if scale is None else a * np.float32(scale)

    # -- layers -------------------------------------------------------------------------------------------------
    def input(self, name, c, h, w):
        return self.layer("Input", name, [], [name], {0: w, 1: h, 2: c})

    def conv(self, name, bottom, cin, cout, k, s=1, p=0, group=1, bias=True, top=None, type_=None, dilation=1, gain=1.0, quant=None, requant=None):
        """requant=<scale>: an int8 layer whose output is requantised to int8 at that scale (param 8=101 and one more scale in the .bin, what
        ncnn2int8's fuse_requantize writes); a net that holds one needs Net.SetQuantized(True) and Net.SetRequantized(True)."""
        if requant is None and self.requant:
            requant = self.requant.get(name)
        fan_in = cin // group * k * k
        wsize = cout * (cin // group) * k * k
        type_ = type_ or ("ConvolutionDepthWise" if group > 1 else "Convolution")  # what ncnn's converter writes; both load alike
        params = {0: cout, 1: k, 3: s, 4: p, 5: int(bias), 6: wsize, 7: group}
        if dilation != 1:  # ncnn's id 2 (written only when set); a net that holds one needs Net.SetDilated(True)
            params = {0: cout, 1: k, 2: dilation, 3: s, 4: p, 5: int(bias), 6: wsize, 7: group}
        s_in = self._scale_of(name, quant)
        if s_in is not None:
            params[8] = 1 if requant is None else 101
        elif requant is not None:
            raise ValueError(f"layer {name}: only an int8 layer has a requantised output")
        top = self.layer(type_, name, [bottom], [top or name], params)
        w = self._uniform(wsize, -1, 1, np.sqrt(6.0 / fan_in) * gain)
        b = self._uniform(cout, -0.1, 0.1) if bias else None
        self._weights(name, w, cout, b, s_in, None if requant is None else float(requant))
        if self.trace is not None:
            self._note("conv", name, bottom, top, dict(w=w.reshape(cout, cin // group, k, k), b=b, s=s, p=p, group=group))
        return top

    def deconv(self, name, bottom, cin, cout, k, s=1, p=0, op=0, group=1, bias=True):
        """ncnn's Deconvolution (DeconvolutionDepthWise with a group): weights [cout][cin/group][k][k], not flipped; `op` = output padding
        on the right / bottom (ids 18 / 19).  He-uniform over the taps that reach one output, ceil(k / s) per axis."""
        fan_in = cin // group * (-(-k // s)) ** 2
        wsize = cout * (cin // group) * k * k
        params = {0: cout, 1: k, 3: s, 4: p, 5: int(bias), 6: wsize}
        if op:
            params.update({18: op, 19: op})
        if group > 1:
            params[7] = group
        top = self.layer("DeconvolutionDepthWise" if group > 1 else "Deconvolution", name, [bottom], [name], params)
        self._tagged(self._uniform(wsize, -1, 1, np.sqrt(6.0 / fan_in)))
        if bias:
            self._raw(self._uniform(cout, -0.1, 0.1))
        return top

    def deconv_bn_relu(self, name, bottom, cin, cout, k, s=1, p=0, op=0):
        x = self.deconv(name, bottom, cin, cout, k, s, p, op)
        x = self.bn(name + "_bn", x, cout)
        x = self.scale(name + "_scale", x, cout)
        return self.relu(name + "_relu", x)

    def relu(self, name, bottom, slope=None):
        """slope: ncnn's leaky ReLU (param 0); None writes no params, the plain layer."""
        self._note("relu", name, bottom, name, dict(slope=slope))
        return self.layer("ReLU", name, [bottom], [name], None if slope is None else {0: f"{slope:.6f}"})

    def instance_norm(self, name, bottom, c, eps=1e-3, affine=True):
        """ncnn's InstanceNorm: gamma U(0.5, 1.5) and beta U(-0.1, 0.1), raw fp32, only when affine."""
        top = self.layer("InstanceNorm", name, [bottom], [name], {0: c, 1: f"{eps:.6e}", 2: int(affine)})
        if affine:
            self._raw(self._uniform(c, 0.5, 1.5))
            self._raw(self._uniform(c, -0.1, 0.1))
        return top

    def prelu(self, name, bottom, num_slope):
        top = self.layer("PReLU", name, [bottom], [name], {0: num_slope})
        self._raw(self._uniform(num_slope, 0.05, 0.35))
        return top

    def tanh(self, name, bottom):
        return self.layer("TanH", name, [bottom], [name])

    def sigmoid(self, name, bottom):
        return self.layer("Sigmoid", name, [bottom], [name])

    def clip(self, name, bottom, lo, hi):
        return self.layer("Clip", name, [bottom], [name], {0: f"{lo:.6f}", 1: f"{hi:.6f}"})

    def conv_in_relu(self, name, bottom, cin, cout, k, s=1, p=0, relu=True, slope=None):
        x = self.conv(name, bottom, cin, cout, k, s, p)
        x = self.instance_norm(name + "_in", x, cout)
        return self.relu(name + "_relu", x, slope) if relu else x

    def deconv_in_relu(self, name, bottom, cin, cout, k, s=1, p=0, op=0):
        x = self.deconv(name, bottom, cin, cout, k, s, p, op)
        x = self.instance_norm(name + "_in", x, cout)
        return self.relu(name + "_relu", x)

    def pool(self, name, bottom, k=2, s=2, p=0, avg=False, global_=False):
        self._note("pool", name, bottom, name, dict(k=k, s=s, p=p, avg=avg, global_=global_))
        return self.layer("Pooling", name, [bottom], [name], {0: int(avg), 1: k, 2: s, 3: p, 4: int(global_)})

    def fc(self, name, bottom, cin, cout, bias=True, gain=1.0, quant=None):
        params = {0: cout, 1: int(bias), 2: cin * cout}
        s_in = self._scale_of(name, quant)
        if s_in is not None:
            params[8] = 1
        top = self.layer("InnerProduct", name, [bottom], [name], params)
        w = self._uniform(cin * cout, -1, 1, np.sqrt(6.0 / cin) * gain)
        b = self._uniform(cout, -0.1, 0.1) if bias else None
        self._weights(name, w, cout, b, s_in)
        if self.trace is not None:
            self._note("fc", name, bottom, top, dict(w=w.reshape(cout, cin), b=b))
        return top

    def bn(self, name, bottom, c, eps=1e-5):
        top = self.layer("BatchNorm", name, [bottom], [name], {0: c, 1: f"{eps:.6e}"})
        slope, mean, var, bias = self._uniform(c, 0.5, 1.5), self._uniform(c, -0.1, 0.1), self._uniform(c, 0.5, 1.5), self._uniform(c, -0.1, 0.1)
        for a in (slope, mean, var, bias):
            self._raw(a)
        if self.trace is not None:
            root = np.sqrt(var + np.float32(eps))
            self._note("affine", name, bottom, top, dict(mul=slope / root, add=bias - slope * mean / root))
        return top

    def scale(self, name, bottom, c, bias=True):
        top = self.layer("Scale", name, [bottom], [name], {0: c, 1: int(bias)})
        mul = self._uniform(c, 0.5, 1.5)
        self._raw(mul)
        add = self._uniform(c, -0.1, 0.1) if bias else None
        if bias:
            self._raw(add)
        if self.trace is not None:
            self._note("affine", name, bottom, top, dict(mul=mul, add=add if bias else np.zeros(c, np.float32)))
        return top

    def split(self, name, bottom, n=2):
        tops = [f"{name}_{i}" for i in range(n)]
        self._note("split", name, bottom, tops, {})
        self.layer("Split", name, [bottom], tops)
        return tops

    def eltwise(self, name, a, b):
        return self.layer("Eltwise", name, [a, b], [name], {0: 1})

    def concat(self, name, bottoms, axis=0, rank=None):
        """axis: relative to the bottoms' rank; anything but 0 on blobs of rank 3 needs Net.SetDetection(True).  rank: the bottoms' rank where it
        is not 3, for numpy_forward."""
        self._note("concat", name, list(bottoms), name, dict(axis=axis) if rank is None else dict(axis=axis, rank=rank))
        return self.layer("Concat", name, list(bottoms), [name], {0: axis})

    # -- the SSD detection head (a net that holds one of these needs Net.SetDetection(True)) ------------------------
    def permute(self, name, bottom, order):
        """ncnn's Permute: 0=order_type (3: NCHW -> NHWC)."""
        self._note("permute", name, bottom, name, dict(order=int(order)))
        return self.layer("Permute", name, [bottom], [name], {0: int(order)})

    def flatten(self, name, bottom):
        return self.layer("Flatten", name, [bottom], [name])

    def reshape(self, name, bottom, w, h=None, c=None):
        """ncnn's Reshape: 0=w 1=h 2=c, an absent id = the dimension does not exist, 0 = the bottom's extent, -1 = inferred."""
        params = {0: int(w)}
        if h is not None:
            params[1] = int(h)
        if c is not None:
            params[2] = int(c)
        self._note("reshape", name, bottom, name, dict(w=int(w), h=h, c=c))
        return self.layer("Reshape", name, [bottom], [name], params)

    def normalize(self, name, bottom, c, scale=20.0, eps=1e-10, channel_shared=False):
        """ncnn's Normalize in its SSD form (conv4_3_norm): across channels, per pixel, one learnt scale per channel drawn around `scale`."""
        n = 1 if channel_shared else c
        top = self.layer("Normalize", name, [bottom], [name], {0: 0, 1: int(channel_shared), 2: f"{eps:.6e}", 3: n, 4: 1})
        self._raw(self._uniform(n, 0.9 * scale, 1.1 * scale))
        return top

    def priorbox(self, name, bottom, image, min_sizes, max_sizes=(), ratios=(), flip=True, clip=False, variances=(0.1, 0.1, 0.2, 0.2), offset=0.5,
                 step=None):
        """ncnn's PriorBox: bottoms (feature map, image blob); steps and image extents come from the bottoms unless `step` is given."""
        arr = lambda v: ",".join([str(len(v))] + [f"{float(x):.6f}" for x in v])
        params = {-23300: arr(min_sizes)}
        if len(max_sizes):
            params[-23301] = arr(max_sizes)
        if len(ratios):
            params[-23302] = arr(ratios)
        params.update({3 + k: f"{variances[k]:.6f}" for k in range(4)})
        params.update({7: int(flip), 8: int(clip), 9: -233, 10: -233, 11: f"{-233.0 if step is None else step:.6f}",
                       12: f"{-233.0 if step is None else step:.6f}", 13: f"{offset:.6f}"})
        return self.layer("PriorBox", name, [bottom, image], [name], params)

    def detection_output(self, name, loc, conf, prior, num_class, nms_threshold=0.45, nms_top_k=100, keep_top_k=100, confidence_threshold=0.25):
        return self.layer("DetectionOutput", name, [loc, conf, prior], [name],
                          {0: int(num_class), 1: f"{nms_threshold:.6f}", 2: int(nms_top_k), 3: int(keep_top_k), 4: f"{confidence_threshold:.6f}"})

    def ssd_head(self, image, sources, num_class, conf_gain, loc_gain=0.5, **detection):
        """The SSD head over `sources` = [(tag, blob, channels, priors per cell, priorbox arguments)]: per source a 3x3 location and a 3x3
        confidence convolution, each Permute(3) -> Flatten, and a PriorBox; the three Concats; the confidence as Reshape (num_class, -1) ->
        Softmax(axis 1) -> Flatten; DetectionOutput "detection_out".  Every source is read three times, through a Split.  conf_gain
        spreads the logits so that the scores cover (0, 1) instead of sitting at 1 / num_class."""
        locs, confs, priors = [], [], []
        for tag, x, c, per, box in sources:
            a, b, p = self.split(tag + "_mbox_split", x, 3)
            loc = self.conv(tag + "_mbox_loc", a, c, 4 * per, 3, 1, 1, gain=loc_gain)
            locs.append(self.flatten(tag + "_mbox_loc_flat", self.permute(tag + "_mbox_loc_perm", loc, 3)))
            conf = self.conv(tag + "_mbox_conf", b, c, num_class * per, 3, 1, 1, gain=conf_gain)
            confs.append(self.flatten(tag + "_mbox_conf_flat", self.permute(tag + "_mbox_conf_perm", conf, 3)))
            priors.append(self.priorbox(tag + "_mbox_priorbox", p, image, **box))
        loc = self.concat("mbox_loc", locs, 0)
        conf = self.concat("mbox_conf", confs, 0)
        prior = self.concat("mbox_priorbox", priors, 1)
        conf = self.reshape("mbox_conf_reshape", conf, num_class, -1)
        conf = self.flatten("mbox_conf_flatten", self.softmax("mbox_conf_softmax", conf, axis=1))
        return self.detection_output("detection_out", loc, conf, prior, num_class, **detection)

    # -- the YOLO heads (a net that holds one of these needs Net.SetYolo()) ----------------------------------------------
    def reorg(self, name, bottom, stride, mode=None):
        """ncnn's Reorg: 0=stride, 1=mode (written only when given): [c][h][w] -> [c * stride^2][h / stride][w / stride]."""
        self._note("reorg", name, bottom, name, dict(stride=int(stride), mode=int(mode or 0)))
        return self.layer("Reorg", name, [bottom], [name], {0: int(stride)} if mode is None else {0: int(stride), 1: int(mode)})

    @staticmethod
    def _array(values, fmt):
        return ",".join([str(len(values))] + [fmt(v) for v in values])

    def yolo_detection_output(self, name, bottoms, num_class, num_box, biases, confidence_threshold=0.01, nms_threshold=0.45):
        """ncnn's YoloDetectionOutput (YOLOv2): -23304=biases, num_box pairs (width, height) in cells."""
        return self.layer("YoloDetectionOutput", name, list(bottoms), [name],
                          {0: int(num_class), 1: int(num_box), 2: f"{confidence_threshold:.6f}", 3: f"{nms_threshold:.6f}",
                           -23304: self._array(biases, lambda v: f"{float(v):.6f}")})

    def yolov3_detection_output(self, name, bottoms, num_class, num_box, biases, mask, anchors_scale, confidence_threshold=0.01, nms_threshold=0.45):
        """ncnn's Yolov3DetectionOutput: -23304=biases (anchor pairs in pixels), -23305=mask (num_box anchors per bottom), -23306=anchors_scale
        (the stride of every bottom)."""
        return self.layer("Yolov3DetectionOutput", name, list(bottoms), [name],
                          {0: int(num_class), 1: int(num_box), 2: f"{confidence_threshold:.6f}", 3: f"{nms_threshold:.6f}",
                           -23304: self._array(biases, lambda v: f"{float(v):.6f}"), -23305: self._array(mask, lambda v: f"{float(v):.6f}"),
                           -23306: self._array(anchors_scale, lambda v: f"{float(v):.6f}")})

    # -- the two-stage detectors (a net that holds one of these needs Net.SetRoi(); rpn_softmax needs Net.SetDetection(True)) ----------
    def rpn_softmax(self, name, bottom, anchors=9):
        """The RPN's two-way softmax as py-faster-rcnn writes it: Reshape [2A][h][w] -> [2][A * h][w], Softmax along the channels, Reshape back
        to [2A][h][w].  Foreground plane A + q against background plane q."""
        trace, self.trace = self.trace, None  # one note for the three layers
        x = self.reshape(name + "_reshape", bottom, 0, -1, 2)
        x = self.softmax(name + "_prob", x, axis=0)
        top = self.reshape(name + "_prob_reshape", x, 0, -1, 2 * anchors)
        self.trace = trace
        self._note("rpn_softmax", name, bottom, top, dict(anchors=anchors))
        return top

    def proposal(self, name, score, bbox, im_info, feat_stride=16, base_size=16, pre_nms_topN=6000, after_nms_topN=300, nms_thresh=0.7, min_size=16,
                 with_scores=False):
        """ncnn's Proposal: 0=feat_stride 1=base_size 2=pre_nms_topN 3=after_nms_topN 4=nms_thresh 5=min_size; the top [after_nms_topN][1][4]
        (and, with_scores, a second top name + "_scores")."""
        tops = [name, name + "_scores"] if with_scores else [name]
        a = dict(feat_stride=int(feat_stride), base_size=int(base_size), pre_nms_topN=int(pre_nms_topN), after_nms_topN=int(after_nms_topN),
                 nms_thresh=float(nms_thresh), min_size=int(min_size))
        self._note("proposal", name, [score, bbox, im_info], tops, a)
        self.layer("Proposal", name, [score, bbox, im_info], tops, {0: a["feat_stride"], 1: a["base_size"], 2: a["pre_nms_topN"], 3: a["after_nms_topN"],
                                                                     4: f"{nms_thresh:.6f}", 5: a["min_size"]})
        return tops if with_scores else name

    def roi_pooling(self, name, features, rois, pooled_w=7, pooled_h=7, spatial_scale=0.0625):
        """ncnn's ROIPooling: 0=pooled_width 1=pooled_height 2=spatial_scale; the top holds one row per ROI."""
        self._note("roi_pooling", name, [features, rois], name, dict(pooled_w=pooled_w, pooled_h=pooled_h, spatial_scale=spatial_scale))
        return self.layer("ROIPooling", name, [features, rois], [name], {0: int(pooled_w), 1: int(pooled_h), 2: f"{spatial_scale:.6f}"})

    def roi_align(self, name, features, rois, pooled_w=7, pooled_h=7, spatial_scale=0.0625, sampling_ratio=0, aligned=False, version=0):
        """ncnn's ROIAlign: + 3=sampling_ratio 4=aligned 5=version (0 ncnn's original, 1 detectron2's)."""
        a = dict(pooled_w=pooled_w, pooled_h=pooled_h, spatial_scale=spatial_scale, sampling_ratio=int(sampling_ratio), aligned=int(aligned), version=int(version))
        self._note("roi_align", name, [features, rois], name, a)
        return self.layer("ROIAlign", name, [features, rois], [name],
                          {0: int(pooled_w), 1: int(pooled_h), 2: f"{spatial_scale:.6f}", 3: a["sampling_ratio"], 4: a["aligned"], 5: a["version"]})

    def psroi_pooling(self, name, features, rois, output_dim, pooled_w=7, pooled_h=7, spatial_scale=0.0625):
        """ncnn's PSROIPooling: + 3=output_dim; the features hold output_dim * pooled_h * pooled_w channels."""
        self._note("psroi_pooling", name, [features, rois], name, dict(output_dim=int(output_dim), pooled_w=pooled_w, pooled_h=pooled_h, spatial_scale=spatial_scale))
        return self.layer("PSROIPooling", name, [features, rois], [name], {0: int(pooled_w), 1: int(pooled_h), 2: f"{spatial_scale:.6f}", 3: int(output_dim)})

    # -- the framing layers (a net that holds one of these needs Net.SetFrame()) ------------------------------------------------
    def padding(self, name, bottom, top=0, bottom_=0, left=0, right=0, type_=0, value=None, per_channel=0, front=0, behind=0):
        """ncnn's Padding: 0=top 1=bottom 2=left 3=right, and where set 4=type (0 constant, 1 replicate, 2 reflect), 5=value,
        6=per_channel_pad_data_size (that many raw floats in the .bin, U(-1, 1)), 7=front, 8=behind."""
        params = {0: int(top), 1: int(bottom_), 2: int(left), 3: int(right)}
        if type_:
            params[4] = int(type_)
        if value is not None:
            params[5] = f"{value:.6f}"
        if per_channel:
            params[6] = int(per_channel)
        if front or behind:
            params.update({7: int(front), 8: int(behind)})
        pc = self._uniform(int(per_channel), -1, 1) if per_channel else None
        if per_channel:
            self._raw(pc)
        self._note("padding", name, bottom, name, dict(top=top, bottom=bottom_, left=left, right=right, type_=type_, value=0.0 if value is None else float(f"{value:.6f}"),
                                                       per_channel=pc, front=front, behind=behind))
        return self.layer("Padding", name, [bottom], [name], params)

    def crop(self, name, bottom, woffset=0, hoffset=0, coffset=0, outw=None, outh=None, outc=None, woffset2=0, hoffset2=0, coffset2=0, like=None):
        """ncnn's Crop: 0=woffset 1=hoffset 2=coffset, and where set 3=outw 4=outh 5=outc (else -233: what the offsets leave) and 6=woffset2
        7=hoffset2 8=coffset2; like: the reference blob of the two-bottom form, whose (c, h, w) the top takes."""
        params = {0: int(woffset), 1: int(hoffset), 2: int(coffset)}
        for k, v in ((3, outw), (4, outh), (5, outc)):
            if v is not None:
                params[k] = int(v)
        for k, v in ((6, woffset2), (7, hoffset2), (8, coffset2)):
            if v:
                params[k] = int(v)
        bottoms = [bottom] if like is None else [bottom, like]
        self._note("crop", name, bottoms if like is not None else bottom, name,
                   dict(woffset=woffset, hoffset=hoffset, coffset=coffset, outw=-233 if outw is None else outw, outh=-233 if outh is None else outh,
                        outc=-233 if outc is None else outc, woffset2=woffset2, hoffset2=hoffset2, coffset2=coffset2))
        return self.layer("Crop", name, bottoms, [name], params)

    def pixel_shuffle(self, name, bottom, r, mode=None):
        """ncnn's PixelShuffle: 0=upscale_factor, 1=mode (written only when given): [C * r^2][h][w] -> [C][h * r][w * r]."""
        self._note("pixel_shuffle", name, bottom, name, dict(r=int(r), mode=int(mode or 0)))
        return self.layer("PixelShuffle", name, [bottom], [name], {0: int(r)} if mode is None else {0: int(r), 1: int(mode)})

    # -- the transformer layers (a net that holds one of these needs Net.SetTransformer() and Net.SetDetection()) -------------------
    def memory_data(self, name, w, h=0, c=0, scale=1.0):
        """ncnn's MemoryData: 0=w 1=h 2=c (written where non-zero: the rank), w * h * c raw floats, U(-1, 1) * scale."""
        params = {0: int(w)}
        if h:
            params[1] = int(h)
        if c:
            params[2] = int(c)
        data = self._uniform(int(w) * max(int(h), 1) * max(int(c), 1), -1, 1, scale)
        self._raw(data)
        self._note("memory_data", name, [], name, dict(data=data, shape=(max(int(c), 1), max(int(h), 1), int(w))))
        return self.layer("MemoryData", name, [], [name], params)

    def layer_norm(self, name, bottom, size, eps=None, affine=True):
        """ncnn's LayerNorm: 0=affine_size, 1=eps (written only when given; 0.001), 2=affine (written only when off); gamma and beta raw."""
        params = {0: int(size)}
        if eps is not None:
            params[1] = f"{eps:.6e}"
        if not affine:
            params[2] = 0
        gamma = self._uniform(int(size), 0.5, 1.5) if affine else None
        beta = self._uniform(int(size), -0.1, 0.1) if affine else None
        if affine:
            self._raw(gamma)
            self._raw(beta)
        self._note("layer_norm", name, bottom, name, dict(size=int(size), eps=0.001 if eps is None else float(f"{eps:.6e}"), gamma=gamma, beta=beta))
        return self.layer("LayerNorm", name, [bottom], [name], params)

    def gelu(self, name, bottom, fast=False):
        """ncnn's GELU: 0=fast_gelu (written only when set)."""
        self._note("gelu", name, bottom, name, dict(fast=bool(fast)))
        return self.layer("GELU", name, [bottom], [name], {0: 1} if fast else {})

    def binary(self, name, op, a, b):
        """ncnn's BinaryOp 0=op (0 add, 1 sub, 2 mul, 3 div, 4 max, 5 min): b a blob name (two bottoms) or a number (1=1 2=b)."""
        if isinstance(b, str):
            self._note("binary", name, [a, b], name, dict(op=int(op), scalar=None))
            return self.layer("BinaryOp", name, [a, b], [name], {0: int(op)})
        self._note("binary", name, a, name, dict(op=int(op), scalar=float(f"{b:.6e}")))
        return self.layer("BinaryOp", name, [a], [name], {0: int(op), 1: 1, 2: f"{b:.6e}"})

    def multi_head_attention(self, name, q, embed, heads, k=None, v=None, gain=1.0, scale=None):
        """ncnn's MultiHeadAttention: 0=embed_dim 1=num_heads 2=weight_data_size (6=scale only when given); bottoms q [, k [, v]]; the .bin holds
        q, k, v and out weights (tagged, [out][in]) each followed by its raw bias."""
        bottoms = [q] + ([k] if k is not None else []) + ([v] if v is not None else [])
        params = {0: int(embed), 1: int(heads), 2: int(embed) * int(embed)}
        if scale is not None:
            params[6] = f"{scale:.6e}"
        weights = []
        for _ in range(4):
            w = self._uniform(embed * embed, -1, 1, np.sqrt(6.0 / embed) * gain)
            b = self._uniform(embed, -0.1, 0.1)
            self._tagged(w)
            self._raw(b)
            weights += [w if self.dry else w.reshape(embed, embed), b]
        self._note("mha", name, bottoms if len(bottoms) > 1 else q, name, dict(heads=int(heads), weights=weights, scale=None if scale is None else float(f"{scale:.6e}")))
        return self.layer("MultiHeadAttention", name, bottoms, [name], params)

    def fc_tokens(self, name, bottom, cin, cout, bias=True, gain=1.0):
        """An InnerProduct on a blob of rank 2 [T][cin]: once per token, [T][cout] (Net.SetTransformer())."""
        top = self.layer("InnerProduct", name, [bottom], [name], {0: cout, 1: int(bias), 2: cin * cout})
        w = self._uniform(cin * cout, -1, 1, np.sqrt(6.0 / cin) * gain)
        b = self._uniform(cout, -0.1, 0.1) if bias else None
        self._weights(name, w, cout, b)
        if self.trace is not None:
            self._note("fc_tokens", name, bottom, top, dict(w=w.reshape(cout, cin), b=b))
        return top

    # -- the recurrent layers (a net that holds one of these needs Net.SetRecurrent() and Net.SetDetection()) -----------------------
    def _recurrent(self, type_, cell, name, bottom, size, hidden, direction, states_in, states_out):
        """ncnn's LSTM / GRU / RNN: 0=num_output 1=weight_data_size 2=direction (LSTM: 3=hidden_size); weight_xc [nd][G * H][size], bias_c
        ([nd][4][H], RNN [nd][H]) and weight_hc [nd][G * H][H], each tagged, all U(-1, 1) / sqrt(H): the scaling at which a float32
        recurrence stays next to the float64 one however long the sequence.  states_in: blob names of the initial hidden (and cell) state;
        states_out: also write the final states as tops <name>_h (and <name>_c).  -> the sequence top, or the list of tops."""
        gates, nd = {0: 4, 1: 3, 2: 1}[cell], 2 if direction == 2 else 1
        k = 2 if cell == 0 else 1
        if len(states_in) not in (0, k):
            raise ValueError(f"layer {name}: {type_} takes {k} state bottoms or none")
        params = {0: int(hidden), 1: nd * gates * int(hidden) * int(size), 2: int(direction)}
        if cell == 0:
            params[3] = int(hidden)
        scale = 1.0 / np.sqrt(hidden)
        wx = self._uniform(nd * gates * hidden * size, -1, 1, scale)
        bias = self._uniform(nd * (1 if cell == 2 else 4) * hidden, -1, 1, scale)
        wh = self._uniform(nd * gates * hidden * hidden, -1, 1, scale)
        for a in (wx, bias, wh):
            self._tagged(a)
        bottoms = [bottom] + list(states_in)
        tops = [name] + ([name + "_h", name + "_c"][:k] if states_out else [])
        if self.trace is not None:
            self._note("recurrent", name, bottoms if len(bottoms) > 1 else bottom, tops if len(tops) > 1 else name,
                       dict(cell=cell, direction=int(direction), wx=wx.reshape(nd, gates * hidden, size), bias=bias.reshape(nd, -1, hidden), wh=wh.reshape(nd, gates * hidden, hidden)))
        self.layer(type_, name, bottoms, tops, params)
        return tops if len(tops) > 1 else name

    def lstm(self, name, bottom, size, hidden, direction=0, states_in=(), states_out=False):
        """ncnn's LSTM on a blob of rank 2 [T][size] -> [T][nd * hidden]; gate rows I, F, O, G."""
        return self._recurrent("LSTM", 0, name, bottom, size, hidden, direction, states_in, states_out)

    def gru(self, name, bottom, size, hidden, direction=0, states_in=(), states_out=False):
        """ncnn's GRU; gate rows R, U, N, bias rows R, U, WN, BN."""
        return self._recurrent("GRU", 1, name, bottom, size, hidden, direction, states_in, states_out)

    def rnn(self, name, bottom, size, hidden, direction=0, states_in=(), states_out=False):
        """ncnn's RNN (tanh)."""
        return self._recurrent("RNN", 2, name, bottom, size, hidden, direction, states_in, states_out)

    def pool_rect(self, name, bottom, kw, kh, sw, sh):
        """A max Pooling with a rectangular kernel and stride, unpadded: ncnn's 1 / 11 and 2 / 12.  (A padded one is written as a zero Padding in
        front of it where the bottom is not negative: the reference places a padded window at minus the SUM of both pads, and this runtime
        with it.)"""
        self._note("pool_rect", name, bottom, name, dict(kw=kw, kh=kh, sw=sw, sh=sh))
        return self.layer("Pooling", name, [bottom], [name], {0: 0, 1: kw, 11: kh, 2: sw, 12: sh})

    def shuffle(self, name, bottom, group, reverse=False):
        """ncnn's ShuffleChannel: 0=group, 1=reverse (written only when set)."""
        return self.layer("ShuffleChannel", name, [bottom], [name], {0: group, 1: 1} if reverse else {0: group})

    def slice(self, name, bottom, sizes):
        """ncnn's Slice along the channels: -23300=count,sizes (an entry of -233: an equal share of what is left), 1=axis 0."""
        tops = [f"{name}_{i}" for i in range(len(sizes))]
        self.layer("Slice", name, [bottom], tops, {-23300: ",".join(map(str, [len(sizes)] + list(sizes))), 1: 0})
        return tops

    def swish(self, name, bottom):
        """ncnn's Swish: y = x / (1 + exp(-x)), no params."""
        return self.layer("Swish", name, [bottom], [name])

    def hard_sigmoid(self, name, bottom, alpha=0.2, beta=0.5):
        """ncnn's HardSigmoid: y = min(max(alpha * x + beta, 0), 1); 0=alpha, 1=beta."""
        return self.layer("HardSigmoid", name, [bottom], [name], {0: f"{alpha:.6f}", 1: f"{beta:.6f}"})

    def binary_mul(self, name, a, b):
        """ncnn's BinaryOp 0=2 (mul) with two bottoms: a tensor and a [c][1][1] gate, in either order (the converters' SE multiply)."""
        return self.layer("BinaryOp", name, [a, b], [name], {0: 2})

    def scale_by(self, name, bottom, gate):
        """ncnn's Scale 0=-233 with two bottoms: the scale comes from the second one (Caffe's two-bottom Scale, SENet's multiply)."""
        return self.layer("Scale", name, [bottom, gate], [name], {0: -233})

    def se_block(self, name, bottom, c, r, spelling="caffe", mact="relu", gact="sigmoid", alpha=0.2, beta=0.5, gate_first=False, gain=1.0, quant=(None, None)):
        """A squeeze-and-excitation block on `bottom` ([c] channels, reduction to r): Split, global average Pooling, two dense layers with
        `mact` ("relu", "swish" or None) between them, `gact` ("sigmoid" or "hard_sigmoid"), and the multiply.  spelling "caffe":
        InnerProduct layers and Scale 0=-233 (SENet as published); "converter": 1x1 Convolution layers and BinaryOp mul (what ncnn's
        converters write for EfficientNet and RegNetY).  gate_first puts the gate first among BinaryOp's bottoms.  `gain` scales the first dense layer's
        weights: the gate's logits scale with the squeezed activations, and a net whose activations grow with depth passes the inverse of
        that growth, so that the logits stay of order one as in a trained net and the gate does not saturate.  `quant` = the `quant=` of the
        first and of the second dense layer (see __init__).  Returns the gated top."""
        keep, sq = self.split(name + "_split", bottom)
        g = self.pool(name + "_gap", sq, 1, 1, avg=True, global_=True)
        dense = (lambda nm, x, i, o, gain=1.0, quant=None: self.fc(nm, x, i, o, gain=gain, quant=quant)) if spelling == "caffe" else \
                (lambda nm, x, i, o, gain=1.0, quant=None: self.conv(nm, x, i, o, 1, type_="Convolution", gain=gain, quant=quant))
        g = dense(name + ("_fc1" if spelling == "caffe" else "_conv1"), g, c, r, gain, quant[0])
        if mact == "relu":
            g = self.relu(name + "_relu", g)
        elif mact == "swish":
            g = self.swish(name + "_swish", g)
        g = dense(name + ("_fc2" if spelling == "caffe" else "_conv2"), g, r, c, quant=quant[1])
        g = self.sigmoid(name + "_sigmoid", g) if gact == "sigmoid" else self.hard_sigmoid(name + "_hsigmoid", g, alpha, beta)
        if spelling == "caffe":
            return self.scale_by(name + "_scale", keep, g)
        return self.binary_mul(name + "_mul", g, keep) if gate_first else self.binary_mul(name + "_mul", keep, g)

    def hard_swish(self, name, bottom, alpha=None, beta=None):
        """ncnn's HardSwish: y = x * min(max(alpha * x + beta, 0), 1); 0=alpha, 1=beta, written only when given (defaults 0.2 and 0.5).  A
        net that holds one needs Net.SetExtendedLayers(True)."""
        return self.layer("HardSwish", name, [bottom], [name], None if alpha is None else {0: f"{alpha:.6f}", 1: f"{0.5 if beta is None else beta:.6f}"})

    def interp(self, name, bottom, mode="bilinear", scale=None, size=None, align_corner=False, like=None):
        """ncnn's Interp: 0=resize_type (1 nearest, 2 bilinear), 1 / 2 = height / width scale, 3 / 4 = output height / width, 6=align_corner.
        scale: one value or (height, width); size: (height, width); like: a second bottom whose height and width the output takes.  A net
        that holds one needs Net.SetExtendedLayers(True)."""
        params = {0: {"nearest": 1, "bilinear": 2}[mode]}
        if like is None and size is not None:
            params.update({3: int(size[0]), 4: int(size[1])})
        elif like is None:
            hs, ws = scale if isinstance(scale, (tuple, list)) else (scale, scale)
            params.update({1: f"{hs:.6f}", 2: f"{ws:.6f}"})
        if align_corner:
            params[6] = 1
        self._note("interp", name, bottom, name, dict(mode=mode, scale=scale, size=size, like=like))
        return self.layer("Interp", name, [bottom] + ([like] if like is not None else []), [name], params)

    def lrn(self, name, bottom, local_size, alpha, beta, bias=1.0, region=0):
        """ncnn's LRN: 0=region_type (0 across channels, 1 within channel), 1=local_size, 2=alpha, 3=beta, 4=bias.  A net that holds one
        needs Net.SetExtendedLayers(True)."""
        return self.layer("LRN", name, [bottom], [name], {0: int(region), 1: int(local_size), 2: f"{alpha:.8e}", 3: f"{beta:.8e}", 4: f"{bias:.8e}"})

    def conv_bn_swish(self, name, bottom, cin, cout, k, s=1, p=0, group=1, swish=True):
        x = self.conv_bn_relu(name, bottom, cin, cout, k, s, p, group, relu=False)
        return self.swish(name + "_swish", x) if swish else x

    def dropout(self, name, bottom, scale=None):
        return self.layer("Dropout", name, [bottom], [name], {} if scale is None else {0: f"{scale:.6f}"})

    def softmax(self, name, bottom, axis=None, rank=None):
        """axis: ncnn's 0=axis with 1=fixbug0 (needs Net.SetDetection(True)); None writes no params, the plain layer.  rank: the bottom's rank
        where it is not 3, for numpy_forward."""
        self._note("softmax", name, bottom, name, dict(axis=axis) if rank is None else dict(axis=axis, rank=rank))
        return self.layer("Softmax", name, [bottom], [name], None if axis is None else {0: int(axis), 1: 1})

    def conv_bn_relu(self, name, bottom, cin, cout, k, s=1, p=0, group=1, relu=True, dilation=1):
        # bias on every dense conv: the reference Winograd output transform reads bias[k] unconditionally and
        # ConvLayer passes NULL without bias_term; none on depthwise, whose bias blob the reference
        # Net sizes wrongly
        x = self.conv(name, bottom, cin, cout, k, s, p, group, bias=(group == 1), dilation=dilation)
        x = self.bn(name + "_bn", x, cout)
        x = self.scale(name + "_scale", x, cout)
        return self.relu(name + "_relu", x) if relu else x

    def finish(self):
        text = "7767517\n%d %d\n" % (len(self.lines), self.blob_count) + "\n".join(self.lines) + "\n"
        return text.encode(), (self.nbytes if self.dry else bytes(self.bin))  # dry: the .bin size instead of the .bin


def _roi_ref():
    """tests/roi_ref.py, the float32 restatement of feather_roi.h: numpy_forward's Proposal and ROI layers are that text, not a second one."""
    try:
        import roi_ref
    except ImportError:
        import os
        import sys
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
        import roi_ref
    return roi_ref


def _frame_ref():
    """tests/frame_ref.py, the restatement of feather_frame.h: numpy_forward's Padding, Crop and PixelShuffle are that text, not a second one."""
    try:
        import frame_ref
    except ImportError:
        import os
        import sys
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
        import frame_ref
    return frame_ref


def _attn_ref():
    """tests/attn_ref.py, the restatement of feather_attn.h: numpy_forward's transformer layers are that text, not a second one."""
    try:
        import attn_ref
    except ImportError:
        import os
        import sys
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
        import attn_ref
    return attn_ref


def _rnn_ref():
    """tests/rnn_ref.py, the restatement of feather_rnn.h: numpy_forward's recurrent layers are that text, not a second one."""
    try:
        import rnn_ref
    except ImportError:
        import os
        import sys
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
        import rnn_ref
    return rnn_ref


def numpy_forward(trace, input_name, x=None):
    """A plain numpy forward (fp32 values, sums in float64) of the layers a GraphBuilder recorded in `trace` -- Convolution, InnerProduct,
    ReLU (plain or leaky), BatchNorm, Scale, Pooling, Split, Concat on channels, Reorg, nearest Interp by a whole scale, the RPN's softmax, a
    Softmax over the channels of [N][C][1][1], Proposal and the three ROI layers (tests/roi_ref.py in float32), Padding, Crop and PixelShuffle
    (tests/frame_ref.py, bit copies) -- from the input `x`
    [N][C][H][W], or from several: `input_name` a dict {name: array} and no `x`.  Every blob by name.  It exists to calibrate input scales
    and to feed the restatement of a detection head."""
    blobs = {k: np.asarray(v, np.float32) for k, v in input_name.items()} if isinstance(input_name, dict) else {input_name: np.asarray(x, np.float32)}
    for kind, name, bottom, top, a in trace:
        v = blobs[bottom] if isinstance(bottom, str) else [blobs[b] for b in bottom]
        if kind == "split":
            for t in top:
                blobs[t] = v
            continue
        if kind == "proposal":
            ref = _roi_ref()
            rois, scores = ref.proposal(v[0], v[1], v[2].reshape(-1, 3), ref.generate_anchors(a["base_size"]), a["feat_stride"], a["pre_nms_topN"],
                                        a["after_nms_topN"], a["nms_thresh"], a["min_size"])
            blobs[top[0]] = rois.reshape(rois.shape[0], -1, 1, 4)
            if len(top) > 1:
                blobs[top[1]] = scores.reshape(scores.shape[0], -1, 1, 1)
            continue
        if kind == "memory_data":
            batch = next(iter(blobs.values())).shape[0]
            blobs[top] = np.broadcast_to(np.asarray(a["data"], np.float32).reshape((1,) + a["shape"]), (batch,) + a["shape"]).copy()
            continue
        if kind == "recurrent":  # blobs of rank 2: [n][1][T][F]; the states [n][1][nd][H]
            vs = [v] if isinstance(bottom, str) else v
            got = _rnn_ref().layer(a["cell"], a["direction"], vs[0][:, 0], a["wx"], a["bias"], a["wh"], vs[1][:, 0] if len(vs) > 1 else None,
                                   vs[2][:, 0] if len(vs) > 2 else None)
            for t, y in zip([top] if isinstance(top, str) else top, got):
                blobs[t] = y[:, None].astype(np.float32)
            continue
        if kind == "concat" and "rank" in a:
            y = np.concatenate(v, axis=4 - a["rank"] + a["axis"])
        elif kind == "softmax" and "rank" in a:
            ax = 4 - a["rank"] + a["axis"]
            e = np.exp(v.astype(np.float64) - v.max(axis=ax, keepdims=True))
            y = e / e.sum(axis=ax, keepdims=True)
        elif kind == "reshape":
            ext = [a["w"], 1 if a["h"] is None else a["h"], 1 if a["c"] is None else a["c"]]
            ext = [v.shape[3 - i] if e == 0 else e for i, e in enumerate(ext)]
            y = v.reshape(v.shape[0], ext[2], ext[1], ext[0])
        elif kind == "permute" and a["order"] == 1 and v.shape[1] == 1:  # rank 2: (h, w) -> (w, h)
            y = v.transpose(0, 1, 3, 2)
        elif kind == "layer_norm":
            rows = v.reshape(v.shape[0], -1, a["size"])
            y = _attn_ref().layer_norm(rows, a["gamma"], a["beta"], a["eps"]).reshape(v.shape)
        elif kind == "gelu":
            y = _attn_ref().gelu(v, a["fast"])
        elif kind == "binary":
            y = _attn_ref().binary(a["op"], v, np.float32(a["scalar"])) if a["scalar"] is not None else _attn_ref().binary(a["op"], v[0], v[1])
        elif kind == "mha":
            q, k, w_ = (v, v, v) if isinstance(bottom, str) else (v[0], v[1], v[-1])
            y = _attn_ref().multi_head_attention(q[:, 0], k[:, 0], w_[:, 0], a["heads"], a["weights"], a["scale"])[:, None]
        elif kind == "fc_tokens":
            y = v.astype(np.float64) @ a["w"].astype(np.float64).T
            if a["b"] is not None:
                y += a["b"]
        elif kind == "concat" and a["axis"] == 0:
            y = np.concatenate(v, axis=1)
        elif kind == "rpn_softmax":
            A = a["anchors"]
            bg, fg = v[:, :A].astype(np.float64), v[:, A:].astype(np.float64)
            m = np.maximum(bg, fg)
            eb, ef = np.exp(bg - m), np.exp(fg - m)
            y = np.concatenate([eb / (eb + ef), ef / (eb + ef)], axis=1)
        elif kind == "softmax" and a["axis"] is None and v.shape[2:] == (1, 1):
            e = np.exp(v.astype(np.float64) - v.max(axis=1, keepdims=True))
            y = e / e.sum(axis=1, keepdims=True)
        elif kind == "roi_pooling":
            y = _roi_ref().roi_pool(v[0], v[1], a["pooled_w"], a["pooled_h"], a["spatial_scale"])
        elif kind == "roi_align":
            y = _roi_ref().roi_align(v[0], v[1], a["pooled_w"], a["pooled_h"], a["spatial_scale"], a["sampling_ratio"], a["aligned"], a["version"])
        elif kind == "psroi_pooling":
            y = _roi_ref().psroi_pool(v[0], v[1], a["output_dim"], a["pooled_w"], a["pooled_h"], a["spatial_scale"])
        elif kind == "padding":
            y = _frame_ref().pad(v, a["top"], a["bottom"], a["left"], a["right"], a["type_"], a["value"], a["per_channel"], a["front"], a["behind"])
        elif kind == "crop":
            two = not isinstance(bottom, str)
            y = _frame_ref().crop(v[0] if two else v, like=v[1] if two else None, **a)
        elif kind == "pixel_shuffle":
            y = _frame_ref().pixel_shuffle(v, a["r"], a["mode"])
        elif kind == "pool_rect" and (v.shape[2] - a["kh"]) % a["sh"] == 0 and (v.shape[3] - a["kw"]) % a["sw"] == 0:
            oh, ow = (v.shape[2] - a["kh"]) // a["sh"] + 1, (v.shape[3] - a["kw"]) // a["sw"] + 1
            y = np.max([v[:, :, i:i + (oh - 1) * a["sh"] + 1:a["sh"], j:j + (ow - 1) * a["sw"] + 1:a["sw"]] for i in range(a["kh"]) for j in range(a["kw"])], axis=0)
        elif kind == "pool" and a["global_"] and a["avg"]:
            y = v.astype(np.float64).mean(axis=(2, 3), keepdims=True)
        elif kind == "reorg":
            st, (n, c, h, wd) = a["stride"], v.shape
            t = v[:, :, :h // st * st, :wd // st * st].reshape(n, c, h // st, st, wd // st, st).transpose(0, 1, 3, 5, 2, 4)  # [n][q][sh][sw][i][j]
            y = (t if a["mode"] == 0 else t.transpose(0, 2, 3, 1, 4, 5)).reshape(n, c * st * st, h // st, wd // st)
        elif kind == "interp" and a["mode"] == "nearest" and a["like"] is None and a["size"] is None and float(a["scale"]) == int(a["scale"]):
            y = v.repeat(int(a["scale"]), axis=2).repeat(int(a["scale"]), axis=3)
        elif kind == "relu" and a["slope"] is not None:
            y = np.where(v > 0, v, v * np.float32(a["slope"]))
        elif kind == "conv":
            w, s, p, group = a["w"].astype(np.float64), a["s"], a["p"], a["group"]
            k, cg, kh, kw = w.shape
            n, c, h, wd = v.shape
            ho, wo = (h + 2 * p - kh) // s + 1, (wd + 2 * p - kw) // s + 1
            vp = np.zeros((n, c, h + 2 * p, wd + 2 * p))
            vp[:, :, p:p + h, p:p + wd] = v
            y = np.zeros((n, k, ho, wo))
            kg = k // group
            for g in range(group):
                for i in range(kh):
                    for j in range(kw):
                        win = vp[:, g * cg:(g + 1) * cg, i:i + (ho - 1) * s + 1:s, j:j + (wo - 1) * s + 1:s]
                        y[:, g * kg:(g + 1) * kg] += np.einsum("nchw,kc->nkhw", win, w[g * kg:(g + 1) * kg, :, i, j])
            if a["b"] is not None:
                y += a["b"].reshape(1, -1, 1, 1)
        elif kind == "fc":
            y = v.reshape(v.shape[0], -1).astype(np.float64) @ a["w"].astype(np.float64).T
            if a["b"] is not None:
                y += a["b"]
            y = y.reshape(v.shape[0], -1, 1, 1)
        elif kind == "relu" and a["slope"] is None:
            y = np.maximum(v, 0)
        elif kind == "affine":
            y = v * a["mul"].reshape(1, -1, 1, 1) + a["add"].reshape(1, -1, 1, 1)
        elif kind == "pool" and not a["global_"] and not a["p"] and not a["avg"] and v.shape[2] % a["s"] == 0 and a["k"] == a["s"]:
            n, c, h, wd = v.shape
            y = v.reshape(n, c, h // a["k"], a["k"], wd // a["k"], a["k"]).max(axis=(3, 5))
        else:
            raise ValueError(f"numpy_forward has no {kind} layer like {name}")
        blobs[top] = y.astype(np.float32)
    return blobs


def input_scales(trace, input_name, x):
    """{layer name: 127 / absmax(bottom)} for every Convolution and InnerProduct of `trace`, from one numpy_forward of `x`.  The absmax
    is rounded up to a multiple of 1/64 first, so that the last bits of a sum (they may differ between numpy builds) do not reach the scale."""
    blobs = numpy_forward(trace, input_name, x)
    return {name: float(np.float32(127) / np.float32(max(np.ceil(float(np.abs(blobs[bottom]).max()) * 64), 1) / 64))
            for kind, name, bottom, _, _ in trace if kind in ("conv", "fc")}


def tiny_quant(seed=29, size=16, dry=False):
    """A 16-px net whose Convolution and InnerProduct layers are all int8 (Net.SetQuantized(True)) and all exactly restatable: a 3 -> 16 first
    layer (the generic route), 16 -> 32 at stride 1 and 32 -> 32 at stride 2 (the MFMA route) with a BatchNorm + Scale + ReLU tail, a
    depthwise 3x3, a 1x1 to 24 channels (no multiple of 16) without a bias, ReLUs, a 2x2 max pooling and an InnerProduct.  The input
    scales are calibrated: the fp32 net with the same seed runs once on a seeded input through numpy_forward (input_scales)."""
    def build(quant, trace=False):
        g = GraphBuilder(seed, dry, quant=quant)
        g.trace = [] if trace else None
        x = g.input("data", 3, size, size)
        x = g.relu("relu1", g.conv("conv1", x, 3, 16, 3, 1, 1))
        x = g.relu("relu2", g.conv("conv2", x, 16, 32, 3, 1, 1))
        x = g.conv("conv3", x, 32, 32, 3, 2, 1)
        x = g.relu("conv3_relu", g.scale("conv3_scale", g.bn("conv3_bn", x, 32), 32))
        x = g.relu("relu_dw", g.conv("dw", x, 32, 32, 3, 1, 1, group=32))
        x = g.relu("relu_pw", g.conv("pw", x, 32, 24, 1, bias=False))
        x = g.pool("pool", x, 2, 2)
        g.fc("fc", x, 24 * (size // 4) ** 2, 10)
        return g
    if dry:
        return build({}).finish() + ("data", "fc")
    calib = np.random.default_rng(seed + 1).uniform(-1, 1, (4, 3, size, size)).astype(np.float32)
    scales = input_scales(build(None, trace=True).trace, "data", calib)
    return build(scales).finish() + ("data", "fc")


# The _int8 nets with their chains of int8 convolutions requantised (Net.SetQuantized(True) and Net.SetRequantized(True)), up to the last
# int8 convolution in front of an fp32 reader, every output scale the default input scale of its readers (what fuse_requantize writes): nets
# for timing.  Each equals its _int8 build bit for bit.  Those with a BatchNorm behind the requantised layers need fusion level >= 2.
def _requant(names):
    return dict.fromkeys(names, QUANT_DEFAULT_SCALE)


def vgg16_int8_rq(seed=1234, classes=1000, size=224, dry=False):
    """Every convolution but conv5_3, whose reader (through pool5) is the InnerProduct fc6."""
    names = [f"conv{s}_{i}" for s, n in enumerate((2, 2, 3, 3, 3), 1) for i in range(1, n + 1)]
    return vgg16(seed, classes, size, dry, quant={}, requant=_requant(names[:-1]))


def resnet50_int8_rq(seed=1234, classes=1000, size=224, dry=False):
    """conv1 (read through pool1 and res2a's Split by two int8 convolutions) and branch2a / branch2b of every block; branch2c and branch1
    stay fp32-out for the Eltwise.  Fusion level >= 2."""
    tags = [f"res{si + 2}{chr(ord('a') + b)}" for si, blocks in enumerate((3, 4, 6, 3)) for b in range(blocks)]
    return resnet50(seed, classes, size, dry, quant={}, requant=_requant(["conv1"] + [t + br for t in tags for br in ("_branch2a", "_branch2b")]))


def mobilenet_v1_int8_rq(seed=1234, classes=1000, size=224, dry=False):
    """Every convolution but conv14_pw, whose reader is the average pooling.  Fusion level >= 2."""
    names = ["conv1"] + [f"conv{i}_{k}" for i in range(2, 15) for k in ("dw", "pw")]
    return mobilenet_v1(seed, classes, size, dry, quant={}, requant=_requant(names[:-1]))


def tiny_requant(seed=31, size=16, dry=False, twin=False, mismatch=None, bn=True, fc=True):
    """tiny_quant's layers with the activations between the int8 convolutions kept int8 (Net.SetQuantized(True) and
    Net.SetRequantized(True)): conv1, conv2, conv3 (BatchNorm + Scale + ReLU tail) and dw have a requantised output (8=101), at the input
    scale of their readers as ncnn2int8's fuse_requantize writes it.  The readers are reached through a ReLU (conv2, pw), through a 2x2 max
    pooling (conv3) and through a Split with two int8 readers (dw and the 1x1 `side`); pw and side write fp32 for the Eltwise, the pooling
    and the InnerProduct behind them.  The BatchNorm behind conv3 exists only folded: the net needs fusion level >= 2.
    twin=True: the same model with 100 subtracted from those terms and the extra scales removed (SetQuantized alone): every fp32 blob of
    the two is equal bit for bit.  mismatch=<layer>: that reader's input scale is multiplied by 1.25, so it differs from its producer's
    output scale, and the net differs from the twin.  bn=False: without the BatchNorm and Scale, a net every fusion level loads.  fc=False: without the InnerProduct, a net that takes any
    input size (the output is `pool`)."""
    def build(quant, outs=None, trace=False):
        g = GraphBuilder(seed, dry, quant=quant)
        g.trace = [] if trace else None
        q = (lambda reader: None) if outs is None else (lambda reader: outs[reader])
        x = g.input("data", 3, size, size)
        x = g.relu("relu1", g.conv("conv1", x, 3, 16, 3, 1, 1, requant=q("conv2")))
        x = g.relu("relu2", g.conv("conv2", x, 16, 32, 3, 1, 1, requant=q("conv3")))
        x = g.pool("pool2", x, 2, 2)
        x = g.conv("conv3", x, 32, 32, 3, 1, 1, requant=q("dw"))
        x = g.relu("conv3_relu", g.scale("conv3_scale", g.bn("conv3_bn", x, 32), 32) if bn else x)
        a, b = (x, x) if trace else g.split("split", x)  # (the calibration run has no Split and no sum: it draws the same weights)
        a = g.relu("relu_dw", g.conv("dw", a, 32, 32, 3, 1, 1, group=32, requant=q("pw")))
        a = g.relu("relu_pw", g.conv("pw", a, 32, 24, 1, bias=False))
        b = g.conv("side", b, 32, 24, 1)
        x = g.pool("pool", a if trace else g.eltwise("sum", a, b), 2, 2)
        if fc:
            g.fc("fc", x, 24 * (size // 4) ** 2, 10)
        return g
    readers = ("conv2", "conv3", "dw", "pw")
    out = "fc" if fc else "pool"
    if dry:
        return build({}, None if twin else dict.fromkeys(readers, 1.0)).finish() + ("data", out)
    calib = np.random.default_rng(seed + 1).uniform(-1, 1, (4, 3, size, size)).astype(np.float32)
    scales = input_scales(build(None, trace=True).trace, "data", calib)
    scales["side"] = scales["dw"]  # one output scale serves both readers of the Split
    outs = {r: scales[r] for r in readers}  # fuse_requantize: a producer's output scale is its reader's input scale
    if mismatch:
        scales[mismatch] = float(np.float32(scales[mismatch] * 1.25))
    return build(scales, None if twin else outs).finish() + ("data", out)


def tiny_requant_twin(seed=31, size=16, dry=False):
    """tiny_requant's twin: fp32 between the int8 layers (SetQuantized alone)."""
    return tiny_requant(seed, size, dry, twin=True)


def vgg16(seed=1234, classes=1000, size=224, dry=False, quant=None, requant=None):
    g = GraphBuilder(seed, dry, quant, requant)
    x = g.input("data", 3, size, size)
    cin = 3
    for stage, (n, c) in enumerate([(2, 64), (2, 128), (3, 256), (3, 512), (3, 512)], 1):
        for i in range(1, n + 1):
            x = g.relu(f"relu{stage}_{i}", g.conv(f"conv{stage}_{i}", x, cin, c, 3, 1, 1))
            cin = c
        x = g.pool(f"pool{stage}", x, 2, 2)
    feat = 512 * (size // 32) ** 2
    x = g.dropout("drop6", g.relu("relu6", g.fc("fc6", x, feat, 4096)))
    x = g.dropout("drop7", g.relu("relu7", g.fc("fc7", x, 4096, 4096)))
    x = g.softmax("prob", g.fc("fc8", x, 4096, classes))
    return g.finish() + ("data", "prob")


def resnet50(seed=1234, classes=1000, size=224, dry=False, quant=None, requant=None):
    """Caffe ResNet-50: conv-BN-Scale-ReLU, stride on the first 1x1 of each stage, explicit Split for the shortcut."""
    g = GraphBuilder(seed, dry, quant, requant)
    x = g.input("data", 3, size, size)
    x = g.conv_bn_relu("conv1", x, 3, 64, 7, 2, 3)
    x = g.pool("pool1", x, 3, 2)
    cin = 64
    for si, (mid, out, blocks, stride) in enumerate([(64, 256, 3, 1), (128, 512, 4, 2), (256, 1024, 6, 2), (512, 2048, 3, 2)]):
        for b in range(blocks):
            s = stride if b == 0 else 1
            tag = f"res{si + 2}{chr(ord('a') + b)}"
            main, short = g.split(tag + "_split", x)
            if b == 0:
                short = g.conv_bn_relu(tag + "_branch1", short, cin, out, 1, s, 0, relu=False)
            y = g.conv_bn_relu(tag + "_branch2a", main, cin, mid, 1, s, 0)
            y = g.conv_bn_relu(tag + "_branch2b", y, mid, mid, 3, 1, 1)
            y = g.conv_bn_relu(tag + "_branch2c", y, mid, out, 1, 1, 0, relu=False)
            x = g.relu(tag + "_relu", g.eltwise(tag, short, y))
            cin = out
    x = g.pool("pool5", x, 7, 1, avg=True, global_=True)
    x = g.softmax("prob", g.fc("fc1000", x, 2048, classes))
    return g.finish() + ("data", "prob")


def mobilenet_v1(seed=1234, classes=1000, size=224, dry=False, quant=None, requant=None):
    g = GraphBuilder(seed, dry, quant, requant)
    x = g.input("data", 3, size, size)
    x = g.conv_bn_relu("conv1", x, 3, 32, 3, 2, 1)
    cfg = [(32, 64, 1), (64, 128, 2), (128, 128, 1), (128, 256, 2), (256, 256, 1), (256, 512, 2)] + [(512, 512, 1)] * 5 + \
          [(512, 1024, 2), (1024, 1024, 1)]
    for i, (c, k, s) in enumerate(cfg, 2):
        x = g.conv_bn_relu(f"conv{i}_dw", x, c, c, 3, s, 1, group=c)
        x = g.conv_bn_relu(f"conv{i}_pw", x, c, k, 1, 1, 0)
    x = g.pool("pool6", x, 7, 1, avg=True, global_=True)
    x = g.softmax("prob", g.fc("fc7", x, 1024, classes))
    return g.finish() + ("data", "prob")


def vgg16_int8(seed=1234, classes=1000, size=224, dry=False):
    """vgg16 with every Convolution and InnerProduct int8 at the default input scale: a net for timing, not for accuracy (Net.SetQuantized(True))."""
    return vgg16(seed, classes, size, dry, quant={})


def resnet50_int8(seed=1234, classes=1000, size=224, dry=False):
    """resnet50 with every Convolution and InnerProduct int8 at the default input scale (Net.SetQuantized(True)); see vgg16_int8."""
    return resnet50(seed, classes, size, dry, quant={})


def mobilenet_v1_int8(seed=1234, classes=1000, size=224, dry=False):
    """mobilenet_v1 with every Convolution and InnerProduct int8 at the default input scale (Net.SetQuantized(True)); see vgg16_int8."""
    return mobilenet_v1(seed, classes, size, dry, quant={})


def squeezenet_v11(seed=1234, classes=1000, size=224, dry=False):
    g = GraphBuilder(seed, dry)
    x = g.input("data", 3, size, size)
    x = g.relu("relu_conv1", g.conv("conv1", x, 3, 64, 3, 2, 0))
    x = g.pool("pool1", x, 3, 2)
    cin = 64

    def fire(name, x, cin, sq, ex):
        s = g.relu(name + "_relu_squeeze", g.conv(name + "_squeeze1x1", x, cin, sq, 1))
        a, b = g.split(name + "_split", s)
        a = g.relu(name + "_relu_e1", g.conv(name + "_expand1x1", a, sq, ex, 1))
        b = g.relu(name + "_relu_e3", g.conv(name + "_expand3x3", b, sq, ex, 3, 1, 1))
        return g.concat(name + "_concat", [a, b])

    for i, (sq, ex) in enumerate([(16, 64), (16, 64), (32, 128), (32, 128), (48, 192), (48, 192), (64, 256), (64, 256)], 2):
        x = fire(f"fire{i}", x, cin, sq, ex)
        cin = 2 * ex
        if i in (3, 5):
            x = g.pool(f"pool{i}", x, 3, 2)
    x = g.dropout("drop9", x)
    x = g.relu("relu_conv10", g.conv("conv10", x, 512, classes, 1))
    x = g.pool("pool10", x, 13, 1, avg=True, global_=True)
    x = g.softmax("prob", x)
    return g.finish() + ("data", "prob")


def tiny_allsorts(seed=7, size=20, dry=False):
    """A small net touching every registered layer type (layer_factory.cpp:55-67) for the Net parity tests."""
    g = GraphBuilder(seed, dry)
    x = g.input("data", 3, size, size)
    x = g.relu("relu1", g.conv("conv1", x, 3, 16, 3, 1, 1))             # IM2COL (C=3)
    x = g.conv_bn_relu("conv2", x, 16, 16, 3, 1, 1)                      # Winograd + BN + Scale + ReLU
    a, b = g.split("split1", x)
    a = g.conv_bn_relu("dw", a, 16, 16, 3, 1, 1, group=16)               # depthwise
    b = g.scale("scale_b", g.conv("pw", b, 16, 16, 1), 16, bias=False)   # 1x1 + bare Scale
    x = g.relu("relu_sum", g.eltwise("sum", a, b))
    x = g.pool("pool1", x, 3, 2)                                         # max, ceil mode
    c, d = g.split("split2", x)
    c = g.relu("relu_c", g.conv("conv_c", c, 16, 8, 1))
    d = g.pool("pool_d", d, 3, 1, p=1, avg=True)                         # average with the reference's pad rule
    x = g.concat("cat", [c, d])
    x = g.dropout("drop", x, scale=0.5)
    x = g.pool("gap", x, 1, 1, avg=True, global_=True)
    x = g.relu("relu_fc", g.fc("fc1", x, 24, 32))
    x = g.softmax("prob", g.fc("fc2", x, 32, 10))
    return g.finish() + ("data", "prob")


def tiny_plain(seed=31, size=8, dry=False):
    """A small net of main-library layers only -- Convolution (3x3 on RGB, 1x1, depthwise), Pooling, ReLU, Split, Eltwise, Concat, InnerProduct,
    Softmax -- whose largest blob (conv1: 32 x size x size) sits right behind the input and whose planes stay too small for Winograd: a batch
    that takes that blob past 2^31 floats needs no Winograd scratch and about 22 GB in all at size 8."""
    g = GraphBuilder(seed, dry)
    x = g.input("data", 3, size, size)
    x = g.relu("relu1", g.conv("conv1", x, 3, 32, 3, 1, 1))
    x = g.pool("pool1", x, 2, 2)
    a, b = g.split("split1", x)
    a = g.relu("relu_a", g.conv("pw_a", a, 32, 32, 1))
    b = g.conv("dw_b", b, 32, 32, 3, 1, 1, group=32)
    x = g.relu("relu_sum", g.eltwise("sum", a, b))
    c, d = g.split("split2", x)
    c = g.conv("pw_c", c, 32, 16, 1)
    x = g.concat("cat", [c, d])
    x = g.pool("gap", x, 1, 1, avg=True, global_=True)
    x = g.softmax("prob", g.fc("fc", x, 48, 10))
    return g.finish() + ("data", "prob")


def resnext50_32x4d(seed=1234, classes=1000, size=224, dry=False):
    """Caffe-style ResNeXt-50 (32x4d): 1x1 reduce, grouped 3x3 (32 groups) with the stage's stride, 1x1 expand, BN + Scale + ReLU after
    each, projection shortcuts.  Its grouped layers (1 < group < C) run through libfeather_gconv.so."""
    g = GraphBuilder(seed, dry)
    x = g.input("data", 3, size, size)
    x = g.conv_bn_relu("conv1", x, 3, 64, 7, 2, 3)
    x = g.pool("pool1", x, 3, 2)
    cin = 64
    for si, (mid, out, blocks, stride) in enumerate([(128, 256, 3, 1), (256, 512, 4, 2), (512, 1024, 6, 2), (1024, 2048, 3, 2)]):
        for b in range(blocks):
            s = stride if b == 0 else 1
            tag = f"resx{si + 2}{chr(ord('a') + b)}"
            main, short = g.split(tag + "_split", x)
            if b == 0:
                short = g.conv_bn_relu(tag + "_branch1", short, cin, out, 1, s, 0, relu=False)
            y = g.conv_bn_relu(tag + "_branch2a", main, cin, mid, 1, 1, 0)
            y = g.conv_bn_relu(tag + "_branch2b", y, mid, mid, 3, s, 1, group=32)
            y = g.conv_bn_relu(tag + "_branch2c", y, mid, out, 1, 1, 0, relu=False)
            x = g.relu(tag + "_relu", g.eltwise(tag, short, y))
            cin = out
    x = g.pool("pool5", x, 7, 1, avg=True, global_=True)
    x = g.softmax("prob", g.fc("fc1000", x, 2048, classes))
    return g.finish() + ("data", "prob")


def tiny_grouped(seed=11, size=21, dry=False):
    """A small net of grouped convolutions (1 < group < C) in every position the Net runtime has to get right: behind a ReLU, behind
    BatchNorm + Scale + ReLU, in front of an Eltwise sum and of a 2x2 pooling (fusions that must decline a grouped layer)."""
    g = GraphBuilder(seed, dry)
    x = g.input("data", 3, size, size)
    x = g.relu("relu1", g.conv("conv1", x, 3, 16, 3, 1, 1))
    x = g.relu("relu_g1", g.conv("g1", x, 16, 16, 3, 1, 1, group=4))                    # grouped 3x3 / s1, bias + ReLU, odd plane
    x = g.conv_bn_relu("g2", x, 16, 32, 3, 2, 1, group=2)                                 # grouped 3x3 / s2, no bias, BN + Scale + ReLU
    a, b = g.split("split1", x)
    a = g.conv("g3", a, 32, 32, 1, group=4, type_="Convolution")                          # grouped 1x1, then a residual sum
    x = g.relu("relu_sum", g.eltwise("sum", a, b))
    x = g.relu("relu_g4", g.conv("g4", x, 32, 10, 3, 1, 0, group=2, bias=False))          # group 2, 16 -> 5 channels, no bias, no pad
    x = g.pool("pool1", x, 2, 2)
    x = g.pool("gap", x, 1, 1, avg=True, global_=True)
    x = g.softmax("prob", g.fc("fc", x, 10, 10))
    return g.finish() + ("data", "prob")


def tiny_deconv(seed=13, size=16, dry=False):
    """A small net of transposed convolutions in every form the Net runtime has to get right, nothing above 16 px: k4 s2 p1 behind a ReLU,
    k2 s2 p0 with a BatchNorm + Scale + ReLU tail, a depthwise bilinear-style k4 s2 p1 and a grouped k4 s2 p1 layer, a Concat of the three,
    k3 s2 p1 with output padding 1, and k3 s1 p1."""
    g = GraphBuilder(seed, dry)
    x = g.input("data", 3, size, size)
    x = g.relu("relu1", g.conv("conv1", x, 3, 16, 3, 2, 1))
    x = g.relu("relu2", g.conv("conv2", x, 16, 32, 3, 2, 1))
    x = g.relu("relu3", g.conv("conv3", x, 32, 32, 3, 2, 1))
    x = g.relu("relu_d1", g.deconv("d1", x, 32, 32, 4, 2, 1))                       # k4 s2 p1 + ReLU (the MFMA route)
    a, b, c = g.split("split1", x, 3)
    a = g.deconv_bn_relu("d2", a, 32, 32, 2, 2, 0)                                   # k2 s2 p0, BN + Scale + ReLU
    b = g.deconv("dw_up", b, 32, 32, 4, 2, 1, group=32, bias=False)                  # depthwise, FCN's bilinear up-sampling shape
    c = g.relu("relu_gd", g.deconv("gd", c, 32, 16, 4, 2, 1, group=4))              # grouped
    x = g.concat("cat", [a, b, c])
    x = g.relu("relu_d3", g.deconv("d3", x, 80, 24, 3, 2, 1, op=1))                 # k3 s2 p1, output padding 1
    x = g.deconv("d4", x, 24, 8, 3, 1, 1)                                            # k3 s1 p1 (the generic kernel)
    return g.finish() + ("data", "d4")


def style_transfer(seed=1234, size=256, dry=False):
    """Johnson et al.'s feed-forward style-transfer net: 9x9 convolution, two stride-2 convolutions, five 128-channel residual blocks at a
    quarter of the resolution, two k3 s2 p1 deconvolutions with output padding 1, 9x9 convolution to 3 channels.  BatchNorm + Scale
    stand where the paper has InstanceNorm (the arithmetic per layer is the same affine map, and it folds into the convolutions);
    `style_transfer_in` is the net as published, with InstanceNorm and a TanH output."""
    g = GraphBuilder(seed, dry)
    x = g.input("data", 3, size, size)
    x = g.conv_bn_relu("conv1", x, 3, 32, 9, 1, 4)
    x = g.conv_bn_relu("conv2", x, 32, 64, 3, 2, 1)
    x = g.conv_bn_relu("conv3", x, 64, 128, 3, 2, 1)
    for i in range(1, 6):
        a, b = g.split(f"res{i}_split", x)
        a = g.conv_bn_relu(f"res{i}a", a, 128, 128, 3, 1, 1)
        a = g.conv_bn_relu(f"res{i}b", a, 128, 128, 3, 1, 1, relu=False)
        x = g.eltwise(f"res{i}", a, b)
    x = g.deconv_bn_relu("deconv1", x, 128, 64, 3, 2, 1, op=1)
    x = g.deconv_bn_relu("deconv2", x, 64, 32, 3, 2, 1, op=1)
    x = g.conv("out", x, 32, 3, 9, 1, 4)
    return g.finish() + ("data", "out")


def unet_k4(seed=1234, size=256, dry=False):
    """A five-level pix2pix-style generator: k4 s2 p1 convolutions down (32 .. 256 channels), k4 s2 p1 deconvolutions up, every decoder
    level concatenated with the encoder level of its size."""
    g = GraphBuilder(seed, dry)
    x = g.input("data", 3, size, size)
    widths = (32, 64, 128, 256, 256)
    skips, cin = [], 3
    for i, cw in enumerate(widths, 1):
        x = g.relu(f"e{i}_relu", g.conv(f"e{i}", x, cin, cw, 4, 2, 1)) if i == 1 else g.conv_bn_relu(f"e{i}", x, cin, cw, 4, 2, 1)
        cin = cw
        if i < len(widths):
            x, skip = g.split(f"e{i}_split", x)
            skips.append((skip, cw))
    for i, cw in zip((5, 4, 3, 2), (256, 128, 64, 32)):
        x = g.deconv_bn_relu(f"d{i}", x, cin, cw, 4, 2, 1)
        skip, sw = skips.pop()
        x = g.concat(f"cat{i - 1}", [x, skip])
        cin = cw + sw
    x = g.deconv("d1", x, cin, 3, 4, 2, 1)
    return g.finish() + ("data", "d1")


def tiny_generative(seed=17, size=24, dry=False):
    """A small generative net with every layer of libfeather_inorm.so, nothing above 24 px: InstanceNorm on a 4-aligned plane (24 x 24) behind
    a leaky ReLU, without affine weights on 12 x 12 behind a plain ReLU, on an odd plane (5 x 5) and on a 1 x 1 plane; a convolution followed
    directly by a leaky ReLU (which no convolution epilogue may absorb); PReLU per channel and shared; Sigmoid, Clip and a TanH output.  The
    1 x 1 branch ends in the blob `gate`, the image branch in `out`."""
    g = GraphBuilder(seed, dry)
    x = g.input("data", 3, size, size)
    x = g.conv_in_relu("conv1", x, 3, 16, 3, 1, 1, slope=0.2)                        # InstanceNorm + leaky ReLU
    x = g.relu("lrelu2", g.conv("conv2", x, 16, 32, 3, 2, 1), slope=0.2)             # Convolution + leaky ReLU: two layers at every level
    x = g.relu("relu2", g.instance_norm("in2", x, 32, affine=False))                 # no gamma / beta, plain ReLU
    x = g.prelu("prelu3", g.instance_norm("in3", g.conv("conv3", x, 32, 32, 3, 2, 0), 32, eps=1e-5), 32)  # odd plane, PReLU per channel
    a, b = g.split("split", x)
    a = g.pool("gap", a, global_=True, avg=True)
    a = g.sigmoid("gate", g.prelu("prelu4", g.instance_norm("in4", a, 32), 1))       # a plane of one pixel: y = beta; shared PReLU
    b = g.deconv_in_relu("d1", b, 32, 16, 4, 2, 1)                                   # Deconvolution + InstanceNorm + ReLU
    b = g.clip("clip", g.deconv("d2", b, 16, 8, 4, 2, 1), -0.5, 0.75)
    b = g.tanh("out", g.conv("conv_out", b, 8, 3, 3, 1, 1))
    return g.finish() + ("data", "out")


def style_transfer_in(seed=1234, size=256, dry=False):
    """Johnson et al.'s style-transfer net as published: `style_transfer` with InstanceNorm (affine) where that one has BatchNorm + Scale,
    and a TanH on the output."""
    g = GraphBuilder(seed, dry)
    x = g.input("data", 3, size, size)
    x = g.conv_in_relu("conv1", x, 3, 32, 9, 1, 4)
    x = g.conv_in_relu("conv2", x, 32, 64, 3, 2, 1)
    x = g.conv_in_relu("conv3", x, 64, 128, 3, 2, 1)
    for i in range(1, 6):
        a, b = g.split(f"res{i}_split", x)
        a = g.conv_in_relu(f"res{i}a", a, 128, 128, 3, 1, 1)
        a = g.conv_in_relu(f"res{i}b", a, 128, 128, 3, 1, 1, relu=False)
        x = g.eltwise(f"res{i}", a, b)
    x = g.deconv_in_relu("deconv1", x, 128, 64, 3, 2, 1, op=1)
    x = g.deconv_in_relu("deconv2", x, 64, 32, 3, 2, 1, op=1)
    x = g.tanh("out", g.conv("conv_out", x, 32, 3, 9, 1, 4))
    return g.finish() + ("data", "out")


def pix2pix_unet(seed=1234, size=256, dry=False):
    """`unet_k4` as pix2pix publishes it: leaky ReLU (0.2) in the encoder, InstanceNorm on every level but the first, plain ReLU in the
    decoder, TanH on the output."""
    g = GraphBuilder(seed, dry)
    x = g.input("data", 3, size, size)
    widths = (32, 64, 128, 256, 256)
    skips, cin = [], 3
    for i, cw in enumerate(widths, 1):
        x = g.relu(f"e{i}_relu", g.conv(f"e{i}", x, cin, cw, 4, 2, 1), 0.2) if i == 1 else g.conv_in_relu(f"e{i}", x, cin, cw, 4, 2, 1, slope=0.2)
        cin = cw
        if i < len(widths):
            x, skip = g.split(f"e{i}_split", x)
            skips.append((skip, cw))
    for i, cw in zip((5, 4, 3, 2), (256, 128, 64, 32)):
        x = g.deconv_in_relu(f"d{i}", x, cin, cw, 4, 2, 1)
        skip, sw = skips.pop()
        x = g.concat(f"cat{i - 1}", [x, skip])
        cin = cw + sw
    x = g.tanh("out", g.deconv("d1", x, cin, 3, 4, 2, 1))
    return g.finish() + ("data", "out")


def _v2_basic(g, tag, x, c):
    """ShuffleNet v2's basic unit on c channels: Slice in two, the second half through 1x1 - depthwise 3x3 - 1x1, Concat, ShuffleChannel(2)."""
    h = c // 2
    keep, y = g.slice(tag + "_slice", x, [-233, -233])
    y = g.conv_bn_relu(tag + "_pw1", y, h, h, 1)
    y = g.conv_bn_relu(tag + "_dw", y, h, h, 3, 1, 1, group=h, relu=False)
    y = g.conv_bn_relu(tag + "_pw2", y, h, h, 1)
    return g.shuffle(tag + "_shuffle", g.concat(tag + "_concat", [keep, y]), 2)


def _v2_down(g, tag, x, cin, cout):
    """ShuffleNet v2's stride-2 unit: both branches see the whole input and halve the plane; Concat, ShuffleChannel(2)."""
    h = cout // 2
    a, b = g.split(tag + "_split", x)
    a = g.conv_bn_relu(tag + "_b1_dw", a, cin, cin, 3, 2, 1, group=cin, relu=False)
    a = g.conv_bn_relu(tag + "_b1_pw", a, cin, h, 1)
    b = g.conv_bn_relu(tag + "_b2_pw1", b, cin, h, 1)
    b = g.conv_bn_relu(tag + "_b2_dw", b, h, h, 3, 2, 1, group=h, relu=False)
    b = g.conv_bn_relu(tag + "_b2_pw2", b, h, h, 1)
    return g.shuffle(tag + "_shuffle", g.concat(tag + "_concat", [a, b]), 2)


def _v1_unit(g, tag, x, cin, cout, group, stride, first_group=None):
    """ShuffleNet v1's unit: grouped 1x1 to cout / 4, ShuffleChannel(group), depthwise 3x3, grouped 1x1; stride 1 adds the input, stride 2
    concatenates a 3x3 / s2 average pooling of it (no pad: the reference's ceil rule gives the depthwise branch's size) and the branch
    makes up the remaining cout - cin channels."""
    mid = cout // 4
    main, short = g.split(tag + "_split", x)
    y = g.conv_bn_relu(tag + "_g1", main, cin, mid, 1, group=first_group or group)
    y = g.shuffle(tag + "_shuffle", y, group)
    y = g.conv_bn_relu(tag + "_dw", y, mid, mid, 3, stride, 1, group=mid, relu=False)
    if stride == 1:
        y = g.conv_bn_relu(tag + "_g2", y, mid, cout, 1, group=group, relu=False)
        return g.relu(tag + "_relu", g.eltwise(tag + "_sum", short, y))
    y = g.conv_bn_relu(tag + "_g2", y, mid, cout - cin, 1, group=group, relu=False)
    short = g.pool(tag + "_pool", short, 3, 2, avg=True)
    return g.relu(tag + "_relu", g.concat(tag + "_concat", [short, y]))


def tiny_shuffle(seed=19, size=28, dry=False):
    """A small ShuffleNet on ShuffleNet's own late plane sizes: a v2 stride-2 unit (28 -> 14 px), a v2 basic unit and an unequal three-way
    Slice on 14 x 14 (196 floats: 16-byte accesses), a reversed shuffle behind a three-way Concat, a v1 unit with grouped 1x1 convolutions
    and ShuffleChannel(3), a v1 stride-2 unit (14 -> 7 px, average-pooled shortcut) and a v2 basic unit on 7 x 7 (49 floats: the 4-byte
    path).  Fusion level 2 collapses u1_concat -> u1_shuffle -> u2_slice, u2_concat -> u2_shuffle -> three, cat3 -> unshuffle and
    u3_concat -> u3_shuffle."""
    g = GraphBuilder(seed, dry)
    x = g.input("data", 3, size, size)
    x = g.conv_bn_relu("conv1", x, 3, 16, 3, 1, 1)
    x = _v2_down(g, "u1", x, 16, 32)                                     # Concat -> ShuffleChannel, then the next unit's Slice
    x = _v2_basic(g, "u2", x, 32)                                        # ends in Concat -> ShuffleChannel -> Slice(3) below
    a, b, c = g.slice("three", x, [5, -233, 14])                         # 5 / 13 / 14 channels: unequal, one share
    b = g.relu("relu_b", g.conv("conv_b", b, 13, 13, 1))
    x = g.shuffle("unshuffle", g.concat("cat3", [a, b, c]), 4, reverse=True)  # Concat -> ShuffleChannel(reverse) on 32 channels
    x = g.conv_bn_relu("conv2", x, 32, 24, 1)
    x = _v1_unit(g, "v1a", x, 24, 24, 3, 1)                              # grouped 1x1 (24 -> 6, group 3), ShuffleChannel(3), residual sum
    x = _v1_unit(g, "v1b", x, 24, 60, 3, 2)                              # the stride-2 form: average-pooled shortcut, Concat
    x = _v2_basic(g, "u3", x, 60)                                        # 7 x 7 planes
    x = g.pool("gap", x, 1, 1, avg=True, global_=True)
    x = g.softmax("prob", g.fc("fc", x, 60, 10))
    return g.finish() + ("data", "prob")


def shufflenet_v2_x1_0(seed=1234, classes=1000, size=224, dry=False):
    """ShuffleNet v2 1.0x: 24-channel stem, stages of 116 / 232 / 464 channels with 4 / 8 / 4 units (a stride-2 unit, then basic units), a
    1024-channel 1x1 convolution, global pooling, classifier.  Every basic unit's head is a Slice; its tail is Concat -> ShuffleChannel(2)."""
    g = GraphBuilder(seed, dry)
    x = g.input("data", 3, size, size)
    x = g.conv_bn_relu("conv1", x, 3, 24, 3, 2, 1)
    x = g.pool("pool1", x, 3, 2)
    cin = 24
    for si, (c, units) in enumerate([(116, 4), (232, 8), (464, 4)], 2):
        x = _v2_down(g, f"stage{si}_1", x, cin, c)
        for u in range(2, units + 1):
            x = _v2_basic(g, f"stage{si}_{u}", x, c)
        cin = c
    x = g.conv_bn_relu("conv5", x, cin, 1024, 1)
    x = g.pool("gap", x, 7, 1, avg=True, global_=True)
    x = g.softmax("prob", g.fc("fc", x, 1024, classes))
    return g.finish() + ("data", "prob")


def shufflenet_v1_g3(seed=1234, classes=1000, size=224, dry=False):
    """ShuffleNet v1 with 3 groups: 24-channel stem, stages of 240 / 480 / 960 channels with 4 / 8 / 4 units.  The first 1x1 of stage 2 is
    dense (24 input channels), as published; stride-2 units concatenate a 3x3 / s2 average pooling of their input."""
    g = GraphBuilder(seed, dry)
    x = g.input("data", 3, size, size)
    x = g.conv_bn_relu("conv1", x, 3, 24, 3, 2, 1)
    x = g.pool("pool1", x, 3, 2)
    cin = 24
    for si, (c, units) in enumerate([(240, 4), (480, 8), (960, 4)], 2):
        x = _v1_unit(g, f"stage{si}_1", x, cin, c, 3, 2, first_group=1 if si == 2 else None)
        for u in range(2, units + 1):
            x = _v1_unit(g, f"stage{si}_{u}", x, c, c, 3, 1)
        cin = c
    x = g.pool("gap", x, 7, 1, avg=True, global_=True)
    x = g.softmax("prob", g.fc("fc", x, cin, classes))
    return g.finish() + ("data", "prob")


def tiny_dilated(seed=23, size=16, dry=False):
    """A small net of dilated convolutions in every form the Net runtime has to get right, nothing above 16 px (Net.SetDilated(True)):
    a stride-1 "same" layer behind a ReLU (the MFMA route, 64-row tile), one in front of an Eltwise sum, a stride-2 layer with a BatchNorm + Scale +
    ReLU tail (the 128-row tile), a depthwise and a grouped dilated layer, and a layer whose dilation exceeds the plane in front of a 2x2
    pooling (fusions that must decline a dilated layer)."""
    g = GraphBuilder(seed, dry)
    x = g.input("data", 3, size, size)
    x = g.relu("relu1", g.conv("conv1", x, 3, 16, 3, 1, 1))
    x = g.relu("relu_a1", g.conv("a1", x, 16, 64, 3, 1, 2, dilation=2))                     # group 1, stride 1: the MFMA route
    a, b = g.split("split1", x)
    a = g.conv("a2", a, 64, 64, 3, 1, 2, dilation=2)                                        # in front of a residual sum
    x = g.relu("relu_sum", g.eltwise("sum", a, b))
    x = g.conv_bn_relu("a3", x, 64, 96, 3, 2, 2, dilation=2)                                # stride 2; BN + Scale + ReLU
    x = g.relu("relu_dw", g.conv("a_dw", x, 96, 96, 3, 1, 2, group=96, bias=False, dilation=2))  # depthwise
    x = g.relu("relu_g", g.conv("a_g", x, 96, 48, 3, 1, 3, group=4, dilation=3))            # 1 < group < C: this library, not gconv
    x = g.relu("relu_far", g.conv("a_far", x, 48, 48, 3, 1, 12, dilation=12))               # only the centre tap ever lands inside
    x = g.pool("pool1", x, 2, 2)
    x = g.conv("head", x, 48, 8, 1)
    return g.finish() + ("data", "head")


def _deeplab_trunk(g, size):
    """VGG-16 as DeepLab runs it: 3x3 / stride-2 / pad-1 poolings, pool4 and pool5 at stride 1, conv5_* at dilation 2."""
    x = g.input("data", 3, size, size)
    cin = 3
    for stage, (n, c) in enumerate([(2, 64), (2, 128), (3, 256), (3, 512), (3, 512)], 1):
        d = 2 if stage == 5 else 1
        for i in range(1, n + 1):
            x = g.relu(f"relu{stage}_{i}", g.conv(f"conv{stage}_{i}", x, cin, c, 3, 1, d, dilation=d))
            cin = c
        x = g.pool(f"pool{stage}", x, 3, 2 if stage < 4 else 1, 1)
    return x


def _deeplab_head(g, x, tag, rate, classes):
    x = g.dropout("drop6" + tag, g.relu("relu6" + tag, g.conv("fc6" + tag, x, 512, 1024, 3, 1, rate, dilation=rate)))
    x = g.dropout("drop7" + tag, g.relu("relu7" + tag, g.conv("fc7" + tag, x, 1024, 1024, 1)))
    return g.conv("fc8" + tag, x, 1024, classes, 1)


def deeplab_largefov(seed=1234, classes=21, size=321, dry=False):
    """DeepLab-LargeFOV (Chen et al., ICLR 2015): the VGG-16 trunk at output stride 8, fc6 as a 3x3 convolution at dilation 12 with 1024
    channels, fc7 / fc8 1x1; the output is the class score map (41 x 41 at 321 pixels).  Net.SetDilated(True)."""
    g = GraphBuilder(seed, dry)
    x = _deeplab_head(g, _deeplab_trunk(g, size), "", 12, classes)
    return g.finish() + ("data", "fc8")


def deeplab_v2_aspp(seed=1234, classes=21, size=321, dry=False):
    """DeepLab v2's atrous spatial pyramid pooling on the VGG-16 trunk: four fc6 - fc8 branches at rates 6 / 12 / 18 / 24, summed by a chain
    of two-input Eltwise layers.  Net.SetDilated(True)."""
    g = GraphBuilder(seed, dry)
    tops = g.split("pool5_split", _deeplab_trunk(g, size), 4)
    heads = [_deeplab_head(g, t, f"_{j + 1}", rate, classes) for j, (t, rate) in enumerate(zip(tops, (6, 12, 18, 24)))]
    x = g.eltwise("fc8_sum2", heads[0], heads[1])
    x = g.eltwise("fc8_sum3", x, heads[2])
    x = g.eltwise("fc8_sum", x, heads[3])
    return g.finish() + ("data", "fc8_sum")


def tiny_se(seed=29, size=24, dry=False):
    """A small net of squeeze-and-excitation blocks in every form the Net runtime has to get right, nothing above 24 px: block `a` in
    Caffe's spelling (InnerProduct, ReLU, Sigmoid, Scale 0=-233; R = 4) inside a residual unit, followed by Eltwise + ReLU; block `b` in
    the converters' spelling (1x1 Convolution, Swish, Sigmoid, BinaryOp mul; C = 24, R = 6, no multiple of 4) on a 12 x 12 plane behind a
    Swish; block `c` with no activation between its 1x1 convolutions, a HardSigmoid gate and the gate first among BinaryOp's bottoms, on
    an odd 5 x 5 plane (R = 5), followed by nothing; block `d` whose gate blob is also read by a classifier of its own (`aux`), so that
    fusion level 2 must leave it layer by layer."""
    g = GraphBuilder(seed, dry)
    x = g.input("data", 3, size, size)
    x = g.relu("relu1", g.conv("conv1", x, 3, 16, 3, 1, 1))
    short, y = g.split("res_split", x)
    y = g.conv_bn_relu("conv2", y, 16, 16, 3, 1, 1, relu=False)
    y = g.se_block("a", y, 16, 4, "caffe")
    x = g.relu("res_relu", g.eltwise("res", short, y))
    x = g.conv_bn_swish("conv3", x, 16, 24, 3, 2, 1)                                   # 12 x 12, Swish as a layer of its own
    x = g.se_block("b", x, 24, 6, "converter", mact="swish")
    x = g.relu("relu4", g.conv("conv4", x, 24, 20, 3, 2, 0))                            # 5 x 5
    x = g.se_block("c", x, 20, 5, "converter", mact=None, gact="hard_sigmoid", alpha=1.0 / 6, beta=0.5, gate_first=True)
    keep, sq = g.split("d_split", x)
    gate = g.sigmoid("d_sigmoid", g.conv("d_conv2", g.relu("d_relu", g.conv("d_conv1", g.pool("d_gap", sq, 1, 1, avg=True, global_=True), 20, 5, 1)), 5, 20, 1))
    g0, g1 = g.split("d_gate_split", gate)
    x = g.scale_by("d_scale", keep, g0)
    g.fc("aux", g1, 20, 4)                                                              # the gate's second consumer
    x = g.pool("gap", x, 1, 1, avg=True, global_=True)
    x = g.softmax("prob", g.fc("fc", x, 20, 10))
    return g.finish() + ("data", "prob")


def se_resnet50(seed=1234, classes=1000, size=224, dry=False):
    """SE-ResNet-50 (Hu et al.) in Caffe's spelling: `resnet50` with a squeeze-and-excitation block (InnerProduct, ReLU, InnerProduct,
    Sigmoid, Scale 0=-233; reduction 16) behind the last 1x1 of every bottleneck, then the residual Eltwise and its ReLU.  With these random
    weights every residual sum about doubles the variance of the activations; a ReLU net does not mind, but the gate's logits would reach
    several hundred by the last stage, where a Sigmoid turns the fp32 rounding of its input (1e-6 of several hundred) into a gate error of
    1e-3.  So the first excite layer of unit k is scaled by 2^(-k/2) and the logits stay of order one, as in the published net."""
    g = GraphBuilder(seed, dry)
    unit = 0
    x = g.input("data", 3, size, size)
    x = g.conv_bn_relu("conv1", x, 3, 64, 7, 2, 3)
    x = g.pool("pool1", x, 3, 2)
    cin = 64
    for si, (mid, out, blocks, stride) in enumerate([(64, 256, 3, 1), (128, 512, 4, 2), (256, 1024, 6, 2), (512, 2048, 3, 2)]):
        for b in range(blocks):
            s = stride if b == 0 else 1
            tag = f"res{si + 2}{chr(ord('a') + b)}"
            main, short = g.split(tag + "_split", x)
            if b == 0:
                short = g.conv_bn_relu(tag + "_branch1", short, cin, out, 1, s, 0, relu=False)
            y = g.conv_bn_relu(tag + "_branch2a", main, cin, mid, 1, s, 0)
            y = g.conv_bn_relu(tag + "_branch2b", y, mid, mid, 3, 1, 1)
            y = g.conv_bn_relu(tag + "_branch2c", y, mid, out, 1, 1, 0, relu=False)
            y = g.se_block(tag + "_se", y, out, out // 16, "caffe", gain=2.0 ** (-0.5 * unit))
            unit += 1
            x = g.relu(tag + "_relu", g.eltwise(tag, short, y))
            cin = out
    x = g.pool("pool5", x, 7, 1, avg=True, global_=True)
    x = g.softmax("prob", g.fc("fc1000", x, 2048, classes))
    return g.finish() + ("data", "prob")


def efficientnet_b0(seed=1234, classes=1000, size=224, dry=False):
    """EfficientNet-B0 (Tan & Le) in the converters' spelling: MBConv units of a 1x1 expansion, a 3x3 or 5x5 depthwise convolution, a
    squeeze-and-excitation block (1x1 Convolution, Swish, 1x1 Convolution, Sigmoid, BinaryOp mul; reduction to a quarter of the unit's
    input channels) and a 1x1 projection, Swish everywhere else, a residual Eltwise where the unit keeps its shape.  BatchNorm + Scale
    behind every convolution outside the SE blocks, as in the other zoo nets."""
    g = GraphBuilder(seed, dry)
    x = g.input("data", 3, size, size)
    x = g.conv_bn_swish("stem", x, 3, 32, 3, 2, 1)
    cin, unit = 32, 0
    for expand, k, stride, cout, repeats in [(1, 3, 1, 16, 1), (6, 3, 2, 24, 2), (6, 5, 2, 40, 2), (6, 3, 2, 80, 3), (6, 5, 1, 112, 3), (6, 5, 2, 192, 4),
                                             (6, 3, 1, 320, 1)]:
        for rep in range(repeats):
            unit += 1
            tag, s, mid = f"mb{unit}", (stride if rep == 0 else 1), cin * expand
            residual = s == 1 and cin == cout
            if residual:
                x, short = g.split(tag + "_split", x)
            y = g.conv_bn_swish(tag + "_expand", x, cin, mid, 1) if expand != 1 else x
            y = g.conv_bn_swish(tag + "_dw", y, mid, mid, k, s, k // 2, group=mid)
            y = g.se_block(tag + "_se", y, mid, max(1, cin // 4), "converter", mact="swish")
            y = g.conv_bn_swish(tag + "_project", y, mid, cout, 1, swish=False)
            x = g.eltwise(tag + "_add", short, y) if residual else y
            cin = cout
    x = g.conv_bn_swish("head", x, cin, 1280, 1)
    x = g.pool("gap", x, 1, 1, avg=True, global_=True)
    x = g.softmax("prob", g.fc("fc", x, 1280, classes))
    return g.finish() + ("data", "prob")


def tiny_resample(seed=37, size=24, dry=False):
    """A small net of Interp and HardSwish layers in every form the Net runtime has to get right, nothing above 24 px
    (Net.SetExtendedLayers(True)): HardSwish with ncnn's defaults and with MobileNet-V3's 1/6 and 0.5; `up1`, a nearest x2 whose top is read
    by the Eltwise `sum1` alone, with a ReLU behind it (fusion level 2 makes the three one layer; the sum's other operand, `lat`, is produced
    between them); `up2`, a second nearest x2 whose top has two readers and must stay as written; `shrink` and `aligned`, bilinear layers
    with a scale per axis that turn the 12 x 12 plane into 5 x 7 and (align_corner) 9 x 13; `to_ref`, bilinear to the size of a second
    bottom (5 x 7 -> 9 x 13); `down`, nearest from 12 x 12 to a given 5 x 5.  Every size but the last follows the input's."""
    g = GraphBuilder(seed, dry)
    x = g.input("data", 3, size, size)
    x = g.hard_swish("hs1", g.conv("conv1", x, 3, 8, 3, 1, 1))                          # ncnn's defaults, 24 x 24
    big, x = g.split("split0", x)
    x = g.hard_swish("hs2", g.conv("conv2", x, 8, 16, 3, 2, 1), 1.0 / 6, 0.5)           # 12 x 12
    lat_in, down_in, odd_in = g.split("split1", x, 3)
    y = g.relu("relu3", g.conv("conv3", down_in, 16, 16, 3, 2, 1))                      # 6 x 6
    up1 = g.interp("up1", y, "nearest", scale=2.0)                                      # 12 x 12
    lat = g.conv("lat", lat_in, 16, 16, 1)                                              # produced between up1 and sum1
    x = g.relu("sum1_relu", g.eltwise("sum1", lat, up1))                                # up1 -> sum1 -> sum1_relu: one layer at level 2
    s_a, s_b, s_c = g.split("split2", x, 3)
    up2 = g.interp("up2", s_a, "nearest", scale=2.0)                                    # 24 x 24, read by `side` and by `sum2`
    side = g.conv("side", up2, 16, 8, 1)
    t = g.eltwise("sum2", up2, g.conv("big_pw", big, 8, 16, 1))
    head_a = g.pool("gap_a", g.concat("cat_a", [t, side]), 1, 1, avg=True, global_=True)
    q = g.interp("shrink", odd_in, "bilinear", scale=(0.45, 0.6))                       # 12 x 12 -> 5 x 7
    ref_a, ref_b = g.split("split3", g.interp("aligned", s_b, "bilinear", scale=(0.75, 1.1), align_corner=True))  # 12 x 12 -> 9 x 13
    q = g.relu("q_relu", g.conv("q_conv", q, 16, 16, 3, 1, 1))
    z = g.interp("to_ref", q, "bilinear", like=ref_a)                                   # 5 x 7 -> 9 x 13, the size of its second bottom
    head_b = g.pool("gap_b", g.concat("cat_b", [z, ref_b]), 1, 1, avg=True, global_=True)
    d = g.interp("down", s_c, "nearest", size=(5, 5))                                   # 12 x 12 -> 5 x 5, the size given
    head_c = g.pool("gap_c", g.relu("d_relu", g.conv("d_conv", d, 16, 8, 3, 1, 0)), 1, 1, avg=True, global_=True)
    x = g.concat("heads", [head_a, head_b, head_c])
    x = g.softmax("prob", g.fc("fc", x, 64, 10))
    return g.finish() + ("data", "prob")


def _divisible(v, d=8):
    """MobileNet's channel rounding: to the nearest multiple of d, at least d and never below 90 % of v."""
    n = max(d, int(v + d / 2) // d * d)
    return n + d if n < 0.9 * v else n


def _mobilenet_v3(g, rows, last, hidden, classes, size, se_gain=lambda unit: 1.0):
    """The layers both MobileNet-V3 nets share; rows: (kernel, expansion, out, SE, activation, stride).  se_gain(unit) scales the first
    excite layer of that unit (se_block's `gain`)."""
    hs = lambda nm, t: g.hard_swish(nm + "_hs", t, 1.0 / 6, 0.5)
    x = g.input("data", 3, size, size)
    x = hs("conv1", g.conv_bn_relu("conv1", x, 3, 16, 3, 2, 1, relu=False))
    cin = 16
    for i, (k, exp, cout, se, act, s) in enumerate(rows, 1):
        tag = f"b{i}"
        nl = hs if act == "HS" else (lambda nm, t: g.relu(nm + "_relu", t))
        residual = s == 1 and cin == cout
        if residual:
            x, short = g.split(tag + "_split", x)
        y = x
        if exp != cin:
            y = nl(tag + "_expand", g.conv_bn_relu(tag + "_expand", y, cin, exp, 1, relu=False))
        y = nl(tag + "_dw", g.conv_bn_relu(tag + "_dw", y, exp, exp, k, s, k // 2, group=exp, relu=False))
        if se:
            y = g.se_block(tag + "_se", y, exp, _divisible(exp / 4), "converter", mact="relu", gact="hard_sigmoid", alpha=1.0 / 6, beta=0.5, gain=se_gain(i))
        y = g.conv_bn_relu(tag + "_project", y, exp, cout, 1, relu=False)
        x = g.eltwise(tag + "_add", short, y) if residual else y
        cin = cout
    x = hs("conv_last", g.conv_bn_relu("conv_last", x, cin, last, 1, relu=False))
    x = g.pool("gap", x, 1, 1, avg=True, global_=True)
    x = hs("fc1", g.conv("fc1", x, last, hidden, 1, type_="Convolution"))
    x = g.softmax("prob", g.conv("fc2", x, hidden, classes, 1, type_="Convolution"))
    return g.finish() + ("data", "prob")


def mobilenet_v3_large(seed=1234, classes=1000, size=224, dry=False):
    """MobileNet-V3-Large (Howard et al. 2019) in the converters' spelling: inverted-residual units of a 1x1 expansion, a 3x3 or 5x5
    depthwise convolution, a squeeze-and-excitation block (reduction to a quarter, rounded to a multiple of 8; ReLU inside, a
    HardSigmoid(1/6, 0.5) gate, BinaryOp mul) and a 1x1 projection; ReLU in the early units, HardSwish(1/6, 0.5) in the stem, the late units
    and the tail; residuals as Eltwise.  BatchNorm + Scale behind every convolution outside the SE blocks and the classifier.  With these
    random weights the activations grow by about the square root of two per unit, and the gate's logits with them: by the late units every
    HardSigmoid gate would be a step function of its logit's sign, which turns the fp32 rounding of a logit next to zero into a gate error
    of one.  So the first excite layer of unit k is scaled by 2^(-k/2), as in `se_resnet50`, and the gates stay inside their ramp as in a
    trained net.  Net.SetExtendedLayers(True)."""
    rows = [(3, 16, 16, 0, "RE", 1), (3, 64, 24, 0, "RE", 2), (3, 72, 24, 0, "RE", 1), (5, 72, 40, 1, "RE", 2), (5, 120, 40, 1, "RE", 1),
            (5, 120, 40, 1, "RE", 1), (3, 240, 80, 0, "HS", 2), (3, 200, 80, 0, "HS", 1), (3, 184, 80, 0, "HS", 1), (3, 184, 80, 0, "HS", 1),
            (3, 480, 112, 1, "HS", 1), (3, 672, 112, 1, "HS", 1), (5, 672, 160, 1, "HS", 2), (5, 960, 160, 1, "HS", 1), (5, 960, 160, 1, "HS", 1)]
    return _mobilenet_v3(GraphBuilder(seed, dry), rows, 960, 1280, classes, size, se_gain=lambda unit: 2.0 ** (-0.5 * unit))


def mobilenet_v3_small(seed=1234, classes=1000, size=224, dry=False):
    """MobileNet-V3-Small: `mobilenet_v3_large`'s units in the paper's small configuration.  Net.SetExtendedLayers(True)."""
    rows = [(3, 16, 16, 1, "RE", 2), (3, 72, 24, 0, "RE", 2), (3, 88, 24, 0, "RE", 1), (5, 96, 40, 1, "HS", 2), (5, 240, 40, 1, "HS", 1),
            (5, 240, 40, 1, "HS", 1), (5, 120, 48, 1, "HS", 1), (5, 144, 48, 1, "HS", 1), (5, 288, 96, 1, "HS", 2), (5, 576, 96, 1, "HS", 1),
            (5, 576, 96, 1, "HS", 1)]
    return _mobilenet_v3(GraphBuilder(seed, dry), rows, 576, 1024, classes, size)


def deeplab_largefov_full(seed=1234, classes=21, size=321, dry=False):
    """`deeplab_largefov` with its last layer: the class scores (1/8 resolution) resized to the input's size by a bilinear Interp.
    Net.SetDilated(True) and Net.SetExtendedLayers(True)."""
    g = GraphBuilder(seed, dry)
    x = _deeplab_head(g, _deeplab_trunk(g, size), "", 12, classes)
    g.interp("fc8_interp", x, "bilinear", size=(size, size))
    return g.finish() + ("data", "fc8_interp")


def unet_bilinear(seed=1234, size=256, dry=False):
    """`unet_k4` with a bilinear Interp x2 and a 3x3 convolution where that net has a k4 s2 p1 Deconvolution: the decoder of U-Nets that
    avoid the checkerboard of transposed convolutions.  Net.SetExtendedLayers(True)."""
    g = GraphBuilder(seed, dry)
    x = g.input("data", 3, size, size)
    widths = (32, 64, 128, 256, 256)
    skips, cin = [], 3
    for i, cw in enumerate(widths, 1):
        x = g.relu(f"e{i}_relu", g.conv(f"e{i}", x, cin, cw, 4, 2, 1)) if i == 1 else g.conv_bn_relu(f"e{i}", x, cin, cw, 4, 2, 1)
        cin = cw
        if i < len(widths):
            x, skip = g.split(f"e{i}_split", x)
            skips.append((skip, cw))
    for i, cw in zip((5, 4, 3, 2), (256, 128, 64, 32)):
        x = g.conv_bn_relu(f"d{i}", g.interp(f"u{i}", x, "bilinear", scale=2.0), cin, cw, 3, 1, 1)
        skip, sw = skips.pop()
        x = g.concat(f"cat{i - 1}", [x, skip])
        cin = cw + sw
    x = g.conv("d1", g.interp("u1", x, "bilinear", scale=2.0), cin, 3, 3, 1, 1)
    return g.finish() + ("data", "d1")


FPN_OUTPUTS = ("fpn_p2", "fpn_p3", "fpn_p4", "fpn_p5")


def fpn_resnet50(seed=1234, size=224, dry=False):
    """A feature pyramid network (Lin et al. 2017) on `resnet50`'s stages: C2 .. C5 (256 .. 2048 channels at strides 4 .. 32), a 1x1 lateral
    convolution to 256 channels on each, the top-down path -- a nearest Interp of the level above to the lateral's size (x2), added to it --
    and a 3x3 output convolution per level.  The outputs are FPN_OUTPUTS; the builder names the finest.  Net.SetExtendedLayers(True)."""
    g = GraphBuilder(seed, dry)
    x = g.input("data", 3, size, size)
    x = g.conv_bn_relu("conv1", x, 3, 64, 7, 2, 3)
    x = g.pool("pool1", x, 3, 2)
    cin, feats = 64, []
    for si, (mid, out, blocks, stride) in enumerate([(64, 256, 3, 1), (128, 512, 4, 2), (256, 1024, 6, 2), (512, 2048, 3, 2)]):
        for b in range(blocks):
            s = stride if b == 0 else 1
            tag = f"res{si + 2}{chr(ord('a') + b)}"
            main, short = g.split(tag + "_split", x)
            if b == 0:
                short = g.conv_bn_relu(tag + "_branch1", short, cin, out, 1, s, 0, relu=False)
            y = g.conv_bn_relu(tag + "_branch2a", main, cin, mid, 1, s, 0)
            y = g.conv_bn_relu(tag + "_branch2b", y, mid, mid, 3, 1, 1)
            y = g.conv_bn_relu(tag + "_branch2c", y, mid, out, 1, 1, 0, relu=False)
            x = g.relu(tag + "_relu", g.eltwise(tag, short, y))
            cin = out
        if si < 3:
            x, c = g.split(f"c{si + 2}_split", x)
        else:
            c = x
        feats.append((c, out))
    top = None
    for level in (5, 4, 3, 2):
        c, width = feats[level - 2]
        m = g.conv(f"fpn_lat{level}", c, width, 256, 1)
        if top is not None:
            m = g.eltwise(f"fpn_sum{level}", m, g.interp(f"fpn_up{level}", top, "nearest", like=m))
        if level > 2:
            m, top = g.split(f"fpn_m{level}_split", m)
        g.conv(f"fpn_p{level}", m, 256, 256, 3, 1, 1)
    return g.finish() + ("data", "fpn_p2")


def tiny_lrn(seed=41, size=16, dry=False):
    """A small net of LRN layers in every form the Net runtime has to get right (Net.SetExtendedLayers(True)): `norm1`, across 20 channels
    (more than one chunk of 16) in front of a 3 x 3 / stride-2 max pooling whose last window hangs over the 16 x 16 plane (fusion level 2
    makes the two one layer); `norm2`, within channel with beta 0.5, in front of a 2 x 2 average pooling (one layer too); `norm3`, beta 0.6
    and bias 2, whose top is read by `pool3` and by `conv3` and must stay as written; `norm4` behind the pooling `pool4` (Pooling -> LRN is
    not fused) and in front of a global pooling (not fused either); `norm5` on 3 channels, fewer than its local_size 5, in front of a padded
    3 x 3 / stride-1 average pooling."""
    g = GraphBuilder(seed, dry)
    x = g.input("data", 3, size, size)
    x = g.relu("relu1", g.conv("conv1", x, 3, 20, 3, 1, 1))
    x = g.pool("pool1", g.lrn("norm1", x, 5, 1.0, 0.75), 3, 2)                          # 16 x 16 -> 8 x 8, ceil mode
    x = g.relu("relu2", g.conv("conv2", x, 20, 12, 3, 1, 1))
    x = g.pool("pool2", g.lrn("norm2", x, 3, 2.0, 0.5, region=1), 2, 2, avg=True)       # 4 x 4
    a, b, c = g.split("split1", x, 3)
    n3 = g.lrn("norm3", a, 5, 0.5, 0.6, bias=2.0)                                       # read twice
    head_a = g.pool("gap_a", g.pool("pool3", n3, 2, 2), 1, 1, avg=True, global_=True)
    head_b = g.pool("gap_b", g.relu("relu3", g.conv("conv3", n3, 12, 8, 1)), 1, 1, avg=True, global_=True)
    head_c = g.pool("gap_c", g.lrn("norm4", g.pool("pool4", b, 2, 2), 3, 1.0, 0.75), 1, 1, avg=True, global_=True)
    n5 = g.lrn("norm5", g.conv("conv5", c, 12, 3, 1), 5, 1.0, 0.75)                     # 3 channels, local_size 5
    head_d = g.pool("gap_d", g.pool("pool5", n5, 3, 1, 1, avg=True), 1, 1, avg=True, global_=True)
    x = g.concat("heads", [head_a, head_b, head_c, head_d])
    x = g.softmax("prob", g.fc("fc", x, 35, 10))
    return g.finish() + ("data", "prob")


def _pool3s2(v):
    return -(-(v - 3) // 2) + 1  # 3 x 3 / stride 2, ceil mode


def _alexnet(seed, classes, size, dry, norm_first):
    g = GraphBuilder(seed, dry)
    x = g.input("data", 3, size, size)

    def stage(i, x, cin, cout, k, s, p, group):
        x = g.relu(f"relu{i}", g.conv(f"conv{i}", x, cin, cout, k, s, p, group))
        if norm_first:
            return g.pool(f"pool{i}", g.lrn(f"norm{i}", x, 5, 1e-4, 0.75), 3, 2)
        return g.lrn(f"norm{i}", g.pool(f"pool{i}", x, 3, 2), 5, 1e-4, 0.75)

    x = stage(1, x, 3, 96, 11, 4, 0, 1)
    x = stage(2, x, 96, 256, 5, 1, 2, 2)
    x = g.relu("relu3", g.conv("conv3", x, 256, 384, 3, 1, 1))
    x = g.relu("relu4", g.conv("conv4", x, 384, 384, 3, 1, 1, 2))
    x = g.relu("relu5", g.conv("conv5", x, 384, 256, 3, 1, 1, 2))
    x = g.pool("pool5", x, 3, 2)
    feat = 256 * _pool3s2(_pool3s2(_pool3s2((size - 11) // 4 + 1))) ** 2
    x = g.dropout("drop6", g.relu("relu6", g.fc("fc6", x, feat, 4096)))
    x = g.dropout("drop7", g.relu("relu7", g.fc("fc7", x, 4096, 4096)))
    x = g.softmax("prob", g.fc("fc8", x, 4096, classes))
    return g.finish() + ("data", "prob")


def alexnet(seed=1234, classes=1000, size=227, dry=False):
    """BVLC AlexNet: 227 px, conv2 / conv4 / conv5 in two groups, norm1 / norm2 (LRN 5 / 1e-4 / 0.75) in front of pool1 / pool2.  The
    smallest input is 67 px (pool5 then sees a 3 x 3 plane)."""
    return _alexnet(seed, classes, size, dry, norm_first=True)


def caffenet(seed=1234, classes=1000, size=227, dry=False):
    """BVLC reference CaffeNet: AlexNet with pool1 / pool2 in front of norm1 / norm2."""
    return _alexnet(seed, classes, size, dry, norm_first=False)


def googlenet(seed=1234, classes=1000, size=224, dry=False):
    """BVLC GoogLeNet (Inception v1) without the two auxiliary classifiers: pool1 -> norm1 and norm2 -> pool2 (LRN 5 / 1e-4 / 0.75), nine
    inception modules, global average pooling.  Four ceil-mode 3 x 3 / stride-2 poolings behind a stride-2 convolution: the smallest input
    that leaves every one of them a non-empty output is 31 px (16, 8, 4, 2 and 1 pixels a side)."""
    g = GraphBuilder(seed, dry)
    x = g.input("data", 3, size, size)
    x = g.relu("conv1/relu_7x7", g.conv("conv1/7x7_s2", x, 3, 64, 7, 2, 3))
    x = g.lrn("pool1/norm1", g.pool("pool1/3x3_s2", x, 3, 2), 5, 1e-4, 0.75)
    x = g.relu("conv2/relu_3x3_reduce", g.conv("conv2/3x3_reduce", x, 64, 64, 1))
    x = g.relu("conv2/relu_3x3", g.conv("conv2/3x3", x, 64, 192, 3, 1, 1))
    x = g.pool("pool2/3x3_s2", g.lrn("conv2/norm2", x, 5, 1e-4, 0.75), 3, 2)
    cin = 192

    def inception(tag, x, cin, n1, n3r, n3, n5r, n5, pp):
        a, b, c, d = g.split(tag + "/split", x, 4)
        a = g.relu(tag + "/relu_1x1", g.conv(tag + "/1x1", a, cin, n1, 1))
        b = g.relu(tag + "/relu_3x3_reduce", g.conv(tag + "/3x3_reduce", b, cin, n3r, 1))
        b = g.relu(tag + "/relu_3x3", g.conv(tag + "/3x3", b, n3r, n3, 3, 1, 1))
        c = g.relu(tag + "/relu_5x5_reduce", g.conv(tag + "/5x5_reduce", c, cin, n5r, 1))
        c = g.relu(tag + "/relu_5x5", g.conv(tag + "/5x5", c, n5r, n5, 5, 1, 2))
        d = g.pool(tag + "/pool", d, 3, 1, 1)
        d = g.relu(tag + "/relu_pool_proj", g.conv(tag + "/pool_proj", d, cin, pp, 1))
        return g.concat(tag + "/output", [a, b, c, d]), n1 + n3 + n5 + pp

    cfg = {"3a": (64, 96, 128, 16, 32, 32), "3b": (128, 128, 192, 32, 96, 64),
           "4a": (192, 96, 208, 16, 48, 64), "4b": (160, 112, 224, 24, 64, 64), "4c": (128, 128, 256, 24, 64, 64),
           "4d": (112, 144, 288, 32, 64, 64), "4e": (256, 160, 320, 32, 128, 128),
           "5a": (256, 160, 320, 32, 128, 128), "5b": (384, 192, 384, 48, 128, 128)}
    for tag, widths in cfg.items():
        x, cin = inception("inception_" + tag, x, cin, *widths)
        if tag in ("3b", "4e"):
            x = g.pool(f"pool{tag[0]}/3x3_s2", x, 3, 2)
    x = g.pool("pool5/7x7_s1", x, 7, 1, avg=True, global_=True)
    x = g.dropout("pool5/drop_7x7_s1", x)
    x = g.softmax("prob", g.fc("loss3/classifier", x, 1024, classes))
    return g.finish() + ("data", "prob")


def tiny_ssd(seed=43, size=(20, 28), dry=False):
    """A small SSD (Net.SetDetection(True)): a 20 x 28 image, three source maps -- 10 x 14 behind a Normalize, 5 x 7 and 3 x 4 -- with 3, 6 and 4
    priors per cell (678 priors), 3 classes.  size = (height, width)."""
    h, w = size
    g = GraphBuilder(seed, dry)
    data, image = g.split("data_split", g.input("data", 3, h, w), 2)
    x = g.pool("pool1", g.relu("relu1", g.conv("conv1", data, 3, 16, 3, 1, 1)), 2, 2)
    a = g.relu("relu2", g.conv("conv2", x, 16, 24, 3, 1, 1))
    a, keep = g.split("split2", a, 2)
    b = g.relu("relu3", g.conv("conv3", keep, 24, 32, 3, 2, 1))
    b, keep = g.split("split3", b, 2)
    c = g.relu("relu4", g.conv("conv4", keep, 32, 32, 3, 2, 1))
    sources = [("conv2_norm", g.normalize("conv2_norm", a, 24, scale=2.0), 24, 3, dict(min_sizes=[4.0], ratios=[2.0])),
               ("conv3", b, 32, 6, dict(min_sizes=[8.0], max_sizes=[12.0], ratios=[2.0, 3.0], clip=True)),
               ("conv4", c, 32, 4, dict(min_sizes=[12.0], max_sizes=[16.0], ratios=[2.0, 3.0], flip=False))]
    g.ssd_head(image, sources, 3, conf_gain=2.0, nms_threshold=0.45, nms_top_k=40, keep_top_k=20, confidence_threshold=0.95)
    return g.finish() + ("data", "detection_out")


def mobilenet_ssd(seed=1234, classes=21, size=300, dry=False, confidence_threshold=0.25, conf_gain=0.2):
    """MobileNet-SSD (the Caffe model ncnn's example application runs): the MobileNet v1 trunk at 300 px, four extra 1x1 / 3x3-stride-2 pairs,
    six source maps of 19, 10, 5, 3, 2 and 1 cells with 3, 6, 6, 6, 6, 6 priors per cell: 1917 priors.  Net.SetDetection(True)."""
    g = GraphBuilder(seed, dry)
    data, image = g.split("data_split", g.input("data", 3, size, size), 2)
    x = g.conv_bn_relu("conv0", data, 3, 32, 3, 2, 1)
    cfg = [(32, 64, 1), (64, 128, 2), (128, 128, 1), (128, 256, 2), (256, 256, 1), (256, 512, 2)] + [(512, 512, 1)] * 5 + \
          [(512, 1024, 2), (1024, 1024, 1)]
    maps = {}
    for i, (c, k, s) in enumerate(cfg, 1):
        x = g.conv_bn_relu(f"conv{i}_dw", x, c, c, 3, s, 1, group=c)
        x = g.conv_bn_relu(f"conv{i}", x, c, k, 1, 1, 0)
        if i in (11, 13):
            maps[i], x = g.split(f"conv{i}_split", x, 2)
    cin = 1024
    for i, (mid, out) in enumerate([(256, 512), (128, 256), (128, 256), (64, 128)], 14):
        x = g.conv_bn_relu(f"conv{i}_1", x, cin, mid, 1, 1, 0)
        x = g.conv_bn_relu(f"conv{i}_2", x, mid, out, 3, 2, 1)
        cin = out
        if i < 17:
            maps[i], x = g.split(f"conv{i}_split", x, 2)
        else:
            maps[i] = x
    box = lambda mn, mx: dict(min_sizes=[mn], max_sizes=[mx], ratios=[2.0, 3.0])
    sources = [("conv11", maps[11], 512, 3, dict(min_sizes=[60.0], ratios=[2.0])), ("conv13", maps[13], 1024, 6, box(105.0, 150.0)),
               ("conv14_2", maps[14], 512, 6, box(150.0, 195.0)), ("conv15_2", maps[15], 256, 6, box(195.0, 240.0)),
               ("conv16_2", maps[16], 256, 6, box(240.0, 285.0)), ("conv17_2", maps[17], 128, 6, box(285.0, 300.0))]
    g.ssd_head(image, sources, classes, conf_gain=conf_gain, loc_gain=0.02, nms_threshold=0.45, nms_top_k=100, keep_top_k=100, confidence_threshold=confidence_threshold)
    return g.finish() + ("data", "detection_out")


def vgg16_ssd300(seed=1234, classes=21, size=300, dry=False, confidence_threshold=0.01):
    """SSD300 on VGG-16 (Liu et al., ECCV 2016): conv4_3 behind a Normalize (scale 20), pool5 3x3 / stride 1, fc6 as a 3x3 convolution at
    dilation 6, fc7 1x1, four extra pairs; source maps of 38, 19, 10, 5, 3 and 1 cells with 4, 6, 6, 6, 4, 4 priors per cell: 8732 priors.
    Net.SetDetection(True) and Net.SetDilated(True)."""
    g = GraphBuilder(seed, dry)
    data, image = g.split("data_split", g.input("data", 3, size, size), 2)
    x, cin, maps = data, 3, {}
    for stage, (n, c) in enumerate([(2, 64), (2, 128), (3, 256), (3, 512), (3, 512)], 1):
        for i in range(1, n + 1):
            x = g.relu(f"relu{stage}_{i}", g.conv(f"conv{stage}_{i}", x, cin, c, 3, 1, 1))
            cin = c
        if stage == 4:
            maps["conv4_3"], x = g.split("conv4_3_split", x, 2)
        x = g.pool(f"pool{stage}", x, 2, 2) if stage < 5 else g.pool("pool5", x, 3, 1, 1)  # ceil mode: 75 -> 38
    x = g.relu("relu6", g.conv("fc6", x, 512, 1024, 3, 1, 6, dilation=6))
    x = g.relu("relu7", g.conv("fc7", x, 1024, 1024, 1))
    maps["fc7"], x = g.split("fc7_split", x, 2)
    cin = 1024
    for i, (mid, out, s, p) in enumerate([(256, 512, 2, 1), (128, 256, 2, 1), (128, 256, 1, 0), (128, 256, 1, 0)], 6):
        x = g.relu(f"conv{i}_1_relu", g.conv(f"conv{i}_1", x, cin, mid, 1))
        x = g.relu(f"conv{i}_2_relu", g.conv(f"conv{i}_2", x, mid, out, 3, s, p))
        cin = out
        if i < 9:
            maps[f"conv{i}_2"], x = g.split(f"conv{i}_2_split", x, 2)
        else:
            maps[f"conv{i}_2"] = x
    norm = g.normalize("conv4_3_norm", maps["conv4_3"], 512, scale=20.0)
    box = lambda mn, mx, r, st: dict(min_sizes=[mn], max_sizes=[mx], ratios=r, step=st)
    sources = [("conv4_3_norm", norm, 512, 4, box(30.0, 60.0, [2.0], 8.0)), ("fc7", maps["fc7"], 1024, 6, box(60.0, 111.0, [2.0, 3.0], 16.0)),
               ("conv6_2", maps["conv6_2"], 512, 6, box(111.0, 162.0, [2.0, 3.0], 32.0)), ("conv7_2", maps["conv7_2"], 256, 6, box(162.0, 213.0, [2.0, 3.0], 64.0)),
               ("conv8_2", maps["conv8_2"], 256, 4, box(213.0, 264.0, [2.0], 100.0)), ("conv9_2", maps["conv9_2"], 256, 4, box(264.0, 315.0, [2.0], 300.0))]
    g.ssd_head(image, sources, classes, conf_gain=2.0, loc_gain=0.25, nms_threshold=0.45, nms_top_k=400, keep_top_k=200, confidence_threshold=confidence_threshold)
    return g.finish() + ("data", "detection_out")


def tiny_yolov2(seed=47, size=(12, 20), dry=False, trace=None, confidence_threshold=0.3, nms_threshold=0.45):
    """A small YOLOv2 (Net.SetYolo()): a 12 x 20 image, convolutions of 3 -> 8 channels, the passthrough of YOLOv2 -- a Reorg 0=2 of the
    full-resolution map concatenated with the trunk behind a pooling -- a 1x1 head of 2 boxes x (5 + 3 classes) on 6 x 10 cells and
    YoloDetectionOutput.  size = (height, width); trace: a list that receives the layers for numpy_forward."""
    h, w = size
    g = GraphBuilder(seed, dry)
    g.trace = trace
    x = g.relu("relu1", g.conv("conv1", g.input("data", 3, h, w), 3, 8, 3, 1, 1))
    fine, x = g.split("split1", x, 2)
    x = g.relu("relu2", g.conv("conv2", g.pool("pool1", x, 2, 2), 8, 8, 3, 1, 1))
    x = g.concat("route", [g.reorg("reorg", fine, 2), x])
    head = g.conv("head", x, 40, 2 * (5 + 3), 1, gain=3.0)
    g.yolo_detection_output("detection_out", [head], 3, 2, [1.5, 2.0, 3.0, 2.5], confidence_threshold, nms_threshold)
    return g.finish() + ("data", "detection_out")


def tiny_yolov3(seed=53, size=(16, 24), dry=False, trace=None, confidence_threshold=0.3, nms_threshold=0.45):
    """A small YOLOv3 (Net.SetYolo() and Net.SetExtendedLayers(True)): a 16 x 24 image, a head on 4 x 6 cells (stride 4), a nearest Interp x2
    of its branch concatenated with the 8 x 12 map and a second head there (stride 2); Yolov3DetectionOutput with 2 of 4 anchors per scale
    through masks, 3 classes.  size = (height, width); trace: a list that receives the layers for numpy_forward."""
    h, w = size
    g = GraphBuilder(seed, dry)
    g.trace = trace
    x = g.pool("pool1", g.relu("relu1", g.conv("conv1", g.input("data", 3, h, w), 3, 8, 3, 1, 1)), 2, 2)
    fine, x = g.split("split1", x, 2)
    x = g.relu("relu2", g.conv("conv2", x, 8, 16, 3, 2, 1))
    coarse, x = g.split("split2", x, 2)
    head1 = g.conv("head1", coarse, 16, 2 * (5 + 3), 1, gain=3.0)
    x = g.interp("up", g.relu("relu3", g.conv("conv3", x, 16, 8, 1)), mode="nearest", scale=2.0)
    x = g.relu("relu4", g.conv("conv4", g.concat("route", [x, fine]), 16, 8, 3, 1, 1))
    head2 = g.conv("head2", x, 8, 2 * (5 + 3), 1, gain=3.0)
    g.yolov3_detection_output("detection_out", [head1, head2], 3, 2, [3.0, 4.0, 5.0, 3.0, 7.0, 9.0, 10.0, 6.0], [2, 3, 0, 1], [4.0, 2.0],
                              confidence_threshold, nms_threshold)
    return g.finish() + ("data", "detection_out")


def yolov2_tiny_voc(seed=1234, classes=20, size=416, dry=False, confidence_threshold=0.25, nms_threshold=0.45):
    """YOLOv2-tiny for VOC (Redmon & Farhadi 2017, tiny-yolo-voc.cfg as darknet2ncnn writes it): six 3x3 convolutions of 16 .. 512 channels,
    each BatchNorm + Scale + leaky ReLU 0.1 and a 2x2 max pooling (the sixth with stride 1, padded right and below), two of 1024, a linear 1x1
    head of 5 boxes x (5 + 20) = 125 channels on 13 x 13 cells at 416 px, YoloDetectionOutput.  Net.SetYolo()."""
    g = GraphBuilder(seed, dry)
    x, cin = g.input("data", 3, size, size), 3
    for i, c in enumerate((16, 32, 64, 128, 256, 512), 1):
        x = g.relu(f"conv{i}_leaky", g.scale(f"conv{i}_scale", g.bn(f"conv{i}_bn", g.conv(f"conv{i}", x, cin, c, 3, 1, 1, bias=False), c), c), 0.1)
        x = g.pool(f"pool{i}", x, 2, 2) if i < 6 else g.layer("Pooling", "pool6", [x], ["pool6"], {0: 0, 1: 2, 2: 1, 3: 0, 4: 0, 14: 1, 15: 1})
        cin = c
    for i in (7, 8):
        x = g.relu(f"conv{i}_leaky", g.scale(f"conv{i}_scale", g.bn(f"conv{i}_bn", g.conv(f"conv{i}", x, cin, 1024, 3, 1, 1, bias=False), 1024), 1024), 0.1)
        cin = 1024
    head = g.conv("conv9", x, 1024, 5 * (5 + classes), 1)
    g.yolo_detection_output("detection_out", [head], classes, 5, [1.08, 1.19, 3.42, 4.41, 6.63, 11.38, 9.42, 5.11, 16.62, 10.52], confidence_threshold,
                            nms_threshold)
    return g.finish() + ("data", "detection_out")


def mobilenetv2_yolov3(seed=1234, classes=20, size=352, dry=False, confidence_threshold=0.25, nms_threshold=0.45):
    """MobileNetV2-YOLOv3 at 352 px, the topology of the MobileNet-YOLO model ncnn's yolov3 example runs: the MobileNetV2 trunk (Sandler et al.
    2018) to 1280 channels on 11 x 11 cells, depthwise-separable head convolutions, a linear 1x1 head of 3 boxes x (5 + 20) = 75 channels
    there; a DeconvolutionDepthWise x2 of the head's trunk added (Eltwise SUM) to a lateral of the 22 x 22 map, and a second head on it;
    Yolov3DetectionOutput over both with masks 3, 4, 5 and 0, 1, 2 and strides 32 and 16.  Net.SetYolo()."""
    g = GraphBuilder(seed, dry)
    x = g.conv_bn_relu("conv1", g.input("data", 3, size, size), 3, 32, 3, 2, 1)
    cin, unit, maps = 32, 0, {}

    def dwpw(name, x, cin, cout, s=1, relu=True):
        x = g.conv_bn_relu(name + "/dw", x, cin, cin, 3, s, 1, group=cin)
        return g.conv_bn_relu(name, x, cin, cout, 1, relu=relu)

    for t, c, n, s in ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1)):
        for i in range(n):
            unit += 1
            stride = s if i == 0 else 1
            keep = None
            if stride == 1 and cin == c:
                keep, x = g.split(f"block{unit}_split", x, 2)
            y = g.conv_bn_relu(f"block{unit}_expand", x, cin, cin * t, 1) if t != 1 else x
            y = g.conv_bn_relu(f"block{unit}_dw", y, cin * t, cin * t, 3, stride, 1, group=cin * t)
            y = g.conv_bn_relu(f"block{unit}_project", y, cin * t, c, 1, relu=False)
            x = g.eltwise(f"block{unit}_sum", keep, y) if keep is not None else y
            cin = c
        if c == 96:
            maps[16], x = g.split("stride16_split", x, 2)
    x = g.conv_bn_relu("conv_last", x, 320, 1280, 1)
    x = dwpw("yolo/conv1", x, 1280, 1024)
    up, x = g.split("yolo/split", x, 2)
    head1 = g.conv("yolo/conv4", dwpw("yolo/conv2", x, 1024, 1024), 1024, 3 * (5 + classes), 1)
    up = g.deconv("upsample", g.conv_bn_relu("yolo/reduce", up, 1024, 512, 1), 512, 512, 4, 2, 1, group=512, bias=False)
    x = g.eltwise("yolo/sum", up, dwpw("yolo/lateral", maps[16], 96, 512))
    head2 = g.conv("yolo/conv5", dwpw("yolo/conv3", x, 512, 512), 512, 3 * (5 + classes), 1)
    g.yolov3_detection_output("detection_out", [head1, head2], classes, 3, [20, 37, 49, 94, 73, 201, 143, 265, 153, 121, 280, 279], [3, 4, 5, 0, 1, 2],
                              [32.0, 16.0], confidence_threshold, nms_threshold)
    return g.finish() + ("data", "detection_out")


def _rpn(g, x, cin, mid, im_info, gain=1.0, **proposal):
    """The region proposal network of py-faster-rcnn on the map `x`: a 3x3 convolution + ReLU, the 1x1 score (2 * 9) and delta (4 * 9) heads, the
    two-way softmax and Proposal -> the ROIs."""
    x = g.relu("rpn_relu/3x3", g.conv("rpn_conv/3x3", x, cin, mid, 3, 1, 1))
    a, b = g.split("rpn_split", x, 2)
    score = g.rpn_softmax("rpn_cls", g.conv("rpn_cls_score", a, mid, 18, 1, gain=gain))
    bbox = g.conv("rpn_bbox_pred", b, mid, 36, 1, gain=0.3)
    return g.proposal("rois", score, bbox, im_info, **proposal)


def tiny_faster_rcnn(seed=59, size=(48, 64), dry=False, trace=None, rois=16):
    """A small Faster R-CNN (Net.SetDetection(True) for the RPN's softmax, Net.SetRoi()): a 48 x 64 image, a trunk of two convolutions and two
    poolings to 16 channels on 12 x 16 cells (stride 4), a 3x3 RPN convolution, rpn_cls_score through Reshape -> Softmax -> Reshape into
    Proposal (feat_stride 4, base_size 2: anchors of 8 .. 64 px; 200 -> `rois` ROIs), ROIPooling 3 x 3, two InnerProduct layers over the
    batch of n * rois regions, cls_prob (Softmax, 5 classes) and bbox_pred.  Inputs "data" and "im_info" ([n][1][1][3]); outputs "rois",
    "cls_prob", "bbox_pred".  size = (height, width); trace: a list that receives the layers for numpy_forward."""
    h, w = size
    g = GraphBuilder(seed, dry)
    g.trace = trace
    x = g.pool("pool1", g.relu("relu1", g.conv("conv1", g.input("data", 3, h, w), 3, 8, 3, 1, 1)), 2, 2)
    x = g.pool("pool2", g.relu("relu2", g.conv("conv2", x, 8, 16, 3, 1, 1)), 2, 2)
    im_info = g.input("im_info", 1, 1, 3)
    feat, x = g.split("feat_split", x, 2)
    r = _rpn(g, x, 16, 16, im_info, gain=0.25, feat_stride=4, base_size=2, pre_nms_topN=200, after_nms_topN=rois, nms_thresh=0.7, min_size=4)
    x = g.roi_pooling("roi_pool", feat, r, 3, 3, 0.25)
    x = g.relu("relu6", g.fc("fc6", x, 16 * 9, 32))
    x = g.relu("relu7", g.fc("fc7", x, 32, 32))
    a, b = g.split("fc7_split", x, 2)
    g.softmax("cls_prob", g.fc("cls_score", a, 32, 5))
    g.fc("bbox_pred", b, 32, 20)
    return g.finish() + ("data", "cls_prob")


def tiny_rfcn(seed=61, size=(48, 64), dry=False, trace=None, rois=16):
    """A small R-FCN (Net.SetDetection(True), Net.SetRoi()): the trunk and the RPN of tiny_faster_rcnn, a 1x1 convolution to 5 classes x 3 x 3
    position-sensitive score maps, PSROIPooling 3 x 3 and a global average Pooling: the vote.  Inputs "data" and "im_info"; outputs "rois" and
    "cls_score" ([n * rois][5][1][1])."""
    h, w = size
    g = GraphBuilder(seed, dry)
    g.trace = trace
    x = g.pool("pool1", g.relu("relu1", g.conv("conv1", g.input("data", 3, h, w), 3, 8, 3, 1, 1)), 2, 2)
    x = g.pool("pool2", g.relu("relu2", g.conv("conv2", x, 8, 16, 3, 1, 1)), 2, 2)
    im_info = g.input("im_info", 1, 1, 3)
    feat, x = g.split("feat_split", x, 2)
    r = _rpn(g, x, 16, 16, im_info, gain=0.25, feat_stride=4, base_size=2, pre_nms_topN=200, after_nms_topN=rois, nms_thresh=0.7, min_size=4)
    maps = g.conv("rfcn_cls", feat, 16, 5 * 9, 1)
    g.pool("cls_score", g.psroi_pooling("psroi_cls", maps, r, 5, 3, 3, 0.25), 3, 3, avg=True, global_=True)
    return g.finish() + ("data", "cls_score")


def faster_rcnn_vgg16(seed=1234, classes=21, size=(600, 800), dry=False):
    """Faster R-CNN on VGG-16 (Ren et al., NIPS 2015; py-faster-rcnn's VGG16 test.prototxt): conv1_1 .. conv5_3 without pool5 (stride 16: 38 x 50
    cells at 600 x 800), the RPN on 512 channels, Proposal 6000 -> 300, ROIPooling 7 x 7, fc6 / fc7 of 4096 over the 300 regions of every
    image, cls_prob over 21 classes and bbox_pred.  Net.SetDetection(True) and Net.SetRoi(); inputs "data" and "im_info"."""
    h, w = size
    g = GraphBuilder(seed, dry)
    x, cin = g.input("data", 3, h, w), 3
    for stage, (n, c) in enumerate([(2, 64), (2, 128), (3, 256), (3, 512), (3, 512)], 1):
        for i in range(1, n + 1):
            x = g.relu(f"relu{stage}_{i}", g.conv(f"conv{stage}_{i}", x, cin, c, 3, 1, 1))
            cin = c
        if stage < 5:
            x = g.pool(f"pool{stage}", x, 2, 2)
    im_info = g.input("im_info", 1, 1, 3)
    feat, x = g.split("conv5_3_split", x, 2)
    r = _rpn(g, x, 512, 512, im_info)
    x = g.roi_pooling("roi_pool5", feat, r, 7, 7, 0.0625)
    x = g.dropout("drop6", g.relu("relu6", g.fc("fc6", x, 512 * 49, 4096)))
    x = g.dropout("drop7", g.relu("relu7", g.fc("fc7", x, 4096, 4096)))
    a, b = g.split("fc7_split", x, 2)
    g.softmax("cls_prob", g.fc("cls_score", a, 4096, classes))
    g.fc("bbox_pred", b, 4096, 4 * classes)
    return g.finish() + ("data", "cls_prob")


def rfcn_resnet50(seed=1234, classes=21, size=(600, 800), dry=False):
    """R-FCN on ResNet-50 (Dai et al., NIPS 2016): conv1 .. conv4 at stride 16, conv5 at stride 1 and dilation 2, a 1x1 convolution to 1024
    channels, the RPN on conv4, position-sensitive score maps of 21 x 7 x 7 and class-agnostic box maps of 8 x 7 x 7, PSROIPooling 7 x 7 over
    300 ROIs and a global average Pooling each: cls_prob and bbox_pred.  Net.SetDetection(True), Net.SetRoi() and Net.SetDilated(True)."""
    h, w = size
    g = GraphBuilder(seed, dry)
    x = g.input("data", 3, h, w)
    x = g.pool("pool1", g.conv_bn_relu("conv1", x, 3, 64, 7, 2, 3), 3, 2)
    im_info = g.input("im_info", 1, 1, 3)
    cin, rois = 64, None
    for si, (mid, out, blocks, stride, dilation) in enumerate([(64, 256, 3, 1, 1), (128, 512, 4, 2, 1), (256, 1024, 6, 2, 1), (512, 2048, 3, 1, 2)]):
        for b in range(blocks):
            s = stride if b == 0 else 1
            tag = f"res{si + 2}{chr(ord('a') + b)}"
            main, short = g.split(tag + "_split", x)
            if b == 0:
                short = g.conv_bn_relu(tag + "_branch1", short, cin, out, 1, s, 0, relu=False)
            y = g.conv_bn_relu(tag + "_branch2a", main, cin, mid, 1, s, 0)
            y = g.conv_bn_relu(tag + "_branch2b", y, mid, mid, 3, 1, dilation, dilation=dilation)
            y = g.conv_bn_relu(tag + "_branch2c", y, mid, out, 1, 1, 0, relu=False)
            x = g.relu(tag + "_relu", g.eltwise(tag, short, y))
            cin = out
        if si == 2:  # the RPN reads conv4
            x, rpn = g.split("res4f_split", x, 2)
            rois = _rpn(g, rpn, 1024, 512, im_info)
    x = g.relu("conv_new_1_relu", g.conv("conv_new_1", x, 2048, 1024, 1))
    a, b = g.split("conv_new_1_split", x, 2)
    ra, rb = g.split("rois_split", rois, 2)
    cls = g.psroi_pooling("psroipooled_cls_rois", g.conv("rfcn_cls", a, 1024, classes * 49, 1), ra, classes, 7, 7, 0.0625)
    g.softmax("cls_prob", g.pool("ave_cls_score_rois", cls, 7, 7, avg=True, global_=True))
    box = g.psroi_pooling("psroipooled_loc_rois", g.conv("rfcn_bbox", b, 1024, 8 * 49, 1), rb, 8, 7, 7, 0.0625)
    g.pool("bbox_pred", box, 7, 7, avg=True, global_=True)
    return g.finish() + ("data", "cls_prob")


def tiny_frame(seed=67, size=(8, 10), dry=False, trace=None):
    """A small image-to-image net with every framing layer (Net.SetFrame()), nothing above 24 px: a reflect Padding in front of the first
    convolution; branch a -- a zero Padding (0, 1, 0, 1) in front of a stride-2 pad-0 convolution (TensorFlow's "SAME": fusion level 2 folds
    it), a PixelShuffle 0=2 and the plain ReLU it absorbs; branch b -- a replicate Padding, a one-bottom Crop by sizes, a constant Padding with
    per-channel values, a PixelShuffle 0=3 1=1 and a one-bottom Crop by second offsets; branch c -- a channel Padding (7=1 8=2, value 0.5) and a
    two-bottom Crop whose reference is branch a.  size = (height, width), both even; trace: a list that receives the layers for numpy_forward."""
    h, w = size
    g = GraphBuilder(seed, dry)
    g.trace = trace
    x = g.padding("pad_reflect", g.input("data", 3, h, w), 2, 2, 2, 2, type_=2)
    x = g.relu("relu1", g.conv("conv1", x, 3, 8, 3))  # (h + 2, w + 2)
    a, b, c = g.split("split1", x, 3)
    a = g.relu("relu2", g.conv("conv_s2", g.padding("pad_same", a, 0, 1, 0, 1), 8, 8, 3, 2))  # (h / 2 + 1, w / 2 + 1)
    a = g.relu("relu_ps", g.pixel_shuffle("ps0", g.conv("conv_up", a, 8, 16, 1), 2))  # 4 x (h + 2, w + 2)
    a, ref = g.split("split2", a, 2)
    b = g.padding("pad_rep", b, 1, 2, 3, 0, type_=1)
    b = g.crop("crop_one", b, 2, 1, outw=w + 2, outh=h + 2)
    b = g.pool("pool_b", g.conv("conv_b", b, 8, 9, 1), 2, 2)  # 9 x (h / 2 + 1, w / 2 + 1)
    b = g.padding("pad_pc", b, 1, 0, 0, 1, per_channel=9)
    b = g.pixel_shuffle("ps1", b, 3, mode=1)  # 1 x (3 h / 2 + 6, 3 w / 2 + 6)
    b = g.crop("crop_b", b, 2, 1, woffset2=w // 2 + 2, hoffset2=h // 2 + 3)
    c = g.crop("crop_ref", g.padding("pad_ch", c, value=0.5, front=1, behind=2), coffset=2, like=ref)
    g.conv("out", g.concat("cat", [a, c, b]), 9, 3, 3, 1, 1)
    return g.finish() + ("data", "out")


def _encoder_block(g, tag, x, embed, heads, hidden, gain=1.0):
    """One pre-norm encoder block on tokens `x` [T][embed]: x + MHA(LN(x)), then x + FC(GELU(FC(LN(x)))).  -> (the block's output, written by a
    BinaryOp add)."""
    skip, y = g.split(tag + "_s1", x, 2)
    y = g.multi_head_attention(tag + "_attn", g.layer_norm(tag + "_ln1", y, embed), embed, heads, gain=gain)
    x = g.binary(tag + "_add1", 0, skip, y)
    skip, y = g.split(tag + "_s2", x, 2)
    y = g.fc_tokens(tag + "_fc1", g.layer_norm(tag + "_ln2", y, embed), embed, hidden, gain=gain)
    y = g.fc_tokens(tag + "_fc2", g.gelu(tag + "_gelu", y), hidden, embed, gain=gain)
    return g.binary(tag + "_add2", 0, skip, y)


def _vit(g, size, patch, embed, heads, depth, hidden, classes, gain=1.0):
    """The Vision Transformer (Dosovitskiy et al. 2021) as ncnn's converter writes it: a stride-`patch` convolution, Reshape to [embed][P], Permute
    to [P][embed], the class token (MemoryData) concatenated in front, the position embedding (MemoryData) added, `depth` pre-norm encoder
    blocks, a final LayerNorm, the class token taken by Reshape to rank 3 and Crop, and the head."""
    h, w = size if isinstance(size, tuple) else (size, size)
    tokens = (h // patch) * (w // patch) + 1
    x = g.conv("patch_embed", g.input("data", 3, h, w), 3, embed, patch, patch)
    x = g.permute("to_tokens", g.reshape("flat", x, -1, embed), 1)
    x = g.concat("with_cls", [g.memory_data("cls_token", embed, 1, scale=0.5), x], 0, rank=2)
    x = g.binary("add_pos", 0, x, g.memory_data("pos_embed", embed, tokens, scale=0.5))
    for i in range(depth):
        x = _encoder_block(g, f"blk{i}", x, embed, heads, hidden, gain)
    x = g.layer_norm("norm", x, embed)
    return x, tokens


def tiny_vit(seed=71, size=16, dry=False, trace=None):
    """A small Vision Transformer with every transformer layer (Net.SetTransformer(), SetDetection(), SetFrame()): a 16 x 16 input, 4-px patches,
    E = 16, 2 heads, 2 encoder blocks, class token and position embedding from MemoryData.  Behind the encoder: one cross-attention layer whose
    queries are the tokens and whose keys and values a second LayerNorm of the patch tokens alone (Tq = 17, Tk = 16), a scalar BinaryOp (mul
    0.5), the fast GELU, the class token taken by Reshape to rank 3 and Crop, and the head.  trace: a list that receives the layers for
    numpy_forward."""
    g = GraphBuilder(seed, dry)
    g.trace = trace
    embed, heads = 16, 2
    h, w = size if isinstance(size, tuple) else (size, size)
    x = g.conv("patch_embed", g.input("data", 3, h, w), 3, embed, 4, 4)
    x = g.permute("to_tokens", g.reshape("flat", x, -1, embed), 1)
    patches, x = g.split("split_patches", x, 2)
    tokens = (h // 4) * (w // 4) + 1
    x = g.concat("with_cls", [g.memory_data("cls_token", embed, 1, scale=0.5), x], 0, rank=2)
    x = g.binary("add_pos", 0, x, g.memory_data("pos_embed", embed, tokens, scale=0.5))
    for i in range(2):
        x = _encoder_block(g, f"blk{i}", x, embed, heads, 32)
    x = g.layer_norm("norm", x, embed)
    memory = g.layer_norm("norm_mem", patches, embed, eps=1e-5, affine=False)
    x = g.multi_head_attention("cross", x, embed, heads, k=memory, scale=0.3)
    x = g.gelu("gelu_fast", g.binary("halve", 2, x, 0.5), fast=True)
    x = g.crop("cls", g.reshape("as_rank3", x, embed, tokens, 1), outh=1)
    g.fc("head", x, embed, 10)
    return g.finish() + ("data", "head")


def deit_tiny_patch16_224(seed=1234, classes=1000, size=224, dry=False):
    """DeiT-tiny (Touvron et al. 2021) without the distillation token: patch 16, E = 192, 3 heads, 12 blocks, MLP 768; 197 tokens at 224 px.
    Random weights.  Net.SetTransformer(), SetDetection(), SetFrame()."""
    g = GraphBuilder(seed, dry)
    x, tokens = _vit(g, size, 16, 192, 3, 12, 768, classes, gain=0.5)
    g.fc("head", g.crop("cls", g.reshape("as_rank3", x, 192, tokens, 1), outh=1), 192, classes)
    return g.finish() + ("data", "head")


def vit_base_patch16_224(seed=1234, classes=1000, size=224, dry=False):
    """ViT-B/16 (Dosovitskiy et al. 2021): patch 16, E = 768, 12 heads, 12 blocks, MLP 3072; 197 tokens at 224 px.  Random weights.
    Net.SetTransformer(), SetDetection(), SetFrame()."""
    g = GraphBuilder(seed, dry)
    x, tokens = _vit(g, size, 16, 768, 12, 12, 3072, classes, gain=0.5)
    g.fc("head", g.crop("cls", g.reshape("as_rank3", x, 768, tokens, 1), outh=1), 768, classes)
    return g.finish() + ("data", "head")


def tiny_crnn(seed=73, size=(8, 24), dry=False, trace=None, classes=11):
    """A small text recogniser with every recurrent layer (Net.SetRecurrent(), SetDetection(), SetTransformer() for the per-token InnerProduct):
    an 8 x 24 image of three channels (a grey one arrives so through PIXEL_GRAY2RGB: a Convolution with ONE input channel is what the reference
    takes for a depthwise layer, and this runtime with it), two 3x3 convolutions each with a 2x2 pooling and a 2x2 convolution that brings the height to 1, Reshape and Permute to
    [T][32] tokens (T = width / 4 - 1), a bidirectional LSTM with H = 8 (a multiple of 4: the matrix kernel where the step route runs), a reverse
    GRU with H = 6 (the direct kernel there) whose final hidden state is the blob gru_h, a forward RNN with H = 8, the per-token InnerProduct and
    a Softmax along the class axis.  Up to FHIP_RNN_SEQUENCE_MAX_N images all three take the sequence route.  trace: a list that receives the
    layers for numpy_forward."""
    g = GraphBuilder(seed, dry)
    g.trace = trace
    h, w = size
    x = g.input("data", 3, h, w)
    x = g.pool("pool1", g.relu("relu1", g.conv("conv1", x, 3, 8, 3, 1, 1)))
    x = g.pool("pool2", g.relu("relu2", g.conv("conv2", x, 8, 16, 3, 1, 1)))
    x = g.relu("relu3", g.conv("conv3", x, 16, 32, 2))
    x = g.permute("to_tokens", g.reshape("flat", x, -1, 32), 1)
    x = g.lstm("bilstm", x, 32, 8, direction=2)
    x, _ = g.gru("gru", x, 16, 6, direction=1, states_out=True)
    x = g.rnn("rnn", x, 6, 8)
    x = g.fc_tokens("classes", x, 8, classes)
    g.softmax("prob", x, axis=1, rank=2)
    return g.finish() + ("data", "prob")


def tiny_lstm_states(seed=79, size=5, hidden=4, steps=3, dry=False, trace=None):
    """One forward LSTM fed its initial hidden and cell states through the Inputs `hidden` and `cell` ([1][1][hidden] each, per image) and
    writing its final states as the tops l_h and l_c: a sequence net run in pieces.  The Input `data` is [1][steps][size], taken to rank 2 by
    a Reshape.  Net.SetRecurrent(), SetDetection()."""
    g = GraphBuilder(seed, dry)
    g.trace = trace
    x = g.reshape("seq", g.input("data", 1, steps, size), size, steps)
    g.input("hidden", 1, 1, hidden)
    g.input("cell", 1, 1, hidden)
    g.lstm("l", x, size, hidden, states_in=("hidden", "cell"), states_out=True)
    return g.finish() + ("data", "l")


def _crnn_conv(g, name, x, cin, cout, k=3, p=1, bn=False):
    x = g.conv(name, x, cin, cout, k, 1, p)
    if bn:
        x = g.bn(name + "_bn", x, cout)
    return g.relu(name + "_relu", x)


def crnn_vgg_bilstm(seed=1234, classes=37, size=(32, 100), dry=False, trace=None):
    """CRNN (Shi et al. 2015) as published but for its input: the grey 32 x 100 image arrives as three equal channels (PIXEL_GRAY2RGB), because a
    Convolution with ONE input channel is what the reference takes for a depthwise layer, and this runtime with it: 1152 weights more than the
    published 8.3 million.  Seven convolutions 64, 128, 256, 256, 512, 512, 512 (3x3 pad 1, the last
    2x2 pad 0) with BatchNorm behind the third, fifth and seventh; max poolings 2x2 behind the first two and 2x2 stride (2, 1) pad (0, 1) behind
    the fourth and sixth (each written as a zero Padding of one column on either side and an unpadded Pooling, the same numbers behind a ReLU),
    which leave a [512][1][26] map; Reshape and Permute to 26 tokens; two BiLSTM(256), each with its linear layer (256,
    then the 37 classes); Softmax along the class axis.  Random weights.  Net.SetRecurrent(), SetDetection(), SetTransformer(), SetFrame()."""
    g = GraphBuilder(seed, dry)
    g.trace = trace  # (numpy_forward has no rectangular Pooling: the trace serves the layers one by one)
    h, w = size
    x = g.input("data", 3, h, w)
    x = g.pool("pool1", _crnn_conv(g, "conv1", x, 3, 64))
    x = g.pool("pool2", _crnn_conv(g, "conv2", x, 64, 128))
    x = _crnn_conv(g, "conv4", _crnn_conv(g, "conv3", x, 128, 256, bn=True), 256, 256)
    x = g.pool_rect("pool3", g.padding("pad3", x, left=1, right=1), 2, 2, 1, 2)
    x = _crnn_conv(g, "conv6", _crnn_conv(g, "conv5", x, 256, 512, bn=True), 512, 512)
    x = g.pool_rect("pool4", g.padding("pad4", x, left=1, right=1), 2, 2, 1, 2)
    x = _crnn_conv(g, "conv7", x, 512, 512, 2, 0, bn=True)
    x = g.permute("to_tokens", g.reshape("flat", x, -1, 512), 1)
    x = g.fc_tokens("embed1", g.lstm("bilstm1", x, 512, 256, direction=2), 512, 256)
    x = g.fc_tokens("embed2", g.lstm("bilstm2", x, 256, 256, direction=2), 512, classes)
    g.softmax("prob", x, axis=1, rank=2)
    return g.finish() + ("data", "prob")


def crnn_lite_lstm(seed=1234, classes=37, size=(32, 100), hidden=48, dry=False, trace=None):
    """A mobile-sized recogniser in the manner of chineseocr-lite and PaddleOCR's mobile models: a 32 x 100 image of three channels, a 3x3 stride-2 convolution, three
    depthwise-separable blocks (16 -> 32 -> 64 -> 96) with the poolings of CRNN, a 2x2 convolution that brings the height to 1, ONE BiLSTM with
    H = 48 (or 96) and the per-token classifier.  Its Wh fits the chip's LDS, so a small batch takes the sequence route: one launch for the
    whole recurrence.  Random weights.  Net.SetRecurrent(), SetDetection(), SetTransformer(), SetFrame()."""
    g = GraphBuilder(seed, dry)
    g.trace = trace  # (numpy_forward has no rectangular Pooling: the trace serves the layers one by one)
    h, w = size
    x = g.conv_bn_relu("conv1", g.input("data", 3, h, w), 3, 16, 3, 2, 1)
    for i, (c, k) in enumerate(((16, 32), (32, 64), (64, 96)), 2):
        x = g.conv_bn_relu(f"conv{i}_dw", x, c, c, 3, 1, 1, group=c)
        x = g.conv_bn_relu(f"conv{i}_pw", x, c, k, 1, 1, 0)
        x = g.pool(f"pool{i}", x) if i == 2 else g.pool_rect(f"pool{i}", g.padding(f"pad{i}", x, left=1, right=1), 2, 2, 1, 2)
    x = g.conv_bn_relu("conv5", x, 96, 96, 2)
    x = g.permute("to_tokens", g.reshape("flat", x, -1, 96), 1)
    x = g.fc_tokens("classes", g.lstm("bilstm", x, 96, hidden, direction=2), 2 * hidden, classes)
    g.softmax("prob", x, axis=1, rank=2)
    return g.finish() + ("data", "prob")


def espcn_x3(seed=1234, size=(180, 240), channels=1, dry=False):
    """ESPCN (Shi et al. 2016) x3: 5x5 -> 64, 3x3 -> 32, 3x3 -> channels * 9, TanH between them, and the sub-pixel layer, PixelShuffle 0=3
    (Net.SetFrame()).  The paper runs it on the luma plane (channels = 1).  size = (height, width) of the low-resolution input."""
    h, w = size
    g = GraphBuilder(seed, dry)
    x = g.tanh("tanh1", g.conv("conv1", g.input("data", channels, h, w), channels, 64, 5, 1, 2))
    x = g.tanh("tanh2", g.conv("conv2", x, 64, 32, 3, 1, 1))
    g.pixel_shuffle("out", g.conv("conv3", x, 32, channels * 9, 3, 1, 1), 3)
    return g.finish() + ("data", "out")


def srresnet_x4(seed=1234, size=96, dry=False, blocks=16):
    """SRResNet (Ledig et al. 2017) x4 as published: 9x9 -> 64 and PReLU, 16 residual blocks (3x3, BatchNorm, PReLU, 3x3, BatchNorm, sum), a
    3x3 + BatchNorm and the long skip, two up-sampling stages (3x3 -> 256, PixelShuffle 0=2, PReLU) and a 9x9 -> 3 (Net.SetFrame())."""
    g = GraphBuilder(seed, dry)
    x = g.prelu("prelu1", g.conv("conv1", g.input("data", 3, size, size), 3, 64, 9, 1, 4), 1)
    x, skip = g.split("split0", x)
    for i in range(1, blocks + 1):
        a, b = g.split(f"res{i}_split", x)
        a = g.prelu(f"res{i}_prelu", g.scale(f"res{i}a_scale", g.bn(f"res{i}a_bn", g.conv(f"res{i}a", a, 64, 64, 3, 1, 1), 64), 64), 1)
        a = g.scale(f"res{i}b_scale", g.bn(f"res{i}b_bn", g.conv(f"res{i}b", a, 64, 64, 3, 1, 1), 64), 64)
        x = g.eltwise(f"res{i}", a, b)
    x = g.scale("conv2_scale", g.bn("conv2_bn", g.conv("conv2", x, 64, 64, 3, 1, 1), 64), 64)
    x = g.eltwise("long_skip", x, skip)
    for i in (1, 2):
        x = g.prelu(f"up{i}_prelu", g.pixel_shuffle(f"up{i}_ps", g.conv(f"up{i}", x, 64, 256, 3, 1, 1), 2), 1)
    g.conv("out", x, 64, 3, 9, 1, 4)
    return g.finish() + ("data", "out")


def cyclegan_resnet9(seed=1234, size=256, dry=False, blocks=9):
    """CycleGAN's ResNet generator with 9 blocks as published (Net.SetFrame()): reflection Padding 3 and a 7x7, two stride-2 3x3, nine residual
    blocks whose two 3x3 convolutions each stand behind a reflection Padding 1, two transposed 3x3 and reflection Padding 3 with a 7x7 and
    TanH; InstanceNorm (no affine, as published) behind every convolution but the last."""
    g = GraphBuilder(seed, dry)

    def cir(name, x, cin, cout, k, s=1, p=0, relu=True):
        x = g.instance_norm(name + "_in", g.conv(name, x, cin, cout, k, s, p), cout, affine=False)
        return g.relu(name + "_relu", x) if relu else x

    x = g.padding("pad1", g.input("data", 3, size, size), 3, 3, 3, 3, type_=2)
    x = cir("conv1", x, 3, 64, 7)
    x = cir("conv2", x, 64, 128, 3, 2, 1)
    x = cir("conv3", x, 128, 256, 3, 2, 1)
    for i in range(1, blocks + 1):
        a, b = g.split(f"res{i}_split", x)
        a = cir(f"res{i}a", g.padding(f"res{i}a_pad", a, 1, 1, 1, 1, type_=2), 256, 256, 3)
        a = cir(f"res{i}b", g.padding(f"res{i}b_pad", a, 1, 1, 1, 1, type_=2), 256, 256, 3, relu=False)
        x = g.eltwise(f"res{i}", a, b)
    x = g.relu("deconv1_relu", g.instance_norm("deconv1_in", g.deconv("deconv1", x, 256, 128, 3, 2, 1, op=1), 128, affine=False))
    x = g.relu("deconv2_relu", g.instance_norm("deconv2_in", g.deconv("deconv2", x, 128, 64, 3, 2, 1, op=1), 64, affine=False))
    g.tanh("out", g.conv("conv_out", g.padding("pad_out", x, 3, 3, 3, 3, type_=2), 64, 3, 7))
    return g.finish() + ("data", "out")


def mobilenet_v1_tf(seed=1234, classes=1000, size=224, dry=False):
    """`mobilenet_v1` as a converter writes it from TensorFlow (Net.SetFrame()): every stride-2 convolution has pad 0 and stands behind an
    explicit `Padding 0=0 1=1 2=0 3=1`, TensorFlow's "SAME" on an even plane.  Fusion level 2 folds those Paddings into the convolutions."""
    g = GraphBuilder(seed, dry)
    x = g.input("data", 3, size, size)
    x = g.conv_bn_relu("conv1", g.padding("conv1_pad", x, 0, 1, 0, 1), 3, 32, 3, 2, 0)
    cfg = [(32, 64, 1), (64, 128, 2), (128, 128, 1), (128, 256, 2), (256, 256, 1), (256, 512, 2)] + [(512, 512, 1)] * 5 + \
          [(512, 1024, 2), (1024, 1024, 1)]
    for i, (c, k, s) in enumerate(cfg, 2):
        if s == 2:
            x = g.conv_bn_relu(f"conv{i}_dw", g.padding(f"conv{i}_pad", x, 0, 1, 0, 1), c, c, 3, 2, 0, group=c)
        else:
            x = g.conv_bn_relu(f"conv{i}_dw", x, c, c, 3, 1, 1, group=c)
        x = g.conv_bn_relu(f"conv{i}_pw", x, c, k, 1, 1, 0)
    x = g.pool("pool6", x, 7, 1, avg=True, global_=True)
    x = g.softmax("prob", g.fc("fc7", x, 1024, classes))
    return g.finish() + ("data", "prob")


GROUPED_LAYERS = {"tiny_grouped": ("g1", "g2", "g3", "g4")}

MODELS = {"vgg16": vgg16, "resnet50": resnet50, "mobilenet_v1": mobilenet_v1, "squeezenet_v1.1": squeezenet_v11,
          "tiny_allsorts": tiny_allsorts, "resnext50_32x4d": resnext50_32x4d, "tiny_grouped": tiny_grouped,
          "tiny_deconv": tiny_deconv, "style_transfer": style_transfer, "unet_k4": unet_k4,
          "tiny_generative": tiny_generative, "style_transfer_in": style_transfer_in, "pix2pix_unet": pix2pix_unet,
          "tiny_shuffle": tiny_shuffle, "shufflenet_v2_x1_0": shufflenet_v2_x1_0, "shufflenet_v1_g3": shufflenet_v1_g3,
          "tiny_dilated": tiny_dilated, "deeplab_largefov": deeplab_largefov, "deeplab_v2_aspp": deeplab_v2_aspp,
          "tiny_se": tiny_se, "se_resnet50": se_resnet50, "efficientnet_b0": efficientnet_b0,
          "tiny_resample": tiny_resample, "mobilenet_v3_large": mobilenet_v3_large, "mobilenet_v3_small": mobilenet_v3_small,
          "deeplab_largefov_full": deeplab_largefov_full, "unet_bilinear": unet_bilinear, "fpn_resnet50": fpn_resnet50,
          "tiny_lrn": tiny_lrn, "alexnet": alexnet, "caffenet": caffenet, "googlenet": googlenet,
          "tiny_quant": tiny_quant, "vgg16_int8": vgg16_int8, "resnet50_int8": resnet50_int8, "mobilenet_v1_int8": mobilenet_v1_int8,
          "tiny_requant": tiny_requant, "tiny_requant_twin": tiny_requant_twin,
          "vgg16_int8_rq": vgg16_int8_rq, "resnet50_int8_rq": resnet50_int8_rq, "mobilenet_v1_int8_rq": mobilenet_v1_int8_rq,
          "tiny_ssd": tiny_ssd, "mobilenet_ssd": mobilenet_ssd, "vgg16_ssd300": vgg16_ssd300,
          "tiny_yolov2": tiny_yolov2, "tiny_yolov3": tiny_yolov3, "yolov2_tiny_voc": yolov2_tiny_voc, "mobilenetv2_yolov3": mobilenetv2_yolov3,
          "tiny_faster_rcnn": tiny_faster_rcnn, "tiny_rfcn": tiny_rfcn, "faster_rcnn_vgg16": faster_rcnn_vgg16, "rfcn_resnet50": rfcn_resnet50,
          "tiny_frame": tiny_frame, "espcn_x3": espcn_x3, "srresnet_x4": srresnet_x4, "cyclegan_resnet9": cyclegan_resnet9,
          "mobilenet_v1_tf": mobilenet_v1_tf, "tiny_vit": tiny_vit, "deit_tiny_patch16_224": deit_tiny_patch16_224, "vit_base_patch16_224": vit_base_patch16_224}

DECONV_LAYERS = {"tiny_deconv": ("d1", "d2", "dw_up", "gd", "d3", "d4"), "style_transfer": ("deconv1", "deconv2"), "unet_k4": ("d5", "d4", "d3", "d2", "d1")}

# nets that need Net.SetDilated(True), and the layers of each that run through libfeather_atrous.so
DILATED_LAYERS = {"tiny_dilated": ("a1", "a2", "a3", "a_dw", "a_g", "a_far"),
                  "deeplab_largefov": ("conv5_1", "conv5_2", "conv5_3", "fc6"),
                  "deeplab_v2_aspp": ("conv5_1", "conv5_2", "conv5_3", "fc6_1", "fc6_2", "fc6_3", "fc6_4"),
                  "deeplab_largefov_full": ("conv5_1", "conv5_2", "conv5_3", "fc6")}

# nets that need Net.SetExtendedLayers(True) (Interp, HardSwish: libfeather_resample.so; LRN: libfeather_lrn.so)
EXTENDED_NETS = ("tiny_resample", "mobilenet_v3_large", "mobilenet_v3_small", "deeplab_largefov_full", "unet_bilinear", "fpn_resnet50",
                 "tiny_lrn", "alexnet", "caffenet", "googlenet")

# nets that need Net.SetQuantized(True) (int8 Convolution / InnerProduct layers: libfeather_qconv.so), and the quantised layers of the small one
QUANTIZED_NETS = ("tiny_quant", "vgg16_int8", "resnet50_int8", "mobilenet_v1_int8")
QUANT_LAYERS = {"tiny_quant": ("conv1", "conv2", "conv3", "dw", "pw", "fc")}
# nets that need Net.SetRequantized(True) on top of it (int8 convolutions with a requantised int8 output: libfeather_q8.so) and, for the
# BatchNorm behind such a layer, fusion level >= 2; the requantised layers and all int8 layers of the small one
REQUANTIZED_NETS = ("tiny_requant", "vgg16_int8_rq", "resnet50_int8_rq", "mobilenet_v1_int8_rq")
REQUANT_LAYERS = {"tiny_requant": ("conv1", "conv2", "conv3", "dw")}
QUANT_LAYERS["tiny_requant"] = QUANT_LAYERS["tiny_requant_twin"] = ("conv1", "conv2", "conv3", "dw", "pw", "side", "fc")

# nets that need Net.SetDetection(True) (the SSD head: libfeather_detect.so); vgg16_ssd300 needs Net.SetDilated(True) as well (DILATED_LAYERS)
DETECTION_NETS = ("tiny_ssd", "mobilenet_ssd", "vgg16_ssd300")
DILATED_LAYERS["vgg16_ssd300"] = ("fc6",)

# nets that need Net.SetYolo() (the YOLO heads: libfeather_yolo.so); tiny_yolov3 needs Net.SetExtendedLayers(True) as well (its Interp)
YOLO_NETS = ("tiny_yolov2", "tiny_yolov3", "yolov2_tiny_voc", "mobilenetv2_yolov3")

# nets that need Net.SetRoi() (Proposal and the ROI layers: libfeather_roi.so) and Net.SetDetection(True) (the RPN's Reshape and axis Softmax);
# rfcn_resnet50 needs Net.SetDilated(True) as well (its conv5).  Each has a second Input, "im_info" [n][1][1][3], and the top "rois"
ROI_NETS = ("tiny_faster_rcnn", "tiny_rfcn", "faster_rcnn_vgg16", "rfcn_resnet50")

# nets that need Net.SetFrame() (Padding, Crop, PixelShuffle: libfeather_frame.so)
# nets that need Net.SetTransformer(), SetDetection() and SetFrame(): Vision Transformers
TRANSFORMER_NETS = ("tiny_vit", "deit_tiny_patch16_224", "vit_base_patch16_224")
FRAME_NETS = ("tiny_frame", "espcn_x3", "srresnet_x4", "cyclegan_resnet9", "mobilenet_v1_tf")
# the zero Paddings of each net that fusion level 2 folds into the convolution behind them, and the Paddings that must stay
ZERO_PADDINGS = {"tiny_frame": (("pad_same",), ("pad_reflect", "pad_rep", "pad_pc", "pad_ch")),
                 "mobilenet_v1_tf": (("conv1_pad", "conv3_pad", "conv5_pad", "conv7_pad", "conv13_pad"), ())}

# the input size a builder's defaults describe, where it is not 224 px
INPUT_SIZE = {"alexnet": 227, "caffenet": 227, "mobilenet_ssd": 300, "vgg16_ssd300": 300, "yolov2_tiny_voc": 416, "mobilenetv2_yolov3": 352}

# the LRN layers of each net that fusion level 2 makes one layer with the Pooling layer behind them, and those that must stay as written
LRN_POOLS = {"tiny_lrn": (("norm1", "norm2", "norm5"), ("norm3", "norm4")), "alexnet": (("norm1", "norm2"), ()), "caffenet": ((), ("norm1", "norm2")),
             "googlenet": (("conv2/norm2",), ("pool1/norm1",))}

# the Interp layers of each net that fusion level 2 collapses with the Eltwise SUM (and ReLU) behind them, and those that must stay
UPSAMPLE_ADDS = {"tiny_resample": (("up1",), ("up2", "shrink", "aligned", "to_ref", "down")),
                 "fpn_resnet50": (("fpn_up4", "fpn_up3", "fpn_up2"), ())}

# the squeeze-and-excitation blocks of each net (the name fusion level 2 keeps: the block's Pooling layer) that collapse into one layer,
# and those that must not
SE_BLOCKS = {"tiny_se": (("a_gap", "b_gap", "c_gap"), ("d_gap",))}
