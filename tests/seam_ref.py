"""One float64 evaluator for every layer type feather::Net's create_layer accepts: the yardstick of tests/test_seams_cpu.py and
tests/test_seams_gpu.py, whose nets put layers of different families next to each other.

The family restatements form a tree (gconv_ref -> deconv_ref -> inorm_ref -> {shuffle_ref -> atrous_ref, gate_ref}) and no leaf of it can
run a net that holds, say, a dilated convolution and a channel gate.  `Net` here composes what those files already define -- it adds no
mathematics of its own -- and rounds every blob to float32 as they do.  Where two files define the same operation, ONE is used:

  Convolution / ConvolutionDepthWise   gconv_ref.conv; with a dilation (ncnn's ids 2 / 12) atrous_ref.atrous, as atrous_ref.Net chooses
  Deconvolution / ...DepthWise         deconv_ref.deconv
  ReLU (any slope)                     inorm_ref.leaky (gconv_ref.Net's np.where is its slope-0 case)
  InstanceNorm, PReLU, TanH, Clip      inorm_ref.instance_norm / inorm_ref.activation
  Sigmoid                              inorm_ref.activation("sigmoid") (gate_ref.sigmoid is the same formula)
  Swish, HardSigmoid                   gate_ref.swish / gate_ref.hard_sigmoid
  BinaryOp mul, two-bottom Scale       gate_ref.channel_gate, the gate picked as gate_ref.Net picks it
  ShuffleChannel, Slice                shuffle_ref.channel_shuffle / shuffle_ref.channel_slice
  Pooling, InnerProduct, BatchNorm,    gconv_ref.Net.run on that one layer: Pooling is oracle.netcheck._pool with its pad, ceil and
  Scale, Softmax                       empty-window rules
  Eltwise                              the float32 sum of gconv_ref / inorm_ref / gate_ref (shuffle_ref's float64 sum rounds the same
                                       but for double rounding)
  Concat                               numpy's concatenate, as every file has it
  Dropout                              oracle.netcheck.PortNet.run on that one layer: y = x * scale.  deconv_ref and inorm_ref pass the
                                       blob through whatever the scale; none of their nets holds a scaled Dropout
  Split                                the tops are the bottom

The .bin is read by gate_ref.Net (inorm_ref.Net's reader, with a two-bottom Scale reading nothing); the .param by
shuffle_ref.parse_param (oracle.netcheck.parse_param plus ncnn's array params).

An int8 layer (8=int8_scale_term: tests/qseam_ref.py) is no float64 operation.  The reader steps over it -- the int8 tag, the bytes padded
to 4, then the bias, K weight scales and one input scale, as qconv_ref._Bin reads them -- and keeps what it read in `Net.q`; `run` takes
such a layer's top from `given` (a dict of blobs; a layer ALL of whose tops are given is skipped, whatever its type) and refuses to run
without it.  Without `given` and without int8 layers everything is as it was.
"""
from __future__ import annotations

import numpy as np

import atrous_ref
import deconv_ref
import gate_ref
import gconv_ref
import inorm_ref
import shuffle_ref
from inorm_ref import plane_nerr  # noqa: F401  (the metric of the seam tests, re-exported)
from gconv_ref import nerr  # noqa: F401

BY_GCONV_NET = ("Pooling", "InnerProduct", "BatchNorm", "Scale", "Softmax")


class _One:
    """What gconv_ref.Net.run / PortNet.run need of `self` to evaluate one layer."""

    def __init__(self, layer, w):
        self.layers, self.w = [layer], w


def _gated(type_, bottoms, pd):
    return type_ == "Scale" and pd.get(0, 0) == -233 and len(bottoms) == 2


QUANT_TYPES = ("Convolution", "ConvolutionDepthWise", "InnerProduct")


def is_int8(layer):
    return layer[0] in QUANT_TYPES and layer[4].get(8, 0) != 0


class Net:
    def __init__(self, param: bytes, weights: bytes):
        self.layers = shuffle_ref.parse_param(param)
        self.q = {}
        if not any(is_int8(layer) for layer in self.layers):
            reader = gate_ref.Net(param, weights)
            self.w, self.read = reader.w, reader.read
            return
        # layer by layer: gate_ref.Net reads the fp32 layers (one one-layer net each, from where the last one stopped), this one the int8 ones
        import qconv_ref
        rows = param.decode().splitlines()[2:]
        assert len(rows) == len(self.layers)
        self.w, self.read = {}, 0
        for row, layer in zip(rows, self.layers):
            type_, name, _, _, pd = layer
            if not is_int8(layer):
                reader = gate_ref.Net(f"7767517\n1 1\n{row}\n".encode(), memoryview(weights)[self.read:])
                self.w.update(reader.w)
                self.read += reader.read
                continue
            rd = qconv_ref._Bin(weights)
            rd.at = self.read
            if type_ == "InnerProduct":
                k, bias_term, kh, kw, group = pd.get(0, 0), pd.get(1, 0), 1, 1, 1
                cg = pd.get(2, 0) // k
            else:
                k, kw, bias_term, group = pd.get(0, 0), pd.get(1, 0), pd.get(5, 0), pd.get(7, 1)
                kh = pd.get(11, kw)
                cg = pd.get(6, 0) // (k * kh * kw)
            wq = rd.int8(k * cg * kh * kw).reshape(k, cg, kh, kw)
            b = rd.raw(k) if bias_term else None
            self.q[name] = dict(wq=wq, b=b, s_w=rd.raw(k), s_in=rd.raw(1)[0], group=group)
            self.read = rd.at

    def run(self, input_name: str, x: np.ndarray, output_name: str = None, keep: bool = False, given: dict = None):
        from oracle.netcheck import PortNet
        blobs = {input_name: np.ascontiguousarray(x, np.float32)}
        given = given or {}
        for layer in self.layers:
            type_, name, bottoms, tops, pd = layer
            if type_ == "Input":
                continue
            if tops and all(t in given for t in tops):
                for t in tops:
                    blobs[t] = given[t]
                continue
            if is_int8(layer):
                raise RuntimeError(f"int8 layer {name} is not restated in float64: its top must be given")
            a = blobs[bottoms[0]]
            if type_ == "Split":
                for t in tops:
                    blobs[t] = a
                continue
            if type_ == "Slice":
                assert pd.get(1, 0) == 0 and len(pd[-23300]) == len(tops)
                for t, y in zip(tops, shuffle_ref.channel_slice(a, pd[-23300])):
                    blobs[t] = y
                continue
            if type_ in ("Convolution", "ConvolutionDepthWise"):
                wgt, b, group = self.w[name]
                sw, pw = pd.get(3, 1), pd.get(4, 0)
                sh, ph = pd.get(13, sw), pd.get(14, pw)
                dil = atrous_ref.dilation_of(pd)
                if dil != (1, 1):
                    y = atrous_ref.atrous(a, wgt, b, group, (sh, sw), (pw, pw, ph, ph), dil)
                else:
                    y = gconv_ref.conv(a, wgt, b, group, (sh, sw), (pw, pw, ph, ph))
            elif type_ in deconv_ref.DECONV_TYPES:
                wgt, b, group = self.w[name]
                _, _, _, stride, pads, out_pads, _, _, _ = deconv_ref.deconv_geometry(pd)
                y = deconv_ref.deconv(a, wgt, b, group, stride, pads, out_pads)
            elif type_ == "ReLU":
                y = inorm_ref.leaky(a.astype(np.float64), np.float64(np.float32(pd.get(0, 0.0))))
            elif type_ == "InstanceNorm":
                gamma, beta = self.w[name]
                assert pd.get(0, 0) == a.shape[1]
                y = inorm_ref.instance_norm(a, gamma, beta, np.float32(pd.get(1, 0.001)))
            elif type_ == "PReLU":
                s = self.w[name]
                assert s.size in (1, a.shape[1])
                y = inorm_ref.activation(a, "prelu", slope=s[0], slopes=None if s.size == 1 else s)
            elif type_ == "Sigmoid":
                y = inorm_ref.activation(a, "sigmoid")
            elif type_ == "TanH":
                y = inorm_ref.activation(a, "tanh")
            elif type_ == "Clip":
                y = inorm_ref.activation(a, "clip", lo=np.float32(pd.get(0, -inorm_ref.FLT_MAX)), hi=np.float32(pd.get(1, inorm_ref.FLT_MAX)))
            elif type_ == "Swish":
                y = gate_ref.swish(a)
            elif type_ == "HardSigmoid":
                y = gate_ref.hard_sigmoid(a, np.float64(np.float32(pd.get(0, 0.2))), np.float64(np.float32(pd.get(1, 0.5))))
            elif _gated(type_, bottoms, pd):
                assert not pd.get(1, 0)
                y = gate_ref.channel_gate(a, blobs[bottoms[1]])
            elif type_ == "BinaryOp":
                assert pd.get(0, 0) == 2 and len(bottoms) == 2
                b = blobs[bottoms[1]]
                gate_first = a.shape[2:] == (1, 1) and b.shape[2:] != (1, 1)
                y = gate_ref.channel_gate(b, a) if gate_first else gate_ref.channel_gate(a, b)
            elif type_ == "ShuffleChannel":
                y = shuffle_ref.channel_shuffle(a, pd.get(0, 1), bool(pd.get(1, 0)))
            elif type_ == "Concat":
                assert pd.get(0, 0) == 0
                y = np.concatenate([blobs[b] for b in bottoms], axis=1)
            elif type_ == "Dropout":
                y = PortNet.run(_One(layer, self.w), bottoms[0], a, tops[0])
            elif type_ == "Eltwise":
                assert len(bottoms) == 2 and a.shape == blobs[bottoms[1]].shape, name
                y = a + blobs[bottoms[1]]  # float32, the line of gconv_ref.Net.run (its blob table starts from ONE input, so it is not called)
            elif type_ in BY_GCONV_NET:
                y = gconv_ref.Net.run(_One(layer, self.w), bottoms[0], a, tops[0])
            else:
                raise RuntimeError(f"layer type {type_} is not restated")
            blobs[tops[0]] = np.ascontiguousarray(y, np.float32)
        return blobs if keep else blobs[output_name]

