"""Python host-side mirror of the transposed-convolution route (include/feather_hip/feather_deconv.h, ``libfeather_deconv.so``): ncnn's
Deconvolution / DeconvolutionDepthWise.  Same shape as ``ConvBooster`` (GetBufferSize / Init / Forward on a parameter object, the caller
owns every tensor); ``input_*`` is the small tensor, ``output_channels`` and ``input_channels`` are the whole layer's, weights are
``[K][C/group][kh][kw]`` (``torch``'s ``conv_transpose2d`` weight with the first two axes swapped per group).  Every call goes through the
C-ABI; there is no fallback path.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

from . import _lib
from .booster import FeatherHipError, None_, ReLU, _ptr, _stream


def _check(rc: int, what: str):
    if rc != 0:
        msg = _lib.load_deconv_library().fhip_deconv_last_error().decode(errors="replace")
        raise FeatherHipError(f"{what} failed with code {rc}: {msg}")


@dataclass
class DeconvParam:
    """fhip_deconv_param + the ``batch`` extension of ConvParam."""
    output_channels: int = 0
    input_channels: int = 0
    input_h: int = 0
    input_w: int = 0
    kernel_h: int = 0
    kernel_w: int = 0
    output_h: int = 0
    output_w: int = 0
    stride_h: int = 1
    stride_w: int = 1
    pad_left: int = 0
    pad_bottom: int = 0
    pad_right: int = 0
    pad_top: int = 0
    group: int = 1
    bias_term: bool = False
    activation: int = None_
    output_pad_right: int = 0
    output_pad_bottom: int = 0
    batch: int = 1

    def _c(self) -> _lib.fhip_deconv_param:
        return _lib.fhip_deconv_param(self.output_channels, self.input_channels, self.input_h, self.input_w, self.kernel_h, self.kernel_w,
                                      self.output_h, self.output_w, self.stride_h, self.stride_w, self.pad_left, self.pad_bottom,
                                      self.pad_right, self.pad_top, self.group, 1 if self.bias_term else 0, int(self.activation),
                                      self.output_pad_right, self.output_pad_bottom)

    def AssignOutputDim(self):
        c = self._c()
        _check(_lib.load_deconv_library().fhip_deconv_assign_output_dim(ctypes.byref(c)), "fhip_deconv_assign_output_dim")
        self.output_h, self.output_w = c.output_h, c.output_w

    @staticmethod
    def make(ic, oc, h, k=4, s=2, p=1, op=0, group=1, bias=True, act=ReLU, w=None, batch=1) -> "DeconvParam":
        q = DeconvParam(output_channels=oc, input_channels=ic, input_h=h, input_w=h if w is None else w, kernel_h=k, kernel_w=k, stride_h=s,
                        stride_w=s, pad_left=p, pad_bottom=p, pad_right=p, pad_top=p, group=group, bias_term=bool(bias), activation=act,
                        output_pad_right=op, output_pad_bottom=op, batch=batch)
        q.AssignOutputDim()
        return q


class Deconv:
    """The C-ABI triple of libfeather_deconv.so.  Does not allocate: the caller owns every tensor."""

    @staticmethod
    def Supported(param: DeconvParam) -> bool:
        c = param._c()
        return _lib.load_deconv_library().fhip_deconv_supported(ctypes.byref(c)) == 1

    def GetBufferSize(self, param: DeconvParam):
        """(scratch_bytes, packed_bytes) for param.batch images."""
        b, k = ctypes.c_size_t(), ctypes.c_size_t()
        c = param._c()
        _check(_lib.load_deconv_library().fhip_deconv_get_buffer_size(ctypes.byref(c), max(param.batch, 1), ctypes.byref(b), ctypes.byref(k)),
               "fhip_deconv_get_buffer_size")
        return b.value, k.value

    def Init(self, param: DeconvParam, processed_kernel, kernel) -> int:
        """Weights [K][C/group][kh][kw] -> the layout the selected route reads, on the current stream."""
        c = param._c()
        _check(_lib.load_deconv_library().fhip_deconv_init(ctypes.byref(c), _ptr(processed_kernel), _ptr(kernel), _stream()), "fhip_deconv_init")
        return 0

    def Forward(self, param: DeconvParam, output, input, processed_kernel, buffer, bias_arr) -> int:
        c = param._c()
        _check(_lib.load_deconv_library().fhip_deconv_forward(ctypes.byref(c), max(param.batch, 1), _ptr(output), _ptr(input),
                                                              _ptr(processed_kernel), _ptr(buffer), _ptr(bias_arr), _stream()),
               "fhip_deconv_forward")
        return 0

    def Route(self, param: DeconvParam) -> str:
        """The kernel instantiation Forward launches for this layer (fhip_deconv_route)."""
        name = ctypes.create_string_buffer(160)
        c = param._c()
        _check(_lib.load_deconv_library().fhip_deconv_route(ctypes.byref(c), name, len(name)), "fhip_deconv_route")
        return name.value.decode()


class DeconvLayer:
    """A transposed-convolution layer ready to run: packs the weights once, Forward per batch (the caller side, as booster.ConvLayer)."""

    def __init__(self, param: DeconvParam, weight, bias=None):
        import torch
        self.param = param
        self.param.AssignOutputDim()
        self.deconv = Deconv()
        self.buffer_bytes, self.packed_bytes = self.deconv.GetBufferSize(param)
        self.bias = bias
        self.packed = torch.empty(max(self.packed_bytes // 4, 1), dtype=torch.float32, device=weight.device)
        self.deconv.Init(param, self.packed, weight.contiguous())

    def out_shape(self):
        p = self.param
        return (max(p.batch, 1), p.output_channels, p.output_h, p.output_w)

    def Forward(self, x, out=None):
        import torch
        if out is None:
            out = torch.empty(self.out_shape(), dtype=torch.float32, device=x.device)
        self.deconv.Forward(self.param, out, x, self.packed, None, self.bias)
        return out
