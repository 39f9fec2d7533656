"""Python host-side mirror of the grouped-convolution route (include/feather_hip/feather_gconv.h, ``libfeather_gconv.so``): a layer with
``1 < group < input_channels``, which ``ConvBooster.SelectAlgo`` refuses like the reference does.  Same shape as ``ConvBooster``
(GetBufferSize / Init / Forward on a ``ConvParam``, the caller owns every tensor); ``output_channels`` and ``input_channels`` are the
whole layer's.  Every call goes through the C-ABI; there is no fallback path.
"""
from __future__ import annotations

import ctypes

from . import _lib
from .booster import ConvParam, FeatherHipError, _ptr, _stream


def _check(rc: int, what: str):
    if rc != 0:
        msg = _lib.load_gconv_library().fhip_gconv_last_error().decode(errors="replace")
        raise FeatherHipError(f"{what} failed with code {rc}: {msg}")


class GroupedConv:
    """The C-ABI triple of libfeather_gconv.so.  Does not allocate: the caller owns every tensor."""

    @staticmethod
    def Supported(param: ConvParam) -> bool:
        c = param._c()
        return _lib.load_gconv_library().fhip_gconv_supported(ctypes.byref(c)) == 1

    def GetBufferSize(self, param: ConvParam):
        """(scratch_bytes, packed_bytes) for param.batch images."""
        b, k = ctypes.c_size_t(), ctypes.c_size_t()
        c = param._c()
        _check(_lib.load_gconv_library().fhip_gconv_get_buffer_size(ctypes.byref(c), max(param.batch, 1), ctypes.byref(b), ctypes.byref(k)),
               "fhip_gconv_get_buffer_size")
        return b.value, k.value

    def Init(self, param: ConvParam, processed_kernel, kernel) -> int:
        """Weights [K][C/group][kh][kw] -> the layout the kernels read, on the current stream."""
        c = param._c()
        _check(_lib.load_gconv_library().fhip_gconv_init(ctypes.byref(c), _ptr(processed_kernel), _ptr(kernel), _stream()), "fhip_gconv_init")
        return 0

    def Forward(self, param: ConvParam, output, input, processed_kernel, buffer, bias_arr) -> int:
        c = param._c()
        _check(_lib.load_gconv_library().fhip_gconv_forward(ctypes.byref(c), max(param.batch, 1), _ptr(output), _ptr(input),
                                                            _ptr(processed_kernel), _ptr(buffer), _ptr(bias_arr), _stream()),
               "fhip_gconv_forward")
        return 0

    def Route(self, param: ConvParam, output, input) -> str:
        """The kernel instantiation Forward launches for these tensors (fhip_gconv_route)."""
        name = ctypes.create_string_buffer(96)
        c = param._c()
        _check(_lib.load_gconv_library().fhip_gconv_route(ctypes.byref(c), _ptr(output), _ptr(input), name, len(name)), "fhip_gconv_route")
        return name.value.decode()


class GroupedConvLayer:
    """A grouped layer ready to run: packs the weights once, Forward per batch (the caller side, as booster.ConvLayer)."""

    def __init__(self, param: ConvParam, weight, bias=None):
        import torch
        self.param = param
        self.param.AssignOutputDim()
        self.conv = GroupedConv()
        self.buffer_bytes, self.packed_bytes = self.conv.GetBufferSize(param)
        self.bias = bias
        self.packed = torch.empty(max(self.packed_bytes // 4, 1), dtype=torch.float32, device=weight.device)
        self.conv.Init(param, self.packed, weight.contiguous())

    def out_shape(self):
        p = self.param
        return (max(p.batch, 1), p.output_channels, p.output_h, p.output_w)

    def Forward(self, x, out=None):
        import torch
        if out is None:
            out = torch.empty(self.out_shape(), dtype=torch.float32, device=x.device)
        self.conv.Forward(self.param, out, x, self.packed, None, self.bias)
        return out
