"""Python host-side mirror of the dilated-convolution route (include/feather_hip/feather_atrous.h, ``libfeather_atrous.so``): a
Convolution layer with dilation > 1.  Same shape as ``ConvBooster`` (GetBufferSize / Init / Forward on a parameter object, the caller owns
every tensor); ``output_channels`` and ``input_channels`` are the whole layer's, weights are ``[K][C/group][kh][kw]`` (``torch``'s
``conv2d`` weight).  Every call goes through the C-ABI; there is no fallback path.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

from . import _lib
from ._side_conv import SideConv, SideConvLayer, SideConvParam, SideSymbols
from .booster import ReLU, _ptr, _stream


class _Library(SideSymbols):
    _load = staticmethod(_lib.load_atrous_library)
    _prefix = "fhip_atrous"


@dataclass
class AtrousParam(_Library, SideConvParam):
    """fhip_atrous_param + the ``batch`` extension of ConvParam."""
    dilation_h: int = 2
    dilation_w: int = 2
    batch: int = 1

    def _c(self) -> _lib.fhip_atrous_param:
        return _lib.fhip_atrous_param(*self._common(), self.dilation_h, self.dilation_w)

    @staticmethod
    def make(ic, oc, h, k=3, s=1, d=2, p=None, group=1, bias=True, act=ReLU, w=None, batch=1) -> "AtrousParam":
        """`p` = None: the "same" padding of a stride-1 layer, d * (k - 1) / 2."""
        if p is None:
            p = d * (k - 1) // 2
        q = AtrousParam(output_channels=oc, input_channels=ic, input_h=h, input_w=h if w is None else w, kernel_h=k, kernel_w=k, stride_h=s,
                        stride_w=s, pad_left=p, pad_bottom=p, pad_right=p, pad_top=p, group=group, bias_term=bool(bias), activation=act,
                        dilation_h=d, dilation_w=d, batch=batch)
        q.AssignOutputDim()
        return q


class AtrousConv(_Library, SideConv):
    """The C-ABI triple of libfeather_atrous.so.  Does not allocate: the caller owns every tensor.  `route` (a name Route() can return)
    runs that kernel instead of the selected one (fhip_atrous_*_route): pack and run under the same name."""

    def GetBufferSize(self, param: AtrousParam, route: str = None):
        """(scratch_bytes, packed_bytes) for param.batch images."""
        if route is None:
            return super().GetBufferSize(param)
        b, k = ctypes.c_size_t(), ctypes.c_size_t()
        c = param._c()
        self._call("get_buffer_size_route", ctypes.byref(c), max(param.batch, 1), route.encode(), ctypes.byref(b), ctypes.byref(k))
        return b.value, k.value

    def Init(self, param: AtrousParam, processed_kernel, kernel, route: str = None) -> int:
        """Weights [K][C/group][kh][kw] -> the layout the route reads, on the current stream."""
        if route is None:
            return super().Init(param, processed_kernel, kernel)
        c = param._c()
        self._call("init_route", ctypes.byref(c), _ptr(processed_kernel), _ptr(kernel), _stream(), route.encode())
        return 0

    def Forward(self, param: AtrousParam, output, input, processed_kernel, buffer, bias_arr, route: str = None) -> int:
        if route is None:
            return super().Forward(param, output, input, processed_kernel, buffer, bias_arr)
        c = param._c()
        self._call("forward_route", ctypes.byref(c), max(param.batch, 1), _ptr(output), _ptr(input), _ptr(processed_kernel), _ptr(buffer),
                   _ptr(bias_arr), _stream(), route.encode())
        return 0


class AtrousLayer(SideConvLayer):
    """A dilated convolution ready to run: packs the weights once, Forward per batch (the caller side, as booster.ConvLayer)."""
    _conv = AtrousConv

    def __init__(self, param: AtrousParam, weight, bias=None, route: str = None):
        self.route = route
        super().__init__(param, weight, bias, route)
