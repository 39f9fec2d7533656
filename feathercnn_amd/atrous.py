"""Python host-side mirror of the dilated-convolution route (include/feather_hip/feather_atrous.h, ``libfeather_atrous.so``): a
Convolution layer with dilation > 1.  Same shape as ``ConvBooster`` (GetBufferSize / Init / Forward on a parameter object, the caller owns
every tensor); ``output_channels`` and ``input_channels`` are the whole layer's, weights are ``[K][C/group][kh][kw]`` (``torch``'s
``conv2d`` weight).  Every call goes through the C-ABI; there is no fallback path.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

from . import _lib
from .booster import FeatherHipError, None_, ReLU, _ptr, _stream


def _check(rc: int, what: str):
    if rc != 0:
        msg = _lib.load_atrous_library().fhip_atrous_last_error().decode(errors="replace")
        raise FeatherHipError(f"{what} failed with code {rc}: {msg}")


@dataclass
class AtrousParam:
    """fhip_atrous_param + the ``batch`` extension of ConvParam."""
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
    dilation_h: int = 2
    dilation_w: int = 2
    batch: int = 1

    def _c(self) -> _lib.fhip_atrous_param:
        return _lib.fhip_atrous_param(self.output_channels, self.input_channels, self.input_h, self.input_w, self.kernel_h, self.kernel_w,
                                      self.output_h, self.output_w, self.stride_h, self.stride_w, self.pad_left, self.pad_bottom,
                                      self.pad_right, self.pad_top, self.group, 1 if self.bias_term else 0, int(self.activation),
                                      self.dilation_h, self.dilation_w)

    def AssignOutputDim(self):
        c = self._c()
        _check(_lib.load_atrous_library().fhip_atrous_assign_output_dim(ctypes.byref(c)), "fhip_atrous_assign_output_dim")
        self.output_h, self.output_w = c.output_h, c.output_w

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


class AtrousConv:
    """The C-ABI triple of libfeather_atrous.so.  Does not allocate: the caller owns every tensor.  `route` (a name Route() can return)
    runs that kernel instead of the selected one (fhip_atrous_*_route): pack and run under the same name."""

    @staticmethod
    def Supported(param: AtrousParam) -> bool:
        c = param._c()
        return _lib.load_atrous_library().fhip_atrous_supported(ctypes.byref(c)) == 1

    def GetBufferSize(self, param: AtrousParam, route: str = None):
        """(scratch_bytes, packed_bytes) for param.batch images."""
        b, k = ctypes.c_size_t(), ctypes.c_size_t()
        c, lib = param._c(), _lib.load_atrous_library()
        if route is None:
            _check(lib.fhip_atrous_get_buffer_size(ctypes.byref(c), max(param.batch, 1), ctypes.byref(b), ctypes.byref(k)), "fhip_atrous_get_buffer_size")
        else:
            _check(lib.fhip_atrous_get_buffer_size_route(ctypes.byref(c), max(param.batch, 1), route.encode(), ctypes.byref(b), ctypes.byref(k)),
                   "fhip_atrous_get_buffer_size_route")
        return b.value, k.value

    def Init(self, param: AtrousParam, processed_kernel, kernel, route: str = None) -> int:
        """Weights [K][C/group][kh][kw] -> the layout the route reads, on the current stream."""
        c, lib = param._c(), _lib.load_atrous_library()
        if route is None:
            _check(lib.fhip_atrous_init(ctypes.byref(c), _ptr(processed_kernel), _ptr(kernel), _stream()), "fhip_atrous_init")
        else:
            _check(lib.fhip_atrous_init_route(ctypes.byref(c), _ptr(processed_kernel), _ptr(kernel), _stream(), route.encode()), "fhip_atrous_init_route")
        return 0

    def Forward(self, param: AtrousParam, output, input, processed_kernel, buffer, bias_arr, route: str = None) -> int:
        c, lib = param._c(), _lib.load_atrous_library()
        if route is None:
            _check(lib.fhip_atrous_forward(ctypes.byref(c), max(param.batch, 1), _ptr(output), _ptr(input), _ptr(processed_kernel), _ptr(buffer),
                                           _ptr(bias_arr), _stream()), "fhip_atrous_forward")
        else:
            _check(lib.fhip_atrous_forward_route(ctypes.byref(c), max(param.batch, 1), _ptr(output), _ptr(input), _ptr(processed_kernel),
                                                 _ptr(buffer), _ptr(bias_arr), _stream(), route.encode()), "fhip_atrous_forward_route")
        return 0

    def Route(self, param: AtrousParam) -> str:
        """The kernel instantiation Forward launches for this layer (fhip_atrous_route)."""
        name = ctypes.create_string_buffer(160)
        c = param._c()
        _check(_lib.load_atrous_library().fhip_atrous_route(ctypes.byref(c), name, len(name)), "fhip_atrous_route")
        return name.value.decode()


class AtrousLayer:
    """A dilated convolution ready to run: packs the weights once, Forward per batch (the caller side, as booster.ConvLayer)."""

    def __init__(self, param: AtrousParam, weight, bias=None, route: str = None):
        import torch
        self.param = param
        self.param.AssignOutputDim()
        self.route = route
        self.conv = AtrousConv()
        self.buffer_bytes, self.packed_bytes = self.conv.GetBufferSize(param, route)
        self.bias = bias
        self.packed = torch.empty(max(self.packed_bytes // 4, 1), dtype=torch.float32, device=weight.device)
        self.conv.Init(param, self.packed, weight.contiguous(), route)

    def out_shape(self):
        p = self.param
        return (max(p.batch, 1), p.output_channels, p.output_h, p.output_w)

    def Forward(self, x, out=None):
        import torch
        if out is None:
            out = torch.empty(self.out_shape(), dtype=torch.float32, device=x.device)
        self.conv.Forward(self.param, out, x, self.packed, None, self.bias, self.route)
        return out
