"""What the Python mirrors of the three convolution side libraries share (gconv.py, deconv.py, atrous.py): the parameter fields, the C-ABI
triple Supported / GetBufferSize / Init / Forward / Route over ``fhip_<x>_*`` and the layer that is ready to run.  A library's mirror names
its loader and its symbol prefix; everything else is here.  Every call goes through the C-ABI; there is no fallback path.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

from . import _lib
from .booster import None_, _ptr, _stream


class SideSymbols:
    """The symbols fhip_<x>_* of one library: a subclass sets `_load` (the library's loader in _lib) and `_prefix` ("fhip_<x>")."""
    _load = None
    _prefix = ""

    @classmethod
    def _fn(cls, name):
        return getattr(cls._load(), f"{cls._prefix}_{name}")

    @classmethod
    def _call(cls, name, *args):
        """fhip_<x>_<name>(*args); raises FeatherHipError with the library's last error when it refuses."""
        _lib.checker(cls._load, f"{cls._prefix}_last_error")(cls._fn(name)(*args), f"{cls._prefix}_{name}")


@dataclass
class SideConvParam(SideSymbols):
    """The fields fhip_deconv_param and fhip_atrous_param share with fhip_conv_param, in the order of the C structs.  A subclass adds the two
    fields of its own and ``batch`` (the extension of ConvParam), and `_c()`, its C struct."""
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

    def _common(self):
        return (self.output_channels, self.input_channels, self.input_h, self.input_w, self.kernel_h, self.kernel_w, self.output_h, self.output_w,
                self.stride_h, self.stride_w, self.pad_left, self.pad_bottom, self.pad_right, self.pad_top, self.group, 1 if self.bias_term else 0,
                int(self.activation))

    def AssignOutputDim(self):
        c = self._c()
        self._call("assign_output_dim", ctypes.byref(c))
        self.output_h, self.output_w = c.output_h, c.output_w


class SideConv(SideSymbols):
    """The C-ABI triple of one library.  Does not allocate: the caller owns every tensor."""

    @classmethod
    def Supported(cls, param) -> bool:
        c = param._c()
        return cls._fn("supported")(ctypes.byref(c)) == 1

    def GetBufferSize(self, param):
        """(scratch_bytes, packed_bytes) for param.batch images."""
        b, k = ctypes.c_size_t(), ctypes.c_size_t()
        c = param._c()
        self._call("get_buffer_size", ctypes.byref(c), max(param.batch, 1), ctypes.byref(b), ctypes.byref(k))
        return b.value, k.value

    def Init(self, param, processed_kernel, kernel) -> int:
        """Weights [K][C/group][kh][kw] -> the layout the selected route reads, on the current stream."""
        c = param._c()
        self._call("init", ctypes.byref(c), _ptr(processed_kernel), _ptr(kernel), _stream())
        return 0

    def Forward(self, param, output, input, processed_kernel, buffer, bias_arr) -> int:
        c = param._c()
        self._call("forward", ctypes.byref(c), max(param.batch, 1), _ptr(output), _ptr(input), _ptr(processed_kernel), _ptr(buffer), _ptr(bias_arr),
                   _stream())
        return 0

    def Route(self, param, *tensors) -> str:
        """The kernel instantiation Forward launches for this layer (fhip_<x>_route); `tensors`: the pointers the library's call takes."""
        name = ctypes.create_string_buffer(160)
        c = param._c()
        self._call("route", ctypes.byref(c), *(_ptr(t) for t in tensors), name, len(name))
        return name.value.decode()


class SideConvLayer:
    """A layer ready to run: packs the weights once, Forward per batch (the caller side, as booster.ConvLayer).  A subclass sets `_conv`, the
    SideConv it runs on, and `_attr`, the attribute that holds it; `extra` goes to the three calls after their own arguments."""
    _conv = None
    _attr = "conv"

    def __init__(self, param, weight, bias=None, *extra):
        import torch
        self.param = param
        self.param.AssignOutputDim()
        self._extra = extra
        conv = self._conv()
        setattr(self, self._attr, conv)
        self.buffer_bytes, self.packed_bytes = conv.GetBufferSize(param, *extra)
        self.bias = bias
        self.packed = torch.empty(max(self.packed_bytes // 4, 1), dtype=torch.float32, device=weight.device)
        conv.Init(param, self.packed, weight.contiguous(), *extra)

    def out_shape(self):
        p = self.param
        return (max(p.batch, 1), p.output_channels, p.output_h, p.output_w)

    def Forward(self, x, out=None):
        import torch
        if out is None:
            out = torch.empty(self.out_shape(), dtype=torch.float32, device=x.device)
        getattr(self, self._attr).Forward(self.param, out, x, self.packed, None, self.bias, *self._extra)
        return out
