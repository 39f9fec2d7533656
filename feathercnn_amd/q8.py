"""Python host-side mirror of the int8 route on q8 tensors (include/feather_hip/feather_q8.h, ``libfeather_q8.so``): a Convolution or
ConvolutionDepthWise layer with int8 weights whose input, output or both are q8 tensors -- ``torch.int8 [n][ceil(C / 16)][h][w][16]`` -- and
the layers that live between two of them.  Same shape as ``QuantConv`` (GetBufferSize / Init / Forward on a parameter object, the caller owns
every tensor).  Every call goes through the C-ABI; there is no fallback path.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

from . import _lib
from ._side_conv import SideConv, SideConvParam, SideSymbols
from .booster import None_, _ptr, _stream


class _Library(SideSymbols):
    _load = staticmethod(_lib.load_q8_library)
    _prefix = "fhip_q8"


@dataclass
class Q8Param(_Library, SideConvParam):
    """fhip_q8_param + the ``batch`` extension of ConvParam."""
    dilation_h: int = 1
    dilation_w: int = 1
    int8_scale_term: int = 1
    input_int8: bool = True
    output_int8: bool = True
    batch: int = 1

    def _c(self) -> _lib.fhip_q8_param:
        return _lib.fhip_q8_param(*self._common(), self.dilation_h, self.dilation_w, self.int8_scale_term, int(self.input_int8), int(self.output_int8))

    @staticmethod
    def make(ic, oc, h, k=3, s=1, p=0, group=1, bias=True, act=None_, w=None, batch=1, pads=None, input_int8=True, output_int8=True) -> "Q8Param":
        """`pads` = (left, right, top, bottom) where they differ."""
        pl, pr, pt, pb = pads if pads is not None else (p, p, p, p)
        q = Q8Param(output_channels=oc, input_channels=ic, input_h=h, input_w=h if w is None else w, kernel_h=k, kernel_w=k, stride_h=s,
                    stride_w=s, pad_left=pl, pad_bottom=pb, pad_right=pr, pad_top=pt, group=group, bias_term=bool(bias), activation=act,
                    input_int8=input_int8, output_int8=output_int8, batch=batch)
        q.AssignOutputDim()
        return q


def q8_shape(batch: int, channels: int, h: int, w: int):
    """The shape of the q8 tensor of an NCHW tensor."""
    return (batch, (channels + 15) // 16, h, w, 16)


def q8_pack(x, s: float, out=None):
    """fp32 NCHW -> the q8 tensor of quantise(x; s), pad bytes 0 (fhip_q8_quantize_forward)."""
    import torch
    n, c, h, w = x.shape
    if out is None:
        out = torch.empty(q8_shape(n, c, h, w), dtype=torch.int8, device=x.device)
    _Library._call("quantize_forward", _ptr(out), _ptr(x), n, c, h, w, float(s), _stream())
    return out


def q8_unpack(q, channels: int, s: float = 1.0, out=None):
    """A q8 tensor -> fp32 NCHW, float(q) / s (fhip_q8_dequantize_forward); s = 1 gives the integers."""
    import torch
    n, _, h, w, _ = q.shape
    if out is None:
        out = torch.empty((n, channels, h, w), dtype=torch.float32, device=q.device)
    _Library._call("dequantize_forward", _ptr(out), _ptr(q), n, channels, h, w, float(s), _stream())
    return out


def q8_relu(q, out=None):
    """max(q, 0) on a q8 tensor (fhip_q8_relu_forward); out=q runs in place."""
    import torch
    if out is None:
        out = torch.empty_like(q)
    _Library._call("relu_forward", _ptr(out), _ptr(q), q.numel(), _stream())
    return out


def q8_max_pool(q, channels: int, kernel=2, stride=2, pad=0, global_pooling=False, out=None):
    """Max pooling of a q8 tensor with PoolingLayer's geometry (fhip_q8_max_pool_forward)."""
    import torch
    n, cb, h, w, _ = q.shape
    p = _lib.fhip_pool_param(channels=channels, input_h=h, input_w=w, kernel_h=kernel, kernel_w=kernel, stride_h=stride, stride_w=stride, pad_left=pad,
                             pad_right=pad, pad_top=pad, pad_bottom=pad, pooling_type=0, global_pooling=int(global_pooling))
    if out is None:
        oh, ow = ctypes.c_int(), ctypes.c_int()
        _lib.checker(_lib.load_library, "fhip_last_error")(_lib.load_library().fhip_pooling_output_dim(ctypes.byref(p), ctypes.byref(oh), ctypes.byref(ow)),
                                                           "fhip_pooling_output_dim")
        out = torch.empty((n, cb, oh.value, ow.value, 16), dtype=torch.int8, device=q.device)
    _Library._call("max_pool_forward", ctypes.byref(p), n, _ptr(out), _ptr(q), _stream())
    return out


def q8_route(param: Q8Param) -> str:
    """The kernel instantiation fhip_q8_forward launches for this layer."""
    return Q8Conv().Route(param)


class Q8Conv(_Library, SideConv):
    """The C-ABI triple of libfeather_q8.so.  Does not allocate: the caller owns every tensor.  `route` (a name Route() can return) runs that
    kernel instead of the selected one (fhip_q8_*_route): pack and run under the same name."""

    def GetBufferSize(self, param: Q8Param, route: str = None):
        """(scratch_bytes, packed_bytes) for param.batch images."""
        if route is None:
            return super().GetBufferSize(param)
        b, k = ctypes.c_size_t(), ctypes.c_size_t()
        c = param._c()
        self._call("get_buffer_size_route", ctypes.byref(c), max(param.batch, 1), route.encode(), ctypes.byref(b), ctypes.byref(k))
        return b.value, k.value

    def Init(self, param: Q8Param, processed_kernel, kernel, route: str = None) -> int:
        """int8 weights [K][C/group][kh][kw] -> the layout the route reads, on the current stream."""
        if route is None:
            return super().Init(param, processed_kernel, kernel)
        c = param._c()
        self._call("init_route", ctypes.byref(c), _ptr(processed_kernel), _ptr(kernel), _stream(), route.encode())
        return 0

    def Forward(self, param: Q8Param, output, input, processed_kernel, dequant, bias_arr, s_in: float = 1.0, s_out: float = 1.0, route: str = None) -> int:
        c = param._c()
        args = (ctypes.byref(c), max(param.batch, 1), _ptr(output), _ptr(input), _ptr(processed_kernel), None, _ptr(dequant), _ptr(bias_arr),
                float(s_in), float(s_out), _stream())
        if route is None:
            self._call("forward", *args)
        else:
            self._call("forward_route", *args, route.encode())
        return 0
