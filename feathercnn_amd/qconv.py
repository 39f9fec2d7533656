"""Python host-side mirror of the int8 convolution route (include/feather_hip/feather_qconv.h, ``libfeather_qconv.so``): a Convolution,
ConvolutionDepthWise or InnerProduct layer with int8 weights, fp32 in and out.  Same shape as ``ConvBooster`` (GetBufferSize / Init /
Forward on a parameter object, the caller owns every tensor); weights are ``torch.int8 [K][C/group][kh][kw]``.  Every call goes through
the C-ABI; there is no fallback path.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._side_conv import SideConv, SideConvParam, SideSymbols
from .booster import None_, _ptr, _stream


class _Library(SideSymbols):
    _load = staticmethod(_lib.load_qconv_library)
    _prefix = "fhip_qconv"


@dataclass
class QuantParam(_Library, SideConvParam):
    """fhip_qconv_param + the ``batch`` extension of ConvParam."""
    dilation_h: int = 1
    dilation_w: int = 1
    int8_scale_term: int = 1
    batch: int = 1

    def _c(self) -> _lib.fhip_qconv_param:
        return _lib.fhip_qconv_param(*self._common(), self.dilation_h, self.dilation_w, self.int8_scale_term)

    @staticmethod
    def make(ic, oc, h, k=3, s=1, p=0, group=1, bias=True, act=None_, w=None, batch=1, pads=None) -> "QuantParam":
        """`pads` = (left, right, top, bottom) where they differ."""
        pl, pr, pt, pb = pads if pads is not None else (p, p, p, p)
        q = QuantParam(output_channels=oc, input_channels=ic, input_h=h, input_w=h if w is None else w, kernel_h=k, kernel_w=k, stride_h=s,
                       stride_w=s, pad_left=pl, pad_bottom=pb, pad_right=pr, pad_top=pt, group=group, bias_term=bool(bias), activation=act,
                       batch=batch)
        q.AssignOutputDim()
        return q


def dequant_scales(s_w, s_in: float) -> np.ndarray:
    """d[k] = 1 / (s_in * s_w[k]) as the library computes it on the host (fhip_qconv_dequant_scales); 0 where s_w[k] == 0."""
    s_w = np.ascontiguousarray(s_w, dtype=np.float32)
    d = np.empty_like(s_w)
    _Library._call("dequant_scales", d.ctypes.data_as(ctypes.c_void_p), s_w.ctypes.data_as(ctypes.c_void_p), int(s_w.size), float(s_in))
    return d


def quantize(x, s_in: float, out=None):
    """int8 tensor of x's shape: fhip_quantize_forward, the header's rounding rule as a kernel of its own."""
    import torch
    if out is None:
        out = torch.empty(x.shape, dtype=torch.int8, device=x.device)
    lib = _lib.load_qconv_library()
    _lib.checker(_lib.load_qconv_library, "fhip_qconv_last_error")(
        lib.fhip_quantize_forward(_ptr(out), _ptr(x), x.numel(), float(s_in), _stream()), "fhip_quantize_forward")
    return out


def qconv_route(param: QuantParam) -> str:
    """The kernel instantiation fhip_qconv_forward launches for this layer."""
    return QuantConv().Route(param)


class QuantConv(_Library, SideConv):
    """The C-ABI triple of libfeather_qconv.so.  Does not allocate: the caller owns every tensor.  `route` (a name Route() can return) runs
    that kernel instead of the selected one (fhip_qconv_*_route): pack and run under the same name."""

    def GetBufferSize(self, param: QuantParam, route: str = None):
        """(scratch_bytes, packed_bytes) for param.batch images."""
        if route is None:
            return super().GetBufferSize(param)
        b, k = ctypes.c_size_t(), ctypes.c_size_t()
        c = param._c()
        self._call("get_buffer_size_route", ctypes.byref(c), max(param.batch, 1), route.encode(), ctypes.byref(b), ctypes.byref(k))
        return b.value, k.value

    def Init(self, param: QuantParam, processed_kernel, kernel, route: str = None) -> int:
        """int8 weights [K][C/group][kh][kw] -> the layout the route reads, on the current stream."""
        if route is None:
            return super().Init(param, processed_kernel, kernel)
        c = param._c()
        self._call("init_route", ctypes.byref(c), _ptr(processed_kernel), _ptr(kernel), _stream(), route.encode())
        return 0

    def Forward(self, param: QuantParam, output, input, processed_kernel, dequant, bias_arr, s_in: float, route: str = None) -> int:
        c = param._c()
        args = (ctypes.byref(c), max(param.batch, 1), _ptr(output), _ptr(input), _ptr(processed_kernel), None, _ptr(dequant), _ptr(bias_arr),
                float(s_in), _stream())
        if route is None:
            self._call("forward", *args)
        else:
            self._call("forward_route", *args, route.encode())
        return 0
