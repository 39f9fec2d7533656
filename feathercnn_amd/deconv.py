"""Python host-side mirror of the transposed-convolution route (include/feather_hip/feather_deconv.h, ``libfeather_deconv.so``): ncnn's
Deconvolution / DeconvolutionDepthWise.  Same shape as ``ConvBooster`` (GetBufferSize / Init / Forward on a parameter object, the caller
owns every tensor); ``input_*`` is the small tensor, ``output_channels`` and ``input_channels`` are the whole layer's, weights are
``[K][C/group][kh][kw]`` (``torch``'s ``conv_transpose2d`` weight with the first two axes swapped per group).  Every call goes through the
C-ABI; there is no fallback path.
"""
from __future__ import annotations

from dataclasses import dataclass

from . import _lib
from ._side_conv import SideConv, SideConvLayer, SideConvParam, SideSymbols
from .booster import ReLU


class _Library(SideSymbols):
    _load = staticmethod(_lib.load_deconv_library)
    _prefix = "fhip_deconv"


@dataclass
class DeconvParam(_Library, SideConvParam):
    """fhip_deconv_param + the ``batch`` extension of ConvParam."""
    output_pad_right: int = 0
    output_pad_bottom: int = 0
    batch: int = 1

    def _c(self) -> _lib.fhip_deconv_param:
        return _lib.fhip_deconv_param(*self._common(), self.output_pad_right, self.output_pad_bottom)

    @staticmethod
    def make(ic, oc, h, k=4, s=2, p=1, op=0, group=1, bias=True, act=ReLU, w=None, batch=1) -> "DeconvParam":
        q = DeconvParam(output_channels=oc, input_channels=ic, input_h=h, input_w=h if w is None else w, kernel_h=k, kernel_w=k, stride_h=s,
                        stride_w=s, pad_left=p, pad_bottom=p, pad_right=p, pad_top=p, group=group, bias_term=bool(bias), activation=act,
                        output_pad_right=op, output_pad_bottom=op, batch=batch)
        q.AssignOutputDim()
        return q


class Deconv(_Library, SideConv):
    """The C-ABI triple of libfeather_deconv.so.  Does not allocate: the caller owns every tensor."""


class DeconvLayer(SideConvLayer):
    """A transposed-convolution layer ready to run: packs the weights once, Forward per batch (the caller side, as booster.ConvLayer)."""
    _conv = Deconv
    _attr = "deconv"
