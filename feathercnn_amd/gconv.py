"""Python host-side mirror of the grouped-convolution route (include/feather_hip/feather_gconv.h, ``libfeather_gconv.so``): a layer with
``1 < group < input_channels``, which ``ConvBooster.SelectAlgo`` refuses like the reference does.  Same shape as ``ConvBooster``
(GetBufferSize / Init / Forward on a ``ConvParam``, the caller owns every tensor); ``output_channels`` and ``input_channels`` are the
whole layer's.  Every call goes through the C-ABI; there is no fallback path.
"""
from __future__ import annotations

from . import _lib
from ._side_conv import SideConv, SideConvLayer
from .booster import ConvParam  # noqa: F401  (the parameter object of this route)


class GroupedConv(SideConv):
    """The C-ABI triple of libfeather_gconv.so.  Does not allocate: the caller owns every tensor.  Route(param, output, input): the choice
    depends on the alignment of the two tensors."""
    _load = staticmethod(_lib.load_gconv_library)
    _prefix = "fhip_gconv"


class GroupedConvLayer(SideConvLayer):
    """A grouped layer ready to run: packs the weights once, Forward per batch (the caller side, as booster.ConvLayer)."""
    _conv = GroupedConv
