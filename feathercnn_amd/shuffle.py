"""Python host-side mirror of include/feather_hip/feather_shuffle.h (``libfeather_shuffle.so``): ncnn's ShuffleChannel and Slice and the
general channel map on torch CUDA tensors.  Every call goes through the C-ABI on the current stream; there is no fallback path.
"""
from __future__ import annotations

import ctypes

from . import _lib
from .booster import _ptr, _stream

MAX_BLOBS = 4  # FHIP_CHANNEL_MAP_MAX_BLOBS
SHARE = -233   # FHIP_SLICE_SHARE
ROUTES = {"4b": 0, "16b": 1}
KINDS = {"map": 0, "shuffle": 1, "slice": 2}


_check = _lib.checker(_lib.load_shuffle_library, "fhip_shuffle_last_error")


def _nchw(x, what):
    import torch
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f"{what} needs a contiguous float32 [N][C][H][W] tensor")
    return x.shape


def _pointers(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _ints(values):
    return (ctypes.c_int * len(values))(*[int(v) for v in values])


def slice_sizes(c: int, sizes) -> list:
    """Slice sizes with their -233 entries resolved against c channels (fhip_channel_slice_resolve; host only)."""
    out = (ctypes.c_int * max(len(sizes), 1))()
    _check(_lib.load_shuffle_library().fhip_channel_slice_resolve(int(c), _ints(sizes), len(sizes), out), "fhip_channel_slice_resolve")
    return list(out)[:len(sizes)]


def channel_route(kind, h, w, tensors) -> str:
    """The kernel instantiation the entry point `kind` ("map", "shuffle", "slice") launches for h x w planes between these tensors."""
    name = ctypes.create_string_buffer(96)
    _check(_lib.load_shuffle_library().fhip_channel_map_route(KINDS[kind], h, w, _pointers(tensors), len(tensors), name, len(name)),
           "fhip_channel_map_route")
    return name.value.decode()


def channel_shuffle(x, group: int, reverse: bool = False, out=None):
    """ncnn's ShuffleChannel of a contiguous float32 [N][C][H][W] CUDA tensor: out channel i * group + k = in channel k * (C / group) + i;
    reverse applies the inverse permutation.  out must not be x."""
    import torch
    n, c, h, w = _nchw(x, "channel_shuffle")
    if out is None:
        out = torch.empty_like(x)
    _check(_lib.load_shuffle_library().fhip_channel_shuffle_forward(_ptr(out), _ptr(x), n, c, h, w, int(group), int(bool(reverse)), _stream()),
           "fhip_channel_shuffle_forward")
    return out


def channel_slice(x, sizes, outs=None):
    """ncnn's Slice along the channels: a list of tensors with sizes[j] channels each (-233: an equal share of what is left), written by one
    launch."""
    import torch
    n, c, h, w = _nchw(x, "channel_slice")
    if outs is None:
        outs = [torch.empty((n, s, h, w), dtype=torch.float32, device=x.device) for s in slice_sizes(c, sizes)]
    for o in outs:
        _nchw(o, "channel_slice")
    _check(_lib.load_shuffle_library().fhip_channel_slice_forward(_pointers(outs), _ptr(x), n, c, h, w, _ints(sizes), len(sizes), _stream()),
           "fhip_channel_slice_forward")
    return outs


class ChannelMap:
    """fhip_channel_map: `tables[j]` lists, for every channel of output j, the pair (source index, source channel); `src_channels[s]` is the
    channel count of source s.  Built and checked once on the host, kept on the device; forward() is one launch."""

    def __init__(self, src_channels, tables):
        self.src_channels = [int(c) for c in src_channels]
        self.out_channels = [len(t) for t in tables]
        flat = [int(v) for t in tables for pair in t for v in pair]
        self._lib = _lib.load_shuffle_library()
        self._map = ctypes.c_void_p()
        _check(self._lib.fhip_channel_map_create(ctypes.byref(self._map), _ints(self.src_channels), len(self.src_channels), _ints(self.out_channels),
                                                 len(self.out_channels), _ints(flat)), "fhip_channel_map_create")

    def forward(self, srcs, outs=None, route=None):
        import torch
        n, _, h, w = _nchw(srcs[0], "channel_map")
        for s, c in zip(srcs, self.src_channels):
            if tuple(_nchw(s, "channel_map")) != (n, c, h, w):
                raise ValueError("sources must be [N][src_channels[s]][H][W] of one batch and plane size")
        if len(srcs) != len(self.src_channels):
            raise ValueError("one tensor per source")
        if outs is None:
            outs = [torch.empty((n, c, h, w), dtype=torch.float32, device=srcs[0].device) for c in self.out_channels]
        for o, c in zip(outs, self.out_channels):
            if tuple(_nchw(o, "channel_map")) != (n, c, h, w):
                raise ValueError("outputs must be [N][out_channels[j]][H][W]")
        if len(outs) != len(self.out_channels):
            raise ValueError("one tensor per output")
        for t in list(srcs) + list(outs):
            _ptr(t)
        if route is None:
            _check(self._lib.fhip_channel_map_forward(self._map, _pointers(outs), _pointers(srcs), n, h, w, _stream()), "fhip_channel_map_forward")
        else:
            _check(self._lib.fhip_channel_map_forward_route(ROUTES[route], self._map, _pointers(outs), _pointers(srcs), n, h, w, _stream()),
                   "fhip_channel_map_forward_route")
        return outs

    def close(self):
        if self._map:
            self._lib.fhip_channel_map_destroy(self._map)
            self._map = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def channel_map(srcs, tables, outs=None, route=None):
    """One launch of the general form: outs[j][:, r] = srcs[s][:, c] for (s, c) = tables[j][r].  Builds the device table on every call; keep a
    ChannelMap to build it once."""
    m = ChannelMap([s.shape[1] for s in srcs], tables)
    try:
        return m.forward(srcs, outs, route)
    finally:
        import torch
        torch.cuda.current_stream().synchronize()  # the table must outlive the launch
        m.close()
