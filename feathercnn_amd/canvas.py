"""Chained Winograd runs whose layers hold 2x2 image canvases (include/feather_hip/feather_canvas.h), on torch CUDA tensors: what the Net
runtime does at fusion level 3 for VGG-16's 56- and 14-pixel layers, layer by layer, with the scratch tensors kept for inspection."""
from __future__ import annotations

import ctypes

from . import _lib
from .booster import _check, _ptr, _stream

ENTRY, INSIDE, EXIT = 1, 2, 3


def plan_canvas(param, batch: int, canvas: bool):
    """fhip_winograd_f63_plan_canvas: the plan a layer runs with, plain (canvas=False) or on canvases of four images."""
    pl, c = _lib.fhip_winograd_plan(), param._c()
    _check(_lib.load_library().fhip_winograd_f63_plan_canvas(ctypes.byref(c), int(batch), 2 if canvas else 1, ctypes.byref(pl)),
           "fhip_winograd_f63_plan_canvas")
    return pl


def canvas_param(param, batch: int):
    """The layer as ONE pad-1 image of 2H + 2 pixels per side (a fhip_conv_param), or None when the layer / batch does not qualify."""
    q, c = _lib.fhip_conv_param(), param._c()
    return q if _lib.load_library().fhip_winograd_f63_canvas_param(ctypes.byref(c), int(batch), ctypes.byref(q)) == 0 else None


_check_canvas = _lib.checker(_lib.load_canvas_library, "fhip_canvas_last_error")


def forward_chained_canvas(layers, x, pools, canvas, fill=None, keep=False):
    """A run of Winograd ConvLayers, layer i on canvases where canvas[i]; pools[i] = a 2x2 max pooling follows layer i.  layers[0] is plain
    and transforms `x`; a canvas stretch starts and ends at a pooled boundary or ends the run.  fill: value V, M and the output are filled
    with before the run (NaN: nothing a kernel does not write may reach a result).  keep=True: -> (output, [(V, M, plan) of every layer]),
    V and M cloned as the layer saw them."""
    import torch
    lib, clib = _lib.load_library(), _lib.load_canvas_library()
    batch, dev = x.shape[0], x.device
    assert not canvas[0] and len(layers) == len(pools) == len(canvas)
    plans = [plan_canvas(l.param, batch, cv) for l, cv in zip(layers, canvas)]
    new = (lambda n: torch.full((n,), fill, dtype=torch.float32, device=dev)) if fill is not None else (lambda n: torch.empty(n, dtype=torch.float32, device=dev))
    vbuf = [new(max(pl.v_bytes for pl in plans[k::2]) // 4) if plans[k::2] else None for k in (0, 1)]
    m = new(max(pl.m_bytes for pl in plans) // 4)
    last = layers[-1].param
    oh, ow = (last.output_h // 2, last.output_w // 2) if pools[-1] else (last.output_h, last.output_w)
    out = new(batch * last.output_channels * oh * ow).reshape(batch, last.output_channels, oh, ow)
    kept = []
    for i, l in enumerate(layers):
        c, v = l.param._c(), vbuf[i & 1]
        bias = _ptr(l.bias) if l.bias is not None else None
        if i == 0:
            _check(lib.fhip_winograd_f63_input_transform(ctypes.byref(c), batch, _ptr(v), _ptr(x), _stream()), "fhip_winograd_f63_input_transform")
        if canvas[i]:
            cp = canvas_param(l.param, batch)
            _check(lib.fhip_winograd_f63_tile_gemm(ctypes.byref(cp), batch // 4, _ptr(m), _ptr(l.packed), _ptr(v), _stream()), "fhip_winograd_f63_tile_gemm")
        else:
            _check(lib.fhip_winograd_f63_tile_gemm(ctypes.byref(c), batch, _ptr(m), _ptr(l.packed), _ptr(v), _stream()), "fhip_winograd_f63_tile_gemm")
        if keep:
            kept.append((v.clone(), m.clone(), plans[i]))
        if i + 1 < len(layers):
            cn, vn = layers[i + 1].param._c(), vbuf[(i + 1) & 1]
            if canvas[i] or canvas[i + 1]:
                form = ENTRY if not canvas[i] else INSIDE if canvas[i + 1] else EXIT
                assert bool(pools[i]) == (form != INSIDE)
                _check_canvas(clib.fhip_canvas_output_to_next_input(form, ctypes.byref(c), ctypes.byref(cn), batch, ctypes.byref(plans[i]),
                                                                    ctypes.byref(plans[i + 1]), _ptr(vn), _ptr(m), bias, _stream()),
                              "fhip_canvas_output_to_next_input")
            else:
                _check(lib.fhip_winograd_f63_output_to_next_input(ctypes.byref(c), ctypes.byref(cn), batch, _ptr(vn), _ptr(m), bias, int(pools[i]), _stream()),
                       "fhip_winograd_f63_output_to_next_input")
        elif canvas[i]:
            _check_canvas(clib.fhip_canvas_output_transform(ctypes.byref(c), batch, ctypes.byref(plans[i]), _ptr(out), _ptr(m), bias, int(pools[i]), _stream()),
                          "fhip_canvas_output_transform")
        else:
            _check(lib.fhip_conv_forward_chained(ctypes.byref(c), batch, _ptr(out), None, _ptr(l.packed), _ptr(v), _ptr(m), bias, None, None, int(pools[i]),
                                                 _stream()), "fhip_conv_forward_chained")
    return (out, kept) if keep else out
