"""numpy restatements of include/feather_hip/feather_resample.h -- Interp (nearest, bilinear) and HardSwish -- and of whole nets that hold
such layers: the yardstick of tests/test_resample_cpu.py, tests/test_resample_gpu.py and the resample seam tests.

Two forms of every definition:
  dtype=np.float32   the header's operation order, every difference, product and sum rounded to float32 on its own (numpy never fuses a
                     multiply into an add): what the library must equal BIT FOR BIT;
  dtype=np.float64   the same expressions in float64 -- the coefficients are still the header's, computed in double and rounded once to
                     float32 -- for the normalised bound of whole nets.
The reference project has no Interp layer; tests/test_resample_cpu.py ties the float64 form to torch.nn.functional.interpolate.

`Net` evaluates the new layers and hands every other layer to the restatements tests/seam_ref.py composes.
"""
from __future__ import annotations

import numpy as np

import gate_ref
import seam_ref
import shuffle_ref
from gconv_ref import nerr  # noqa: F401  (the project's parity metric, re-exported)
from inorm_ref import plane_nerr  # noqa: F401

NEAREST, BILINEAR = 1, 2
MODES = {"nearest": NEAREST, "bilinear": BILINEAR}
RESAMPLE_TYPES = ("Interp", "HardSwish")


def output_dim(in_h, in_w, height_scale=1.0, width_scale=1.0, output_height=0, output_width=0):
    """The header's output size: the given one where non-zero, else int(in * scale) with the product in float32."""
    oh = output_height or int(np.float32(in_h) * np.float32(height_scale))
    ow = output_width or int(np.float32(in_w) * np.float32(width_scale))
    return oh, ow


def nearest_index(n_in, n_out, scale=0.0):
    """sy = min(int(dy * hs), in - 1), the product in float32; hs = 1 / scale where the scale decided the size, else in / (float)out."""
    step = np.float32(1) / np.float32(scale) if scale else np.float32(n_in) / np.float32(n_out)
    prod = np.arange(n_out, dtype=np.float32) * np.float32(step)
    assert prod.dtype == np.float32
    return np.minimum(prod.astype(np.int64), n_in - 1)


def bilinear_taps(n_in, n_out, align_corner=False):
    """(i0, i1, f): the two taps of every output coordinate, clamped into the plane, and the float32 weight of the second
    (mat_pixel_resize.cpp:51-66: the source position in double, rounded once)."""
    d = np.arange(n_out, dtype=np.float64)
    if align_corner:
        f = (d * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)).astype(np.float32)
    else:
        f = ((d + 0.5) * (n_in / n_out) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    low = s < 0
    s = np.where(low, 0, s)
    f = np.where(low, np.float32(0), f)
    high = s >= n_in - 1
    s = np.where(high, n_in - 2, s)
    f = np.where(high, np.float32(1), f).astype(np.float32)
    return np.maximum(s, 0), np.minimum(s + 1, n_in - 1), f


def interp(x, mode, out_h, out_w, align_corner=False, height_scale=0.0, width_scale=0.0, residual=None, relu=False, dtype=np.float32) -> np.ndarray:
    """x [N][C][H][W] -> [N][C][out_h][out_w].  height_scale / width_scale: the layer's scale where it decided the size, 0 where the size
    was given (read by nearest only).  Then + residual and ReLU, each on its own."""
    mode = MODES.get(mode, mode)
    x = np.asarray(x, dtype)
    in_h, in_w = x.shape[2:]
    if mode == NEAREST:
        y = x[:, :, nearest_index(in_h, out_h, height_scale)][:, :, :, nearest_index(in_w, out_w, width_scale)]
    else:
        assert mode == BILINEAR, mode
        y0, y1, fy = bilinear_taps(in_h, out_h, align_corner)
        x0, x1, fx = bilinear_taps(in_w, out_w, align_corner)
        fx, fy = fx.astype(dtype), fy.astype(dtype).reshape(-1, 1)
        gx, gy = dtype(1) - fx, dtype(1) - fy
        s0, s1 = x[:, :, y0], x[:, :, y1]
        r0 = s0[..., x0] * gx + s0[..., x1] * fx
        r1 = s1[..., x0] * gx + s1[..., x1] * fx
        y = r0 * gy + r1 * fy
    if residual is not None:
        y = y + np.asarray(residual, dtype)
    y = np.maximum(y, 0) if relu else y
    assert y.dtype == dtype
    return np.ascontiguousarray(y)


def hard_swish(x, alpha=0.2, beta=0.5, dtype=np.float32) -> np.ndarray:
    """lower = -beta / alpha, upper = 1 / alpha + lower (float32, as the library computes them); 0 below lower, x above upper, else
    x * (x * alpha + beta).  alpha and beta are taken as the float32 values the library is handed."""
    a32, b32 = np.float32(alpha), np.float32(beta)
    lower = -b32 / a32
    upper = np.float32(1) / a32 + lower
    x = np.asarray(x, dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        mid = x * (x * dtype(a32) + dtype(b32))
    return np.where(x < dtype(lower), dtype(0), np.where(x > dtype(upper), x, mid)).astype(dtype)


class Net(gate_ref.Net):
    """The float64 evaluator of nets with Interp and HardSwish (every blob rounded to float32, as the family's evaluators do).  The .bin
    is read by gate_ref.Net's reader (the new layers have no weights); every layer that is not new is evaluated as tests/seam_ref.py
    evaluates it, so a net may hold any type create_layer accepts, a dilated convolution included."""

    def __init__(self, param: bytes, weights: bytes):
        super().__init__(param, weights)
        self.layers = shuffle_ref.parse_param(param)

    def run(self, input_name, x, output_name=None, keep=False, inputs=None):
        blobs = {input_name: np.ascontiguousarray(x, np.float32)}
        for k, v in (inputs or {}).items():
            blobs[k] = np.ascontiguousarray(v, np.float32)
        for layer in self.layers:
            type_, name, bottoms, tops, pd = layer
            if type_ == "Input":
                continue
            a = blobs[bottoms[0]]
            if type_ == "Interp":
                if len(bottoms) == 2:
                    (oh, ow), hs, ws = blobs[bottoms[1]].shape[2:], 0.0, 0.0
                else:
                    oh, ow = output_dim(a.shape[2], a.shape[3], pd.get(1, 1.0), pd.get(2, 1.0), pd.get(3, 0), pd.get(4, 0))
                    hs, ws = (0.0 if pd.get(3, 0) else pd.get(1, 1.0)), (0.0 if pd.get(4, 0) else pd.get(2, 1.0))
                blobs[tops[0]] = interp(a, pd.get(0, 0), oh, ow, bool(pd.get(6, 0)), hs, ws, dtype=np.float64).astype(np.float32)
            elif type_ == "HardSwish":
                blobs[tops[0]] = hard_swish(a, pd.get(0, 0.2), pd.get(1, 0.5), dtype=np.float64).astype(np.float32)
            elif type_ == "Split":
                for t in tops:
                    blobs[t] = a
            elif type_ == "Slice":
                for t, y in zip(tops, shuffle_ref.channel_slice(a, pd[-23300])):
                    blobs[t] = y
            elif type_ == "Eltwise":
                assert len(bottoms) == 2 and a.shape == blobs[bottoms[1]].shape, name
                blobs[tops[0]] = a + blobs[bottoms[1]]  # float32, seam_ref's line
            elif type_ == "Concat":
                blobs[tops[0]] = np.ascontiguousarray(np.concatenate([blobs[b] for b in bottoms], axis=1))
            elif type_ == "BinaryOp" or seam_ref._gated(type_, bottoms, pd):
                b = blobs[bottoms[1]]
                gate_first = type_ == "BinaryOp" and a.shape[2:] == (1, 1) and b.shape[2:] != (1, 1)
                y = gate_ref.channel_gate(b, a) if gate_first else gate_ref.channel_gate(a, b)
                blobs[tops[0]] = np.ascontiguousarray(y, np.float32)
            else:  # one bottom, one top: seam_ref.Net.run on a net of that one layer
                assert len(bottoms) == 1 and len(tops) == 1, (type_, name)
                blobs[tops[0]] = seam_ref.Net.run(seam_ref._One(layer, self.w), bottoms[0], a, tops[0])
        return blobs if keep else blobs[output_name]
