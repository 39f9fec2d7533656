"""numpy restatements of include/feather_hip/feather_lrn.h -- local response normalisation across channels and within a channel, and
the Pooling layer behind it -- and of whole nets that hold LRN layers: the yardstick of tests/test_lrn_cpu.py and tests/test_lrn_gpu.py.

Two forms of the definition:
  dtype=np.float32   the header's steps one by one, every product and sum rounded to float32 on its own, the squares added in the header's
                     order, the power by np.power in float32: what the library must equal up to the power's few ulp;
  dtype=np.float64   the same expressions in float64 (alpha / local_size is still the float32 quotient the library is handed).
`drop` removes taps from the window's sum: the perturbations tests/test_lrn_cpu.py proves visible.

`Net` evaluates LRN layers and hands every other layer to tests/resample_ref.py's evaluator.
"""
from __future__ import annotations

import copy

import numpy as np

import resample_ref
from gconv_ref import nerr  # noqa: F401  (the project's parity metric, re-exported)
from inorm_ref import plane_nerr  # noqa: F401

ACROSS, WITHIN = 0, 1


def scale_a(region, local_size, alpha):
    """a of the header: alpha / local_size (across) or alpha / local_size^2 (within), divided in float32."""
    ls = np.float32(local_size)
    return np.float32(alpha) / (ls if region == ACROSS else ls * ls)


def window_sum(q, region, local_size, drop=()):
    """The sum of the squares q [N][C][H][W] over every element's window, added in the header's order from zero in q's dtype.  Taps outside
    the tensor are left out.  drop: across channels, a collection of (c, c') -- tap c' is left out of channel c's sum."""
    n, c, h, w = q.shape
    half = local_size // 2
    s = np.zeros_like(q)
    if region == ACROSS:
        for k in range(-half, half + 1):  # ascending c' = c + k
            lo, hi = max(0, -k), min(c, c - k)  # channels whose tap c + k exists
            if lo >= hi:
                continue
            add = q[:, lo + k:hi + k].copy()
            for (cc, tap) in drop:
                if tap - cc == k and lo <= cc < hi:
                    add[:, cc - lo] = 0
            s[:, lo:hi] = s[:, lo:hi] + add
    else:
        for dy in range(-half, half + 1):  # rows ascending, columns ascending within a row
            for dx in range(-half, half + 1):
                ylo, yhi = max(0, -dy), min(h, h - dy)
                xlo, xhi = max(0, -dx), min(w, w - dx)
                if ylo >= yhi or xlo >= xhi:
                    continue
                s[:, :, ylo:yhi, xlo:xhi] = s[:, :, ylo:yhi, xlo:xhi] + q[:, :, ylo + dy:yhi + dy, xlo + dx:xhi + dx]
    assert s.dtype == q.dtype
    return s


def lrn(x, local_size=5, alpha=1.0, beta=0.75, bias=1.0, region=ACROSS, dtype=np.float32, drop=()) -> np.ndarray:
    x = np.asarray(x, dtype)
    a = dtype(scale_a(region, local_size, alpha))
    q = x * x
    s = window_sum(q, region, local_size, drop)
    d = dtype(np.float32(bias)) + a * s
    y = x * np.power(d, -dtype(np.float32(beta)))
    assert y.dtype == dtype
    return np.ascontiguousarray(y)


def pool_output_dim(h, w, k, s, pad):
    """fhip_pooling_output_dim: ceil((in + pads - k) / stride) + 1, the quotient in float32; pad = (left, right, top, bottom)."""
    oh = int(np.ceil(np.float32(h + pad[2] + pad[3] - k) / np.float32(s))) + 1
    ow = int(np.ceil(np.float32(w + pad[0] + pad[1] - k) / np.float32(s))) + 1
    return oh, ow


def pooling(x, k, s, pad=(0, 0, 0, 0), avg=False) -> np.ndarray:
    """fhip_pooling's generic kernel in x's dtype: window origin o * stride - pad_top - pad_bottom (both pads), clipped to the plane; max, or
    the sum in rows ascending and columns ascending divided by the number of taps inside the plane."""
    n, c, h, w = x.shape
    oh, ow = pool_output_dim(h, w, k, s, pad)
    y = np.empty((n, c, oh, ow), x.dtype)
    for oy in range(oh):
        y0 = oy * s - pad[2] - pad[3]
        ya, yb = max(y0, 0), min(y0 + k, h)
        for ox in range(ow):
            x0 = ox * s - pad[0] - pad[1]
            xa, xb = max(x0, 0), min(x0 + k, w)
            if avg:
                t = np.zeros((n, c), x.dtype)
                for yy in range(ya, yb):
                    for xx in range(xa, xb):
                        t = t + x[:, :, yy, xx]
                count = max(yb - ya, 0) * max(xb - xa, 0)
                with np.errstate(invalid="ignore", divide="ignore"):
                    y[:, :, oy, ox] = t / x.dtype.type(count)
            else:
                win = x[:, :, ya:yb, xa:xb].reshape(n, c, -1)
                y[:, :, oy, ox] = win.max(axis=2) if win.shape[2] else -np.finfo(np.float32).max
    return y


class Net(resample_ref.Net):
    """The float64 evaluator of nets with LRN layers (every blob rounded to float32, as the family's evaluators do): LRN here, every other
    layer by resample_ref.Net on a net of that one layer."""

    def run(self, input_name, x, output_name=None, keep=False, inputs=None):
        blobs = {input_name: np.ascontiguousarray(x, np.float32)}
        for k, v in (inputs or {}).items():
            blobs[k] = np.ascontiguousarray(v, np.float32)
        one = copy.copy(self)
        for layer in self.layers:
            type_, name, bottoms, tops, pd = layer
            if type_ == "Input":
                continue
            if type_ == "LRN":
                y = lrn(blobs[bottoms[0]], pd.get(1, 5), pd.get(2, 1.0), pd.get(3, 0.75), pd.get(4, 1.0), pd.get(0, 0), dtype=np.float64)
                blobs[tops[0]] = y.astype(np.float32)
                continue
            one.layers = [layer]
            got = resample_ref.Net.run(one, bottoms[0], blobs[bottoms[0]], keep=True, inputs={b: blobs[b] for b in bottoms[1:]})
            for t in tops:
                blobs[t] = got[t]
        return blobs if keep else blobs[output_name]
