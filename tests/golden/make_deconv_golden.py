#!/usr/bin/env python
"""Generate tests/golden/deconv_golden.npz: transposed convolutions computed by the REAL reference through an identity.

The reference has no transposed convolution, but for group 1 with kernel - 1 - pad >= 0 the definition (include/feather_hip/feather_deconv.h)
equals a stride-1 CONVOLUTION with the spatially flipped kernel w[k][c][kh-1-i][kw-1-j] (same [K][C] order) of the input with stride - 1
zeros inserted between pixels and kernel - 1 - pad zeros around it (output_pad more at the bottom / right), and that convolution the
reference does compute.  For a handful of small geometries this script draws seeded inputs, weights and bias, builds the stuffed and
pre-padded input on the host, runs the compiled reference (oracle/_ref, see oracle/Makefile) on it without padding, and records the
outputs.  Data only; the fixtures travel to machines without the reference.

    python tests/golden/make_deconv_golden.py     (needs oracle/_ref/libfeather_ref.so)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle  # noqa: E402
from oracle import Geom  # noqa: E402

import deconv_ref as R  # noqa: E402

# name, C, K, H, W, k, stride, pad, output_pad, bias, relu, batch
CASES = [
    ("k4s2p1", 16, 40, 6, 6, 4, 2, 1, 0, 1, 1, 1),
    ("k4s2p1_odd", 16, 40, 5, 7, 4, 2, 1, 0, 1, 0, 1),
    ("k2s2p0", 16, 48, 6, 6, 2, 2, 0, 0, 1, 1, 1),
    ("k3s2p1_op1", 16, 24, 7, 6, 3, 2, 1, 1, 1, 1, 1),
    ("k3s1p1", 16, 48, 7, 9, 3, 1, 1, 0, 1, 1, 1),          # stride 1: the reference takes its Winograd route
    ("k5s3p2_op1", 8, 6, 4, 5, 5, 3, 2, 1, 1, 0, 2),        # the generic kernel
    ("k4s2p1_rgb_head", 16, 3, 8, 8, 4, 2, 1, 0, 1, 0, 2),
    ("k3s2p1_nobias", 3, 8, 7, 9, 3, 2, 1, 1, 0, 1, 2),
]


def stuffed(x, k, s, p, op):
    """The input with s - 1 zeros between pixels, k - 1 - p zeros around it and op more at the bottom / right."""
    n, c, h, w = x.shape
    e = k - 1 - p
    assert e >= 0
    z = np.zeros((n, c, (h - 1) * s + 1 + 2 * e + op, (w - 1) * s + 1 + 2 * e + op), np.float32)
    z[:, :, e:e + (h - 1) * s + 1:s, e:e + (w - 1) * s + 1:s] = x
    return z


def main():
    if not oracle.have_ref():
        raise SystemExit("oracle/_ref/libfeather_ref.so missing: run `make -C oracle ref` where the reference sources exist")
    ref = oracle.ref()
    out = {"names": np.array([c[0] for c in CASES])}
    for i, (name, c, k, h, w, ks, s, p, op, bias, relu, batch) in enumerate(CASES):
        x, wt, b = R.synth(c, k, h, w, ks, ks, 1, batch, seed=20261017 + i, sh=s, sw=s)
        z = stuffed(x, ks, s, p, op)
        geom = Geom(c, k, z.shape[2], z.shape[3], ks, ks, 1, 1, 0, 0, 0, 0, 1, bias, relu)
        assert ref.select_algo(geom) >= 0
        y = ref.forward(geom, z, np.ascontiguousarray(wt[:, :, ::-1, ::-1]), b if bias else None)
        out[name + "/geom"] = np.array([c, k, h, w, ks, s, p, op, bias, relu, batch], np.int32)
        out[name + "/x"] = x
        out[name + "/w"] = wt
        out[name + "/b"] = b
        out[name + "/y"] = y
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "deconv_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(CASES)} cases, {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
