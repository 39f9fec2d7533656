#!/usr/bin/env python
"""Generate tests/golden/atrous_golden.npz: dilated convolutions computed by the REAL reference through an identity.

The reference has no dilation, but a dilated convolution IS the plain convolution with the zero-stuffed kernel: d - 1 zeros between the
taps, a kernel of d * (k - 1) + 1 pixels with the same stride and pads (include/feather_hip/feather_atrous.h).  For a handful of small
geometries this script draws seeded inputs, weights and bias, stuffs the kernel on the host, runs the compiled reference (oracle/_ref, see
oracle/Makefile) on it, and records inputs, the UN-stuffed weights and the outputs.  Data only; the fixtures travel to machines without
the reference.

    python tests/golden/make_atrous_golden.py     (needs oracle/_ref/libfeather_ref.so)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle  # noqa: E402
from oracle import Geom  # noqa: E402

import atrous_ref as R  # noqa: E402

# name, C, K, H, W, k, stride, pad, dilation, bias, relu, batch
CASES = [
    ("k3d2p2_row4", 16, 48, 9, 8, 3, 1, 2, 2, 1, 1, 1),
    ("k3d2p2_w7", 16, 48, 8, 7, 3, 1, 2, 2, 1, 0, 1),
    ("k3d2p2_s2", 16, 48, 9, 9, 3, 2, 2, 2, 1, 1, 2),
    ("k3d6p6_far", 16, 48, 5, 8, 3, 1, 6, 6, 1, 1, 1),
    ("k3d2p0_valid", 16, 48, 10, 12, 3, 1, 0, 2, 0, 1, 1),
    ("k3d2p2_c3", 3, 8, 7, 9, 3, 1, 2, 2, 1, 0, 2),           # the generic kernel
    ("k3d3p3_class_head", 16, 3, 8, 8, 3, 1, 3, 3, 1, 0, 2),
    ("k5d2p4", 8, 6, 9, 9, 5, 1, 4, 2, 0, 1, 1),
]


def main():
    if not oracle.have_ref():
        raise SystemExit("oracle/_ref/libfeather_ref.so missing: run `make -C oracle ref` where the reference sources exist")
    ref = oracle.ref()
    out = {"names": np.array([c[0] for c in CASES])}
    for i, (name, c, k, h, w, ks, s, p, d, bias, relu, batch) in enumerate(CASES):
        x, wt, b = R.synth(c, k, h, w, ks, ks, 1, batch, seed=20261018 + i)
        z = R.stuffed_kernel(wt, (d, d))
        geom = Geom(c, k, h, w, z.shape[2], z.shape[3], s, s, p, p, p, p, 1, bias, relu)
        assert ref.select_algo(geom) >= 0
        y = ref.forward(geom, x, np.ascontiguousarray(z), b if bias else None)
        out[name + "/geom"] = np.array([c, k, h, w, ks, s, p, d, bias, relu, batch], np.int32)
        out[name + "/x"] = x
        out[name + "/w"] = wt
        out[name + "/b"] = b
        out[name + "/y"] = y
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "atrous_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(CASES)} cases, {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
