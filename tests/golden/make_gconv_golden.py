#!/usr/bin/env python
"""Generate tests/golden/gconv_golden.npz: grouped convolutions (1 < group < C) computed by the REAL reference on slices.

The reference's ConvBooster refuses a partial group (avx/booster.cpp:304-308), but a grouped layer is `group` independent group == 1
convolutions on channel slices, and each of those it does compute.  For a handful of small geometries this script draws seeded inputs,
weights and bias, runs the compiled reference (oracle/_ref, see oracle/Makefile) once per group on x[:, g * C/g : (g + 1) * C/g] with
w[g * K/g : (g + 1) * K/g] and records the concatenated outputs.  Data only; the fixtures travel to machines without the reference.

    python tests/golden/make_gconv_golden.py     (needs oracle/_ref/libfeather_ref.so)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle  # noqa: E402
from oracle import Geom  # noqa: E402

import gconv_ref as R  # noqa: E402

# name, C, K, group, H, W, kh, kw, (sh, sw), pads (left, right, top, bottom), bias, relu, batch
CASES = [
    ("g4_3x3_s1", 16, 16, 4, 12, 16, 3, 3, (1, 1), (1, 1, 1, 1), 1, 1, 2),          # C/g = 4, Winograd per slice
    ("g2_3x3_s2", 16, 32, 2, 13, 11, 3, 3, (2, 2), (1, 1, 1, 1), 1, 1, 2),
    ("g4_1x1", 32, 24, 4, 9, 10, 1, 1, (1, 1), (0, 0, 0, 0), 1, 0, 2),
    ("g5_5x5", 10, 15, 5, 11, 12, 5, 5, (1, 1), (2, 2, 2, 2), 1, 1, 1),
    ("g4_3x3_asym_pad", 16, 16, 4, 9, 12, 3, 3, (1, 1), (0, 1, 1, 0), 1, 0, 2),
    ("g3_3x3_odd_cg", 9, 6, 3, 10, 11, 3, 3, (1, 1), (1, 1, 1, 1), 1, 1, 3),         # C/g = 3
    ("g2_3x3_nobias", 8, 8, 2, 10, 16, 3, 3, (2, 2), (1, 1, 1, 1), 0, 1, 2),
    ("g32_resnext", 128, 128, 32, 14, 12, 3, 3, (1, 1), (1, 1, 1, 1), 1, 1, 1),
]


def main():
    if not oracle.have_ref():
        raise SystemExit("oracle/_ref/libfeather_ref.so missing: run `make -C oracle ref` where the reference sources exist")
    ref = oracle.ref()
    out = {"names": np.array([c[0] for c in CASES])}
    for i, (name, c, k, group, h, w, kh, kw, (sh, sw), (pl, pr, pt, pb), bias, relu, batch) in enumerate(CASES):
        x, wt, b = R.synth(c, k, h, w, kh, kw, group, batch, seed=20261016 + i)
        cg, kg = c // group, k // group
        parts = []
        for g in range(group):
            geom = Geom(cg, kg, h, w, kh, kw, sh, sw, pl, pr, pt, pb, 1, bias, relu)
            assert ref.select_algo(geom) >= 0
            parts.append(ref.forward(geom, x[:, g * cg:(g + 1) * cg], wt[g * kg:(g + 1) * kg], b[g * kg:(g + 1) * kg] if bias else None))
        out[name + "/geom"] = np.array([c, k, group, h, w, kh, kw, sh, sw, pl, pr, pt, pb, bias, relu, batch], np.int32)
        out[name + "/x"] = x
        out[name + "/w"] = wt
        out[name + "/b"] = b
        out[name + "/y"] = np.concatenate(parts, axis=1)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gconv_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(CASES)} cases, {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
