"""Record tests/golden/pixel_golden.npz from the reference's own pixel functions.

Compiles the reference tree's src/ncnn/{mat,mat_pixel,mat_pixel_resize}.cpp where it lies (--reference, default /root/reference) with a
small driver of our own, host g++, in a temporary directory outside the repository; runs ncnn::Mat::from_pixels_resize on seeded random
images for every pixel type and a set of sizes (downscale, upscale, identity, extreme aspect ratios, 2-pixel sources); stores inputs and
outputs; deletes the binaries.  Outputs are whole numbers 0..255 and are stored as uint8.  Inputs depend only on the source channel count,
so one image per (channels, size) serves every type.

    python tests/golden/make_pixel_golden.py [--reference DIR]
"""
from __future__ import annotations

import argparse
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from pixels_ref import TYPES, channels  # noqa: E402

# (w, h, target_w, target_h)
SIZES = [(37, 29, 16, 12), (13, 9, 31, 22), (11, 7, 11, 7), (300, 7, 5, 60), (7, 300, 60, 5), (2, 2, 5, 7), (2, 5, 3, 1),
         (40, 30, 96, 72), (96, 80, 23, 19), (37, 29, 37, 15)]

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include "mat.h"
// stdin: type w h tw th, then w*h*cin bytes; stdout: cout*th*tw bytes (the values of the fp32 Mat, all whole numbers 0..255)
int main()
{
    int type, w, h, tw, th, cin;
    while (scanf("%d %d %d %d %d %d", &type, &w, &h, &tw, &th, &cin) == 6)
    {
        getchar();
        unsigned char* px = (unsigned char*)malloc((size_t)w * h * cin);
        if (fread(px, 1, (size_t)w * h * cin, stdin) != (size_t)w * h * cin) return 2;
        ncnn::Mat m = ncnn::Mat::from_pixels_resize(px, type, w, h, tw, th);
        if (m.w != tw || m.h != th) return 3;
        for (int q = 0; q < m.c; ++q)
        {
            const float* p = m.channel(q);
            for (int i = 0; i < tw * th; ++i)
            {
                if (p[i] < 0.f || p[i] > 255.f || p[i] != (float)(int)p[i]) return 4;
                putchar((int)p[i]);
            }
        }
        fflush(stdout);
        free(px);
    }
    return 0;
}
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(HERE, "pixel_golden.npz"))
    a = ap.parse_args()
    src = os.path.join(a.reference, "src", "ncnn")
    tmp = tempfile.mkdtemp(prefix="pixel_golden_")
    try:
        drv = os.path.join(tmp, "driver.cpp")
        open(drv, "w").write(DRIVER)
        exe = os.path.join(tmp, "driver")
        forced = sum((["-include", h] for h in ("cstddef", "cstdlib", "climits", "algorithm", "cmath")), [])
        subprocess.run(["g++", "-std=c++11", "-O2", *forced, "-I" + src, drv] + [os.path.join(src, f) for f in
                       ("mat.cpp", "mat_pixel.cpp", "mat_pixel_resize.cpp")] + ["-o", exe], check=True)
        rng = np.random.default_rng(2024)
        inputs = {}
        for cin in (1, 3, 4):
            for (w, h, _, _) in SIZES:
                inputs.setdefault(f"in_c{cin}_{w}x{h}", rng.integers(0, 256, (h, w, cin), dtype=np.uint8))
        out, cases, stdin, want = {}, [], b"", []
        for name, t in TYPES.items():
            cin, cout = channels(t)
            for (w, h, tw, th) in SIZES:
                px = inputs[f"in_c{cin}_{w}x{h}"]
                stdin += f"{t} {w} {h} {tw} {th} {cin}\n".encode() + px.tobytes()
                want.append((f"out_{name}_{w}x{h}_{tw}x{th}", cout * th * tw, (cout, th, tw)))
                cases.append((name, t, w, h, tw, th))
        raw = subprocess.run([exe], input=stdin, capture_output=True, check=True).stdout
        pos = 0
        for key, size, shape in want:
            out[key] = np.frombuffer(raw[pos:pos + size], dtype=np.uint8).reshape(shape)
            pos += size
        assert pos == len(raw), (pos, len(raw))
        np.savez_compressed(a.out, cases=np.array([(t, w, h, tw, th) for (_, t, w, h, tw, th) in cases], dtype=np.int64),
                            names=np.array([c[0] for c in cases]), **inputs, **out)
        print(f"{a.out}: {len(cases)} cases, {os.path.getsize(a.out)} bytes")
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
