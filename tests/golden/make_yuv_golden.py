"""Record tests/golden/yuv_golden.npz from the reference's own NV21 and pixel functions.

Compiles the reference tree's src/ncnn/{mat,mat_pixel,mat_pixel_resize}.cpp where it lies (--reference, default /root/reference) with a
small driver of our own, host g++, in a temporary directory outside the repository (as make_pixel_golden.py does), and records:
  - both NV21 chains for PIXEL_RGB / RGB2BGR / RGB2GRAY over sizes that downscale, upscale, keep the size, have extreme aspect ratios
    and hit the 4-pixel minimum, target widths that are and are not multiples of 4:
      chain 1: resize_bilinear_yuv420sp -> yuv420sp2rgb -> Mat::from_pixels;  chain 0: yuv420sp2rgb -> Mat::from_pixels_resize;
  - resize_bilinear_c2 and resize_bilinear_yuv420sp on their own;
  - Mat::to_pixels and Mat::to_pixels_resize of fp32 Mats (values in -60..320 with fractions, so truncation and both clamps show).
Outputs are whole numbers 0..255 (or bytes) and are stored as uint8; the seeded inputs are stored too.

    python tests/golden/make_yuv_golden.py [--reference DIR]
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
from pixels_ref import PIXEL_BGR, PIXEL_BGR2RGB, PIXEL_GRAY, PIXEL_RGB, PIXEL_RGB2BGR, PIXEL_RGBA  # noqa: E402
from yuv_ref import TYPES  # noqa: E402

# (w, h, target_w, target_h): both chains
SIZES = [(64, 48, 20, 16), (40, 30, 14, 10), (12, 8, 36, 26), (16, 12, 16, 12), (200, 4, 6, 40), (4, 160, 50, 6), (4, 4, 10, 6),
         (4, 4, 2, 2), (24, 18, 24, 8), (6, 4, 4, 4)]
# chain 0 only: odd target sizes, 2-pixel frames
SIZES0 = [(6, 2, 9, 5), (10, 6, 7, 3), (2, 2, 3, 3), (22, 14, 13, 14)]
C2 = [(9, 7, 4, 11), (2, 2, 3, 3), (30, 20, 12, 8), (5, 9, 5, 9)]
YUV = [(40, 30, 14, 10), (4, 4, 8, 2), (16, 12, 16, 12)]
# (type, w, h, c, target_w, target_h); target == size is to_pixels
TO_PIXELS = [(PIXEL_RGB, 7, 5, 3, 7, 5), (PIXEL_BGR, 7, 5, 3, 7, 5), (PIXEL_GRAY, 7, 5, 1, 7, 5), (PIXEL_RGBA, 7, 5, 4, 7, 5),
             (PIXEL_RGB2BGR, 7, 5, 3, 7, 5), (PIXEL_BGR2RGB, 7, 5, 3, 7, 5), (PIXEL_RGB, 13, 9, 3, 6, 11), (PIXEL_GRAY, 13, 9, 1, 20, 4),
             (PIXEL_RGBA, 8, 8, 4, 3, 3), (PIXEL_BGR2RGB, 9, 6, 3, 17, 12)]

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mat.h"
// stdin, repeated, a tag then numbers then raw input bytes; stdout: the output bytes
//   C type w h tw th resize_first + w*h*3/2 bytes  -> cout*th*tw bytes (the whole-number values of the fp32 Mat)
//   R2 sw sh dw dh + sw*sh*2 bytes                 -> dw*dh*2 bytes of resize_bilinear_c2
//   RY sw sh dw dh + sw*sh*3/2 bytes               -> dw*dh*3/2 bytes of resize_bilinear_yuv420sp
//   P type w h c tw th + c*h*w floats              -> th*tw*cn bytes of to_pixels_resize (to_pixels at equal size)
static unsigned char* in(size_t n) { unsigned char* p = (unsigned char*)malloc(n); if (fread(p, 1, n, stdin) != n) exit(2); return p; }
int main()
{
    char tag[4];
    while (scanf("%3s", tag) == 1)
    {
        if (!strcmp(tag, "C"))
        {
            int type, w, h, tw, th, rf;
            if (scanf("%d %d %d %d %d %d", &type, &w, &h, &tw, &th, &rf) != 6) return 3;
            getchar();
            unsigned char* yuv = in((size_t)w * h * 3 / 2);
            ncnn::Mat m;
            if (rf)
            {
                unsigned char* r = (unsigned char*)malloc((size_t)tw * th * 3 / 2);
                unsigned char* rgb = (unsigned char*)malloc((size_t)tw * th * 3);
                ncnn::resize_bilinear_yuv420sp(yuv, w, h, r, tw, th);
                ncnn::yuv420sp2rgb(r, tw, th, rgb);
                m = ncnn::Mat::from_pixels(rgb, type, tw, th);
                free(r);
                free(rgb);
            }
            else
            {
                unsigned char* rgb = (unsigned char*)malloc((size_t)w * h * 3);
                ncnn::yuv420sp2rgb(yuv, w, h, rgb);
                m = ncnn::Mat::from_pixels_resize(rgb, type, w, h, tw, th);
                free(rgb);
            }
            if (m.w != tw || m.h != th) return 4;
            for (int q = 0; q < m.c; ++q)
            {
                const float* p = m.channel(q);
                for (int i = 0; i < tw * th; ++i)
                {
                    if (p[i] < 0.f || p[i] > 255.f || p[i] != (float)(int)p[i]) return 5;
                    putchar((int)p[i]);
                }
            }
            free(yuv);
        }
        else if (!strcmp(tag, "R2") || !strcmp(tag, "RY"))
        {
            int sw, sh, dw, dh;
            if (scanf("%d %d %d %d", &sw, &sh, &dw, &dh) != 4) return 6;
            getchar();
            const bool c2 = tag[1] == '2';
            unsigned char* src = in(c2 ? (size_t)sw * sh * 2 : (size_t)sw * sh * 3 / 2);
            const size_t n = c2 ? (size_t)dw * dh * 2 : (size_t)dw * dh * 3 / 2;
            unsigned char* dst = (unsigned char*)malloc(n);
            if (c2) ncnn::resize_bilinear_c2(src, sw, sh, dst, dw, dh);
            else ncnn::resize_bilinear_yuv420sp(src, sw, sh, dst, dw, dh);
            fwrite(dst, 1, n, stdout);
            free(src);
            free(dst);
        }
        else if (!strcmp(tag, "P"))
        {
            int type, w, h, c, tw, th;
            if (scanf("%d %d %d %d %d %d", &type, &w, &h, &c, &tw, &th) != 6) return 7;
            getchar();
            ncnn::Mat m(w, h, c);
            for (int q = 0; q < c; ++q)
                if (fread((float*)m.channel(q), sizeof(float), (size_t)w * h, stdin) != (size_t)w * h) return 8;
            const size_t n = (size_t)tw * th * c;
            unsigned char* dst = (unsigned char*)malloc(n);
            m.to_pixels_resize(dst, type, tw, th);
            fwrite(dst, 1, n, stdout);
            free(dst);
        }
        else
            return 9;
        fflush(stdout);
    }
    return 0;
}
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(HERE, "yuv_golden.npz"))
    a = ap.parse_args()
    src = os.path.join(a.reference, "src", "ncnn")
    tmp = tempfile.mkdtemp(prefix="yuv_golden_")
    try:
        drv = os.path.join(tmp, "driver.cpp")
        open(drv, "w").write(DRIVER)
        exe = os.path.join(tmp, "driver")
        forced = sum((["-include", h] for h in ("cstddef", "cstdlib", "climits", "algorithm", "cmath")), [])
        subprocess.run(["g++", "-std=c++11", "-O2", *forced, "-I" + src, drv] + [os.path.join(src, f) for f in
                       ("mat.cpp", "mat_pixel.cpp", "mat_pixel_resize.cpp")] + ["-o", exe], check=True)
        rng = np.random.default_rng(2025)
        arrays, stdin, want = {}, b"", []
        cases = []
        for rf, sizes in ((1, SIZES), (0, SIZES + SIZES0)):
            for (w, h, tw, th) in sizes:
                key = f"in_{w}x{h}"
                if key not in arrays:
                    arrays[key] = rng.integers(0, 256, (h * 3 // 2, w), dtype=np.uint8)
                for name, t in TYPES.items():
                    cout = 1 if name == "RGB2GRAY" else 3
                    stdin += f"C {t} {w} {h} {tw} {th} {rf}\n".encode() + arrays[key].tobytes()
                    want.append((f"out_{name}_{w}x{h}_{tw}x{th}_rf{rf}", (cout, th, tw)))
                    cases.append((t, w, h, tw, th, rf))
        for (sw, sh, dw, dh) in C2:
            arrays[f"c2in_{sw}x{sh}"] = x = rng.integers(0, 256, (sh, sw, 2), dtype=np.uint8)
            stdin += f"R2 {sw} {sh} {dw} {dh}\n".encode() + x.tobytes()
            want.append((f"c2_{sw}x{sh}_{dw}x{dh}", (dh, dw, 2)))
        for (sw, sh, dw, dh) in YUV:
            x = arrays[f"in_{sw}x{sh}"]
            stdin += f"RY {sw} {sh} {dw} {dh}\n".encode() + x.tobytes()
            want.append((f"yuvresize_{sw}x{sh}_{dw}x{dh}", (dh * 3 // 2, dw)))
        for (t, w, h, c, tw, th) in TO_PIXELS:
            key = f"mat_{w}x{h}x{c}"
            if key not in arrays:
                arrays[key] = (rng.integers(-60, 321, (c, h, w)) + rng.choice(np.array([0, 0.25, 0.5, 0.99], np.float32), (c, h, w))
                               ).astype(np.float32)
            stdin += f"P {t} {w} {h} {c} {tw} {th}\n".encode() + arrays[key].tobytes()
            want.append((f"topix_{t}_{w}x{h}x{c}_{tw}x{th}", (th, tw, c)))
        raw = subprocess.run([exe], input=stdin, capture_output=True, check=True).stdout
        pos, out = 0, {}
        for key, shape in want:
            size = int(np.prod(shape))
            out[key] = np.frombuffer(raw[pos:pos + size], dtype=np.uint8).reshape(shape)
            pos += size
        assert pos == len(raw), (pos, len(raw))
        np.savez_compressed(a.out, cases=np.array(cases, dtype=np.int64), c2=np.array(C2, np.int64), yuvresize=np.array(YUV, np.int64),
                            topixels=np.array(TO_PIXELS, np.int64), **arrays, **out)
        print(f"{a.out}: {len(cases)} chain cases, {len(C2)} c2, {len(YUV)} yuv420sp resizes, {len(TO_PIXELS)} to_pixels, "
              f"{os.path.getsize(a.out)} bytes")
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
