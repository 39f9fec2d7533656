/* feather_frame.h -- C-ABI of libfeather_frame.so: the layers that frame an image-to-image net on the MI355X (gfx950) -- ncnn's Padding, Crop and
 * PixelShuffle -- on fp32 blobs with a leading batch.  All three are per image: a batch is n independent images.
 *
 * The reference has none of these layers: this text is the definition, written from what ncnn's padding.cpp, crop.cpp and pixelshuffle.cpp
 * do, with ncnn's parameter ids.  Where it had to decide something, it says "decided here".  tests/frame_ref.py restates it line by line.
 * Nothing is computed but the optional ReLU of PixelShuffle: every other output element is a bit copy of one input element or of the
 * constant, so NaN payloads and -0.0 survive.
 *
 * The window     Padding and Crop are one operation.  For in[n][c][h][w] take six signed margins front, behind (channels), top, bottom (rows),
 *                left, right (columns): a positive margin pads, a negative one crops.  The output is
 *                   [n][c + front + behind][h + top + bottom][w + left + right]
 *                   out[q][y][x] = in[q - front][map(y - top, h)][map(x - left, w)]     where the mapped source exists
 *                type 0 (constant)   map(i, d) = i; an output element whose source channel, row or column lies outside the input is
 *                                    `value` -- or per_channel[q - front] where that array is given and q - front is a source channel
 *                                    (ncnn's per_channel_pad_data; a padded CHANNEL is `value` in either case: decided here)
 *                type 1 (replicate)  map(i, d) = min(max(i, 0), d - 1); any pad is allowed
 *                type 2 (reflect)    map(i, d) = i < 0 ? -i : i >= d ? 2 * (d - 1) - i : i: the edge pixel is not repeated (numpy's "reflect",
 *                                    ncnn's BORDER_REFLECT); a pad of d or more is refused
 *                front / behind > 0 is defined for type 0 only; per_channel likewise.  Negative margins are allowed with every type, and a
 *                side may be cropped while the opposite side is padded.  A window without a positive margin (a crop, or a copy) reads
 *                no border whatever its type says.
 *                ncnn's Padding is the window with margins >= 0 (params 0=top 1=bottom 2=left 3=right 4=type 5=value
 *                6=per_channel_pad_data_size 7=front 8=behind); ncnn's Crop with offsets (woffset, hoffset, coffset) and sizes (outw, outh,
 *                outc) is the window with left = -woffset, right = outw + woffset - w, and so on.
 *
 * PixelShuffle   params 0=upscale_factor r, 1=mode.  in[n][C * r * r][h][w] -> out[n][C][h * r][w * r]:
 *                   mode 0:  out[q][i * r + sh][j * r + sw] = in[q * r * r + sh * r + sw][i][j]        (PyTorch's pixel_shuffle)
 *                   mode 1:  the input channel is (sh * r + sw) * C + q                               (the inverse of Reorg mode 1, feather_yolo.h)
 *                `relu` applies an activation to every element as it is stored:
 *                   0: none (a bit copy)
 *                   1: y = x > 0 ? x : x * slope, one product (ncnn's ReLU 0=slope, the leaky ReLU of feather_inorm.h; with slope 0 a
 *                      negative x gives -0.0 and a NaN stays a NaN)
 *                   2: y = fmaxf(x, 0.f), `slope` ignored: the plain ReLU layer of feather::Net (fhip_relu), the same device maximum.  A NaN
 *                      becomes +0.0; a -0.0 becomes a zero whose sign is that maximum's.  Decided here: it is what lets the Net fuse a
 *                      plain ReLU bit for bit.
 *
 * Limits, refused with FHIP_E_BADARG and never truncated: every dimension >= 1, every output dimension >= 1, fewer than 2^31 elements on
 * either side.  No entry allocates, copies or synchronises: every device entry is one launch and hipGraph-capturable.  Pointers need 4-byte
 * alignment; 16-byte aligned ones take the wider forms.  No layer is in place.  The library is separate from libfeather_hip.so and needs
 * nothing from it but the enums of feather_hip.h; it keeps its own last-error slot. */
#ifndef FEATHER_HIP_FEATHER_FRAME_H_
#define FEATHER_HIP_FEATHER_FRAME_H_

#include <stddef.h>

#include "feather_hip/feather_hip.h"

#ifdef __cplusplus
extern "C"
{
#endif

#define FHIP_FRAME_API __attribute__((visibility("default")))

/* Route code fhip_net_layer_info reports for the layers of a net with fhip_net_set_frame (feather_net.h): Padding, Crop and PixelShuffle. */
#define FHIP_FRAME_NET_ROUTE 112

/* floats of the LDS tile of the PixelShuffle kernel: planes whose output row, r * w floats, passes it take the direct kernel */
#define FHIP_FRAME_TILE 4096
/* the fewest elements a block of the tile kernel moves: smaller planes (min(h * r, FHIP_FRAME_TILE / (r * w)) * r * w below it) take the
 * direct kernel, whose grid is bounded by the element count */
#define FHIP_FRAME_TILE_MIN 1024

/* window types (ncnn's Padding 4=type) */
#define FHIP_FRAME_CONSTANT 0
#define FHIP_FRAME_REPLICATE 1
#define FHIP_FRAME_REFLECT 2

/* `relu` of fhip_pixel_shuffle_forward */
#define FHIP_FRAME_RELU_NONE 0
#define FHIP_FRAME_RELU_SLOPE 1
#define FHIP_FRAME_RELU_PLAIN 2

/* `what` of fhip_frame_route */
enum fhip_frame_op
{
    FHIP_FRAME_WINDOW = 0, /* a = type, w unused, b = 1 where some margin is positive, out_w, aligned16 = 1 where `out` is 16-byte aligned */
    FHIP_FRAME_SHUFFLE = 1 /* a = r, w = the input's w, b = the input's h */
};

/* The (c, h, w) of the window of an input (c, h, w).  FHIP_E_BADARG: a dimension < 1, an output dimension < 1 (or one that does not fit an
 * int), a NULL pointer. */
FHIP_FRAME_API int fhip_frame_window_output_dim(int c, int h, int w, int front, int behind, int top, int bottom, int left, int right, int* out_c,
                                                int* out_h, int* out_w);

/* out = the window of in[n][c][h][w] as defined above: one launch of "fhip::window_kernel<T, V>" on `stream` (a hipStream_t as void*).
 * per_channel: NULL, or a DEVICE array of c floats.  FHIP_E_BADARG: what fhip_frame_window_output_dim refuses, n < 1, 2^31 elements or more on
 * either side, a type outside 0 .. 2, a reflect pad >= its dimension, front / behind > 0 or per_channel with a type other than 0, NULL or
 * unaligned (4 bytes) pointers, out overlapping in. */
FHIP_FRAME_API int fhip_frame_window_forward(int type, float value, const float* per_channel, int n, int c, int h, int w, int front, int behind,
                                             int top, int bottom, int left, int right, float* out, const float* in, void* stream);

/* The (c, h, w) of PixelShuffle's output.  FHIP_E_BADARG: r < 1, a dimension < 1, c % (r * r) != 0, an extent that does not fit an int, a
 * NULL pointer. */
FHIP_FRAME_API int fhip_pixel_shuffle_output_dim(int r, int c, int h, int w, int* out_c, int* out_h, int* out_w);

/* out = PixelShuffle(in[n][c][h][w]) as defined above, c = C * r * r: one launch.  FHIP_E_BADARG: what fhip_pixel_shuffle_output_dim refuses,
 * a mode outside 0 / 1, relu outside 0 .. 2, n < 1, 2^31 elements or more, NULL or unaligned (4 bytes) pointers, out overlapping in. */
FHIP_FRAME_API int fhip_pixel_shuffle_forward(int r, int mode, int relu, float slope, int n, int c, int h, int w, float* out, const float* in,
                                              void* stream);

/* The kernel instantiation a call would launch, as the demangled name without return type and parameters, copied into name[len]:
 *   FHIP_FRAME_WINDOW   "fhip::window_kernel<T, V>".  A lane owns 4 consecutive output pixels of one row.  T is the type (0 .. 2) where
 *                       some margin is positive and 3 where none is -- a crop or a copy, which has no border code at all.  V = 1 where
 *                       out_w % 4 == 0 and `out` is 16-byte aligned: the lane stores one 16-byte vector; V = 0: scalar stores.  Interior
 *                       lanes whose source run is 16-byte aligned load it as one vector in every instantiation.
 *   FHIP_FRAME_SHUFFLE  "fhip::pixel_shuffle_tile_kernel" where r > 1, r * w <= FHIP_FRAME_TILE and a block moves FHIP_FRAME_TILE_MIN elements or
 *                       more: a block loads the r contiguous input rows behind each of a group of output rows into LDS, interleaved, and
 *                       writes the group as one contiguous run, both sides coalesced; else "fhip::pixel_shuffle_direct_kernel": one output
 *                       element per lane, coalesced stores
 * FHIP_E_BADARG: an unknown `what`, NULL name, len < 1, a type outside 0 .. 2, out_w, r, h or w < 1. */
FHIP_FRAME_API int fhip_frame_route(int what, int a, int w, int b, int out_w, int aligned16, char* name, int len);

/* Message of this thread's last failing call of this library ("" if none). */
FHIP_FRAME_API const char* fhip_frame_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* FEATHER_HIP_FEATHER_FRAME_H_ */
