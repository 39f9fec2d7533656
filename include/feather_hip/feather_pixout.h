/* feather_pixout.h -- C-ABI of libfeather_pixout.so: the image OUTPUT path on the MI355X (gfx950), the mirror of fhip_pixels_to_float.
 *
 * A device tensor x[batch][C][h][w] (fp32, dense) becomes uint8 images pixels[batch][target_h][target_w][cn] (interleaved), image n
 * bit-identical to the reference's
 *
 *     ncnn::Mat m = x[n];  if (mean || norm) m.substract_mean_normalize(mean, norm);  m.to_pixels_resize(pixels_n, type, target_w, target_h);
 *
 * (src/ncnn/mat_pixel.cpp:1412-1468: to_rgb / to_gray / to_rgba / to_bgr2rgb, then resize_bilinear_c1 / c3 / c4 of the converted bytes).
 * The library is separate from libfeather_hip.so and needs nothing from it but these headers' constants: link or dlopen either or both.
 * Error codes are fhip_error (feather_hip.h), pixel types FHIP_PIXEL_* (feather_net.h); this library keeps its own last-error slot. */
#ifndef FEATHER_HIP_FEATHER_PIXOUT_H_
#define FEATHER_HIP_FEATHER_PIXOUT_H_

#include <stddef.h>

#include "feather_hip/feather_hip.h"
#include "feather_hip/feather_net.h"

#ifdef __cplusplus
extern "C"
{
#endif

#define FHIP_PIXOUT_API __attribute__((visibility("default")))

/* Channels cn (= C of the tensor) of an OUTPUT pixel type: 3 for FHIP_PIXEL_RGB, _BGR, _RGB2BGR and _BGR2RGB (the last two write the
 * planes in reverse order), 1 for _GRAY, 4 for _RGBA.  FHIP_E_BADARG for every other value: the reference's Mat::to_pixels silently
 * writes nothing for them (and to_pixels_resize then resizes uninitialised memory); here they are refused. */
FHIP_PIXOUT_API int fhip_pixout_channels(int type);

/* x -> pixels on the device, asynchronous on `stream` (a hipStream_t as void*), one launch, no allocation, no copy, no synchronisation:
 * stream-capturable.  Every argument is checked on the host before any device call.
 *   pixels : DEVICE memory, any byte alignment.  Row r of image n starts at pixels + (n * target_h + r) * pitch and is target_w * cn
 *            bytes; the last row ends the buffer, so it holds (batch * target_h - 1) * pitch + target_w * cn bytes.
 *   pitch  : bytes from one output row to the next, 0 = dense (target_w * cn).  Bytes between the rows are not touched.
 *   x      : DEVICE memory, 4-byte aligned, batch * cn * h * w floats.
 *   target : == (w, h) is Mat::to_pixels.  Otherwise the reference's fixed-point bilinear resize of the converted bytes in the output
 *            format; a source 1 pixel wide or high cannot be resized (the reference reads index -1), as on the input side.
 *   mean / norm : HOST arrays of cn floats, indexed by the PLANE of x, or NULL: substract_mean_normalize first, (x - mean) * norm
 *            computed as x * norm + (-(mean * norm)) rounded twice, x - mean or x * norm when one is NULL -- never an FMA.
 * value -> byte is (int) truncation then a clamp to 0..255.  Domain: finite values whose (mapped) magnitude is below 2^31; there the
 * bytes equal the reference's.  Outside it the reference's cast is undefined; here NaN gives 0, -inf and anything below 0 give 0,
 * +inf and anything above 255 give 255.
 * FHIP_E_BADARG: NULL pixels / x, a misaligned x, batch / sizes < 1, a type fhip_pixout_channels refuses, a pitch smaller than a row,
 * a 1-pixel source axis with a resize, more than 2^31 * 256 lanes.  FHIP_E_HIP: the launch failed. */
/* Size limit: FHIP_E_BADARG at 2^31 blocks of 256 lanes or more (batch * target_h * lanes per row: 4 pixels per lane where the rows take vector
 * stores, else one). */
FHIP_PIXOUT_API int fhip_float_to_pixels(unsigned char* pixels, size_t pitch, const float* x, int batch, int type, int w, int h, int target_w,
                                         int target_h, const float* mean, const float* norm, void* stream);

/* The same into HOST memory: converted into a device staging buffer allocated for the call, copied row by row into `pixels_host` (pitch as
 * above, the gaps untouched), `stream` synchronised, the buffer freed.  The uint8 result crosses the bus, not the fp32 tensor. */
FHIP_PIXOUT_API int fhip_float_to_pixels_host(unsigned char* pixels_host, size_t pitch, const float* x, int batch, int type, int w, int h,
                                              int target_w, int target_h, const float* mean, const float* norm, void* stream);

/* Message of this thread's last failing call of this library ("" if none). */
FHIP_PIXOUT_API const char* fhip_pixout_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* FEATHER_HIP_FEATHER_PIXOUT_H_ */
