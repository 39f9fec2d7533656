/* feather_shuffle.h -- C-ABI of libfeather_shuffle.so: ncnn's ShuffleChannel and Slice, and every composition of them with Concat, as ONE
 * kernel family on the MI355X (gfx950): the channel map.
 *
 * The reference has neither layer.  The definitions (this text is the contract), dense NCHW fp32 with a leading batch:
 *
 *   ShuffleChannel  ncnn .param: 0=group (default 1), 1=reverse (default 0); no weights.  View the C channels as [group][C / group] and
 *                   transpose to [C / group][group]:  out channel i * group + k  =  in channel k * (C / group) + i
 *                   (0 <= i < C / group, 0 <= k < group).  reverse = 1 applies the inverse permutation, which is the same shuffle with
 *                   group' = C / group.  group < 1 or C % group != 0 is a parameter error.
 *   Slice           ncnn .param: -23300=count,s0,s1,...  1=axis (default 0 = channels); no weights.  Top j takes the next s_j channels of
 *                   the bottom, in order.  An entry of -233 means an equal share of what is left: (C - used) / (entries left), integer
 *                   division.  Every resolved size must be >= 1 and the sizes must sum to at most C (channels beyond the sum are
 *                   dropped).  Only the channel axis is supported.
 *   channel map     out_j[n][r][h][w] = src_{s(j,r)}[n][c(j,r)][h][w]: every output channel names one channel of one source.  Concat,
 *                   ShuffleChannel, Slice and every chain of them are such tables; at most FHIP_CHANNEL_MAP_MAX_BLOBS sources and as many
 *                   outputs per map.
 *
 * The kernels only copy: results are bit-identical to the sources.  Planes with h * w a multiple of 4 between 16-byte aligned tensors
 * move as 16-byte accesses; everything else (7 x 7 planes, offset pointers) as 4-byte accesses, which are correct for any 4-byte aligned
 * pointer.  One launch per call, on `stream` (a hipStream_t as void*), no allocation, no copy, no synchronisation in any *_forward:
 * hipGraph-capturable.  No output may overlap a source.
 *
 * The library is separate from libfeather_hip.so and needs nothing from it but the enums of feather_hip.h (fhip_error): link or dlopen
 * either or both.  It keeps its own last-error slot. */
#ifndef FEATHER_HIP_FEATHER_SHUFFLE_H_
#define FEATHER_HIP_FEATHER_SHUFFLE_H_

#include <stddef.h>

#include "feather_hip/feather_hip.h"

#ifdef __cplusplus
extern "C"
{
#endif

#define FHIP_SHUFFLE_API __attribute__((visibility("default")))

/* sources, and outputs, of one channel map */
#define FHIP_CHANNEL_MAP_MAX_BLOBS 4
/* the "equal share of what is left" entry of a Slice */
#define FHIP_SLICE_SHARE (-233)

/* `route` of fhip_channel_map_forward_route and the last template argument of the kernel names */
enum fhip_channel_map_route_kind
{
    FHIP_CHANNEL_MAP_ROUTE_4B = 0, /* 4-byte accesses: any plane, any 4-byte aligned pointer */
    FHIP_CHANNEL_MAP_ROUTE_16B = 1 /* 16-byte accesses: h * w a multiple of 4 and every pointer 16-byte aligned */
};

/* `kind` of fhip_channel_map_route: which of the three entry points */
enum fhip_channel_map_kind
{
    FHIP_CHANNEL_MAP_TABLE = 0,   /* fhip_channel_map_forward: the map is a device table */
    FHIP_CHANNEL_MAP_SHUFFLE = 1, /* fhip_channel_shuffle_forward: the map is arithmetic */
    FHIP_CHANNEL_MAP_SLICE = 2    /* fhip_channel_slice_forward: the map is a prefix-sum lookup */
};

/* 0 when a tensor of this shape can be moved (every dimension >= 1, fewer than 2^31 elements in every blob), else FHIP_E_BADARG with a
 * message.  Pure, no device call. */
FHIP_SHUFFLE_API int fhip_channel_map_supported(int n, int c, int h, int w);

/* Slice sizes with their -233 entries resolved against c channels, into resolved[count].  Pure, no device call.  FHIP_E_BADARG: NULL,
 * count < 1, an entry that is neither positive nor -233, a resolved size < 1, a sum above c. */
FHIP_SHUFFLE_API int fhip_channel_slice_resolve(int c, const int* sizes, int count, int* resolved);

/* out[n][c][h][w] = ShuffleChannel(in) as defined above.  FHIP_E_BADARG: an unsupported shape, group < 1, c % group != 0, NULL or
 * misaligned (4 bytes) pointers.  FHIP_E_HIP: the launch failed. */
/* Size limit (every forward entry point of this header and fhip_channel_map_supported): a tensor of 2^31 elements or more (n * c * h * w, of any
 * source or output, and n * rows * h * w of a map) is refused with FHIP_E_BADARG; fhip_channel_map_create refuses 2^24 output channels or more. */
FHIP_SHUFFLE_API int fhip_channel_shuffle_forward(float* out, const float* in, int n, int c, int h, int w, int group, int reverse, void* stream);

/* outs[j][n][sizes_j][h][w] = the j-th slice of in[n][c][h][w]; sizes as in the .param (-233 allowed), count <= FHIP_CHANNEL_MAP_MAX_BLOBS;
 * `outs` and `sizes` are host arrays.  One launch writes every output.  FHIP_E_BADARG: what fhip_channel_slice_resolve refuses, too many
 * outputs, an unsupported shape, NULL or misaligned pointers. */
FHIP_SHUFFLE_API int fhip_channel_slice_forward(float* const* outs, const float* in, int n, int c, int h, int w, const int* sizes, int count,
                                                void* stream);

/* The general form.  A map is built once on the host, checked there, and kept on the device: `entries` holds, for the outputs one after
 * the other and for each of their channels in order, the pair (source index, source channel); sum(out_channels) pairs in all.
 * fhip_channel_map_create allocates and copies (Reshape / Init time, never inside a captured region); the table cannot name anything outside
 * the sources it was built for.  FHIP_E_BADARG: NULL, a count outside 1 .. FHIP_CHANNEL_MAP_MAX_BLOBS, a channel count < 1, a pair that names
 * no source channel.  FHIP_E_HIP: the allocation or the copy failed. */
typedef struct fhip_channel_map fhip_channel_map;
FHIP_SHUFFLE_API int fhip_channel_map_create(fhip_channel_map** map, const int* src_channels, int n_src, const int* out_channels, int n_out,
                                             const int* entries);
FHIP_SHUFFLE_API int fhip_channel_map_destroy(fhip_channel_map* map);

/* outs[j][n][out_channels_j][h][w] from srcs[s][n][src_channels_s][h][w] by the map: one launch whatever the number of sources and outputs.
 * `outs` / `srcs` are host arrays of n_out / n_src device pointers.  FHIP_E_BADARG: NULL, an unsupported shape, misaligned pointers. */
FHIP_SHUFFLE_API int fhip_channel_map_forward(const fhip_channel_map* map, float* const* outs, const float* const* srcs, int n, int h, int w,
                                              void* stream);

/* fhip_channel_map_forward with the access width given instead of selected (fhip_channel_map_route_kind), so that the two can be timed
 * against each other (tools/shuffle_bench.py) and tested.  FHIP_E_BADARG also: an unknown route, 16-byte accesses on a plane or a pointer
 * that does not allow them. */
FHIP_SHUFFLE_API int fhip_channel_map_forward_route(int route, const fhip_channel_map* map, float* const* outs, const float* const* srcs, int n,
                                                    int h, int w, void* stream);

/* The kernel instantiation an entry point (`kind`) launches for planes of h x w between these `count` pointers (only looked at for their
 * alignment), as the demangled name without return type and parameters, e.g. "fhip::channel_map_kernel<0, true>", copied into name[len]. */
FHIP_SHUFFLE_API int fhip_channel_map_route(int kind, int h, int w, const void* const* pointers, int count, char* name, int len);

/* Message of this thread's last failing call of this library ("" if none). */
FHIP_SHUFFLE_API const char* fhip_shuffle_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* FEATHER_HIP_FEATHER_SHUFFLE_H_ */
