/* gcd_amd_pardom.h — gcd_amd/libgcd_amd_pardom.so (gcd_amd/csrc/pardom.hip): the colours of a ParallelDomain point cloud
 * (gcd_amd/geometry.py class_colours, synth_rgb_pardom): a point's colour is its stored RGB, the colour of its semantic
 * class, or a blend of the two, written as float64 for the splat of include/gcd_amd_render.h to read.
 *
 * A library of its own (gcd_amd/csrc/build.py LIBRARIES, gcd_amd/_lib_pardom.py): include/gcd_amd_render.h and its ABI
 * version do not change.  Same rules as gcd_amd.h: raw device pointers, the caller's hipStream_t, no allocation, no
 * synchronisation; every argument is checked before anything is launched, and a non-zero status comes with a message in
 * gcd_pardom_last_error().  Every payload element of `out` and the counter are stored by every call; the only atomic is
 * an integer one, so a result is bit-identical from call to call. */
#ifndef GCD_AMD_PARDOM_H
#define GCD_AMD_PARDOM_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCD_AMD_PARDOM_ABI_VERSION 1
/* rows of a palette: one per value of a uint8 class id */
#define GCD_PARDOM_PALETTE_ROWS 256
/* largest row stride (ids_ld, rgb_ld, out_ld), in elements: byte offsets stay far inside int64 */
#define GCD_PARDOM_MAX_LD 16777216
/* mode */
#define GCD_PARDOM_RGB 0
#define GCD_PARDOM_BLEND 1
#define GCD_PARDOM_PALETTE 2

int gcd_pardom_abi_version(void);
const char* gcd_pardom_last_error(void);

/* ids: uint8, point i at ids[i * ids_ld], 1 <= ids_ld; null in mode RGB, which reads no id.
 * rgb: uint8, channel c of point i at rgb[i * rgb_ld + c], 3 <= rgb_ld; null in mode PALETTE, which reads no colour.
 * palette: float64 [GCD_PARDOM_PALETTE_ROWS, 3], contiguous, 8-byte aligned; rows 0 .. n_classes - 1 are the classes,
 *   1 <= n_classes <= GCD_PARDOM_PALETTE_ROWS.  alpha: in [0, 1] in mode BLEND, not read otherwise.
 * out: float64, channel c of point i at out[i * out_ld + c], 3 <= out_ld, 8-byte aligned; nothing between the rows is
 *   written.  0 <= N < 2^31; strides at most GCD_PARDOM_MAX_LD.  With N == 0 ids, rgb and out are not looked at.
 * Per point and channel, every operation rounded once on its own (no multiply-add is fused):
 *   c32 = (float)rgb / 255.0f                                                       (fp32; the splat's uint8 load)
 *   P   = id < n_classes ? palette[id] : 0                                          (fp64)
 *   RGB:     out = (double)c32
 *   PALETTE: out = P
 *   BLEND:   out = (double)(c32 * (float)(1.0 - alpha)) + alpha * P                 (fp32 product; fp64 product and sum)
 * status: int64 [1], 8-byte aligned: the number of points whose id is >= n_classes (0 in mode RGB), stored by every
 * call.  Such a point takes the class colour 0. */
int gcd_pardom_colours(const uint8_t* ids, int64_t ids_ld, const uint8_t* rgb, int64_t rgb_ld, int64_t N,
                       const double* palette, int n_classes, double alpha, int mode, double* out, int64_t out_ld,
                       int64_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
