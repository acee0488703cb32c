/* gcd_amd_lpips.h — gcd_amd/libgcd_amd_lpips.so (gcd_amd/csrc/lpips.hip): the kernels of the LPIPS perceptual metric
 * (gcd_amd/lpips.py) that libgcd_amd.so does not already have: the ScalingLayer fused into the token-major fp16 packing
 * of the images, ReLU with the 2x2 max-pool of VGG-16, and the normalised squared feature distance of one tap with its
 * 1x1 `lin` weights.  The 13 convolutions of the tower are gcd_gemm_f16 (GCD_GEMM_CONV3X3, fp16 output, bias).
 *
 * A library of its own (gcd_amd/csrc/build.py LIBRARIES, gcd_amd/_lib_lpips.py): include/gcd_amd.h and its ABI version
 * do not change.  Same rules as gcd_amd.h: raw device pointers, the caller's hipStream_t, no allocation, no
 * synchronisation, no atomics; every argument is checked before anything is launched, and a non-zero status comes with
 * a message in gcd_lpips_last_error().  Every payload element of every (non-null) output is stored by every call. */
#ifndef GCD_AMD_LPIPS_H
#define GCD_AMD_LPIPS_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCD_AMD_LPIPS_ABI_VERSION 1
/* widest feature row of gcd_lpips_distance: one wave holds a pixel's row as 8 halves per lane (64 x 8) */
#define GCD_LPIPS_MAX_C 512
/* channels must be a multiple of this (gcd_gemm_f16's K granule; 4 lanes of 8 halves) */
#define GCD_LPIPS_C_MULTIPLE 32
/* most partial sums per image of gcd_lpips_distance (= workgroups per image) */
#define GCD_LPIPS_MAX_BLOCKS 1024
/* most taps whose means one gcd_lpips_distance call adds up */
#define GCD_LPIPS_MAX_TAPS 16
/* most images per call (the y extent of a launch grid) */
#define GCD_LPIPS_MAX_IMAGES 65535
/* image channels gcd_lpips_pack_f16 reads */
#define GCD_LPIPS_IMAGE_CHANNELS 3

int gcd_lpips_abi_version(void);
const char* gcd_lpips_last_error(void);

/* x: fp32 [n, 3, H, W], contiguous.  out16: fp16 [n * H * W, cpad] token-major (row = (image, y, x)), contiguous,
 * 16-byte aligned; cpad % 8 == 0, 8 <= cpad <= GCD_LPIPS_MAX_C.
 *   out16[., c] = fp16(((x * a + b) - shift[c]) / scale[c]) for c < 3, every operation rounded to fp32 on its own, in
 *   that order (no fused multiply-add, IEEE division), one rounding to fp16; columns 3 .. cpad - 1 are stored as zeros.
 * (a, b) = (1, 0) takes images in [-1, 1], (2, -1) frames in [0, 1].  shift, scale: fp32 [3] on the device. */
int gcd_lpips_pack_f16(const float* x, int n, int H, int W, float a, float b, const float* shift, const float* scale,
                       void* out16, int cpad, void* stream);

/* src: fp16 [n, H, W, C] (contiguous, 16-byte aligned, C % 8 == 0): one convolution's output.
 * full: fp16 [n, H, W, C] = max(src, 0), or null; full may be src itself (in place).
 * pooled: fp16 [n, H / 2, W / 2, C] = the 2 x 2, stride 2 max-pool (floor mode: the last row / column of an odd H / W is
 *   dropped) of max(src, 0), or null; needs H, W >= 2.  At least one destination is non-null.
 * NaN propagates through both; -0 becomes +0.  Indices are 64-bit. */
int gcd_lpips_relu_pool_f16(const void* src, void* full, void* pooled, int n, int H, int W, int C, void* stream);

/* One tap of the head.  f0, f1: fp16 [n, HW, C] (contiguous, 16-byte aligned), C % GCD_LPIPS_C_MULTIPLE == 0,
 * C <= GCD_LPIPS_MAX_C; w: fp32 [C].  Per pixel p of image i, in fp32, with both rows in registers:
 *   r0 = 1 / (sqrt(sum_c f0^2) + 1e-10), r1 likewise;  d[i, p] = sum_c (f0 r0 - f1 r1)^2 w[c]
 * (the difference is formed directly, each product rounded on its own: identical rows give exactly 0, and an all-zero
 * row contributes exactly 0).
 * First launch: partials fp32 [n, blocks], partials[i, b] = the sum of d[i, p] over the pixels of workgroup b (pixel
 *   groups b, b + blocks, ... in that order; a workgroup without pixels stores 0).  1 <= blocks <= GCD_LPIPS_MAX_BLOCKS.
 * Second launch: tap_means fp64 [taps, n]: tap_means[tap, i] = (sum_b partials[i, b], in fp64, b ascending) / HW;
 *   if out is non-null: out[i] = fp32(sum_t tap_means[t, i], in fp64, t ascending) — rows t != tap are read as earlier
 *   calls on the same stream left them.  0 <= tap < taps <= GCD_LPIPS_MAX_TAPS.
 * No atomics, fixed slots, fixed order: the result is bit-identical from call to call.  n <= GCD_LPIPS_MAX_IMAGES. */
int gcd_lpips_distance(const void* f0, const void* f1, const float* w, int n, int64_t HW, int C, float* partials,
                       int blocks, double* tap_means, int tap, int taps, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
