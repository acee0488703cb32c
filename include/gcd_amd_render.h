/* gcd_amd_render.h — gcd_amd/libgcd_amd_render.so (gcd_amd/csrc/render.hip): the (source, target) views that GCD's data
 * modules re-render from cached point clouds for every example, on the device.  Two stages:
 *
 *   gcd_render_splat            `project_points_to_pixels`: every point is projected into nc >= 1 cameras in one pass over
 *                               the cloud and splatted with the weight exp(-depth_norm * strength) into its pixel and, at
 *                               0.02 of that, into the (radius // 2, (radius + 1) // 2) neighbourhood
 *   gcd_render_fill_resize_f32  `blur_into_black`, the bilinear resize to the model's resolution and the affine map to
 *                               [-1, 1], stored planar into a slot of a (T, 3, Hp, Wp) batch tensor
 *
 * A library of its own, beside libgcd_amd.so, libgcd_amd_train.so, libgcd_amd_sampler.so and libgcd_amd_metrics.so:
 * include/gcd_amd.h and its ABI version do not change, and the sources are not part of the digest that stamps the traffic
 * profile of the sampler step.  Same rules as gcd_amd.h: raw device pointers, the caller's hipStream_t, no allocation, no
 * synchronisation, no decision on the host between the launches of a call; a non-zero status comes with a message in
 * gcd_render_last_error() and nothing has been launched.
 *
 * Arithmetic of the splat.  The weights span e^-512 .. e^+512, so neither a float sum (order-dependent) nor one
 * fixed-point scale (blind below the scale) will do.  Every pixel keeps four reference exponents: the largest exponent l
 * of any contribution (for the denominator) and, per colour channel, the largest l + ln c among the contributions whose
 * colour c in that channel is non-zero; ln 0.02 of a neighbour is part of l.  They are found with an integer maximum on an
 * order-preserving key of the double.  A second pass adds floor(exp(l - lmax) * 2^F), and per channel
 * floor(exp(l + ln c - max_c) * 2^F), with 64-bit integer adds, F = min(52, 63 - bit_length(N)): at most N contributions
 * of at most 2^F reach one pixel, so a sum cannot overflow, the largest term of every sum is exactly 2^F, and the
 * truncation is at most n_pixel * 2^-F relative for any colours.  The resolve computes S_c / S_d * exp(max_c - lmax_d) in
 * fp64 and rounds once to fp32.  Integer maxima and integer sums do not depend on the order of arrival: two calls on the
 * same operands are bit-identical.  Every element of every output is stored by every call; `scratch` is written before
 * it is read. */
#ifndef GCD_AMD_RENDER_H
#define GCD_AMD_RENDER_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCD_AMD_RENDER_ABI_VERSION 1
/* element types of the cloud: xyz takes F16 / F32 / F64, rgb takes those and U8 (divided by 255.0f in fp32 on load) */
#define GCD_RENDER_F16 0
#define GCD_RENDER_F32 1
#define GCD_RENDER_F64 2
#define GCD_RENDER_U8 3
#define GCD_RENDER_MAX_CAMERAS 8
/* doubles per camera in `cams`: K (3 x 3, row-major) followed by RT (4 x 4, row-major, camera-to-world) */
#define GCD_RENDER_CAM_DOUBLES 25
/* largest Gaussian of the fill stage (odd sizes 1 .. 31) */
#define GCD_RENDER_MAX_KERNEL 31

typedef struct gcd_render_splat_desc {
  const void* xyz;             /* N points, 3 values each, `xyz_ld` elements from one point to the next (>= 3) */
  const void* rgb;             /* N colours (U8: 0 .. 255 for 0 .. 1), 3 values each, `rgb_ld` elements apart (>= 3); a float
                                  colour that is negative, NaN or infinite counts as 0 (sums are unsigned) */
  int64_t xyz_ld, rgb_ld;
  int64_t N;                   /* 0 <= N < 2^31 */
  int32_t xyz_dtype, rgb_dtype;
  const double* cams;          /* device, [nc][GCD_RENDER_CAM_DOUBLES] */
  int32_t nc, H, W, spread_radius;   /* 1 <= nc <= GCD_RENDER_MAX_CAMERAS; 0 <= spread_radius <= 8 */
  float* img;                  /* [nc][H][W * 3] fp32, row stride img_ld, camera stride img_cs (elements) */
  int64_t img_cs, img_ld;
  double* weights;             /* [nc][H][W] fp64, -1 where nothing landed; row stride weights_ld, camera stride weights_cs */
  int64_t weights_cs, weights_ld;
  double* uv;                  /* [nc][N][2] fp64 contiguous, or null: not computed */
  double* depth;               /* [nc][N] fp64 contiguous, or null: not computed */
  int64_t* status;             /* [nc]: the number of points that passed the mask.  0: the reference's .max() would have
                                  raised; here that camera's image is zero and its weights are -1 */
  void* scratch;               /* gcd_render_scratch_bytes(nc, H, W) bytes, 8-byte aligned */
  int64_t scratch_bytes;
} gcd_render_splat_desc;

int gcd_render_abi_version(void);
const char* gcd_render_last_error(void);

/* Bytes of scratch of gcd_render_splat: per camera a 16-byte header and 64 bytes per pixel (four keys, four sums).
 * 0 with a message for sizes the entry refuses. */
int64_t gcd_render_scratch_bytes(int nc, int H, int W);
/* Bytes of scratch of gcd_render_fill_resize_f32: the filled image as three fp64 planes, 3 * H * W * 8. */
int64_t gcd_render_fill_scratch_bytes(int H, int W);

/* xyz_cam = (xyz - t) R and uv = K xyz_cam / z in fp64; uv_int = trunc(uv + 0.5), tested in floating point before the
 * conversion (a value past int32, or a NaN, is outside); mask 0 <= u < W, 0 <= v < H, depth > 0.1.  If the largest masked
 * depth is >= 64: depth := min(sqrt(depth), 32), strength 256, else strength 512; depth_norm = depth / max * 2 - 1 with the
 * maximum taken after that branch; w = exp(-depth_norm * strength).  img = clamp(num / den, 0, 1) rounded once to fp32. */
int gcd_render_splat(const gcd_render_splat_desc* d, void* stream);

/* img [H][W * 3] fp32 (row stride img_ld) -> out[c * out_cs + y * out_rs + x * out_xs] fp32, c < 3, y < Hp, x < Wp.
 * black = ((r + g) + b == 0) in fp32.  The k x k Gaussian (linspace(-(k-1)/2, (k-1)/2, k), exp(-0.5 (x / sigma)^2),
 * normalised, separable, reflect padding) blurs the image and the validity mask; holes take blur_img / max(blur_mask,
 * 1e-7), every other pixel keeps its value.  A 3 x 3 Gaussian with sigma 0.6 follows, then the bilinear resize to (Hp, Wp)
 * (align_corners = false, no antialias; Hp = H, Wp = W is the identity), then value * scale + offset.  All in fp64 from
 * the fp32 image, rounded once.  k odd, 1 <= k <= GCD_RENDER_MAX_KERNEL, sigma > 0; H, W > max(k / 2, 1): reflect padding's
 * own limit. */
int gcd_render_fill_resize_f32(const float* img, int64_t img_ld, int H, int W, int k, double sigma, float* out, int64_t out_cs,
                               int64_t out_rs, int64_t out_xs, int Hp, int Wp, double scale, double offset, void* scratch,
                               int64_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
