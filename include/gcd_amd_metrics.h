/* gcd_amd_metrics.h — gcd_amd/libgcd_amd_metrics.so (gcd_amd/csrc/metrics.hip): the evaluation metrics of GCD's test
 * script (per-frame PSNR / SSIM with their visible / occluded variants, and the sample diversity) computed on the device
 * from the decoded frames, so that a few hundred doubles leave the GPU instead of the frames.  The host version,
 * gcd_amd/metrics.py, stays the oracle of this one.
 *
 * A library of its own, beside libgcd_amd.so, libgcd_amd_train.so and libgcd_amd_sampler.so: include/gcd_amd.h and its
 * ABI version do not change, and the sources are not part of the digest that stamps the traffic profile of the sampler
 * step.  Same rules as gcd_amd.h: raw device pointers, the caller's hipStream_t, no allocation, no synchronisation; a
 * non-zero status comes with a message in gcd_metrics_last_error() and nothing has been launched.
 *
 * Arithmetic: inputs are fp32; every product, window sum, map value and fold is fp64, so a result is the float64
 * evaluation of the fp32 inputs.  No atomics: partial sums go to `scratch` per tile and are folded in a fixed order, two
 * calls on the same inputs give bit-identical results.  Every element of `out` (and `uncertainty`) is stored by every
 * call; `scratch` is written before it is read. */
#ifndef GCD_AMD_METRICS_H
#define GCD_AMD_METRICS_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCD_AMD_METRICS_ABI_VERSION 1
/* flags bit 0: `pred` holds the decoder's raw output in [-1, 1]; clamp((x + 1) * 0.5, 0, 1) is applied in fp32 on load */
#define GCD_METRICS_SIGNED 1
/* doubles per (sample, frame) of gcd_metrics_frames_f32: psnr, ssim, psnr_vis, ssim_vis, psnr_occ, ssim_occ */
#define GCD_METRICS_FRAME_VALUES 6
/* doubles per frame of gcd_metrics_diversity_f32: mean over all, visible, occluded pixels */
#define GCD_METRICS_DIVERSITY_VALUES 3

int gcd_metrics_abi_version(void);
const char* gcd_metrics_last_error(void);

/* Bytes of scratch the two entries below need (0 with a message for sizes they refuse). */
int64_t gcd_metrics_frames_scratch_bytes(int S, int T, int H, int W);
int64_t gcd_metrics_diversity_scratch_bytes(int S, int T, int H, int W);

/* pred [S, T, 3, H, W], gt [T, 3, H, W], reproject [T, 3, H, W] or null: contiguous fp32 images in [0, 1] (pred in
 * [-1, 1] with GCD_METRICS_SIGNED).  out [S, T, 6] fp64.  H, W >= 7; S, T >= 1.
 * Masks: occluded = ((|r0| + |r1|) + |r2|) <= 1e-7f in fp32, visible = its complement.
 *   psnr      10 log10(1 / mean squared error) over the frame's 3 H W values; zero error gives +inf
 *   ssim      7x7 uniform window, K1 = 0.01, K2 = 0.03, data range 1, sample covariance (49 / 48); the map is averaged
 *             over the image cropped by 3 on each side, then over channels
 *   psnr_vis / psnr_occ   the same PSNR over the mask's pixels in all three channels; an empty mask gives NaN
 *   ssim_vis / ssim_occ   the same map averaged over the mask eroded three times by the 3x3 cross (every pixel within
 *             L1 distance 3 is in the mask), cropped by 3; an empty mask or an empty eroded mask gives NaN
 * Without `reproject` there are no masks: the four masked values are stored as 0.0 and mean nothing. */
int gcd_metrics_frames_f32(const float* pred, const float* gt, const float* reproject, int S, int T, int H, int W, int flags,
                           void* scratch, int64_t scratch_bytes, double* out, void* stream);

/* uncertainty [T, H, W] fp32: per pixel the population standard deviation of `pred` over the S samples, per channel,
 * averaged over the channels; computed in fp64 and rounded once.  out [T, 3] fp64: the mean of that (unrounded) map over
 * all pixels, over the visible and over the occluded pixels (masks as above, not eroded); an empty mask gives NaN,
 * and without `reproject` the two masked values are stored as 0.0.  Sizes as above (one rule for both entries). */
int gcd_metrics_diversity_f32(const float* pred, const float* reproject, int S, int T, int H, int W, int flags,
                              float* uncertainty, void* scratch, int64_t scratch_bytes, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
