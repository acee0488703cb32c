/* gcd_amd_clip.h — gcd_amd/libgcd_amd_clip.so (gcd_amd/csrc/clip_vision.hip): the kernels of the CLIP ViT image tower
 * (gcd_amd/clip_vision.py) that libgcd_amd.so does not already have: the kornia-style preprocessing into conv1's patch
 * matrix, the token assembly with ln_pre, self-attention at head dim 80 and the bias + erf-GELU between c_fc and c_proj.
 * The GEMMs and the other LayerNorms of the tower are gcd_gemm_f16 / gcd_layernorm_f16 of libgcd_amd.so.
 *
 * A library of its own (gcd_amd/csrc/build.py LIBRARIES, gcd_amd/_lib_clip.py): include/gcd_amd.h and its ABI
 * version do not change.  Same rules as gcd_amd.h: raw device pointers, the caller's hipStream_t, no allocation, no
 * synchronisation, no atomics; every argument is checked before anything is launched, and a non-zero status comes with
 * a message in gcd_clip_last_error().  Every payload element of every output is stored by every call. */
#ifndef GCD_AMD_CLIP_H
#define GCD_AMD_CLIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCD_AMD_CLIP_ABI_VERSION 1
/* gcd_clip_attn_f16 keeps K and V of one (image, head) in LDS: 288 keys x 80 x 2 x fp16 (with padding 98 KB of 160) */
#define GCD_CLIP_ATTN_MAX_S 288
#define GCD_CLIP_HEAD_DIM 80
/* gcd_clip_preprocess: longest Gaussian (antialias) kernel per axis, and the widest input row (kept in LDS as fp32) */
#define GCD_CLIP_MAX_BLUR 63
#define GCD_CLIP_MAX_WIDTH 8192
/* gcd_clip_tokens_ln_pre: widest model (one row lives in LDS as fp32) */
#define GCD_CLIP_MAX_MODEL_WIDTH 4096

int gcd_clip_abi_version(void);
const char* gcd_clip_last_error(void);

/* x: fp32 [n, 3, H, W] in [-1, 1] with element strides (sn, sc, sh, sw).  Computes, as kornia 0.7.0's
 * geometry.resize(x, (S, S), "bicubic", align_corners=True, antialias) followed by (x + 1) / 2 and (x - mean) / std:
 *   antialias (only if `antialias` and max(H / S, W / S) > 1), per axis with factor f = extent / S:
 *     sigma = max((f - 1) / 2, 0.001), k = int(max(4 sigma, 3)) made odd by adding 1, taps exp(-t^2 / (2 sigma^2)) at
 *     integer t in [-k/2, k/2], normalised; reflect padding; separable;
 *   bicubic with A = -0.75, align_corners = True and clamped tap indices (torch's upsample_bicubic2d).
 * The source coordinates, the tap weights and the final normalisation are evaluated in fp64, the tap sums in fp32.
 * patches16: fp16 [n * G * G, Kp], G = S / P, row (image, gy, gx), column (c, py, px) = conv1's weight order;
 *   columns 3 P P .. Kp - 1 are stored as zeros.  Kp % 32 == 0, Kp >= 3 P P, 16-byte aligned base.
 * img32: optional fp32 [n, 3, S, S] (contiguous), the same values before the rounding to fp16; null to skip.
 * mean, stdev: fp32 [3] on the device.  S % P == 0; H, W > k / 2 of their axis (reflect padding); k <= GCD_CLIP_MAX_BLUR;
 * W <= GCD_CLIP_MAX_WIDTH. */
int gcd_clip_preprocess(const float* x, int64_t sn, int64_t sc, int64_t sh, int64_t sw, int n, int H, int W, int S, int P,
                        int antialias, const float* mean, const float* stdev, void* patches16, int Kp, float* img32,
                        void* stream);

/* tok [n * (G2 + 1), C] fp32 (row stride ldo) = ln_pre(z), z[i, 0] = cls + pos[0], z[i, 1 + p] = patch[i * G2 + p] + pos[1 + p];
 * patch: fp32 [n * G2, C] (row stride ldp), cls [C], pos [G2 + 1, C] (contiguous), gamma / beta [C].
 * Two-pass mean / variance in fp32.  C <= GCD_CLIP_MAX_MODEL_WIDTH. */
int gcd_clip_tokens_ln_pre(const float* patch, int64_t ldp, const float* cls, const float* pos, const float* gamma,
                           const float* beta, float eps, float* tok, int64_t ldo, int n, int G2, int C, void* stream);

/* Non-causal self-attention, head dim 80, v_mfma_f32_16x16x32_f16.  qkv: fp16 [n * S, 3 * heads * 80] (row stride ld,
 * ld % 8 == 0, 16-byte aligned), columns q | k | v, each head-major (gcd_attn_spatial_f16's layout).  out: fp16
 * [n * S, heads * 80] (row stride ldo).  softmax(q k^T / sqrt(80)) v with fp32 scores and softmax, fp16 probabilities,
 * fp32 accumulation.  q_prescaled = 1: q already carries log2(e) / sqrt(80) (folded into W_q).  Keys past S are
 * masked, not zero-scored.  1 <= S <= GCD_CLIP_ATTN_MAX_S.  A query's result does not depend on n. */
int gcd_clip_attn_f16(const void* qkv, int64_t ld, void* out, int64_t ldo, int n, int S, int heads, int q_prescaled,
                      void* stream);

/* out16 [M, N] fp16 (row stride ldo) = gelu(h [M, N] fp32 (row stride ldh) + bias [N]), gelu(x) = x (1 + erf(x / sqrt 2)) / 2.
 * N % 4 == 0, ldh % 4 == 0, ldo % 4 == 0, h 16-byte and out16 8-byte aligned. */
int gcd_clip_bias_gelu_f16(const float* h, int64_t ldh, const float* bias, void* out16, int64_t ldo, int64_t M, int N,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif
