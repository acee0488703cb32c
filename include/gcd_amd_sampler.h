/* gcd_amd_sampler.h — gcd_amd/libgcd_amd_sampler.so (gcd_amd/csrc/sampler_stage.hip): the elementwise update of one
 * sampler STAGE.  A stage is one network evaluation followed by one update of the state; Euler, Euler ancestral and
 * DPM++ 2M take one stage per step, Heun and DPM++ 2S ancestral two (gcd_amd/sampler_stages.py builds the rows).
 *
 * A library of its own, beside libgcd_amd.so and libgcd_amd_train.so: include/gcd_amd.h and its ABI version do not
 * change, and the sources are not part of the digest that stamps the traffic profile of the Euler step.
 * Same rules as gcd_amd.h: raw device pointers, the caller's hipStream_t, no allocation, no synchronisation; a non-zero
 * status comes with a message in gcd_sampler_last_error(). */
#ifndef GCD_AMD_SAMPLER_H
#define GCD_AMD_SAMPLER_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCD_AMD_SAMPLER_ABI_VERSION 1
/* floats per row of the coefficient table */
#define GCD_SAMPLER_ROW 12

int gcd_sampler_abi_version(void);
const char* gcd_sampler_last_error(void);

/* cur [nx, chw] fp32: the state the network was evaluated on, updated IN PLACE (the only aliasing allowed).
 * net [2 nx, chw] fp32: the network's outputs in [uc | c] order.  scale [T]: guidance scale of frame n % T.
 * coef: GCD_SAMPLER_ROW floats in DEVICE memory,
 *     {sigma, a_cur, a_den, a_h0, a_h1, a_noise, s0_cur, s0_den, s1_cur, s1_den, 0, 0}.
 * Per element, with D_. = net_. * (-sigma / sqrt(sigma^2 + 1)) + cur / (sigma^2 + 1) and D = D_u + scale (D_c - D_u):
 *     new = a_cur cur + a_den D + a_h0 h0 + a_h1 h1 + a_noise noise
 *     h0  = s0_cur cur + s0_den D        only if (s0_cur, s0_den) != (0, 0)
 *     h1  = s1_cur cur + s1_den D        only if (s1_cur, s1_den) != (0, 0)
 *     cur = new
 * h0 and h1 are read (old value, for `new`) before they are written.  A term whose coefficient is exactly 0.0f is not
 * LOADED (its buffer may hold anything, NaN included, or not exist yet) and a store whose pair is (0, 0) is not made, so
 * one launch with fixed pointers serves every row.  h0, h1 and noise may be null when no row the caller uses gives them a
 * non-zero coefficient; the kernel never dereferences a null pointer (such a term is dropped).
 * 16-byte accesses when chw % 4 == 0 and every non-null base is 16-byte aligned, a scalar path otherwise. */
int gcd_sampler_stage_f32(float* cur, const float* net, const float* scale, const float* coef, float* h0, float* h1,
                          const float* noise, int nx, int T, int64_t chw, void* stream);

#ifdef __cplusplus
}
#endif
#endif
