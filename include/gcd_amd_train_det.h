/* gcd_amd_train_det.h — the deterministic reductions of gcd_amd/libgcd_amd_train.so (gcd_amd/csrc/train_det.hip).
 * Five entries of the fine-tune step sum with fp32 read-modify-write adds whose order changes from run to run
 * (gcd_rowblock_sum_f32, gcd_layernorm_bwd, gcd_cast_colsum_f32 of gcd_amd.h; gcd_blend_bwd_f32 and gcd_smallm_dgrad of
 * gcd_amd_train.h).  Each has a counterpart here with the same operands and the same destination semantics — the
 * destination holds zeros or the value to add onto, and the entry ADDS its sum — that is a function of (inputs, shapes,
 * dtype) only:
 *   pass 1  every workgroup WRITES its partial sums to its own slot of the caller's `scratch` (nothing to zero first);
 *   pass 2  an ordered fold: one thread owns one destination element, walks that element's slots in index order,
 *           accumulates in fp64, rounds once and does dst += sum.
 * The launch geometry, and with it the order of every sum, is derived from the shapes alone.  Two launches that add
 * into the same destination must be ordered by the caller (both training engines issue everything on one stream): the
 * owning thread's read-modify-write is a plain load and store.
 * `scratch`: >= the entry's *_scratch_floats(...) floats, 16-byte aligned; a smaller one is refused (status 2 and a message
 * in gcd_train_last_error).  Same rules as gcd_amd_train.h otherwise: raw device pointers, leading dimensions in elements,
 * the caller's hipStream_t, no allocation, no synchronisation. */
#ifndef GCD_AMD_TRAIN_DET_H
#define GCD_AMD_TRAIN_DET_H
#include <stdint.h>

#include "gcd_amd_train.h"
#ifdef __cplusplus
extern "C" {
#endif

/* out[b][n] += sum over rows b * rows_per_block .. of x[row][n]  (gcd_rowblock_sum_f32).  N, ldx multiples of 4.
 * Slots per destination element: clamp(rows_per_block / 256, 1, 64). */
int64_t gcd_rowblock_sum_det_scratch_floats(int64_t M, int N, int64_t rows_per_block);
int gcd_rowblock_sum_det_f32(const float* x, int64_t ldx, int64_t M, int N, int64_t rows_per_block, float* out,
                             float* scratch, int64_t scratch_floats, void* stream);

/* LayerNorm backward (gcd_layernorm_bwd): dx as there, bit for bit, from the same single read of x and dy;
 * dgamma[c] += sum dy xhat, dbeta[c] += sum dy.  Slots per column: min(ceil(M / 4), 768) workgroups. */
int64_t gcd_layernorm_bwd_det_scratch_floats(int64_t M, int C);
int gcd_layernorm_bwd_det(const float* x, int64_t ldx, const float* dy, int64_t lddy, int64_t M, int C, const float* gamma,
                          float eps, float* dx, int64_t lddx, float* dgamma, float* dbeta, const float* dx_add,
                          int64_t ld_add, float* scratch, int64_t scratch_floats, void* stream);

/* fp32 -> fp16 / bf16 copy of x and, from the same read, sums[b][c] += column sums of row block b; total[c] (optional)
 * += the sum over all row blocks, folded from the blocks in block order (gcd_cast_colsum_f32).  C multiple of 8. */
int64_t gcd_cast_colsum_det_scratch_floats(int64_t M, int C, int64_t rows_per_block);
int gcd_cast_colsum_det_f32(const float* x, int64_t ldx, void* y16, int64_t ldy, int64_t M, int C, int64_t rows_per_block,
                            float* sums, int to_bf16, float* total, float* scratch, int64_t scratch_floats, void* stream);

/* AlphaBlender backward (gcd_blend_bwd_f32): d_xs, d_xt as there; d_alpha[frame] += sum dy (xs - xt) (d_alpha optional). */
int64_t gcd_blend_bwd_det_scratch_floats(int64_t M, int C, int64_t rows_per_frame);
int gcd_blend_bwd_det_f32(const float* dy, int64_t ld_dy, const float* xs, int64_t ld_s, const float* xt, int64_t ld_t,
                          const float* alpha, int64_t M, int C, int64_t rows_per_frame, float* d_xs, int64_t ld_dxs,
                          int accumulate_xs, float* d_xt, int64_t ld_dxt, float* d_alpha, float* scratch,
                          int64_t scratch_floats, void* stream);

/* Grouped few-row dgrad (gcd_smallm_dgrad with flag 4): dx[m][k] += dact(x[m][k]) sum_n y[m][n] W[n][k], where several
 * problems of the table may share one dx.  Blocks of a problem HERE: ceil(K / 256) — a workgroup walks every n of its
 * (problem, k chunk) and writes a [32][256] tile of partial dx to slot block0 + chunk; `reserved` holds the table index of
 * the FIRST problem with the same dx (its own index when it shares with none before it; members of one group have equal
 * M, K and lddx).  The fold adds, per element of a group's dx, the group's tiles in table order.  flags: 1 = multiply by
 * silu'(x). */
int64_t gcd_smallm_dgrad_det_scratch_floats(int total_blocks);
int gcd_smallm_dgrad_det(const gcd_smallm_problem* table_dev, int n_prob, int total_blocks, float* scratch,
                         int64_t scratch_floats, void* stream);

#ifdef __cplusplus
}
#endif
#endif
