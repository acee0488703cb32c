/* gcd_amd_lora.h — gcd_amd/libgcd_amd_lora.so (gcd_amd/csrc/lora.hip): LoRA fine-tuning by merged weights
 * (gcd_amd/lora.py; ft_strategy `time_lora`).  An adapted Linear keeps its fp32 weight tensor, which holds the merged
 * W = W0 + scale * B A; the engines compute the ordinary weight gradient dW, and the adapter gradients are its projections
 *   dB = scale * dW A^T        dA = scale * B^T dW
 * with A [r, K], B [N, r], W0 / W / dW [N, K], all fp32, row-major and contiguous.
 *
 * A library of its own (gcd_amd/csrc/build.py LIBRARIES, gcd_amd/_lib_lora.py): include/gcd_amd.h and its ABI version do
 * not change.  Same rules as gcd_amd.h: raw device pointers, the caller's hipStream_t, no allocation, no synchronisation;
 * every host argument is checked before anything is launched, and a non-zero status comes with a message in
 * gcd_lora_last_error().  Both entry points are GROUPED: one call covers every adapted layer through a table of
 * gcd_lora_entry in DEVICE memory.  A kernel never indexes past the N, K, r of the entry it reads; an entry whose fields
 * are out of range, whose tile start does not match, or whose partials would not fit the scratch is skipped.  There is no
 * floating-point atomic: every sum has a fixed order, so a result is bit-identical from call to call. */
#ifndef GCD_AMD_LORA_H
#define GCD_AMD_LORA_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCD_AMD_LORA_ABI_VERSION 1
/* largest rank r */
#define GCD_LORA_MAX_RANK 64
/* most entries of one table */
#define GCD_LORA_MAX_ENTRIES 65535
/* largest N and K */
#define GCD_LORA_MAX_DIM 1048576
/* gcd_lora_merge: one workgroup per MERGE_TILE x MERGE_TILE tile of W */
#define GCD_LORA_MERGE_TILE 64
/* gcd_lora_project: one workgroup per PROJECT_TILE x PROJECT_TILE region of dW */
#define GCD_LORA_PROJECT_TILE 256

/* One adapted layer.  merge_tile0 / project_tile0: the running sum, over the entries before this one, of
 * ceil(N / TILE) * ceil(K / TILE) with TILE = GCD_LORA_MERGE_TILE / GCD_LORA_PROJECT_TILE (the first workgroup of this
 * entry in the grouped launch; entries are in ascending order of both).  scratch0: the running sum of
 * gcd_lora_project_scratch_floats(N, K, r), the float offset of this entry's partial sums in `scratch`.
 * gcd_lora_merge reads W0, A, B and writes W; gcd_lora_project reads A, B, dW and writes dA, dB.  dW may be null: the
 * weight's gradient counts as zero (a layer that the backward pass never reached). */
typedef struct {
  const float* W0; /* [N, K] the frozen weight */
  float* W;        /* [N, K] the live (merged) weight */
  const float* A;  /* [r, K] */
  const float* B;  /* [N, r] */
  const float* dW; /* [N, K] or null */
  float* dA;       /* [r, K] */
  float* dB;       /* [N, r] */
  int64_t scratch0;
  int32_t N, K, r;
  float scale;
  int32_t merge_tile0, project_tile0;
} gcd_lora_entry;

int gcd_lora_abi_version(void);
const char* gcd_lora_last_error(void);

/* W[n, k] = W0[n, k] + scale * sum_j B[n, j] A[j, k] for every entry: the sum over j ascending as an fp32 fma chain from
 * zero, then one fma with W0.  A sum that is exactly zero (B == 0) stores W0's own bits.  table: n entries in device
 * memory, 1 <= n <= GCD_LORA_MAX_ENTRIES; tiles: the total of the entries' merge tiles. */
int gcd_lora_merge(const gcd_lora_entry* table, int n, int tiles, void* stream);

/* Floats of scratch one entry needs: ceil(K / PT) * N * r + ceil(N / PT) * r * K with PT = GCD_LORA_PROJECT_TILE, rounded
 * up to a multiple of 4; -1 (and a message) for N, K outside 1 .. GCD_LORA_MAX_DIM or r outside 1 .. GCD_LORA_MAX_RANK. */
int64_t gcd_lora_project_scratch_floats(int N, int K, int r);

/* dB = scale * dW A^T and dA = scale * B^T dW for every entry, zeros where dW is null.  Stage 1: one workgroup per
 * PT x PT region of dW (each element of dW is read once) leaves that region's partial sums in `scratch`; stage 2 adds
 * the partials of a (row | column) in ascending region order and scales.  tiles: the total of the entries' project
 * tiles; max_rank: the largest r of the table (it picks the kernel: up to 16, or up to GCD_LORA_MAX_RANK; an entry with a
 * larger r is skipped by BOTH stages: nothing of it is read, no partial sum is written, its dA and dB keep what they held); scratch: fp32 [scratch_floats] in device memory, at least the sum of the entries' needs. */
int gcd_lora_project(const gcd_lora_entry* table, int n, int tiles, int max_rank, float* scratch, int64_t scratch_floats,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif
