// train_det.hip — the deterministic reductions of libgcd_amd_train.so.  C ABI: include/gcd_amd_train_det.h.
//
// Five sums of the fine-tune step's backward pass (row-block column sums, LayerNorm's affine gradients, the cast + column
// sums of dY, the AlphaBlender's d_alpha, the few-row dgrads that share one dx) in a two-pass form whose result is a
// function of (inputs, shapes, dtype):
//   pass 1  every workgroup WRITES its partial sums to its own slot of the caller's scratch — plain vector stores, nothing
//           to zero first.  For LayerNorm backward and the cast this is the one streaming pass over the big operand that
//           also produces dx / the 16-bit copy;
//   pass 2  an ordered fold: one thread owns one destination element, walks that element's slots in index order in fp64,
//           rounds once and does dst += sum with a plain load and store.  Safe because both training engines issue every
//           launch on one stream: two launches that add into the same destination are ordered.
// The grids are derived from the shapes only (never from the CU count, the environment or a tuning knob), so the order of
// every sum is fixed.  All HBM-bound: 16-byte loads, several rows in flight per thread, 64-bit row offsets.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gcd_amd_train_det.h"
#include "train_common.h"

typedef _Float16 f16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef unsigned short us8 __attribute__((ext_vector_type(8)));

#define CHECK_SCRATCH(what, need)                                                                                   \
  CHECK_ARG(scratch && scratch_floats >= (need) && ((uintptr_t)scratch & 15) == 0,                                  \
            "%s: scratch of %lld floats, need %lld (%s_scratch_floats), 16-byte aligned", what, (long long)scratch_floats, \
            (long long)(need), what)

namespace {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ unsigned short bf16_rne(float f) {
  unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}

// the ordered fold of one destination element: slots src[0], src[stride], ... in index order, fp64.  The loads of a group
// of 16 (then 4) slots are independent and in flight together; the additions run in slot order (a fold over a few
// hundred slots is a chain of memory latencies, not of arithmetic)
__device__ __forceinline__ double fold_slots(const float* __restrict__ src, int nslots, int64_t stride) {
  double s = 0.0;
  int k = 0;
  for (; k + 15 < nslots; k += 16) {
    float v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = src[(int64_t)(k + u) * stride];
#pragma unroll
    for (int u = 0; u < 16; ++u) s += (double)v[u];
  }
  for (; k + 3 < nslots; k += 4) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = src[(int64_t)(k + u) * stride];
#pragma unroll
    for (int u = 0; u < 4; ++u) s += (double)v[u];
  }
  for (; k < nslots; ++k) s += (double)src[(int64_t)k * stride];
  return s;
}

// ---------------------------------------------------------------------------------------------------------------------
// 1. row-block column sums.  Pass 1: grid (ceil(N / 256), nblk, nsplit), block 256 = 64 lanes x 4 columns, 4 row lanes;
//    a thread keeps four rows (4 x 16 B) in flight and sums in fp64; partial[(blk * nsplit + z)][N].
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rowblock_partial_kernel(const float* __restrict__ x, int64_t ldx, int64_t rows, int N,
                                                               float* __restrict__ partial) {
  __shared__ double red[4][256];
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int col = (blockIdx.x * 64 + cl) * 4;
  const int64_t base = (int64_t)blockIdx.y * rows;
  const int64_t step = (int64_t)gridDim.z * 4;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  if (col < N) {
    const float* xp = x + base * ldx + col;
    int64_t r = (int64_t)blockIdx.z * 4 + rl;
    for (; r + 3 * step < rows; r += 4 * step) {
      f32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = *(const f32x4*)(xp + (r + u * step) * ldx);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] += (double)v[u][e];
    }
    for (; r < rows; r += step) {
      const f32x4 v = *(const f32x4*)(xp + r * ldx);
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] += (double)v[e];
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) red[rl][4 * cl + e] = s[e];
  __syncthreads();
  const int c = threadIdx.x, oc = blockIdx.x * 256 + c;
  if (oc < N)
    partial[((int64_t)blockIdx.y * gridDim.z + blockIdx.z) * N + oc] = (float)(red[0][c] + red[1][c] + red[2][c] + red[3][c]);
}

// out[g][n] += the ordered fold of partial[g][0 .. nslots)[n]; one thread per (g, n)
__global__ __launch_bounds__(256) void fold_groups_kernel(const float* __restrict__ partial, int nslots, int N, int64_t total,
                                                          float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int64_t g = e / N;
  const int n = (int)(e - g * N);
  const double s = fold_slots(partial + g * nslots * N + n, nslots, N);
  out[e] = out[e] + (float)s;
}

// ---------------------------------------------------------------------------------------------------------------------
// 2. LayerNorm backward: the row arithmetic of ln_bwd_kernel (backward.hip), operation for operation — dx is bit-equal —
//    with the workgroup's column sums WRITTEN to partial[workgroup][2][C] at the end.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ln_bwd_partial_kernel(const float* __restrict__ x, int64_t ldx,
                                                             const float* __restrict__ dy, int64_t lddy, int64_t M, int C,
                                                             const float* __restrict__ gamma, float eps,
                                                             float* __restrict__ dx, int64_t lddx, float* __restrict__ partial,
                                                             const float* __restrict__ dx_add, int64_t ldadd) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nwave = (int64_t)gridDim.x * 4;
  constexpr int KM = 5;
  f32x4 gv[KM], ag[KM], ab[KM];
#pragma unroll
  for (int k = 0; k < KM; ++k) {
    const int c = 256 * k + 4 * lane;
    gv[k] = c < C ? *(const f32x4*)(gamma + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    ag[k] = ab[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const float invC = 1.0f / (float)C;
  for (int64_t m = wave; m < M; m += nwave) {
    f32x4 xv[KM], dv[KM];
    float s = 0.f, q = 0.f;
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      const int c = 256 * k + 4 * lane;
      const bool ok = c < C;
      xv[k] = ok ? *(const f32x4*)(x + m * ldx + c) : f32x4{0.f, 0.f, 0.f, 0.f};
      dv[k] = ok ? *(const f32x4*)(dy + m * lddy + c) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 4; ++e) s += xv[k][e];
    }
    const float mean = wave_sum(s) * invC;
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      const int c = 256 * k + 4 * lane;
      if (c < C) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = xv[k][e] - mean;
          q = fmaf(d, d, q);
        }
      }
    }
    const float rstd = rsqrtf(wave_sum(q) * invC + eps);
    float m1 = 0.f, m2 = 0.f;
#pragma unroll
    for (int k = 0; k < KM; ++k) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float xh = (xv[k][e] - mean) * rstd;
        const float dh = dv[k][e] * gv[k][e];
        xv[k][e] = xh;
        m1 += dh;
        m2 = fmaf(dh, xh, m2);
        ag[k][e] = fmaf(dv[k][e], xh, ag[k][e]);
        ab[k][e] += dv[k][e];
      }
    }
    m1 = wave_sum(m1) * invC;
    m2 = wave_sum(m2) * invC;
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      const int c = 256 * k + 4 * lane;
      if (c < C) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = rstd * (dv[k][e] * gv[k][e] - m1 - xv[k][e] * m2);
        if (dx_add) o += *(const f32x4*)(dx_add + m * ldadd + c);
        *(f32x4*)(dx + m * lddx + c) = o;
      }
    }
  }
  // the four waves' column sums meet in LDS (wave order 0..3); the workgroup's slot gets them as 16-byte stores
  __shared__ float red[4][2 * 1280];
  const int w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < KM; ++k) {
    const int c = 256 * k + 4 * lane;
    if (c < C) {
      *(f32x4*)(&red[w][c]) = ag[k];
      *(f32x4*)(&red[w][1280 + c]) = ab[k];
    }
  }
  __syncthreads();
  float* pout = partial + (int64_t)blockIdx.x * 2 * C;
  for (int c = threadIdx.x * 4; c < C; c += 1024) {
    const f32x4 a = *(const f32x4*)(&red[0][c]) + *(const f32x4*)(&red[1][c]) + *(const f32x4*)(&red[2][c]) +
                    *(const f32x4*)(&red[3][c]);
    const f32x4 b = *(const f32x4*)(&red[0][1280 + c]) + *(const f32x4*)(&red[1][1280 + c]) +
                    *(const f32x4*)(&red[2][1280 + c]) + *(const f32x4*)(&red[3][1280 + c]);
    *(f32x4*)(pout + c) = a;
    *(f32x4*)(pout + C + c) = b;
  }
}

// dgamma[c] += fold of partial[.][0][c], dbeta[c] += fold of partial[.][1][c]; one thread per (which, c)
__global__ __launch_bounds__(256) void ln_fold_kernel(const float* __restrict__ partial, int nslots, int C,
                                                      float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= 2 * C) return;
  const double s = fold_slots(partial + e, nslots, 2 * (int64_t)C);
  float* dst = e < C ? dgamma + e : dbeta + (e - C);
  *dst = *dst + (float)s;
}

// ---------------------------------------------------------------------------------------------------------------------
// 3. fp32 -> fp16 / bf16 and the column sums of every row chunk in the same pass (the geometry of cast_colsum_kernel,
//    backward.hip): grid (ceil(C / 64), nblk * chunks), block 256 = 8 column groups (8 channels) x 32 row lanes, four rows
//    (8 x 16 B) in flight per thread; partial[(blk * chunks + chunk)][C].
// ---------------------------------------------------------------------------------------------------------------------
template <bool BF>
__global__ __launch_bounds__(256) void cast_colsum_partial_kernel(const float* __restrict__ x, int64_t ldx,
                                                                  unsigned short* __restrict__ y, int64_t ldy,
                                                                  int64_t rows_per_block, int chunks, int rows_per_chunk,
                                                                  int C, float* __restrict__ partial) {
  __shared__ float red[32][65];
  const int t = threadIdx.x, cg = t & 7, rl = t >> 3;
  const int c = blockIdx.x * 64 + cg * 8;
  const int blk = blockIdx.y / chunks, ch = blockIdx.y - blk * chunks;
  const int64_t r_begin = (int64_t)ch * rows_per_chunk;
  int64_t r_end = r_begin + rows_per_chunk;
  if (r_end > rows_per_block) r_end = rows_per_block;
  const int64_t base = (int64_t)blk * rows_per_block;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (c < C) {
    for (int64_t r = r_begin + rl; r < r_end; r += 128) {
      f32x4 a[4], b[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t rr = r + 32 * u;
        if (rr < r_end) {
          const float* src = x + (base + rr) * ldx + c;
          a[u] = *(const f32x4*)src;
          b[u] = *(const f32x4*)(src + 4);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t rr = r + 32 * u;
        if (rr < r_end) {
          us8 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            acc[e] += a[u][e];
            acc[e + 4] += b[u][e];
            if (BF) {
              o[e] = bf16_rne(a[u][e]);
              o[e + 4] = bf16_rne(b[u][e]);
            } else {
              o[e] = __builtin_bit_cast(unsigned short, (f16)a[u][e]);
              o[e + 4] = __builtin_bit_cast(unsigned short, (f16)b[u][e]);
            }
          }
          *(us8*)(y + (base + rr) * ldy + c) = o;
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[rl][cg * 8 + e] = acc[e];
  __syncthreads();
  if (t < 64 && blockIdx.x * 64 + t < C) {
    float s0 = 0.f;
#pragma unroll
    for (int r = 0; r < 32; ++r) s0 += red[r][t];
    partial[(int64_t)blockIdx.y * C + blockIdx.x * 64 + t] = s0;
  }
}

// grid (ceil(C / 256), gy).  gy = nblk (no total): thread (blk, c) folds its block's chunks.  gy = 1 (total wanted): thread
// c owns column c of EVERY block and of the total: it folds block after block, and the total from the blocks' fp64 sums in
// block order.
__global__ __launch_bounds__(256) void cast_colsum_fold_kernel(const float* __restrict__ partial, int nblk, int chunks, int C,
                                                               float* __restrict__ sums, float* __restrict__ total) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const int b0 = total ? 0 : (int)blockIdx.y, b1 = total ? nblk : b0 + 1;
  double tot = 0.0;
  for (int b = b0; b < b1; ++b) {
    const double s = fold_slots(partial + (int64_t)b * chunks * C + c, chunks, C);
    float* dst = sums + (int64_t)b * C + c;
    *dst = *dst + (float)s;
    tot += s;
  }
  if (total) total[c] = total[c] + (float)tot;
}

// ---------------------------------------------------------------------------------------------------------------------
// 4. AlphaBlender backward (blend_bwd_kernel, train_ops.hip): grid (chunks per frame, frames); partial[frame][chunk].
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void blend_bwd_partial_kernel(const float* __restrict__ dy, int64_t lddy,
                                                                const float* __restrict__ xs, int64_t lds_,
                                                                const float* __restrict__ xt, int64_t ldt,
                                                                const float* __restrict__ alpha, int C4, int64_t rows,
                                                                float* __restrict__ dxs, int64_t lddxs, int acc_xs,
                                                                float* __restrict__ dxt, int64_t lddxt, int want_alpha,
                                                                float* __restrict__ partial) {
  const int frame = blockIdx.y;
  const float a = alpha[frame];
  const int64_t total = rows * C4;
  const int64_t m0 = (int64_t)frame * rows;
  float part = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / C4;
    const int c = (int)(i - r * C4) * 4;
    const int64_t m = m0 + r;
    const f32x4 g = *(const f32x4*)(dy + m * lddy + c);
    if (want_alpha) {
      const f32x4 d = *(const f32x4*)(xs + m * lds_ + c) - *(const f32x4*)(xt + m * ldt + c);
      part += g[0] * d[0] + g[1] * d[1] + g[2] * d[2] + g[3] * d[3];
    }
    if (dxs) {
      f32x4 o = a * g;
      if (acc_xs) o += *(const f32x4*)(dxs + m * lddxs + c);
      *(f32x4*)(dxs + m * lddxs + c) = o;
    }
    *(f32x4*)(dxt + m * lddxt + c) = (1.0f - a) * g;
  }
  if (want_alpha) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_down(part, off, 64);
    __shared__ float ws[4];
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = part;
    __syncthreads();
    if (threadIdx.x == 0) partial[(int64_t)frame * gridDim.x + blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
  }
}

__global__ __launch_bounds__(256) void blend_fold_kernel(const float* __restrict__ partial, int chunks, int frames,
                                                         float* __restrict__ dalpha) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= frames) return;
  dalpha[f] = dalpha[f] + (float)fold_slots(partial + (int64_t)f * chunks, chunks, 1);
}

// ---------------------------------------------------------------------------------------------------------------------
// 5. grouped few-row dgrad.  One workgroup per (problem, k chunk of 256) walks EVERY n of the problem: 64 lanes x 4
//    consecutive k (16-byte weight loads) x 4 n lanes; a 64-column slice of dy sits in LDS.  The four n lanes meet in LDS in
//    lane order and the [M][256] tile goes to slot (block0 + chunk) of the scratch.  The fold adds, per element of a dx,
//    the tiles of the problems that share it in table order.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SD_MAXM = 32, SD_NS = 64, SD_TILE = SD_MAXM * 256;

__device__ __forceinline__ float dsilu_f(float v) {
  const float s = 1.0f / (1.0f + __expf(-v));
  return s * (1.0f + v * (1.0f - s));
}

__device__ __forceinline__ int smallm_find_idx(const gcd_smallm_problem* __restrict__ tab, int n_prob, int b) {
  int lo = 0, hi = n_prob - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].block0 <= b) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void smallm_dgrad_partial_kernel(const gcd_smallm_problem* __restrict__ tab, int n_prob,
                                                                   float* __restrict__ scratch) {
  __shared__ float dys[SD_MAXM * SD_NS];
  __shared__ __attribute__((aligned(16))) float red[4][8][256];
  const gcd_smallm_problem p = tab[smallm_find_idx(tab, n_prob, (int)blockIdx.x)];
  const int M = p.M, K = p.K, N = p.N;
  const int kb = (int)blockIdx.x - p.block0;
  const int kl = threadIdx.x & 63, ng = threadIdx.x >> 6;
  const int k4 = kb * 256 + 4 * kl;
  float acc[SD_MAXM][4];
#pragma unroll
  for (int m = 0; m < SD_MAXM; ++m)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[m][e] = 0.f;
  for (int n0 = 0; n0 < N; n0 += SD_NS) {
    const int nn = min(N - n0, SD_NS);
    __syncthreads();
    for (int i = threadIdx.x; i < M * SD_NS; i += 256) {
      const int m = i >> 6, n = i & 63;
      dys[i] = n < nn ? p.y[(int64_t)m * p.ldy + n0 + n] : 0.f;        // (p.y = dy here)
    }
    __syncthreads();
    if (k4 < K)          // K % 4 == 0
      for (int n = ng; n < nn; n += 4) {
        const f32x4 w = *(const f32x4*)(p.W + (int64_t)(n0 + n) * K + k4);
#pragma unroll
        for (int m = 0; m < SD_MAXM; ++m)
          if (m < M) {
            const float d = dys[m * SD_NS + n];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[m][e] += d * w[e];
          }
      }
  }
  float* tile = scratch + (int64_t)blockIdx.x * SD_TILE;
  const int k = kb * 256 + threadIdx.x;
#pragma unroll
  for (int mp = 0; mp < SD_MAXM / 8; ++mp) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) *(f32x4*)(&red[ng][j][4 * kl]) = f32x4{acc[mp * 8 + j][0], acc[mp * 8 + j][1], acc[mp * 8 + j][2], acc[mp * 8 + j][3]};
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int m = mp * 8 + j;
      if (m < M && k < K) {
        float v = red[0][j][threadIdx.x] + red[1][j][threadIdx.x] + red[2][j][threadIdx.x] + red[3][j][threadIdx.x];
        if (p.flags & 1) v *= dsilu_f(p.x[(int64_t)m * p.ldx + k]);
        tile[m * 256 + threadIdx.x] = v;
      }
    }
  }
}

__global__ __launch_bounds__(256) void smallm_dgrad_fold_kernel(const gcd_smallm_problem* __restrict__ tab, int n_prob,
                                                                const float* __restrict__ scratch) {
  const int idx = smallm_find_idx(tab, n_prob, (int)blockIdx.x);
  const gcd_smallm_problem p = tab[idx];
  if (p.reserved != idx) return;          // the first problem of a group owns the group's dx
  const int kb = (int)blockIdx.x - p.block0;
  const int k = kb * 256 + threadIdx.x;
  if (k >= p.K) return;
  double s[SD_MAXM];
#pragma unroll
  for (int m = 0; m < SD_MAXM; ++m) s[m] = 0.0;
  for (int q = idx; q < n_prob; ++q) {
    if (tab[q].reserved != idx) continue;
    const float* tile = scratch + (int64_t)(tab[q].block0 + kb) * SD_TILE + threadIdx.x;
#pragma unroll
    for (int m = 0; m < SD_MAXM; ++m)
      if (m < p.M) s[m] += (double)tile[m * 256];
  }
#pragma unroll
  for (int m = 0; m < SD_MAXM; ++m)
    if (m < p.M) {
      float* dst = p.dx + (int64_t)m * p.lddx + k;
      *dst = *dst + (float)s[m];
    }
}

// ---- launch geometry: functions of the shapes only ---------------------------------------------------------------------
int rowblock_nsplit(int64_t rows_per_block) {
  int64_t n = rows_per_block / 256;
  if (n < 1) n = 1;
  if (n > 64) n = 64;
  return (int)n;
}

int ln_blocks(int64_t M) {
  int64_t b = (M + 3) / 4;
  if (b > 768) b = 768;
  return (int)b;
}

// ~2048 workgroups over the launch, at least 32 rows per chunk
int64_t cast_chunks(int64_t nblk, int colb, int64_t rows_per_block, int* rows_per_chunk) {
  int64_t chunks = (2048 + nblk * colb - 1) / (nblk * colb);
  if (chunks < 1) chunks = 1;
  if (chunks > (rows_per_block + 31) / 32) chunks = (rows_per_block + 31) / 32;
  const int rpc = (int)((rows_per_block + chunks - 1) / chunks);
  chunks = (rows_per_block + rpc - 1) / rpc;
  if (rows_per_chunk) *rows_per_chunk = rpc;
  return chunks;
}

int64_t blend_chunks(int64_t frames, int64_t rows_per_frame, int C) {
  int64_t chunks = (rows_per_frame * (C / 4) + 255) / 256;
  const int64_t cap = frames >= 512 ? 1 : (4096 + frames - 1) / frames;
  if (chunks > cap) chunks = cap;
  return chunks;
}

}  // namespace

extern "C" int64_t gcd_rowblock_sum_det_scratch_floats(int64_t M, int N, int64_t rows_per_block) {
  if (M <= 0 || N <= 0 || rows_per_block <= 0 || M % rows_per_block != 0) return 0;
  return (M / rows_per_block) * rowblock_nsplit(rows_per_block) * N;
}

extern "C" int gcd_rowblock_sum_det_f32(const float* x, int64_t ldx, int64_t M, int N, int64_t rows_per_block, float* out,
                                        float* scratch, int64_t scratch_floats, void* stream) {
  CHECK_ARG(x && out && M > 0 && N > 0 && rows_per_block > 0 && M % rows_per_block == 0,
            "gcd_rowblock_sum_det_f32: M=%lld rows_per_block=%lld", (long long)M, (long long)rows_per_block);
  CHECK_ARG(N % 4 == 0 && ldx % 4 == 0 && ((uintptr_t)x & 15) == 0,
            "gcd_rowblock_sum_det_f32: N=%d / ldx=%lld must be multiples of 4, x 16-byte aligned", N, (long long)ldx);
  const int64_t nblk = M / rows_per_block;
  CHECK_ARG(nblk <= 65535, "gcd_rowblock_sum_det_f32: too many blocks");
  CHECK_SCRATCH("gcd_rowblock_sum_det", gcd_rowblock_sum_det_scratch_floats(M, N, rows_per_block));
  const int nsplit = rowblock_nsplit(rows_per_block);
  hipLaunchKernelGGL(rowblock_partial_kernel, dim3((N + 255) / 256, (unsigned)nblk, (unsigned)nsplit), dim3(256), 0,
                     (hipStream_t)stream, x, ldx, rows_per_block, N, scratch);
  CHECK_LAUNCH("gcd_rowblock_sum_det_f32");
  const int64_t total = nblk * N;
  hipLaunchKernelGGL(fold_groups_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, scratch,
                     nsplit, N, total, out);
  CHECK_LAUNCH("gcd_rowblock_sum_det_f32 (fold)");
  return 0;
}

extern "C" int64_t gcd_layernorm_bwd_det_scratch_floats(int64_t M, int C) {
  if (M <= 0 || C <= 0) return 0;
  return (int64_t)ln_blocks(M) * 2 * C;
}

extern "C" int gcd_layernorm_bwd_det(const float* x, int64_t ldx, const float* dy, int64_t lddy, int64_t M, int C,
                                     const float* gamma, float eps, float* dx, int64_t lddx, float* dgamma, float* dbeta,
                                     const float* dx_add, int64_t ld_add, float* scratch, int64_t scratch_floats,
                                     void* stream) {
  CHECK_ARG(!dx_add || ld_add % 4 == 0, "gcd_layernorm_bwd_det: ld_add");
  CHECK_ARG(x && dy && gamma && dx && dgamma && dbeta, "gcd_layernorm_bwd_det: null pointer");
  CHECK_ARG(C > 0 && C % 4 == 0 && C <= 1280 && ldx % 4 == 0 && lddy % 4 == 0 && lddx % 4 == 0 && M > 0,
            "gcd_layernorm_bwd_det: C=%d (multiple of 4, <= 1280), leading dimensions multiples of 4", C);
  CHECK_SCRATCH("gcd_layernorm_bwd_det", gcd_layernorm_bwd_det_scratch_floats(M, C));
  const int blocks = ln_blocks(M);
  hipLaunchKernelGGL(ln_bwd_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, ldx, dy, lddy, M, C,
                     gamma, eps, dx, lddx, scratch, dx_add, ld_add);
  CHECK_LAUNCH("gcd_layernorm_bwd_det");
  hipLaunchKernelGGL(ln_fold_kernel, dim3((unsigned)((2 * C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, scratch, blocks,
                     C, dgamma, dbeta);
  CHECK_LAUNCH("gcd_layernorm_bwd_det (fold)");
  return 0;
}

extern "C" int64_t gcd_cast_colsum_det_scratch_floats(int64_t M, int C, int64_t rows_per_block) {
  if (M <= 0 || C <= 0 || rows_per_block <= 0 || M % rows_per_block != 0) return 0;
  const int64_t nblk = M / rows_per_block;
  return nblk * cast_chunks(nblk, (C + 63) / 64, rows_per_block, nullptr) * C;
}

extern "C" int gcd_cast_colsum_det_f32(const float* x, int64_t ldx, void* y16, int64_t ldy, int64_t M, int C,
                                       int64_t rows_per_block, float* sums, int to_bf16, float* total, float* scratch,
                                       int64_t scratch_floats, void* stream) {
  CHECK_ARG(x && y16 && sums && M > 0 && C > 0 && C % 8 == 0 && ldx % 4 == 0 && ldy % 8 == 0 &&
                (((uintptr_t)x | (uintptr_t)y16) & 15) == 0,
            "gcd_cast_colsum_det_f32: bad args (C=%d must be a multiple of 8, ldx of 4, ldy of 8, 16-byte aligned rows)", C);
  CHECK_ARG(rows_per_block > 0 && M % rows_per_block == 0, "gcd_cast_colsum_det_f32: M=%lld rows_per_block=%lld",
            (long long)M, (long long)rows_per_block);
  const int64_t nblk = M / rows_per_block;
  const int colb = (C + 63) / 64;
  int rpc = 0;
  const int64_t chunks = cast_chunks(nblk, colb, rows_per_block, &rpc);
  CHECK_ARG(nblk * chunks <= 65535, "gcd_cast_colsum_det_f32: too many row blocks (%lld)", (long long)(nblk * chunks));
  CHECK_SCRATCH("gcd_cast_colsum_det", nblk * chunks * C);
  const dim3 grid(colb, (unsigned)(nblk * chunks));
  if (to_bf16)
    hipLaunchKernelGGL(cast_colsum_partial_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, ldx,
                       (unsigned short*)y16, ldy, rows_per_block, (int)chunks, rpc, C, scratch);
  else
    hipLaunchKernelGGL(cast_colsum_partial_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, ldx,
                       (unsigned short*)y16, ldy, rows_per_block, (int)chunks, rpc, C, scratch);
  CHECK_LAUNCH("gcd_cast_colsum_det_f32");
  hipLaunchKernelGGL(cast_colsum_fold_kernel, dim3((C + 255) / 256, total ? 1u : (unsigned)nblk), dim3(256), 0,
                     (hipStream_t)stream, scratch, (int)nblk, (int)chunks, C, sums, total);
  CHECK_LAUNCH("gcd_cast_colsum_det_f32 (fold)");
  return 0;
}

extern "C" int64_t gcd_blend_bwd_det_scratch_floats(int64_t M, int C, int64_t rows_per_frame) {
  if (M <= 0 || C <= 0 || rows_per_frame <= 0 || M % rows_per_frame != 0) return 0;
  const int64_t frames = M / rows_per_frame;
  return frames * blend_chunks(frames, rows_per_frame, C);
}

extern "C" int gcd_blend_bwd_det_f32(const float* dy, int64_t ld_dy, const float* xs, int64_t ld_s, const float* xt,
                                     int64_t ld_t, const float* alpha, int64_t M, int C, int64_t rows_per_frame, float* d_xs,
                                     int64_t ld_dxs, int accumulate_xs, float* d_xt, int64_t ld_dxt, float* d_alpha,
                                     float* scratch, int64_t scratch_floats, void* stream) {
  CHECK_ARG(dy && alpha && d_xt && (!d_alpha || (xs && xt)), "gcd_blend_bwd_det_f32: null pointer");      // (d_xs optional)
  CHECK_ARG(M > 0 && C > 0 && C % 4 == 0 && rows_per_frame > 0 && M % rows_per_frame == 0 && ld_dy % 4 == 0 &&
                ld_dxs % 4 == 0 && ld_dxt % 4 == 0 && (!d_alpha || (ld_s % 4 == 0 && ld_t % 4 == 0)),
            "gcd_blend_bwd_det_f32: M=%lld C=%d rows=%lld, leading dimensions multiples of 4", (long long)M, C,
            (long long)rows_per_frame);
  const int64_t frames = M / rows_per_frame;
  CHECK_ARG(frames < 65536, "gcd_blend_bwd_det_f32: %lld frames", (long long)frames);
  const int64_t chunks = blend_chunks(frames, rows_per_frame, C);
  if (d_alpha) CHECK_SCRATCH("gcd_blend_bwd_det", frames * chunks);
  hipLaunchKernelGGL(blend_bwd_partial_kernel, dim3((unsigned)chunks, (unsigned)frames), dim3(256), 0, (hipStream_t)stream, dy,
                     ld_dy, xs, ld_s, xt, ld_t, alpha, C / 4, rows_per_frame, d_xs, ld_dxs, accumulate_xs, d_xt, ld_dxt,
                     d_alpha ? 1 : 0, scratch);
  CHECK_LAUNCH("gcd_blend_bwd_det_f32");
  if (d_alpha) {
    hipLaunchKernelGGL(blend_fold_kernel, dim3((unsigned)((frames + 255) / 256)), dim3(256), 0, (hipStream_t)stream, scratch,
                       (int)chunks, (int)frames, d_alpha);
    CHECK_LAUNCH("gcd_blend_bwd_det_f32 (fold)");
  }
  return 0;
}

extern "C" int64_t gcd_smallm_dgrad_det_scratch_floats(int total_blocks) {
  return total_blocks > 0 ? (int64_t)total_blocks * SD_TILE : 0;
}

extern "C" int gcd_smallm_dgrad_det(const gcd_smallm_problem* table_dev, int n_prob, int total_blocks, float* scratch,
                                    int64_t scratch_floats, void* stream) {
  CHECK_ARG(table_dev && n_prob > 0 && total_blocks > 0, "gcd_smallm_dgrad_det: empty table");
  CHECK_SCRATCH("gcd_smallm_dgrad_det", gcd_smallm_dgrad_det_scratch_floats(total_blocks));
  hipLaunchKernelGGL(smallm_dgrad_partial_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, table_dev,
                     n_prob, scratch);
  CHECK_LAUNCH("gcd_smallm_dgrad_det");
  hipLaunchKernelGGL(smallm_dgrad_fold_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, table_dev,
                     n_prob, (const float*)scratch);
  CHECK_LAUNCH("gcd_smallm_dgrad_det (fold)");
  return 0;
}
