// libgcd_amd_lora.so (include/gcd_amd_lora.h): LoRA by merged weights — the merge and the projection of dW.
//
// Both are grouped: a workgroup finds its entry by a binary search over the entries' tile starts, and every index it
// forms is checked against that entry's own N, K, r.  Vector FMA throughout (fp32 in, fp32 out, one rounding per fma).
//
// merge_kernel      One workgroup per 64 x 64 tile of W.  B's 64 x r and A's r x 64 go through LDS; a thread holds a 4 x 4
//                   block of the sum, j ascending.  8 bytes of HBM traffic per 2 r flops: HBM-bound up to r = 16 or so,
//                   VALU-bound at r = 64.
// project_kernel    One workgroup per 256 x 256 region of dW, walked as 4 x 4 tiles of 64 x 64.  A tile of dW is read from
//                   HBM once into LDS and used twice: for dB (a thread owns one row and every fourth j) and for dA (a
//                   thread owns one column and every fourth j).  dB's partial sums live in registers across the four tiles
//                   of a row band, dA's across the whole region.  Partials go to scratch: r / 256 of dW's size each.
//                   Each fma reads about 1.25 LDS words: the kernel is bound by LDS bandwidth, not by HBM.
// reduce_kernel     Stage 2: adds a row's | column's partials in ascending region order, scales, stores; zeros for an
//                   entry without dW.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gcd_amd_lora.h"

static thread_local char g_err[512] = "";
static void gcd_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* gcd_lora_last_error(void) { return g_err; }
extern "C" int gcd_lora_abi_version(void) { return GCD_AMD_LORA_ABI_VERSION; }

#define GCD_CHECK_ARG(cond, ...)  \
  do {                            \
    if (!(cond)) {                \
      gcd_set_error(__VA_ARGS__); \
      return 2;                   \
    }                             \
  } while (0)

#define GCD_CHECK_HIP(expr)                                                  \
  do {                                                                       \
    hipError_t e_ = (expr);                                                  \
    if (e_ != hipSuccess) {                                                  \
      gcd_set_error("%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return 1;                                                              \
    }                                                                        \
  } while (0)

namespace {

constexpr int NT = 256;
constexpr int MT = GCD_LORA_MERGE_TILE;        // 64
constexpr int PT = GCD_LORA_PROJECT_TILE;      // 256
constexpr int ST = 64;                         // a tile of dW in LDS
constexpr int SUB = PT / ST;                   // tiles per region side
constexpr int RED_BLOCKS = 32;                 // workgroups per entry in stage 2
static_assert(MT == 64 && ST == 64 && SUB == 4 && GCD_LORA_MAX_RANK == 64, "the thread mappings below are written for these");

__host__ __device__ inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

__host__ __device__ inline int64_t scratch_floats(int N, int K, int r) {
  const int64_t f = cdiv64(K, PT) * N * r + cdiv64(N, PT) * r * K;
  return (f + 3) / 4 * 4;
}

__device__ __forceinline__ bool entry_ok(const gcd_lora_entry& e) {
  return e.N >= 1 && e.N <= GCD_LORA_MAX_DIM && e.K >= 1 && e.K <= GCD_LORA_MAX_DIM && e.r >= 1 && e.r <= GCD_LORA_MAX_RANK;
}

// The last entry whose tile start is <= blk (starts ascend; equal starts cannot occur: every entry has a tile).
template <bool MERGE>
__device__ __forceinline__ int find_entry(const gcd_lora_entry* __restrict__ tab, int n, int blk) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    const int t0 = MERGE ? tab[mid].merge_tile0 : tab[mid].project_tile0;
    if (t0 <= blk) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ------------------------------------------------------------------------------------------------------------- merge
__global__ __launch_bounds__(NT) void merge_kernel(const gcd_lora_entry* __restrict__ tab, int n) {
  __shared__ __attribute__((aligned(16))) float As[GCD_LORA_MAX_RANK][MT + 4];      // [j][k]
  __shared__ float Bs[MT][GCD_LORA_MAX_RANK + 1];                                   // [row][j]
  const int t = threadIdx.x;
  const gcd_lora_entry e = tab[find_entry<true>(tab, n, blockIdx.x)];
  if (!entry_ok(e)) return;
  const int local = (int)blockIdx.x - e.merge_tile0;
  const int tiles_k = (e.K + MT - 1) / MT, tiles_n = (e.N + MT - 1) / MT;
  if (local < 0 || local >= tiles_k * tiles_n) return;
  const int N = e.N, K = e.K, r = e.r;
  const int n0 = (local / tiles_k) * MT, k0 = (local % tiles_k) * MT;
  // this thread's 4 x 4 block of W0 first: the loads are in flight while A and B go through LDS and the sum is formed
  const int ty = t / 16, tx = t % 16;
  const bool vec = (K % 4 == 0) && aligned16(e.W0) && aligned16(e.W);
  const int kc = k0 + tx * 4;
  float w0[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = n0 + ty * 4 + i;
    const int64_t base = (int64_t)row * K + kc;
#pragma unroll
    for (int c = 0; c < 4; ++c) w0[i][c] = 0.f;
    if (row >= N || kc >= K) continue;
    if (vec) {                                   // K % 4 == 0 and kc % 4 == 0: kc < K means kc + 3 < K
      const float4 v = *reinterpret_cast<const float4*>(e.W0 + base);
      w0[i][0] = v.x; w0[i][1] = v.y; w0[i][2] = v.z; w0[i][3] = v.w;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (kc + c < K) w0[i][c] = e.W0[base + c];
    }
  }
  for (int idx = t; idx < r * MT; idx += NT) {
    const int j = idx / MT, c = idx % MT;
    As[j][c] = (k0 + c < K) ? e.A[(int64_t)j * K + k0 + c] : 0.f;
  }
  for (int idx = t; idx < MT * r; idx += NT) {
    const int row = idx / r, j = idx % r;
    Bs[row][j] = (n0 + row < N) ? e.B[(int64_t)(n0 + row) * r + j] : 0.f;
  }
  __syncthreads();
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[i][c] = 0.f;
  for (int j = 0; j < r; ++j) {
    const float4 a = *reinterpret_cast<const float4*>(&As[j][tx * 4]);
    const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float b = Bs[ty * 4 + i][j];
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[i][c] = fmaf(b, av[c], acc[i][c]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = n0 + ty * 4 + i;
    if (row >= N || kc >= K) continue;
    const int64_t base = (int64_t)row * K + kc;
    float w[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) w[c] = acc[i][c] == 0.f ? w0[i][c] : fmaf(e.scale, acc[i][c], w0[i][c]);      // a zero sum: W0's own bits
    if (vec) {
      *reinterpret_cast<float4*>(e.W + base) = make_float4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (kc + c < K) e.W[base + c] = w[c];
    }
  }
}

// ----------------------------------------------------------------------------------------------------------- project
// JI: j's per thread (every fourth one): 4 covers r <= 16, 16 covers r <= 64 (the host picks the kernel by the table's
// largest rank, which the caller states: an entry above it is skipped by both stages).  Rows of As / columns of Bs from r up to
// 4 JI are zero-filled, so the inner loops carry no predicate; only j < r is stored.
template <int JI>
__device__ __forceinline__ void project_region(const gcd_lora_entry& e, int n0, int k0, float* __restrict__ pb,
                                               float* __restrict__ pa, float (*Ds)[ST + 1], float (*As)[ST + 1],
                                               float (*Bs)[GCD_LORA_MAX_RANK + 1]) {
  const int t = threadIdx.x, N = e.N, K = e.K, r = e.r;
  const int brow = t / 4, bjg = t % 4;         // dB: one row of the tile, j = bjg + 4 i
  const int acol = t % ST, ajg = t / ST;       // dA: one column of the tile, j = ajg + 4 i
  const bool vec = (K % 4 == 0) && aligned16(e.dW);
  float da[SUB][JI];
#pragma unroll
  for (int cs = 0; cs < SUB; ++cs)
#pragma unroll
    for (int i = 0; i < JI; ++i) da[cs][i] = 0.f;
  for (int rs = 0; rs < SUB; ++rs) {
    const int nb = n0 + rs * ST;
    if (nb >= N) break;                        // (uniform)
    __syncthreads();                           // the previous band's readers of Bs are done
    for (int idx = t; idx < ST * 4 * JI; idx += NT) {
      const int row = idx / (4 * JI), j = idx % (4 * JI);
      Bs[row][j] = (nb + row < N && j < r) ? e.B[(int64_t)(nb + row) * r + j] : 0.f;
    }
    float db[JI];
#pragma unroll
    for (int i = 0; i < JI; ++i) db[i] = 0.f;
#pragma unroll
    for (int cs = 0; cs < SUB; ++cs) {
      const int kb = k0 + cs * ST;
      if (kb < K) {                            // (uniform)
        __syncthreads();                       // the previous tile's readers of Ds / As are done
        for (int idx = t; idx < 4 * JI * ST; idx += NT) {
          const int j = idx / ST, c = idx % ST;
          As[j][c] = (j < r && kb + c < K) ? e.A[(int64_t)j * K + kb + c] : 0.f;
        }
        if (vec) {
          const int c4 = (t % 16) * 4;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int row = t / 16 + 16 * i;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (nb + row < N && kb + c4 < K) v = *reinterpret_cast<const float4*>(e.dW + (int64_t)(nb + row) * K + kb + c4);
            Ds[row][c4] = v.x; Ds[row][c4 + 1] = v.y; Ds[row][c4 + 2] = v.z; Ds[row][c4 + 3] = v.w;
          }
        } else {
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int row = t / ST + 4 * i;
            Ds[row][acol] = (nb + row < N && kb + acol < K) ? e.dW[(int64_t)(nb + row) * K + kb + acol] : 0.f;
          }
        }
        __syncthreads();
#pragma unroll 8
        for (int kk = 0; kk < ST; ++kk) {      // dB[row, j] += dW[row, k] A[j, k], k ascending
          const float d = Ds[brow][kk];
#pragma unroll
          for (int i = 0; i < JI; ++i) db[i] = fmaf(d, As[bjg + 4 * i][kk], db[i]);
        }
#pragma unroll 8
        for (int nn = 0; nn < ST; ++nn) {      // dA[j, col] += B[row, j] dW[row, col], row ascending
          const float d = Ds[nn][acol];
#pragma unroll
          for (int i = 0; i < JI; ++i) da[cs][i] = fmaf(Bs[nn][ajg + 4 * i], d, da[cs][i]);
        }
      }
    }
    if (nb + brow < N) {
#pragma unroll
      for (int i = 0; i < JI; ++i) {
        const int j = bjg + 4 * i;
        if (j < r) pb[(int64_t)(nb + brow) * r + j] = db[i];
      }
    }
  }
#pragma unroll
  for (int cs = 0; cs < SUB; ++cs) {
    const int k = k0 + cs * ST + acol;
    if (k < K) {
#pragma unroll
      for (int i = 0; i < JI; ++i) {
        const int j = ajg + 4 * i;
        if (j < r) pa[(int64_t)j * K + k] = da[cs][i];
      }
    }
  }
}

template <int JI>
__global__ __launch_bounds__(NT) void project_kernel(const gcd_lora_entry* __restrict__ tab, int n, float* __restrict__ scratch,
                                                     int64_t scratch_len, int max_rank) {
  __shared__ float Ds[ST][ST + 1];
  __shared__ float As[GCD_LORA_MAX_RANK][ST + 1];
  __shared__ float Bs[ST][GCD_LORA_MAX_RANK + 1];
  const gcd_lora_entry e = tab[find_entry<false>(tab, n, blockIdx.x)];
  if (!entry_ok(e) || e.r > 4 * JI || e.r > max_rank || e.dW == nullptr) return;
  const int local = (int)blockIdx.x - e.project_tile0;
  const int reg_k = (e.K + PT - 1) / PT, reg_n = (e.N + PT - 1) / PT;
  if (local < 0 || local >= reg_k * reg_n) return;
  if (e.scratch0 < 0 || e.scratch0 > scratch_len || scratch_floats(e.N, e.K, e.r) > scratch_len - e.scratch0) return;
  const int cn = local / reg_k, ck = local % reg_k;
  // partials: PB[ck][N][r], then PA[cn][r][K]
  float* pb = scratch + e.scratch0 + (int64_t)ck * e.N * e.r;
  float* pa = scratch + e.scratch0 + (int64_t)reg_k * e.N * e.r + (int64_t)cn * e.r * e.K;
  project_region<JI>(e, cn * PT, ck * PT, pb, pa, Ds, As, Bs);
}

__global__ __launch_bounds__(NT) void reduce_kernel(const gcd_lora_entry* __restrict__ tab, const float* __restrict__ scratch,
                                                    int64_t scratch_len, int max_rank) {
  const gcd_lora_entry e = tab[blockIdx.x];
  if (!entry_ok(e) || e.r > max_rank) return;
  const bool live = e.dW != nullptr;
  if (live && (e.scratch0 < 0 || e.scratch0 > scratch_len || scratch_floats(e.N, e.K, e.r) > scratch_len - e.scratch0)) return;
  const int64_t nb = (int64_t)e.N * e.r, na = (int64_t)e.r * e.K;
  const int reg_k = (e.K + PT - 1) / PT, reg_n = (e.N + PT - 1) / PT;
  const float* pb = scratch + e.scratch0;
  const float* pa = pb + (int64_t)reg_k * nb;
  for (int64_t idx = (int64_t)blockIdx.y * NT + threadIdx.x; idx < nb + na; idx += (int64_t)RED_BLOCKS * NT) {
    float s = 0.f;
    if (idx < nb) {
      if (live)
        for (int c = 0; c < reg_k; ++c) s += pb[(int64_t)c * nb + idx];
      e.dB[idx] = live ? e.scale * s : 0.f;
    } else {
      const int64_t ia = idx - nb;
      if (live)
        for (int c = 0; c < reg_n; ++c) s += pa[(int64_t)c * na + ia];
      e.dA[ia] = live ? e.scale * s : 0.f;
    }
  }
}

}  // namespace

extern "C" int gcd_lora_merge(const gcd_lora_entry* table, int n, int tiles, void* stream) {
  GCD_CHECK_ARG(table != nullptr, "gcd_lora_merge: null table");
  GCD_CHECK_ARG(n >= 1 && n <= GCD_LORA_MAX_ENTRIES, "gcd_lora_merge: n = %d outside 1 .. %d", n, GCD_LORA_MAX_ENTRIES);
  GCD_CHECK_ARG(tiles >= n, "gcd_lora_merge: tiles = %d for %d entries (every entry has at least one)", tiles, n);
  hipLaunchKernelGGL(merge_kernel, dim3((unsigned)tiles), dim3(NT), 0, (hipStream_t)stream, table, n);
  GCD_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int64_t gcd_lora_project_scratch_floats(int N, int K, int r) {
  if (N < 1 || N > GCD_LORA_MAX_DIM || K < 1 || K > GCD_LORA_MAX_DIM || r < 1 || r > GCD_LORA_MAX_RANK) {
    gcd_set_error("gcd_lora_project_scratch_floats: N = %d, K = %d outside 1 .. %d or r = %d outside 1 .. %d", N, K,
                  GCD_LORA_MAX_DIM, r, GCD_LORA_MAX_RANK);
    return -1;
  }
  return scratch_floats(N, K, r);
}

extern "C" int gcd_lora_project(const gcd_lora_entry* table, int n, int tiles, int max_rank, float* scratch,
                                int64_t scratch_len, void* stream) {
  GCD_CHECK_ARG(table != nullptr, "gcd_lora_project: null table");
  GCD_CHECK_ARG(n >= 1 && n <= GCD_LORA_MAX_ENTRIES, "gcd_lora_project: n = %d outside 1 .. %d", n, GCD_LORA_MAX_ENTRIES);
  GCD_CHECK_ARG(tiles >= n, "gcd_lora_project: tiles = %d for %d entries (every entry has at least one)", tiles, n);
  GCD_CHECK_ARG(max_rank >= 1 && max_rank <= GCD_LORA_MAX_RANK, "gcd_lora_project: max_rank = %d outside 1 .. %d", max_rank,
                GCD_LORA_MAX_RANK);
  GCD_CHECK_ARG(scratch != nullptr, "gcd_lora_project: null scratch");
  GCD_CHECK_ARG(scratch_len >= 4 * (int64_t)n, "gcd_lora_project: scratch of %lld floats for %d entries", (long long)scratch_len, n);
  GCD_CHECK_ARG(((uintptr_t)scratch & 3) == 0, "gcd_lora_project: scratch is not aligned to 4 bytes");
  if (max_rank <= 16)
    hipLaunchKernelGGL(project_kernel<4>, dim3((unsigned)tiles), dim3(NT), 0, (hipStream_t)stream, table, n, scratch, scratch_len,
                       max_rank);
  else
    hipLaunchKernelGGL(project_kernel<16>, dim3((unsigned)tiles), dim3(NT), 0, (hipStream_t)stream, table, n, scratch, scratch_len,
                       max_rank);
  GCD_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)n, RED_BLOCKS), dim3(NT), 0, (hipStream_t)stream, table, (const float*)scratch,
                     scratch_len, max_rank);
  GCD_CHECK_HIP(hipGetLastError());
  return 0;
}
