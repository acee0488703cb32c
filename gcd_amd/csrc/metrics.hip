// metrics.hip — libgcd_amd_metrics.so: the evaluation metrics on the device.  C ABI: include/gcd_amd_metrics.h.
//
// gcd_metrics_frames_f32: one workgroup per (sample, frame, 16 x 32 tile of the image).  Per channel the tile of `pred`
// and `gt` with a 3-pixel halo is staged in LDS as fp32; the five 7-wide row sums (x, y, xx, yy, xy) of every staged row
// go to LDS as fp64, the 7 rows are added per output pixel, and the SSIM map value and the squared error are added to
// per-thread fp64 accumulators (whole image, visible, occluded).  The occlusion flags of the tile are staged once with
// the same halo: three erosions by the 3x3 cross are "all 25 pixels within L1 distance 3 are in the mask", and for a
// pixel of the cropped map all of them lie inside the image, so no border rule is ever consulted.  A fixed LDS tree folds
// the 256 threads, the ten partial sums of the tile go to `scratch`, and a second kernel (one workgroup per (sample,
// frame)) folds the tiles in a fixed order and takes the logarithm.  No atomics: bit-identical from call to call.
//
// gcd_metrics_diversity_f32: one thread per pixel and frame (block-strided), the S samples read twice (mean, then the
// squared deviations, as numpy's std does), per-block partial sums to `scratch`, folded per frame the same way.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gcd_amd_metrics.h"

static thread_local char g_err[512] = "";
static void gcd_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* gcd_metrics_last_error(void) { return g_err; }
extern "C" int gcd_metrics_abi_version(void) { return GCD_AMD_METRICS_ABI_VERSION; }

#define GCD_CHECK_ARG(cond, ...)  \
  do {                            \
    if (!(cond)) {                \
      gcd_set_error(__VA_ARGS__); \
      return 2;                   \
    }                             \
  } while (0)

namespace {

constexpr int NT = 256;                      // threads per workgroup, every kernel here
constexpr int TH = 16, TW = 32;              // output tile
constexpr int R = 3, WIN = 7;                // window radius / size; also the erosion radius
constexpr int IH = TH + 2 * R, IW = TW + 2 * R;
constexpr int PER_THREAD = TH * TW / NT;     // output pixels per thread
constexpr int NQ = 10;                       // partial sums per tile, see Q_*
constexpr int NQD = 4;                       // partial sums per diversity block
constexpr int DIV_MAX_BLOCKS = 1024;         // per frame
constexpr int DIV_PIX_PER_THREAD = 4;
enum { Q_SE = 0, Q_SE_VIS, Q_SE_OCC, Q_SS, Q_SS_VIS, Q_SS_OCC, Q_N_VIS, Q_N_OCC, Q_NE_VIS, Q_NE_OCC };
static_assert(TH * TW % NT == 0, "whole output pixels per thread");
static_assert(NQ * NT <= 5 * IH * TW, "the block fold reuses the row-sum buffer");

// pred on load: the decoder's raw output goes through clamp((x + 1) * 0.5, 0, 1) in fp32 (a NaN stays a NaN, as in torch)
__device__ __forceinline__ float to_unit(float x, bool is_signed) {
  if (!is_signed) return x;
  float v = (x + 1.0f) * 0.5f;
  v = v < 0.0f ? 0.0f : v;
  v = v > 1.0f ? 1.0f : v;
  return v;
}

// ((|r0| + |r1|) + |r2|) <= 1e-7f in fp32, in that order: numpy's sum over the channel axis of a float32 array
__device__ __forceinline__ bool occluded_at(const float* __restrict__ rep, int64_t plane, int64_t off) {
  const float s = (fabsf(rep[off]) + fabsf(rep[off + plane])) + fabsf(rep[off + 2 * plane]);
  return s <= 1e-7f;
}

// Fold q[0..n) of every thread over the workgroup in a fixed order; thread 0 ends up with the sums in q.
// red: n * NT doubles of LDS.  Ends with every thread past its last read of red.
template <int N>
__device__ __forceinline__ void block_fold(double (&q)[N], double* red) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < N; ++i) red[i * NT + tid] = q[i];
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int i = 0; i < N; ++i) red[i * NT + tid] += red[i * NT + tid + s];
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < N; ++i) q[i] = red[i * NT];
  __syncthreads();
}

__global__ __launch_bounds__(NT) void metrics_tile_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                          const float* __restrict__ rep, int T, int H, int W, int tiles_x,
                                                          int tiles_y, int is_signed, double* __restrict__ part) {
  __shared__ float sp[IH][IW + 1];
  __shared__ float sg[IH][IW + 1];
  __shared__ unsigned char so[IH][IW + 2];   // 1: occluded, 0: visible (or outside the image: never consulted)
  __shared__ double sh[5 * IH * TW];         // [q][row][col] row sums; the block fold's buffer afterwards

  const int tid = threadIdx.x;
  int64_t b = blockIdx.x;
  const int64_t tile = b % ((int64_t)tiles_x * tiles_y);
  const int tix = (int)(b % tiles_x);
  b /= tiles_x;
  const int tiy = (int)(b % tiles_y);
  b /= tiles_y;
  const int t = (int)(b % T);
  const int64_t s = b / T;
  const int y0 = tiy * TH, x0 = tix * TW;
  const int64_t plane = (int64_t)H * W;
  const float* pbase = pred + ((s * T + t) * 3) * plane;
  const float* gbase = gt + ((int64_t)t * 3) * plane;
  const float* rbase = rep ? rep + ((int64_t)t * 3) * plane : nullptr;

  if (rbase) {
    for (int i = tid; i < IH * IW; i += NT) {
      const int iy = i / IW, ix = i % IW;
      const int y = y0 - R + iy, x = x0 - R + ix;
      unsigned char v = 0;
      if (y >= 0 && y < H && x >= 0 && x < W) v = occluded_at(rbase, plane, (int64_t)y * W + x) ? 1 : 0;
      so[iy][ix] = v;
    }
  }
  __syncthreads();

  // this thread's output pixels: where they are and which sums they feed
  bool in_img[PER_THREAD], in_crop[PER_THREAD], vis[PER_THREAD], occ[PER_THREAD], evis[PER_THREAD], eocc[PER_THREAD];
  double q[NQ];
#pragma unroll
  for (int i = 0; i < NQ; ++i) q[i] = 0.0;
#pragma unroll
  for (int k = 0; k < PER_THREAD; ++k) {
    const int o = tid + k * NT;
    const int oy = o / TW, ox = o % TW;
    const int y = y0 + oy, x = x0 + ox;
    in_img[k] = y < H && x < W;
    in_crop[k] = y >= R && y < H - R && x >= R && x < W - R;
    vis[k] = occ[k] = evis[k] = eocc[k] = false;
    if (rbase && in_img[k]) {
      occ[k] = so[oy + R][ox + R] != 0;
      vis[k] = !occ[k];
      q[Q_N_VIS] += vis[k] ? 1.0 : 0.0;
      q[Q_N_OCC] += occ[k] ? 1.0 : 0.0;
      if (in_crop[k]) {
        int n_occ = 0;
        for (int dy = -R; dy <= R; ++dy) {
          const int w = R - (dy < 0 ? -dy : dy);
          for (int dx = -w; dx <= w; ++dx) n_occ += so[oy + R + dy][ox + R + dx];
        }
        evis[k] = n_occ == 0;
        eocc[k] = n_occ == 2 * R * (R + 1) + 1;
        q[Q_NE_VIS] += evis[k] ? 1.0 : 0.0;
        q[Q_NE_OCC] += eocc[k] ? 1.0 : 0.0;
      }
    }
  }

  const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
  const double inv_np = 1.0 / (double)(WIN * WIN), cov_norm = (double)(WIN * WIN) / (double)(WIN * WIN - 1);
  for (int c = 0; c < 3; ++c) {
    const float* pc = pbase + c * plane;
    const float* gc = gbase + c * plane;
    for (int i = tid; i < IH * IW; i += NT) {
      const int iy = i / IW, ix = i % IW;
      const int y = y0 - R + iy, x = x0 - R + ix;
      float pv = 0.0f, gv = 0.0f;
      if (y >= 0 && y < H && x >= 0 && x < W) {
        const int64_t off = (int64_t)y * W + x;
        pv = to_unit(pc[off], is_signed != 0);
        gv = gc[off];
      }
      sp[iy][ix] = pv;
      sg[iy][ix] = gv;
    }
    __syncthreads();
    for (int i = tid; i < IH * TW; i += NT) {
      const int iy = i / TW, ox = i % TW;
      double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
      for (int j = 0; j < WIN; ++j) {
        const double xv = (double)sp[iy][ox + j], yv = (double)sg[iy][ox + j];
        sx += xv, sy += yv, sxx += xv * xv, syy += yv * yv, sxy += xv * yv;
      }
      sh[0 * IH * TW + i] = sx, sh[1 * IH * TW + i] = sy, sh[2 * IH * TW + i] = sxx, sh[3 * IH * TW + i] = syy;
      sh[4 * IH * TW + i] = sxy;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
      if (!in_img[k]) continue;
      const int o = tid + k * NT;
      const int oy = o / TW, ox = o % TW;
      const double e = (double)sg[oy + R][ox + R] - (double)sp[oy + R][ox + R];
      const double se = e * e;
      q[Q_SE] += se;
      if (vis[k]) q[Q_SE_VIS] += se;
      if (occ[k]) q[Q_SE_OCC] += se;
      if (!in_crop[k]) continue;
      double w[5];
#pragma unroll
      for (int m = 0; m < 5; ++m) {
        double a = 0.0;
#pragma unroll
        for (int j = 0; j < WIN; ++j) a += sh[m * IH * TW + (oy + j) * TW + ox];
        w[m] = a * inv_np;
      }
      const double ux = w[0], uy = w[1];
      const double vx = cov_norm * (w[2] - ux * ux), vy = cov_norm * (w[3] - uy * uy), vxy = cov_norm * (w[4] - ux * uy);
      const double ss = ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
      q[Q_SS] += ss;
      if (evis[k]) q[Q_SS_VIS] += ss;
      if (eocc[k]) q[Q_SS_OCC] += ss;
    }
    __syncthreads();      // sp / sg / sh are restaged by the next channel (or sh reused by the fold)
  }

  block_fold<NQ>(q, sh);
  if (tid == 0) {
    double* dst = part + ((s * T + t) * ((int64_t)tiles_x * tiles_y) + tile) * NQ;
#pragma unroll
    for (int i = 0; i < NQ; ++i) dst[i] = q[i];
  }
}

__device__ __forceinline__ double psnr_of(double se, double n) {
  if (!(n > 0.0)) return nan("");
  const double mse = se / n;
  return mse == 0.0 ? (double)INFINITY : 10.0 * log10(1.0 / mse);
}

// One workgroup per (sample, frame): tiles in a fixed order per thread, then the fixed tree.
__global__ __launch_bounds__(NT) void metrics_fold_kernel(const double* __restrict__ part, int64_t tiles, int H, int W,
                                                          int have_mask, double* __restrict__ out) {
  __shared__ double red[NQ * NT];
  const double* src = part + (int64_t)blockIdx.x * tiles * NQ;
  double q[NQ];
#pragma unroll
  for (int i = 0; i < NQ; ++i) q[i] = 0.0;
  for (int64_t j = threadIdx.x; j < tiles; j += NT) {
#pragma unroll
    for (int i = 0; i < NQ; ++i) q[i] += src[j * NQ + i];
  }
  block_fold<NQ>(q, red);
  if (threadIdx.x == 0) {
    double* o = out + (int64_t)blockIdx.x * GCD_METRICS_FRAME_VALUES;
    const double n_all = (double)H * (double)W, n_crop = (double)(H - 2 * R) * (double)(W - 2 * R);
    o[0] = psnr_of(q[Q_SE], 3.0 * n_all);
    o[1] = q[Q_SS] / (3.0 * n_crop);
    if (have_mask) {
      o[2] = psnr_of(q[Q_SE_VIS], 3.0 * q[Q_N_VIS]);
      o[3] = q[Q_NE_VIS] > 0.0 ? q[Q_SS_VIS] / (3.0 * q[Q_NE_VIS]) : nan("");
      o[4] = psnr_of(q[Q_SE_OCC], 3.0 * q[Q_N_OCC]);
      o[5] = q[Q_NE_OCC] > 0.0 ? q[Q_SS_OCC] / (3.0 * q[Q_NE_OCC]) : nan("");
    } else {
      o[2] = o[3] = o[4] = o[5] = 0.0;
    }
  }
}

__global__ __launch_bounds__(NT) void diversity_kernel(const float* __restrict__ pred, const float* __restrict__ rep, int S,
                                                       int T, int64_t plane, int nb, int is_signed,
                                                       float* __restrict__ unc, double* __restrict__ part) {
  __shared__ double red[NQD * NT];
  const int t = blockIdx.x / nb, b = blockIdx.x % nb;
  const int64_t sample_stride = (int64_t)T * 3 * plane;
  const float* pbase = pred + ((int64_t)t * 3) * plane;
  const float* rbase = rep ? rep + ((int64_t)t * 3) * plane : nullptr;
  double q[NQD] = {0.0, 0.0, 0.0, 0.0};        // sum over all, visible, occluded pixels; visible pixels
  for (int64_t i = (int64_t)b * NT + threadIdx.x; i < plane; i += (int64_t)nb * NT) {
    double acc = 0.0;
    for (int c = 0; c < 3; ++c) {
      const float* p = pbase + c * plane + i;
      double sum = 0.0;
      for (int s = 0; s < S; ++s) sum += (double)to_unit(p[s * sample_stride], is_signed != 0);
      const double mean = sum / (double)S;
      double dev = 0.0;
      for (int s = 0; s < S; ++s) {
        const double d = (double)to_unit(p[s * sample_stride], is_signed != 0) - mean;
        dev += d * d;
      }
      acc += sqrt(dev / (double)S);
    }
    const double u = acc / 3.0;
    unc[(int64_t)t * plane + i] = (float)u;
    q[0] += u;
    if (rbase) {
      if (occluded_at(rbase, plane, i)) {
        q[2] += u;
      } else {
        q[1] += u;
        q[3] += 1.0;
      }
    }
  }
  block_fold<NQD>(q, red);
  if (threadIdx.x == 0) {
    double* dst = part + ((int64_t)t * nb + b) * NQD;
#pragma unroll
    for (int i = 0; i < NQD; ++i) dst[i] = q[i];
  }
}

__global__ __launch_bounds__(NT) void diversity_fold_kernel(const double* __restrict__ part, int nb, int64_t plane,
                                                            int have_mask, double* __restrict__ out) {
  __shared__ double red[NQD * NT];
  const double* src = part + (int64_t)blockIdx.x * nb * NQD;
  double q[NQD] = {0.0, 0.0, 0.0, 0.0};
  for (int j = threadIdx.x; j < nb; j += NT) {
#pragma unroll
    for (int i = 0; i < NQD; ++i) q[i] += src[(int64_t)j * NQD + i];
  }
  block_fold<NQD>(q, red);
  if (threadIdx.x == 0) {
    double* o = out + (int64_t)blockIdx.x * GCD_METRICS_DIVERSITY_VALUES;
    const double n_vis = q[3], n_occ = (double)plane - q[3];
    o[0] = q[0] / (double)plane;
    o[1] = !have_mask ? 0.0 : n_vis > 0.0 ? q[1] / n_vis : nan("");
    o[2] = !have_mask ? 0.0 : n_occ > 0.0 ? q[2] / n_occ : nan("");
  }
}

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

inline int diversity_blocks(int64_t plane) {
  const int64_t nb = cdiv(plane, (int64_t)NT * DIV_PIX_PER_THREAD);
  return (int)(nb > DIV_MAX_BLOCKS ? DIV_MAX_BLOCKS : nb);
}

// The sizes both entries accept; 0 when fine.
int check_sizes(const char* who, int S, int T, int H, int W) {
  GCD_CHECK_ARG(S >= 1 && T >= 1, "%s: empty problem (S=%d T=%d)", who, S, T);
  GCD_CHECK_ARG(H >= WIN && W >= WIN, "%s: H=%d W=%d: the 7x7 window needs at least 7 x 7 pixels", who, H, W);
  const int64_t plane = (int64_t)H * W;
  GCD_CHECK_ARG(plane <= (INT64_MAX / 16) / 3 / T / S, "%s: S=%d x T=%d x 3 x H=%d x W=%d overflows", who, S, T, H, W);
  const int64_t tiles = cdiv(H, TH) * cdiv(W, TW);
  GCD_CHECK_ARG(tiles <= (int64_t)INT32_MAX / T / S, "%s: S=%d x T=%d x %lld tiles exceed the grid limit", who, S, T,
                (long long)tiles);
  return 0;
}

int launch_status(const char* who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    gcd_set_error("%s: launch failed: %s", who, hipGetErrorString(e));
    return 1;
  }
  return 0;
}

}  // namespace

extern "C" int64_t gcd_metrics_frames_scratch_bytes(int S, int T, int H, int W) {
  if (check_sizes("gcd_metrics_frames_scratch_bytes", S, T, H, W)) return 0;
  return (int64_t)S * T * cdiv(H, TH) * cdiv(W, TW) * NQ * (int64_t)sizeof(double);
}

extern "C" int64_t gcd_metrics_diversity_scratch_bytes(int S, int T, int H, int W) {
  if (check_sizes("gcd_metrics_diversity_scratch_bytes", S, T, H, W)) return 0;
  return (int64_t)T * diversity_blocks((int64_t)H * W) * NQD * (int64_t)sizeof(double);
}

extern "C" int gcd_metrics_frames_f32(const float* pred, const float* gt, const float* reproject, int S, int T, int H, int W,
                                      int flags, void* scratch, int64_t scratch_bytes, double* out, void* stream) {
  const char* who = "gcd_metrics_frames_f32";
  GCD_CHECK_ARG(pred && gt && out, "%s: null pointer (pred, gt and out are required)", who);
  if (const int rc = check_sizes(who, S, T, H, W)) return rc;
  GCD_CHECK_ARG((flags & ~GCD_METRICS_SIGNED) == 0, "%s: unknown flags 0x%x", who, flags);
  const int64_t need = gcd_metrics_frames_scratch_bytes(S, T, H, W);
  GCD_CHECK_ARG(scratch && scratch_bytes >= need, "%s: scratch too small: %lld bytes given, %lld needed", who,
                (long long)(scratch ? scratch_bytes : 0), (long long)need);
  GCD_CHECK_ARG(((uintptr_t)scratch & 7u) == 0, "%s: scratch must be 8-byte aligned", who);
  const int tiles_x = (int)cdiv(W, TW), tiles_y = (int)cdiv(H, TH);
  const int64_t tiles = (int64_t)tiles_x * tiles_y;
  hipLaunchKernelGGL(metrics_tile_kernel, dim3((unsigned)(tiles * T * S)), dim3(NT), 0, (hipStream_t)stream, pred, gt,
                     reproject, T, H, W, tiles_x, tiles_y, flags & GCD_METRICS_SIGNED, (double*)scratch);
  if (const int rc = launch_status(who)) return rc;
  hipLaunchKernelGGL(metrics_fold_kernel, dim3((unsigned)(S * T)), dim3(NT), 0, (hipStream_t)stream,
                     (const double*)scratch, tiles, H, W, reproject ? 1 : 0, out);
  return launch_status(who);
}

extern "C" int gcd_metrics_diversity_f32(const float* pred, const float* reproject, int S, int T, int H, int W, int flags,
                                         float* uncertainty, void* scratch, int64_t scratch_bytes, double* out,
                                         void* stream) {
  const char* who = "gcd_metrics_diversity_f32";
  GCD_CHECK_ARG(pred && uncertainty && out, "%s: null pointer (pred, uncertainty and out are required)", who);
  if (const int rc = check_sizes(who, S, T, H, W)) return rc;
  GCD_CHECK_ARG((flags & ~GCD_METRICS_SIGNED) == 0, "%s: unknown flags 0x%x", who, flags);
  const int64_t need = gcd_metrics_diversity_scratch_bytes(S, T, H, W);
  GCD_CHECK_ARG(scratch && scratch_bytes >= need, "%s: scratch too small: %lld bytes given, %lld needed", who,
                (long long)(scratch ? scratch_bytes : 0), (long long)need);
  GCD_CHECK_ARG(((uintptr_t)scratch & 7u) == 0, "%s: scratch must be 8-byte aligned", who);
  const int64_t plane = (int64_t)H * W;
  const int nb = diversity_blocks(plane);
  hipLaunchKernelGGL(diversity_kernel, dim3((unsigned)((int64_t)T * nb)), dim3(NT), 0, (hipStream_t)stream, pred, reproject,
                     S, T, plane, nb, flags & GCD_METRICS_SIGNED, uncertainty, (double*)scratch);
  if (const int rc = launch_status(who)) return rc;
  hipLaunchKernelGGL(diversity_fold_kernel, dim3((unsigned)T), dim3(NT), 0, (hipStream_t)stream, (const double*)scratch, nb,
                     plane, reproject ? 1 : 0, out);
  return launch_status(who);
}
