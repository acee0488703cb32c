// libgcd_amd_loss.so (include/gcd_amd_loss.h): the fine-tune loss on the device.
//
// class_map_kernel     One workgroup per (frame, latent row): it walks the source rows of that row's bins once, in
//                      coalesced order, tests every pixel against the class colours, and counts the matches per (bin,
//                      class) with integer LDS atomics — a pixel of a non-multiple size lies in up to two bins along each
//                      axis.  The map value is then formed from the integer counts in torch's order of operations.
// focal_fwd_kernel     One workgroup of 1024 threads per frame.  Pass 1 forms `all` per element, accumulates sum(all) and
//                      sum(raw wmap) in fp64 and histograms the top 11 bits of the bit patterns; two more passes refine the
//                      keep-th largest value to all of its 31 bits (all >= +0: unsigned bit order is value order); a fourth
//                      sums the values above it.  Elements are re-read (a frame is tens of kilobytes: the cache holds it)
//                      and re-formed, never stored.  fp64 sums: per thread in index order, a fixed butterfly in the wave,
//                      the 16 waves in order.
// focal_bwd_kernel     One workgroup per frame, chunks of 1024 consecutive elements in order: the rank of a tied element
//                      among the ties (ballot + the waves' counts + the running count of the earlier chunks) decides
//                      whether it is one of the `quota` selected ones.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gcd_amd_loss.h"

static thread_local char g_err[512] = "";
static void gcd_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* gcd_loss_last_error(void) { return g_err; }
extern "C" int gcd_loss_abi_version(void) { return GCD_AMD_LOSS_ABI_VERSION; }

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

constexpr int MAP_NT = 256;
constexpr int NT = 1024;               // focal kernels: one workgroup per frame
constexpr int WAVES = NT / 64;
constexpr int BINS = 2048;             // 11 bits per radix pass; two bins per thread
static_assert(BINS == 2 * NT, "select_bin gives every thread two bins");

// -ffp-contract=fast fuses a multiply into the add that uses it whatever the source says; a product that torch rounds on
// its own goes through an empty asm statement, which the combiner cannot see through.
__device__ __forceinline__ float rounded(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

// ------------------------------------------------------------------------------------------------------- class map
struct ClassTable {                    // a kernel argument (not part of the ABI: the entry takes a plain float array)
  float v[GCD_LOSS_MAX_CLASSES][4];    // r, g, b, weight - 1
};

__device__ __forceinline__ int bin_start(int i, int in, int out) { return (int)(((int64_t)i * in) / out); }
__device__ __forceinline__ int bin_end(int i, int in, int out) { return (int)((((int64_t)i + 1) * in + out - 1) / out); }

__global__ __launch_bounds__(MAP_NT) void class_map_kernel(const float* __restrict__ gt, int Hp, int Wp, ClassTable tab, int ncls,
                                                           float* __restrict__ wmap, int Hl, int Wl) {
  __shared__ int cnt[GCD_LOSS_MAX_MAP_W * GCD_LOSS_MAX_CLASSES];
  const int i = blockIdx.x, f = blockIdx.y;
  for (int k = threadIdx.x; k < Wl * GCD_LOSS_MAX_CLASSES; k += MAP_NT) cnt[k] = 0;
  __syncthreads();
  const int r0 = bin_start(i, Hp, Hl), r1 = bin_end(i, Hp, Hl);
  const int64_t plane = (int64_t)Hp * Wp;
  const float* src = gt + (int64_t)f * 3 * plane + (int64_t)r0 * Wp;
  const int items = (r1 - r0) * Wp;          // the strip's rows are consecutive in memory: item = (row - r0) * Wp + x
  for (int it = threadIdx.x; it < items; it += MAP_NT) {
    const float a = src[it], b = src[plane + it], c = src[2 * plane + it];
    unsigned mask = 0;
    for (int k = 0; k < ncls; ++k) {
      const float s = (fabsf(a - tab.v[k][0]) + fabsf(b - tab.v[k][1])) + fabsf(c - tab.v[k][2]);
      mask |= (__fdiv_rn(s, 3.f) < 0.02f ? 1u : 0u) << k;
    }
    if (mask) {
      const int x = it % Wp;
      const int j0 = (int)(((int64_t)x * Wl) / Wp);          // start(j0) <= x < end(j0); j0 + 1 is the one other candidate
      for (int j = j0; j <= j0 + 1 && j < Wl; ++j) {
        if (x < bin_start(j, Wp, Wl) || x >= bin_end(j, Wp, Wl)) continue;
        for (unsigned m = mask; m; m &= m - 1) atomicAdd(&cnt[j * GCD_LOSS_MAX_CLASSES + (__ffs(m) - 1)], 1);
      }
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < Wl; j += MAP_NT) {
    const float pixels = (float)((r1 - r0) * (bin_end(j, Wp, Wl) - bin_start(j, Wp, Wl)));
    float acc = 0.f;
    for (int k = 0; k < ncls; ++k) {
      const float frac = __fdiv_rn((float)cnt[j * GCD_LOSS_MAX_CLASSES + k], pixels);
      acc += rounded(frac * tab.v[k][3]);
    }
    wmap[((int64_t)f * Hl + i) * Wl + j] = acc;
  }
}

// ------------------------------------------------------------------------------------------------------ focal loss
struct Elem {
  float diff, wm, rb, all;
};

__device__ __forceinline__ Elem load_elem(const float* __restrict__ out, const float* __restrict__ tgt,
                                          const float* __restrict__ wmap, int e, int HW, int l1) {
  Elem r;
  r.diff = out[e] - tgt[e];
  const float raw = l1 ? fabsf(r.diff) : r.diff * r.diff;
  r.wm = wmap ? wmap[e % HW] : 0.f;
  r.rb = rounded(raw * r.wm);
  r.all = raw + 0.5f * r.rb;           // (0.5 rb is exact: fused or not, one rounding)
  return r;
}

__device__ __forceinline__ unsigned key_of(float all) { return __float_as_uint(all) & 0x7fffffffu; }

// sum over the workgroup, the same order every time: the wave's butterfly, then the waves in order.  Every thread gets it.
__device__ double block_sum(double v, double* red) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  __syncthreads();                     // (red may still be read from an earlier call)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int i = 1; i < WAVES; ++i) s += red[i];
  return s;
}

// hist holds the counts of BINS bins whose total is >= k >= 1.  Finds the bin of the k-th largest element (higher bin =
// larger value): sel = {bin, k - #elements in higher bins, count of the bin}; clears hist for the next pass.
__device__ void select_bin(int* hist, int* wtot, int* sel, int k) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int h0 = hist[2 * t], h1 = hist[2 * t + 1], s = h0 + h1;
  hist[2 * t] = 0;
  hist[2 * t + 1] = 0;
  int incl = s;                        // inclusive suffix sum over the lanes of the wave
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int v = __shfl_down(incl, d, 64);
    if (lane + d < 64) incl += v;
  }
  if (lane == 0) wtot[wave] = incl;
  __syncthreads();
  int above = incl - s;                // elements in the bins above this thread's pair
  for (int w2 = wave + 1; w2 < WAVES; ++w2) above += wtot[w2];
  if (above < k && k <= above + h1) {
    sel[0] = 2 * t + 1, sel[1] = k - above, sel[2] = h1;
  } else if (above + h1 < k && k <= above + s) {
    sel[0] = 2 * t, sel[1] = k - above - h1, sel[2] = h0;
  }
  __syncthreads();
}

__global__ __launch_bounds__(NT) void focal_fwd_kernel(const float* __restrict__ out, const float* __restrict__ tgt,
                                                       const float* __restrict__ w, const float* __restrict__ wmap, int n, int HW,
                                                       int l1, int keep, float* __restrict__ loss, int32_t* __restrict__ state) {
  __shared__ int hist[BINS];
  __shared__ int wtot[WAVES];
  __shared__ int sel[3];
  __shared__ double red[WAVES];
  const int f = blockIdx.x, t = threadIdx.x;
  out += (int64_t)f * n;
  tgt += (int64_t)f * n;
  if (wmap) wmap += (int64_t)f * HW;
  hist[2 * t] = 0;
  hist[2 * t + 1] = 0;
  __syncthreads();

  double s_all = 0.0, s_rb = 0.0;
  for (int e = t; e < n; e += NT) {
    const Elem v = load_elem(out, tgt, wmap, e, HW, l1);
    s_all += (double)v.all;
    s_rb += (double)v.rb;
    if (keep > 0) atomicAdd(&hist[key_of(v.all) >> 20], 1);
  }
  s_all = block_sum(s_all, red);
  s_rb = block_sum(s_rb, red);         // (its barriers also order the histogram before select_bin)
  const double mean_all = s_all / (double)n, bias_mean = s_rb / (double)n;
  if (keep <= 0) {
    if (t == 0) {
      loss[f] = (float)((mean_all + 0.5 * bias_mean) * (double)w[f]);
      state[2 * f] = 0;
      state[2 * f + 1] = 0;
    }
    return;
  }

  select_bin(hist, wtot, sel, keep);
  const unsigned p1 = (unsigned)sel[0];
  int k = sel[1];
  __syncthreads();                     // sel is read by everyone before the next pass overwrites it
  for (int e = t; e < n; e += NT) {
    const unsigned key = key_of(load_elem(out, tgt, wmap, e, HW, l1).all);
    if ((key >> 20) == p1) atomicAdd(&hist[(key >> 9) & 2047u], 1);
  }
  __syncthreads();
  select_bin(hist, wtot, sel, k);
  const unsigned p2 = (p1 << 11) | (unsigned)sel[0];
  k = sel[1];
  __syncthreads();
  for (int e = t; e < n; e += NT) {
    const unsigned key = key_of(load_elem(out, tgt, wmap, e, HW, l1).all);
    if ((key >> 9) == p2) atomicAdd(&hist[key & 511u], 1);
  }
  __syncthreads();
  select_bin(hist, wtot, sel, k);
  const unsigned tau = (p2 << 9) | (unsigned)sel[0];
  const int quota = sel[1];

  double s_top = 0.0;
  for (int e = t; e < n; e += NT) {
    const float all = load_elem(out, tgt, wmap, e, HW, l1).all;
    if (key_of(all) > tau) s_top += (double)all;
  }
  s_top = block_sum(s_top, red);
  if (t == 0) {
    const double top_mean = (s_top + (double)quota * (double)__uint_as_float(tau)) / (double)keep;
    loss[f] = (float)((0.9 * top_mean + 0.1 * mean_all + 0.5 * bias_mean) * (double)w[f]);
    state[2 * f] = (int32_t)tau;
    state[2 * f + 1] = quota;
  }
}

__global__ __launch_bounds__(NT) void focal_bwd_kernel(const float* __restrict__ out, const float* __restrict__ tgt,
                                                       const float* __restrict__ w, const float* __restrict__ wmap,
                                                       const float* __restrict__ g, const int32_t* __restrict__ state, int n, int HW,
                                                       int l1, int keep, float* __restrict__ dout) {
  __shared__ int wcnt[2][WAVES];
  const int f = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  out += (int64_t)f * n;
  tgt += (int64_t)f * n;
  dout += (int64_t)f * n;
  if (wmap) wmap += (int64_t)f * HW;
  const unsigned tau = (unsigned)state[2 * f];
  const int quota = state[2 * f + 1];
  const double gw = (double)g[f] * (double)w[f], inv_n = 1.0 / (double)n;
  const double c_rest = keep > 0 ? 0.1 * inv_n : inv_n;
  const double c_sel = keep > 0 ? 0.9 / (double)keep + c_rest : c_rest;
  int base = 0;                        // ties among the elements of the earlier chunks
  for (int c0 = 0, it = 0; c0 < n; c0 += NT, ++it) {
    const int e = c0 + t;
    const bool valid = e < n;
    Elem v = {0.f, 0.f, 0.f, 0.f};
    if (valid) v = load_elem(out, tgt, wmap, e, HW, l1);
    const unsigned key = key_of(v.all);
    bool selected = false;
    if (keep > 0) {                    // (uniform)
      const bool tie = valid && key == tau;
      const unsigned long long ballot = __ballot(tie);
      if (lane == 0) wcnt[it & 1][wave] = __popcll(ballot);
      __syncthreads();                 // (two buffers: the next chunk's stores cannot pass this chunk's loads)
      int before = base, total = 0;
      for (int w2 = 0; w2 < WAVES; ++w2) {
        const int c = wcnt[it & 1][w2];
        before += w2 < wave ? c : 0;
        total += c;
      }
      const int rank = before + __popcll(ballot & ((1ull << lane) - 1ull));
      selected = key > tau || (tie && rank < quota);
      base += total;
    }
    if (valid) {
      const double wm = (double)v.wm;
      const double coef = (selected ? c_sel : c_rest) * (1.0 + 0.5 * wm) + 0.5 * wm * inv_n;
      const double diff = (double)out[e] - (double)tgt[e];
      const double draw = l1 ? (diff > 0.0 ? 1.0 : diff < 0.0 ? -1.0 : diff) : 2.0 * diff;
      dout[e] = (float)(gw * coef * draw);
    }
  }
}

int check_focal(const char* who, const void* out, const void* tgt, const void* w, int BT, int n, int HW, int loss_type, int keep) {
  GCD_CHECK_ARG(out && tgt && w, "%s: null operand", who);
  GCD_CHECK_ARG(BT > 0 && BT <= GCD_LOSS_MAX_BT, "%s: BT=%d outside [1, %d]", who, BT, GCD_LOSS_MAX_BT);
  GCD_CHECK_ARG(n > 0 && n <= GCD_LOSS_MAX_N, "%s: n=%d outside [1, %d]", who, n, GCD_LOSS_MAX_N);
  GCD_CHECK_ARG(HW > 0 && n % HW == 0, "%s: HW=%d must divide n=%d", who, HW, n);
  GCD_CHECK_ARG(loss_type == GCD_LOSS_L2 || loss_type == GCD_LOSS_L1, "%s: loss_type=%d is neither GCD_LOSS_L2 nor GCD_LOSS_L1", who,
                loss_type);
  GCD_CHECK_ARG(keep >= 0 && keep <= n, "%s: keep=%d outside [0, n=%d]", who, keep, n);
  return 0;
}

}  // namespace

extern "C" int gcd_loss_class_map(const float* gt_rgb, int BT, int Hp, int Wp, const float* classes, int ncls, float* wmap,
                                  int Hl, int Wl, void* stream) {
  GCD_CHECK_ARG(gt_rgb && classes && wmap, "gcd_loss_class_map: null operand");
  GCD_CHECK_ARG(BT > 0 && BT <= GCD_LOSS_MAX_BT, "gcd_loss_class_map: BT=%d outside [1, %d]", BT, GCD_LOSS_MAX_BT);
  GCD_CHECK_ARG(ncls >= 1 && ncls <= GCD_LOSS_MAX_CLASSES, "gcd_loss_class_map: ncls=%d outside [1, %d]", ncls, GCD_LOSS_MAX_CLASSES);
  GCD_CHECK_ARG(Hl >= 1 && Wl >= 1 && Hl <= Hp && Wl <= Wp, "gcd_loss_class_map: a %dx%d map of %dx%d frames (the map is no larger)",
                Hl, Wl, Hp, Wp);
  GCD_CHECK_ARG(Wl <= GCD_LOSS_MAX_MAP_W, "gcd_loss_class_map: Wl=%d is more than %d", Wl, GCD_LOSS_MAX_MAP_W);
  GCD_CHECK_ARG((int64_t)Hp * Wp < (1ll << 31) / 3, "gcd_loss_class_map: %dx%d frames are too large", Hp, Wp);
  ClassTable tab;
  for (int k = 0; k < GCD_LOSS_MAX_CLASSES; ++k)
    for (int c = 0; c < 4; ++c) tab.v[k][c] = k < ncls ? classes[4 * k + c] : 0.f;
  hipLaunchKernelGGL(class_map_kernel, dim3((unsigned)Hl, (unsigned)BT), dim3(MAP_NT), 0, (hipStream_t)stream, gt_rgb, Hp, Wp, tab,
                     ncls, wmap, Hl, Wl);
  GCD_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int gcd_loss_focal_fwd(const float* out, const float* tgt, const float* w, const float* wmap, int BT, int n, int HW,
                                  int loss_type, int keep, float* loss, int32_t* state, void* stream) {
  if (int rc = check_focal("gcd_loss_focal_fwd", out, tgt, w, BT, n, HW, loss_type, keep)) return rc;
  GCD_CHECK_ARG(loss && state, "gcd_loss_focal_fwd: null loss / state");
  hipLaunchKernelGGL(focal_fwd_kernel, dim3((unsigned)BT), dim3(NT), 0, (hipStream_t)stream, out, tgt, w, wmap, n, HW,
                     loss_type == GCD_LOSS_L1, keep, loss, state);
  GCD_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int gcd_loss_focal_bwd(const float* out, const float* tgt, const float* w, const float* wmap, const float* g,
                                  const int32_t* state, int BT, int n, int HW, int loss_type, int keep, float* dout, void* stream) {
  if (int rc = check_focal("gcd_loss_focal_bwd", out, tgt, w, BT, n, HW, loss_type, keep)) return rc;
  GCD_CHECK_ARG(g && state && dout, "gcd_loss_focal_bwd: null g / state / dout");
  GCD_CHECK_ARG(dout != out && dout != tgt, "gcd_loss_focal_bwd: dout must not alias out or tgt");
  hipLaunchKernelGGL(focal_bwd_kernel, dim3((unsigned)BT), dim3(NT), 0, (hipStream_t)stream, out, tgt, w, wmap, g, state, n, HW,
                     loss_type == GCD_LOSS_L1, keep, dout);
  GCD_CHECK_HIP(hipGetLastError());
  return 0;
}
