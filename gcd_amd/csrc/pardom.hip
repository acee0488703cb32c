// libgcd_amd_pardom.so (include/gcd_amd_pardom.h): the colours of a ParallelDomain point cloud.
//
// status_kernel        One thread: the counter of out-of-range ids starts at 0 (the only work of a call with N == 0).
// colours_kernel       One pass.  A workgroup of 256 threads owns 1024 consecutive points and walks their 3072 output
//                      values in order, thread t taking values t, t + 256, ...: a wave's 64 stores are 512 consecutive
//                      bytes of `out` when out_ld == 3 (a thread per point would store 8 bytes every 24), its colour loads
//                      64 consecutive bytes, and the three lanes of a point read the same id byte.  The palette is staged
//                      in LDS (6 KB) once per workgroup.  Points are indexed in int64 from the workgroup's first point;
//                      the division by 3 is of a number below 3072.  Out-of-range ids are counted with an integer LDS
//                      atomic per workgroup and one integer global atomic per workgroup that found any.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gcd_amd_pardom.h"

static thread_local char g_err[512] = "";
static void gcd_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* gcd_pardom_last_error(void) { return g_err; }
extern "C" int gcd_pardom_abi_version(void) { return GCD_AMD_PARDOM_ABI_VERSION; }

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
constexpr int POINTS = 1024;                 // per workgroup
constexpr int VALUES = 3 * POINTS;
constexpr int PALETTE_VALUES = 3 * GCD_PARDOM_PALETTE_ROWS;
static_assert(VALUES % NT == 0, "every thread takes the same number of values");

// -ffp-contract=fast fuses a multiply into the add that uses it whatever the source says; a product that torch rounds on
// its own goes through an empty asm statement, which the combiner cannot see through.
__device__ __forceinline__ float rounded(float v) {
  asm volatile("" : "+v"(v));
  return v;
}
__device__ __forceinline__ double rounded(double v) {
  asm volatile("" : "+v"(v));
  return v;
}

__global__ void status_kernel(int64_t* __restrict__ status) { *status = 0; }

template <int MODE>
__global__ __launch_bounds__(NT) void colours_kernel(const uint8_t* __restrict__ ids, int64_t ids_ld,
                                                     const uint8_t* __restrict__ rgb, int64_t rgb_ld, int64_t N,
                                                     const double* __restrict__ palette, int n_classes, double alpha,
                                                     float one_minus_alpha, double* __restrict__ out, int64_t out_ld,
                                                     unsigned long long* __restrict__ status) {
  __shared__ double pal[PALETTE_VALUES];
  __shared__ unsigned int bad;
  if (MODE != GCD_PARDOM_RGB) {
    for (int k = threadIdx.x; k < PALETTE_VALUES; k += NT) pal[k] = palette[k];
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
  }
  const int64_t p0 = (int64_t)blockIdx.x * POINTS;
  const int64_t left = N - p0;
  const int values = left < POINTS ? (int)left * 3 : VALUES;
  unsigned int mine = 0;
  for (int e = threadIdx.x; e < values; e += NT) {
    const int lp = e / 3, ch = e - 3 * lp;
    const int64_t p = p0 + lp;
    float c32 = 0.0f;
    double P = 0.0;
    if (MODE != GCD_PARDOM_PALETTE) c32 = (float)rgb[p * rgb_ld + ch] / 255.0f;
    if (MODE != GCD_PARDOM_RGB) {
      const int id = ids[p * ids_ld];
      if (id < n_classes)
        P = pal[3 * id + ch];
      else
        mine += ch == 0;
    }
    double v;
    if (MODE == GCD_PARDOM_RGB)
      v = (double)c32;
    else if (MODE == GCD_PARDOM_PALETTE)
      v = P;
    else
      v = (double)rounded(c32 * one_minus_alpha) + rounded(alpha * P);
    out[p * out_ld + ch] = v;
  }
  if (MODE != GCD_PARDOM_RGB) {
    if (mine) atomicAdd(&bad, mine);
    __syncthreads();
    if (threadIdx.x == 0 && bad) atomicAdd(status, (unsigned long long)bad);
  }
}

}  // namespace

extern "C" int gcd_pardom_colours(const uint8_t* ids, int64_t ids_ld, const uint8_t* rgb, int64_t rgb_ld, int64_t N,
                                  const double* palette, int n_classes, double alpha, int mode, double* out,
                                  int64_t out_ld, int64_t* status, void* stream) {
  const char* who = "gcd_pardom_colours";
  GCD_CHECK_ARG(mode == GCD_PARDOM_RGB || mode == GCD_PARDOM_BLEND || mode == GCD_PARDOM_PALETTE,
                "%s: mode %d is none of RGB (0), BLEND (1), PALETTE (2)", who, mode);
  GCD_CHECK_ARG(N >= 0 && N < ((int64_t)1 << 31), "%s: N = %lld is outside 0 .. 2^31 - 1", who, (long long)N);
  GCD_CHECK_ARG(n_classes >= 1 && n_classes <= GCD_PARDOM_PALETTE_ROWS, "%s: n_classes = %d is outside 1 .. %d", who,
                n_classes, GCD_PARDOM_PALETTE_ROWS);
  GCD_CHECK_ARG(ids_ld >= 1 && ids_ld <= GCD_PARDOM_MAX_LD, "%s: ids_ld = %lld is outside 1 .. %d", who,
                (long long)ids_ld, GCD_PARDOM_MAX_LD);
  GCD_CHECK_ARG(rgb_ld >= 3 && rgb_ld <= GCD_PARDOM_MAX_LD, "%s: rgb_ld = %lld is outside 3 .. %d", who,
                (long long)rgb_ld, GCD_PARDOM_MAX_LD);
  GCD_CHECK_ARG(out_ld >= 3 && out_ld <= GCD_PARDOM_MAX_LD, "%s: out_ld = %lld is outside 3 .. %d", who,
                (long long)out_ld, GCD_PARDOM_MAX_LD);
  GCD_CHECK_ARG(palette != nullptr && ((uintptr_t)palette & 7) == 0, "%s: palette is null or not 8-byte aligned", who);
  GCD_CHECK_ARG(status != nullptr && ((uintptr_t)status & 7) == 0, "%s: status is null or not 8-byte aligned", who);
  if (mode == GCD_PARDOM_BLEND)
    GCD_CHECK_ARG(alpha >= 0.0 && alpha <= 1.0, "%s: alpha = %g is outside [0, 1] (mode BLEND)", who, alpha);
  if (N > 0) {
    GCD_CHECK_ARG(out != nullptr && ((uintptr_t)out & 7) == 0, "%s: out is null or not 8-byte aligned", who);
    GCD_CHECK_ARG(ids != nullptr || mode == GCD_PARDOM_RGB, "%s: ids is null (only mode RGB reads no id)", who);
    GCD_CHECK_ARG(rgb != nullptr || mode == GCD_PARDOM_PALETTE, "%s: rgb is null (only mode PALETTE reads no colour)", who);
  }
  hipStream_t s = (hipStream_t)stream;
  status_kernel<<<1, 1, 0, s>>>(status);
  GCD_CHECK_HIP(hipGetLastError());
  if (N == 0) return 0;
  const unsigned grid = (unsigned)((N + POINTS - 1) / POINTS);
  const float oma = (float)(1.0 - alpha);
  unsigned long long* st = (unsigned long long*)status;
  if (mode == GCD_PARDOM_RGB)
    colours_kernel<GCD_PARDOM_RGB><<<grid, NT, 0, s>>>(ids, ids_ld, rgb, rgb_ld, N, palette, n_classes, alpha, oma, out, out_ld, st);
  else if (mode == GCD_PARDOM_BLEND)
    colours_kernel<GCD_PARDOM_BLEND><<<grid, NT, 0, s>>>(ids, ids_ld, rgb, rgb_ld, N, palette, n_classes, alpha, oma, out, out_ld, st);
  else
    colours_kernel<GCD_PARDOM_PALETTE><<<grid, NT, 0, s>>>(ids, ids_ld, rgb, rgb_ld, N, palette, n_classes, alpha, oma, out, out_ld, st);
  GCD_CHECK_HIP(hipGetLastError());
  return 0;
}
