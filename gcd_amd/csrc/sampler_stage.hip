// sampler_stage.hip — libgcd_amd_sampler.so: the elementwise update of one sampler stage.  C ABI: include/gcd_amd_sampler.h.
//
// Every x-update of the EDM sampler family (Euler with churn, Heun, Euler ancestral, DPM++ 2S ancestral, DPM++ 2M) is a
// linear combination of at most five tensors — the state, the guided denoiser output, two history buffers and a noise
// tensor — whose coefficients depend on the sigma schedule only.  This kernel evaluates one row of such a table
// (gcd_amd/sampler_stages.py) that it reads from DEVICE memory, so that one captured launch with fixed pointers serves
// every stage of every sampler: the hipGraph of FusedStageLoop (gcd_amd/sampling.py) is a linear chain that only differs
// by the 12 floats copied into `coef` before each replay.
//
// HBM-trivial (at most 9 streams of 2 MB at 14 x 72 x 128): plain vector loads and stores, no LDS, no atomics.  A term
// whose coefficient is exactly 0.0f is not loaded and a store whose pair is (0, 0) is not made — uniform branches on the
// row: the first DPM++ 2M step reads no history that does not exist yet (0 * NaN would poison the result), and a stage
// that keeps no history leaves the buffers of the stage before it alone.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gcd_amd_sampler.h"

static thread_local char g_err[512] = "";
static void gcd_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* gcd_sampler_last_error(void) { return g_err; }
extern "C" int gcd_sampler_abi_version(void) { return GCD_AMD_SAMPLER_ABI_VERSION; }

#define GCD_CHECK_ARG(cond, ...)  \
  do {                            \
    if (!(cond)) {                \
      gcd_set_error(__VA_ARGS__); \
      return 2;                   \
    }                             \
  } while (0)

namespace {

// The row, as every thread reads it (uniform: scalar loads), with the derived switches.
struct StageRow {
  float c_skip, c_out;
  float a_cur, a_den, a_h0, a_h1, a_noise, s0_cur, s0_den, s1_cur, s1_den;
  bool need_d, need_cur, st0, st1;
};

__device__ __forceinline__ StageRow load_row(const float* __restrict__ coef, const float* h0, const float* h1,
                                             const float* noise) {
  StageRow r;
  const float sigma = coef[0];
  const float s2 = sigma * sigma + 1.0f;
  r.c_skip = 1.0f / s2;                  // as cfg_euler_kernel (elementwise.hip)
  r.c_out = -sigma / sqrtf(s2);
  r.a_cur = coef[1], r.a_den = coef[2];
  r.a_h0 = h0 ? coef[3] : 0.0f;          // a null optional operand drops its term: never dereferenced
  r.a_h1 = h1 ? coef[4] : 0.0f;
  r.a_noise = noise ? coef[5] : 0.0f;
  r.s0_cur = coef[6], r.s0_den = coef[7], r.s1_cur = coef[8], r.s1_den = coef[9];
  r.st0 = h0 && (r.s0_cur != 0.0f || r.s0_den != 0.0f);
  r.st1 = h1 && (r.s1_cur != 0.0f || r.s1_den != 0.0f);
  r.need_d = r.a_den != 0.0f || (r.st0 && r.s0_den != 0.0f) || (r.st1 && r.s1_den != 0.0f);
  r.need_cur = r.need_d || r.a_cur != 0.0f || (r.st0 && r.s0_cur != 0.0f) || (r.st1 && r.s1_cur != 0.0f);
  return r;
}

// One element.  Operands of switched-off terms arrive as 0.0f and are not used.
__device__ __forceinline__ void stage_elem(const StageRow& r, float sc, float xv, float nu, float nc, float h0v, float h1v,
                                           float nz, float& out, float& o0, float& o1) {
  float den = 0.0f;
  if (r.need_d) {
    const float du = nu * r.c_out + xv * r.c_skip;
    const float dc = nc * r.c_out + xv * r.c_skip;
    den = du + sc * (dc - du);
  }
  float acc = 0.0f;
  if (r.a_cur != 0.0f) acc = r.a_cur * xv;
  if (r.a_den != 0.0f) acc += r.a_den * den;
  if (r.a_h0 != 0.0f) acc += r.a_h0 * h0v;
  if (r.a_h1 != 0.0f) acc += r.a_h1 * h1v;
  if (r.a_noise != 0.0f) acc += r.a_noise * nz;
  out = acc;
  o0 = 0.0f, o1 = 0.0f;
  if (r.st0) {
    if (r.s0_cur != 0.0f) o0 = r.s0_cur * xv;
    if (r.s0_den != 0.0f) o0 += r.s0_den * den;
  }
  if (r.st1) {
    if (r.s1_cur != 0.0f) o1 = r.s1_cur * xv;
    if (r.s1_den != 0.0f) o1 += r.s1_den * den;
  }
}

// chw % 4 == 0 and every base 16-byte aligned: a float4 never straddles two frames.
__global__ __launch_bounds__(256) void sampler_stage_vec_kernel(float* cur, const float* __restrict__ net,
                                                                const float* __restrict__ scale,
                                                                const float* __restrict__ coef, float* h0, float* h1,
                                                                const float* __restrict__ noise, int nx, int T,
                                                                int64_t chw) {
  const StageRow r = load_row(coef, h0, h1, noise);
  const int64_t total = (int64_t)nx * chw;
  const int64_t total4 = total >> 2;
  const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  for (int64_t i4 = (int64_t)blockIdx.x * 256 + threadIdx.x; i4 < total4; i4 += (int64_t)gridDim.x * 256) {
    const int64_t idx = i4 << 2;
    const int n = (int)(idx / chw);
    const float sc = r.need_d ? scale[n % T] : 0.0f;
    const float4 xv = r.need_cur ? *(const float4*)(cur + idx) : zero;
    const float4 nu = r.need_d ? *(const float4*)(net + idx) : zero;
    const float4 nc = r.need_d ? *(const float4*)(net + idx + total) : zero;
    const float4 a = r.a_h0 != 0.0f ? *(const float4*)(h0 + idx) : zero;
    const float4 b = r.a_h1 != 0.0f ? *(const float4*)(h1 + idx) : zero;
    const float4 z = r.a_noise != 0.0f ? *(const float4*)(noise + idx) : zero;
    float4 o, o0, o1;
    stage_elem(r, sc, xv.x, nu.x, nc.x, a.x, b.x, z.x, o.x, o0.x, o1.x);
    stage_elem(r, sc, xv.y, nu.y, nc.y, a.y, b.y, z.y, o.y, o0.y, o1.y);
    stage_elem(r, sc, xv.z, nu.z, nc.z, a.z, b.z, z.z, o.z, o0.z, o1.z);
    stage_elem(r, sc, xv.w, nu.w, nc.w, a.w, b.w, z.w, o.w, o0.w, o1.w);
    if (r.st0) *(float4*)(h0 + idx) = o0;
    if (r.st1) *(float4*)(h1 + idx) = o1;
    *(float4*)(cur + idx) = o;
  }
}

__global__ __launch_bounds__(256) void sampler_stage_scalar_kernel(float* cur, const float* __restrict__ net,
                                                                   const float* __restrict__ scale,
                                                                   const float* __restrict__ coef, float* h0, float* h1,
                                                                   const float* __restrict__ noise, int nx, int T,
                                                                   int64_t chw) {
  const StageRow r = load_row(coef, h0, h1, noise);
  const int64_t total = (int64_t)nx * chw;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int n = (int)(idx / chw);
    const float sc = r.need_d ? scale[n % T] : 0.0f;
    const float xv = r.need_cur ? cur[idx] : 0.0f;
    const float nu = r.need_d ? net[idx] : 0.0f;
    const float nc = r.need_d ? net[idx + total] : 0.0f;
    const float a = r.a_h0 != 0.0f ? h0[idx] : 0.0f;
    const float b = r.a_h1 != 0.0f ? h1[idx] : 0.0f;
    const float z = r.a_noise != 0.0f ? noise[idx] : 0.0f;
    float o, o0, o1;
    stage_elem(r, sc, xv, nu, nc, a, b, z, o, o0, o1);
    if (r.st0) h0[idx] = o0;
    if (r.st1) h1[idx] = o1;
    cur[idx] = o;
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }   // null counts as aligned

}  // namespace

extern "C" int gcd_sampler_stage_f32(float* cur, const float* net, const float* scale, const float* coef, float* h0,
                                     float* h1, const float* noise, int nx, int T, int64_t chw, void* stream) {
  GCD_CHECK_ARG(cur && net && scale && coef, "gcd_sampler_stage_f32: null pointer (cur, net, scale and coef are required)");
  GCD_CHECK_ARG(nx > 0 && T > 0 && chw > 0, "gcd_sampler_stage_f32: empty problem (nx=%d T=%d chw=%lld)", nx, T,
                (long long)chw);
  GCD_CHECK_ARG(chw <= (INT64_MAX / 2) / nx, "gcd_sampler_stage_f32: nx=%d x chw=%lld overflows", nx, (long long)chw);
  const int64_t total = (int64_t)nx * chw;
  const bool vec = chw % 4 == 0 && aligned16(cur) && aligned16(net) && aligned16(h0) && aligned16(h1) && aligned16(noise);
  int64_t blocks = ((vec ? total / 4 : total) + 255) / 256;
  if (blocks > 4096) blocks = 4096;      // the cap of gcd_cfg_euler_step; the stride loop covers the rest
  if (vec)
    hipLaunchKernelGGL(sampler_stage_vec_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, cur, net, scale,
                       coef, h0, h1, noise, nx, T, chw);
  else
    hipLaunchKernelGGL(sampler_stage_scalar_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, cur, net,
                       scale, coef, h0, h1, noise, nx, T, chw);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    gcd_set_error("gcd_sampler_stage_f32: launch failed: %s", hipGetErrorString(e));
    return 1;
  }
  return 0;
}
