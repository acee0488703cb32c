// lpips.hip — libgcd_amd_lpips.so: the kernels of the LPIPS metric that libgcd_amd.so does not have.
// C ABI: include/gcd_amd_lpips.h.  All three are memory-bound streamers: every byte is read once, 16 bytes per lane.
//
// gcd_lpips_pack_f16: 8 lanes per pixel, each stores 16 bytes of the pixel's token row; the lane of columns 0..7 reads
// the three planes and evaluates the ScalingLayer, the others store zeros.
//
// gcd_lpips_relu_pool_f16: one thread per (image, 2 x 2 block, 8 channels), over the ceil(H / 2) x ceil(W / 2) grid so
// that the last row / column of an odd map still gets its ReLU.  A thread reads its (up to) four 16-byte vectors, stores
// their ReLU (if asked) and the maximum of the four (if asked, and if the block is whole).  Every element is read and
// written by one thread only, so `full` may be the source.
//
// gcd_lpips_distance: LP = the power of two >= C / 8 lanes hold one pixel's two rows (8 halves per lane and tensor); a
// wave takes 64 / LP pixels at a time.  The two sums of squares are reduced over the LP lanes by xor shuffles, the
// weighted squared difference of the normalised rows is formed directly in fp32 and accumulated per lane over the
// workgroup's pixels; one shuffle + LDS reduction per workgroup at the end, stored to the workgroup's own slot.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gcd_amd_lpips.h"

static thread_local char g_err[512] = "";
static void gcd_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* gcd_lpips_last_error(void) { return g_err; }
extern "C" int gcd_lpips_abi_version(void) { return GCD_AMD_LPIPS_ABI_VERSION; }

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

typedef _Float16 f16;
typedef f16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int NT = 256;
constexpr int WAVES = NT / 64;

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The library is compiled with -ffp-contract=fast: the backend then fuses a multiply into the add or subtract that uses
// it whatever the source says (the __f*_rn wrappers are plain operators, and `#pragma clang fp contract(off)` does not
// reach the instruction selector's own combine).  The two places whose result depends on every operation being rounded
// on its own pass each product through an empty asm statement, which the combiner cannot see through.
__device__ __forceinline__ float rounded(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

// ((x a + b) - shift) / scale, one rounding per operation (the torch chain this restates has no fused multiply-add)
__device__ __forceinline__ float scaling_chain(float x, float a, float b, float shift, float scale) {
  const float t = rounded(x * a);
  const float u = rounded(t + b);
  return __fdiv_rn(u - shift, scale);
}

// a r0 - b r1 with both products rounded before the subtraction: equal operands give exactly 0
__device__ __forceinline__ float diff_of_products(float a, float r0, float b, float r1) {
  const float p = rounded(a * r0);
  const float q = rounded(b * r1);
  return p - q;
}

// ------------------------------------------------------------------------------------------------------------ pack
__global__ __launch_bounds__(NT) void pack_kernel(const float* __restrict__ x, int64_t HW, int64_t total, float a, float b,
                                                  const float* __restrict__ shift, const float* __restrict__ scale,
                                                  f16x8* __restrict__ out, int vecs) {
  // total = n * HW * vecs work items; item = (pixel, vec), vec fastest: a wave stores 1 KB of consecutive bytes
  const int64_t item = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (item >= total) return;
  const int64_t pix = item / vecs;
  const int v = (int)(item - pix * vecs);
  f16x8 r = {0, 0, 0, 0, 0, 0, 0, 0};
  if (v == 0) {
    const int64_t img = pix / HW, p = pix - img * HW;
    const float* src = x + img * GCD_LPIPS_IMAGE_CHANNELS * HW + p;
#pragma unroll
    for (int c = 0; c < GCD_LPIPS_IMAGE_CHANNELS; ++c) {
      r[c] = (f16)scaling_chain(src[c * HW], a, b, shift[c], scale[c]);
    }
  }
  out[item] = r;
}

// ------------------------------------------------------------------------------------------------------- relu / pool
__device__ __forceinline__ f16x8 relu8(f16x8 v) {
  f16x8 r;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float f = (float)v[i];
    r[i] = f > 0.f ? v[i] : (f != f ? v[i] : (f16)0.f);
  }
  return r;
}

__device__ __forceinline__ f16x8 max8(f16x8 m, f16x8 v) {   // NaN wins, as in torch's max_pool2d
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float a = (float)m[i], b = (float)v[i];
    if (b > a || b != b) m[i] = v[i];
  }
  return m;
}

__global__ __launch_bounds__(NT) void relu_pool_kernel(const f16x8* __restrict__ src, f16x8* full, f16x8* __restrict__ pooled,
                                                       int H, int W, int CV, int Hc, int Wc, int64_t total) {
  // (src and full may alias: no __restrict__ on full)
  const int64_t item = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (item >= total) return;
  const int cv = (int)(item % CV);
  int64_t t = item / CV;
  const int xo = (int)(t % Wc);
  t /= Wc;
  const int yo = (int)(t % Hc);
  const int64_t img = t / Hc;
  const int y0 = 2 * yo, x0 = 2 * xo;
  const bool has_y1 = y0 + 1 < H, has_x1 = x0 + 1 < W;
  const int64_t base = ((img * H + y0) * (int64_t)W + x0) * CV + cv;
  const int64_t dy = (int64_t)W * CV;
  f16x8 v00 = relu8(src[base]), v01 = v00, v10 = v00, v11 = v00;
  if (has_x1) v01 = relu8(src[base + CV]);
  if (has_y1) v10 = relu8(src[base + dy]);
  if (has_x1 && has_y1) v11 = relu8(src[base + dy + CV]);
  if (full) {
    full[base] = v00;
    if (has_x1) full[base + CV] = v01;
    if (has_y1) full[base + dy] = v10;
    if (has_x1 && has_y1) full[base + dy + CV] = v11;
  }
  if (pooled && has_x1 && has_y1) {
    const int Ho = H / 2, Wo = W / 2;
    pooled[((img * Ho + yo) * (int64_t)Wo + xo) * CV + cv] = max8(max8(v00, v01), max8(v10, v11));
  }
}

// ---------------------------------------------------------------------------------------------------------- distance
template <int LP>
__global__ __launch_bounds__(NT) void distance_kernel(const f16x8* __restrict__ f0, const f16x8* __restrict__ f1,
                                                      const float* __restrict__ w, int64_t HW, int CV,
                                                      float* __restrict__ partials) {
  constexpr int PPW = 64 / LP;              // pixels per wave and step
  constexpr int PPB = PPW * WAVES;          // pixels per workgroup and step
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane % LP;                // which 8 channels of the row
  const bool live = sub < CV;               // (C / 8 need not be a power of two: the upper lanes of a group hold zeros)
  const int64_t img = blockIdx.y;
  const f16x8* g0 = f0 + img * HW * CV;
  const f16x8* g1 = f1 + img * HW * CV;
  float wc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) wc[i] = live ? w[sub * 8 + i] : 0.f;
  float acc = 0.f;
  const int64_t groups = (HW + PPB - 1) / PPB;
  for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
    const int64_t p = g * PPB + wave * PPW + lane / LP;
    const bool on = live && p < HW;
    f16x8 a = {0, 0, 0, 0, 0, 0, 0, 0}, b = a;
    if (on) {
      a = g0[p * CV + sub];
      b = g1[p * CV + sub];
    }
    float af[8], bf[8], s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      af[i] = (float)a[i];
      bf[i] = (float)b[i];
      s0 = fmaf(af[i], af[i], s0);
      s1 = fmaf(bf[i], bf[i], s1);
    }
#pragma unroll
    for (int m = 1; m < LP; m <<= 1) {      // butterfly: every lane of the group ends with the same bits
      s0 += __shfl_xor(s0, m, 64);
      s1 += __shfl_xor(s1, m, 64);
    }
    const float r0 = __fdiv_rn(1.f, __fadd_rn(__fsqrt_rn(s0), 1e-10f));
    const float r1 = __fdiv_rn(1.f, __fadd_rn(__fsqrt_rn(s1), 1e-10f));
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float e = diff_of_products(af[i], r0, bf[i], r1);
      d = fmaf(e * e, wc[i], d);
    }
    acc += d;                               // (lanes that are off hold zeros: d == 0)
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
  __shared__ float red[WAVES];
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = red[0];
#pragma unroll
    for (int i = 1; i < WAVES; ++i) s += red[i];
    partials[img * gridDim.x + blockIdx.x] = s;
  }
}

__global__ void distance_finish_kernel(const float* __restrict__ partials, int n, int blocks, double count,
                                       double* tap_means, int tap, int taps, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int b = 0; b < blocks; ++b) s += (double)partials[(int64_t)i * blocks + b];
  const double mean = s / count;
  tap_means[(int64_t)tap * n + i] = mean;
  if (out) {
    double total = 0.0;
    for (int t = 0; t < taps; ++t) total += t == tap ? mean : tap_means[(int64_t)t * n + i];
    out[i] = (float)total;
  }
}

}  // namespace

extern "C" int gcd_lpips_pack_f16(const float* x, int n, int H, int W, float a, float b, const float* shift,
                                  const float* scale, void* out16, int cpad, void* stream) {
  GCD_CHECK_ARG(x && shift && scale && out16, "gcd_lpips_pack_f16: null operand");
  GCD_CHECK_ARG(n > 0 && H > 0 && W > 0, "gcd_lpips_pack_f16: empty problem n=%d H=%d W=%d", n, H, W);
  GCD_CHECK_ARG(cpad % 8 == 0 && cpad >= 8 && cpad <= GCD_LPIPS_MAX_C, "gcd_lpips_pack_f16: cpad=%d must be a multiple of 8 in [8, %d]",
                cpad, GCD_LPIPS_MAX_C);
  GCD_CHECK_ARG(aligned16(out16), "gcd_lpips_pack_f16: out16 must be 16-byte aligned");
  const int64_t HW = (int64_t)H * W;
  const int vecs = cpad / 8;
  const int64_t total = (int64_t)n * HW * vecs;
  const int64_t nblk = (total + NT - 1) / NT;
  GCD_CHECK_ARG(nblk < (1ll << 31), "gcd_lpips_pack_f16: %lld work items are more than one launch takes", (long long)total);
  hipLaunchKernelGGL(pack_kernel, dim3((unsigned)nblk), dim3(NT), 0, (hipStream_t)stream, x, HW, total, a, b, shift, scale,
                     (f16x8*)out16, vecs);
  GCD_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int gcd_lpips_relu_pool_f16(const void* src, void* full, void* pooled, int n, int H, int W, int C, void* stream) {
  GCD_CHECK_ARG(src && (full || pooled), "gcd_lpips_relu_pool_f16: null source, or no destination");
  GCD_CHECK_ARG(n > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "gcd_lpips_relu_pool_f16: bad shape n=%d H=%d W=%d C=%d (C %% 8 == 0)",
                n, H, W, C);
  GCD_CHECK_ARG(!pooled || (H >= 2 && W >= 2), "gcd_lpips_relu_pool_f16: a %dx%d map has no 2x2 block to pool", H, W);
  GCD_CHECK_ARG(aligned16(src) && aligned16(full) && aligned16(pooled), "gcd_lpips_relu_pool_f16: operands must be 16-byte aligned");
  GCD_CHECK_ARG(pooled != src && pooled != full, "gcd_lpips_relu_pool_f16: pooled must not alias src or full");
  const int Hc = (H + 1) / 2, Wc = (W + 1) / 2, CV = C / 8;
  const int64_t total = (int64_t)n * Hc * Wc * CV;
  const int64_t nblk = (total + NT - 1) / NT;
  GCD_CHECK_ARG(nblk < (1ll << 31), "gcd_lpips_relu_pool_f16: %lld work items are more than one launch takes", (long long)total);
  hipLaunchKernelGGL(relu_pool_kernel, dim3((unsigned)nblk), dim3(NT), 0, (hipStream_t)stream, (const f16x8*)src, (f16x8*)full,
                     (f16x8*)pooled, H, W, CV, Hc, Wc, total);
  GCD_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int gcd_lpips_distance(const void* f0, const void* f1, const float* w, int n, int64_t HW, int C, float* partials,
                                  int blocks, double* tap_means, int tap, int taps, float* out, void* stream) {
  GCD_CHECK_ARG(f0 && f1 && w && partials && tap_means, "gcd_lpips_distance: null operand");
  GCD_CHECK_ARG(n > 0 && n <= GCD_LPIPS_MAX_IMAGES && HW > 0, "gcd_lpips_distance: bad shape n=%d HW=%lld (n <= %d)", n,
                (long long)HW, GCD_LPIPS_MAX_IMAGES);
  GCD_CHECK_ARG(C > 0 && C % GCD_LPIPS_C_MULTIPLE == 0 && C <= GCD_LPIPS_MAX_C,
                "gcd_lpips_distance: C=%d must be a multiple of %d, at most %d", C, GCD_LPIPS_C_MULTIPLE, GCD_LPIPS_MAX_C);
  GCD_CHECK_ARG(blocks >= 1 && blocks <= GCD_LPIPS_MAX_BLOCKS, "gcd_lpips_distance: blocks=%d outside [1, %d]", blocks,
                GCD_LPIPS_MAX_BLOCKS);
  GCD_CHECK_ARG(taps >= 1 && taps <= GCD_LPIPS_MAX_TAPS && tap >= 0 && tap < taps, "gcd_lpips_distance: tap %d of %d (at most %d)",
                tap, taps, GCD_LPIPS_MAX_TAPS);
  GCD_CHECK_ARG(aligned16(f0) && aligned16(f1), "gcd_lpips_distance: f0 / f1 must be 16-byte aligned");
  GCD_CHECK_ARG(((uintptr_t)tap_means & 7) == 0 && ((uintptr_t)partials & 3) == 0, "gcd_lpips_distance: misaligned partials / tap_means");
  const int CV = C / 8;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks, (unsigned)n);
  const f16x8 *a = (const f16x8*)f0, *b = (const f16x8*)f1;
  if (CV <= 4)
    hipLaunchKernelGGL(distance_kernel<4>, grid, dim3(NT), 0, s, a, b, w, HW, CV, partials);
  else if (CV <= 8)
    hipLaunchKernelGGL(distance_kernel<8>, grid, dim3(NT), 0, s, a, b, w, HW, CV, partials);
  else if (CV <= 16)
    hipLaunchKernelGGL(distance_kernel<16>, grid, dim3(NT), 0, s, a, b, w, HW, CV, partials);
  else if (CV <= 32)
    hipLaunchKernelGGL(distance_kernel<32>, grid, dim3(NT), 0, s, a, b, w, HW, CV, partials);
  else
    hipLaunchKernelGGL(distance_kernel<64>, grid, dim3(NT), 0, s, a, b, w, HW, CV, partials);
  GCD_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(distance_finish_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, (const float*)partials, n, blocks,
                     (double)HW, tap_means, tap, taps, out);
  GCD_CHECK_HIP(hipGetLastError());
  return 0;
}
