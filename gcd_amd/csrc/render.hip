// render.hip — libgcd_amd_render.so: point clouds to (source, target) frames on the device.  C ABI: include/gcd_amd_render.h.
//
// gcd_render_splat, five launches on the caller's stream:
//   clear     zero the per-camera header (depth-maximum key, visible count) and the 8 words of every pixel
//   depthmax  project every point into every camera (the point is loaded once); per block the largest masked depth and
//             the number of masked points, one integer atomic max / add per block and camera; stores uv / depth if asked
//   expo      re-project (cheaper than storing), l = -depth_norm * strength (+ ln 0.02 for a neighbour); integer atomic
//             max of the order-preserving key of l on the pixel's denominator word and of l + ln c on the word of every
//             channel whose colour c is non-zero
//   sums      re-project, floor(exp(l - lmax) * 2^F) and floor(exp(l + ln c - max_c) * 2^F) added with 64-bit integer atomics
//   resolve   one thread per pixel: weights = S_d / 2^F * exp(lmax_d), img = clamp(S_c / S_d * exp(max_c - lmax_d), 0, 1)
// Integer maxima and sums are independent of the order of arrival, so the result is bit-identical from call to call.
//
// gcd_render_fill_resize_f32, two launches:
//   fill      one workgroup per 16 x 32 tile; per plane (validity mask, r, g, b) the tile with its k / 2 halo (reflect
//             padding) is staged in LDS as fp32, the horizontal pass goes to LDS as fp64, the vertical pass to registers;
//             holes take blur_img / max(blur_mask, 1e-7); the filled image goes to `scratch` as three fp64 planes
//   resize    one thread per output value: the 3 x 3 Gaussian (sigma 0.6, reflect) at the four bilinear taps, the
//             interpolation, scale and offset, one rounding to fp32
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gcd_amd_render.h"

static thread_local char g_err[512] = "";
static void gcd_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* gcd_render_last_error(void) { return g_err; }
extern "C" int gcd_render_abi_version(void) { return GCD_AMD_RENDER_ABI_VERSION; }

#define GCD_CHECK_ARG(cond, ...)  \
  do {                            \
    if (!(cond)) {                \
      gcd_set_error(__VA_ARGS__); \
      return 2;                   \
    }                             \
  } while (0)

namespace {

typedef unsigned long long u64;

constexpr int NT = 256;                      // threads per workgroup, every kernel here
constexpr int MAXC = GCD_RENDER_MAX_CAMERAS;
constexpr int CAMD = GCD_RENDER_CAM_DOUBLES;
constexpr int HDR = 2;                       // u64 words of a camera's header: depth-maximum key, visible count
constexpr int PIXW = 8;                      // u64 words per pixel: keys (den, r, g, b), sums (den, r, g, b)
constexpr int MAX_POINT_BLOCKS = 4096;
constexpr int MAX_RADIUS = 8;
constexpr double LN_NEIGHBOUR = -3.912023005428146;      // ln 0.02
constexpr int TH = 16, TW = 32;              // tile of the fill kernel
constexpr int MAXR = GCD_RENDER_MAX_KERNEL / 2;
constexpr int IH = TH + 2 * MAXR, IW = TW + 2 * MAXR;
constexpr int PER_THREAD = TH * TW / NT;
static_assert(TH * TW % NT == 0, "whole pixels per thread");

struct Taps { double w[GCD_RENDER_MAX_KERNEL]; };

// Order-preserving key of a double that is not NaN: a < b <=> key(a) < key(b); 0 is below every key.
__device__ __forceinline__ u64 key_of(double x) {
  const u64 b = (u64)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double unkey(u64 k) {
  const u64 b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}

__device__ __forceinline__ void load_point(const void* xyz, int64_t ld, int dtype, int64_t i, double (&p)[3]) {
  if (dtype == GCD_RENDER_F16) {
    const __half* s = (const __half*)xyz + i * ld;
#pragma unroll
    for (int j = 0; j < 3; ++j) p[j] = (double)__half2float(s[j]);
  } else if (dtype == GCD_RENDER_F32) {
    const float* s = (const float*)xyz + i * ld;
#pragma unroll
    for (int j = 0; j < 3; ++j) p[j] = (double)s[j];
  } else {
    const double* s = (const double*)xyz + i * ld;
#pragma unroll
    for (int j = 0; j < 3; ++j) p[j] = s[j];
  }
}

// lc[j] = ln(colour j), or -inf for a colour that contributes nothing: 0, negative, NaN or infinite
__device__ __forceinline__ void load_log_colour(const void* rgb, int64_t ld, int dtype, int64_t i, double (&lc)[3]) {
  double c[3];
  if (dtype == GCD_RENDER_U8) {
    const unsigned char* s = (const unsigned char*)rgb + i * ld;
#pragma unroll
    for (int j = 0; j < 3; ++j) c[j] = (double)((float)s[j] / 255.0f);
  } else {
    load_point(rgb, ld, dtype, i, c);
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) lc[j] = (c[j] > 0.0 && c[j] < (double)INFINITY) ? log(c[j]) : -(double)INFINITY;
}

struct Proj {
  double u, v, z;
  int px, py;
  bool in;
};

// xyz_cam = (xyz - t) R, uv = K xyz_cam / (K xyz_cam).z, the mask in floating point: trunc(uv + 0.5) in [0, n) <=> -1 < uv + 0.5 < n
__device__ __forceinline__ Proj project(const double* __restrict__ cam, const double (&p)[3], int H, int W) {
  const double* K = cam;
  const double* RT = cam + 9;
  const double dx = p[0] - RT[3], dy = p[1] - RT[7], dz = p[2] - RT[11];
  const double cx = dx * RT[0] + dy * RT[4] + dz * RT[8];
  const double cy = dx * RT[1] + dy * RT[5] + dz * RT[9];
  const double cz = dx * RT[2] + dy * RT[6] + dz * RT[10];
  const double pu = K[0] * cx + K[1] * cy + K[2] * cz;
  const double pv = K[3] * cx + K[4] * cy + K[5] * cz;
  const double pw = K[6] * cx + K[7] * cy + K[8] * cz;
  Proj r;
  r.u = pu / pw;
  r.v = pv / pw;
  r.z = cz;
  const double tu = r.u + 0.5, tv = r.v + 0.5;
  r.in = tu > -1.0 && tu < (double)W && tv > -1.0 && tv < (double)H && cz > 0.1;
  r.px = r.in ? (int)tu : 0;
  r.py = r.in ? (int)tv : 0;
  return r;
}

// The exponent of a masked point's weight, given the largest masked depth of its camera.
__device__ __forceinline__ double exponent_of(double depth, double gmax) {
  double d = depth, m = gmax, strength = 512.0;
  if (gmax >= 64.0) {
    strength = 256.0;
    d = fmin(sqrt(depth), 32.0);
    m = fmin(sqrt(gmax), 32.0);
  }
  const double depth_norm = d / m * 2.0 - 1.0;
  return -depth_norm * strength;
}

__global__ __launch_bounds__(NT) void clear_kernel(u64* __restrict__ words, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) words[i] = 0;
}

__global__ __launch_bounds__(NT) void depthmax_kernel(const void* __restrict__ xyz, int64_t xyz_ld, int xyz_dtype, int64_t N,
                                                      const double* __restrict__ cams, int nc, int H, int W,
                                                      int64_t cam_words, u64* __restrict__ scratch, double* __restrict__ uv,
                                                      double* __restrict__ depth) {
  __shared__ u64 smax[NT];
  __shared__ unsigned scnt[NT];
  u64 kmax[MAXC];
  unsigned cnt[MAXC];
#pragma unroll
  for (int c = 0; c < MAXC; ++c) kmax[c] = 0, cnt[c] = 0;
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < N; i += (int64_t)gridDim.x * NT) {
    double p[3];
    load_point(xyz, xyz_ld, xyz_dtype, i, p);
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      if (c >= nc) break;
      const Proj r = project(cams + c * CAMD, p, H, W);
      if (uv) {
        uv[((int64_t)c * N + i) * 2] = r.u;
        uv[((int64_t)c * N + i) * 2 + 1] = r.v;
      }
      if (depth) depth[(int64_t)c * N + i] = r.z;
      if (r.in) {
        const u64 k = key_of(r.z);
        kmax[c] = k > kmax[c] ? k : kmax[c];
        cnt[c] += 1;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    if (c >= nc) break;
    smax[threadIdx.x] = kmax[c];
    scnt[threadIdx.x] = cnt[c];
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) {
        const u64 o = smax[threadIdx.x + s];
        if (o > smax[threadIdx.x]) smax[threadIdx.x] = o;
        scnt[threadIdx.x] += scnt[threadIdx.x + s];
      }
      __syncthreads();
    }
    if (threadIdx.x == 0 && scnt[0] != 0) {
      atomicMax(scratch + (int64_t)c * cam_words, smax[0]);
      atomicAdd(scratch + (int64_t)c * cam_words + 1, (u64)scnt[0]);
    }
    __syncthreads();
  }
}

// Pass 0: the exponents' maxima.  Pass 1: the fixed-point sums.
template <int PASS>
__global__ __launch_bounds__(NT) void splat_kernel(const void* __restrict__ xyz, int64_t xyz_ld, int xyz_dtype,
                                                   const void* __restrict__ rgb, int64_t rgb_ld, int rgb_dtype, int64_t N,
                                                   const double* __restrict__ cams, int nc, int H, int W, int left, int right,
                                                   double fscale, int64_t cam_words, u64* __restrict__ scratch) {
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < N; i += (int64_t)gridDim.x * NT) {
    double p[3], lc[3];
    load_point(xyz, xyz_ld, xyz_dtype, i, p);
    load_log_colour(rgb, rgb_ld, rgb_dtype, i, lc);
    for (int c = 0; c < nc; ++c) {
      const Proj r = project(cams + c * CAMD, p, H, W);
      if (!r.in) continue;
      u64* cam_base = scratch + (int64_t)c * cam_words;
      const double gmax = unkey(cam_base[0]);
      const double l0 = exponent_of(r.z, gmax);
      for (int dy = -left; dy <= right; ++dy) {
        const int y = r.py + dy;
        if (y < 0 || y >= H) continue;
        for (int dx = -left; dx <= right; ++dx) {
          const int x = r.px + dx;
          if (x < 0 || x >= W) continue;
          const double l = (dx == 0 && dy == 0) ? l0 : l0 + LN_NEIGHBOUR;
          u64* pix = cam_base + HDR + ((int64_t)y * W + x) * PIXW;
          if (PASS == 0) {
            const u64 k = key_of(l);
            // a stale read only costs an atomic: the words grow monotonically
            if (pix[0] < k) atomicMax(pix + 0, k);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
              if (lc[ch] == -(double)INFINITY) continue;
              const u64 kc = key_of(l + lc[ch]);
              if (pix[1 + ch] < kc) atomicMax(pix + 1 + ch, kc);
            }
          } else {
            const double ed = fmin(exp(l - unkey(pix[0])), 1.0);
            const u64 td = (u64)floor(ed * fscale);
            if (td) atomicAdd(pix + 4, td);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
              if (lc[ch] == -(double)INFINITY) continue;
              const double ec = fmin(exp(l + lc[ch] - unkey(pix[1 + ch])), 1.0);
              const u64 tc = (u64)floor(ec * fscale);
              if (tc) atomicAdd(pix + 5 + ch, tc);
            }
          }
        }
      }
    }
  }
}

__global__ __launch_bounds__(NT) void resolve_kernel(const u64* __restrict__ scratch, int nc, int H, int W, double fscale,
                                                     int64_t cam_words, float* __restrict__ img, int64_t img_cs, int64_t img_ld,
                                                     double* __restrict__ weights, int64_t w_cs, int64_t w_ld,
                                                     int64_t* __restrict__ status) {
  const int64_t plane = (int64_t)H * W;
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i < nc) status[i] = (int64_t)scratch[i * cam_words + 1];
  if (i >= plane * nc) return;
  const int c = (int)(i / plane);
  const int64_t q = i % plane;
  const int y = (int)(q / W), x = (int)(q % W);
  const u64* pix = scratch + (int64_t)c * cam_words + HDR + q * PIXW;
  float* o = img + c * img_cs + y * img_ld + (int64_t)x * 3;
  double* wo = weights + c * w_cs + y * w_ld + x;
  const u64 sd = pix[4];
  if (sd == 0) {
    *wo = -1.0;
    o[0] = o[1] = o[2] = 0.0f;
    return;
  }
  const double ld = unkey(pix[0]);
  *wo = (double)sd / fscale * exp(ld);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const u64 sc = pix[5 + ch];
    double v = 0.0;
    if (sc) v = (double)sc / (double)sd * exp(unkey(pix[1 + ch]) - ld);
    v = v < 0.0 ? 0.0 : v;
    v = v > 1.0 ? 1.0 : v;
    o[ch] = (float)v;
  }
}

__device__ __forceinline__ int reflect(int i, int n) {
  i = i < 0 ? -i : i;
  return i >= n ? 2 * (n - 1) - i : i;
}

__global__ __launch_bounds__(NT) void fill_kernel(const float* __restrict__ img, int64_t img_ld, int H, int W, int k, Taps taps,
                                                  int tiles_x, double* __restrict__ filled) {
  __shared__ float st[IH][IW + 1];
  __shared__ double sh[IH][TW];
  const int tid = threadIdx.x;
  const int rad = k / 2;
  const int ih = TH + 2 * rad, iw = TW + 2 * rad;
  const int y0 = (int)(blockIdx.x / tiles_x) * TH, x0 = (int)(blockIdx.x % tiles_x) * TW;
  const int64_t plane = (int64_t)H * W;
  double blur[4][PER_THREAD];                 // mask, r, g, b
  float centre[3][PER_THREAD];
  for (int pl = 0; pl < 4; ++pl) {
    for (int i = tid; i < ih * iw; i += NT) {
      const int iy = i / iw, ix = i % iw;
      const int y = reflect(y0 - rad + iy, H), x = reflect(x0 - rad + ix, W);
      float v = 0.0f;
      // rows / columns past the ragged edge of the last tile feed no pixel that is stored
      if (y >= 0 && y < H && x >= 0 && x < W) {
        const float* s = img + y * img_ld + (int64_t)x * 3;
        v = pl == 0 ? (((s[0] + s[1]) + s[2]) == 0.0f ? 0.0f : 1.0f) : s[pl - 1];
      }
      st[iy][ix] = v;
    }
    __syncthreads();
    for (int i = tid; i < ih * TW; i += NT) {
      const int iy = i / TW, ox = i % TW;
      double a = 0.0;
      for (int j = 0; j < k; ++j) a += taps.w[j] * (double)st[iy][ox + j];
      sh[iy][ox] = a;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < PER_THREAD; ++t) {
      const int o = tid + t * NT;
      const int oy = o / TW, ox = o % TW;
      double a = 0.0;
      for (int j = 0; j < k; ++j) a += taps.w[j] * sh[oy + j][ox];
      blur[pl][t] = a;
      if (pl > 0) centre[pl - 1][t] = st[oy + rad][ox + rad];
    }
    __syncthreads();          // st / sh are restaged by the next plane
  }
#pragma unroll
  for (int t = 0; t < PER_THREAD; ++t) {
    const int o = tid + t * NT;
    const int y = y0 + o / TW, x = x0 + o % TW;
    if (y >= H || x >= W) continue;
    const bool black = ((centre[0][t] + centre[1][t]) + centre[2][t]) == 0.0f;
    const double den = blur[0][t] > 1e-7 ? blur[0][t] : 1e-7;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
      filled[ch * plane + (int64_t)y * W + x] = black ? blur[1 + ch][t] / den : (double)centre[ch][t];
  }
}

__global__ __launch_bounds__(NT) void resize_kernel(const double* __restrict__ filled, int H, int W, double g0, double g1,
                                                    float* __restrict__ out, int64_t out_cs, int64_t out_rs, int64_t out_xs, int Hp,
                                                    int Wp, double scale, double offset) {
  const int64_t oplane = (int64_t)Hp * Wp;
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= 3 * oplane) return;
  const int ch = (int)(i / oplane);
  const int yo = (int)((i % oplane) / Wp), xo = (int)(i % Wp);
  const double* src = filled + (int64_t)ch * H * W;
  // torch's area_pixel_compute_source_index, align_corners = false
  double sy = ((double)H / (double)Hp) * ((double)yo + 0.5) - 0.5;
  double sx = ((double)W / (double)Wp) * ((double)xo + 0.5) - 0.5;
  sy = sy < 0.0 ? 0.0 : sy;
  sx = sx < 0.0 ? 0.0 : sx;
  int ya = (int)sy, xa = (int)sx;
  ya = ya > H - 1 ? H - 1 : ya;
  xa = xa > W - 1 ? W - 1 : xa;
  const int yb = ya < H - 1 ? ya + 1 : ya, xb = xa < W - 1 ? xa + 1 : xa;
  const double ly = sy - (double)ya, lx = sx - (double)xa;
  const int ys[2] = {ya, yb}, xs[2] = {xa, xb};
  const double g[3] = {g1, g0, g1};
  double tap[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      double acc = 0.0;
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy) {
        const double* row = src + (int64_t)reflect(ys[a] + dy, H) * W;
        double r = 0.0;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) r += g[dx + 1] * row[reflect(xs[b] + dx, W)];
        acc += g[dy + 1] * r;
      }
      tap[a][b] = acc;
    }
  }
  const double v = (1.0 - ly) * ((1.0 - lx) * tap[0][0] + lx * tap[0][1]) + ly * ((1.0 - lx) * tap[1][0] + lx * tap[1][1]);
  out[ch * out_cs + yo * out_rs + xo * out_xs] = (float)(v * scale + offset);
}

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

int check_image(const char* who, int nc, int H, int W) {
  GCD_CHECK_ARG(nc >= 1 && nc <= MAXC, "%s: nc=%d: 1 to %d cameras per call", who, nc, MAXC);
  GCD_CHECK_ARG(H >= 1 && W >= 1 && H <= 32768 && W <= 32768, "%s: H=%d W=%d: an image is 1 to 32768 pixels a side", who, H, W);
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

inline int bit_length(int64_t n) {
  int b = 0;
  while (n > 0) ++b, n >>= 1;
  return b;
}

}  // namespace

extern "C" int64_t gcd_render_scratch_bytes(int nc, int H, int W) {
  if (check_image("gcd_render_scratch_bytes", nc, H, W)) return 0;
  return (int64_t)nc * (HDR + (int64_t)H * W * PIXW) * (int64_t)sizeof(u64);
}

extern "C" int64_t gcd_render_fill_scratch_bytes(int H, int W) {
  if (check_image("gcd_render_fill_scratch_bytes", 1, H, W)) return 0;
  return 3 * (int64_t)H * W * (int64_t)sizeof(double);
}

extern "C" int gcd_render_splat(const gcd_render_splat_desc* d, void* stream) {
  const char* who = "gcd_render_splat";
  GCD_CHECK_ARG(d, "%s: null descriptor", who);
  if (const int rc = check_image(who, d->nc, d->H, d->W)) return rc;
  GCD_CHECK_ARG(d->N >= 0 && d->N < ((int64_t)1 << 31), "%s: N=%lld: 0 <= N < 2^31", who, (long long)d->N);
  GCD_CHECK_ARG(d->cams && d->img && d->weights && d->status, "%s: null pointer (cams, img, weights and status are required)", who);
  GCD_CHECK_ARG(d->N == 0 || (d->xyz && d->rgb), "%s: null pointer (xyz and rgb are required when N > 0)", who);
  GCD_CHECK_ARG(d->xyz_dtype == GCD_RENDER_F16 || d->xyz_dtype == GCD_RENDER_F32 || d->xyz_dtype == GCD_RENDER_F64,
                "%s: bad dtype code %d for xyz (F16, F32 or F64)", who, d->xyz_dtype);
  GCD_CHECK_ARG(d->rgb_dtype >= GCD_RENDER_F16 && d->rgb_dtype <= GCD_RENDER_U8, "%s: bad dtype code %d for rgb (F16, F32, F64 or U8)",
                who, d->rgb_dtype);
  GCD_CHECK_ARG(d->xyz_ld >= 3 && d->rgb_ld >= 3, "%s: xyz_ld=%lld rgb_ld=%lld: a point has 3 values", who, (long long)d->xyz_ld,
                (long long)d->rgb_ld);
  GCD_CHECK_ARG(d->spread_radius >= 0 && d->spread_radius <= MAX_RADIUS, "%s: spread_radius=%d: 0 to %d", who, d->spread_radius,
                MAX_RADIUS);
  GCD_CHECK_ARG(d->img_ld >= (int64_t)d->W * 3 && d->weights_ld >= d->W, "%s: img_ld=%lld weights_ld=%lld: rows overlap (W=%d)", who,
                (long long)d->img_ld, (long long)d->weights_ld, d->W);
  GCD_CHECK_ARG(d->nc == 1 || (d->img_cs >= d->img_ld * d->H && d->weights_cs >= d->weights_ld * d->H),
                "%s: img_cs=%lld weights_cs=%lld: cameras overlap", who, (long long)d->img_cs, (long long)d->weights_cs);
  const int64_t need = gcd_render_scratch_bytes(d->nc, d->H, d->W);
  GCD_CHECK_ARG(d->scratch && d->scratch_bytes >= need, "%s: scratch too small: %lld bytes given, %lld needed", who,
                (long long)(d->scratch ? d->scratch_bytes : 0), (long long)need);
  GCD_CHECK_ARG(((uintptr_t)d->scratch & 7u) == 0, "%s: scratch must be 8-byte aligned", who);
  const int64_t plane = (int64_t)d->H * d->W;
  const int64_t cam_words = HDR + plane * PIXW;
  const int64_t words = cam_words * d->nc;
  const int fbits = 63 - bit_length(d->N) < 52 ? 63 - bit_length(d->N) : 52;
  const double fscale = ldexp(1.0, fbits);
  const int left = d->spread_radius / 2, right = (d->spread_radius + 1) / 2;
  hipStream_t s = (hipStream_t)stream;
  u64* scratch = (u64*)d->scratch;
  int64_t pb = cdiv(d->N, NT);
  pb = pb < 1 ? 1 : pb > MAX_POINT_BLOCKS ? MAX_POINT_BLOCKS : pb;
  int64_t cb = cdiv(words, (int64_t)NT * 8);
  cb = cb > 65536 ? 65536 : cb;
  hipLaunchKernelGGL(clear_kernel, dim3((unsigned)cb), dim3(NT), 0, s, scratch, words);
  if (const int rc = launch_status(who)) return rc;
  hipLaunchKernelGGL(depthmax_kernel, dim3((unsigned)pb), dim3(NT), 0, s, d->xyz, d->xyz_ld, d->xyz_dtype, d->N, d->cams, d->nc, d->H,
                     d->W, cam_words, scratch, d->uv, d->depth);
  if (const int rc = launch_status(who)) return rc;
  hipLaunchKernelGGL(splat_kernel<0>, dim3((unsigned)pb), dim3(NT), 0, s, d->xyz, d->xyz_ld, d->xyz_dtype, d->rgb, d->rgb_ld,
                     d->rgb_dtype, d->N, d->cams, d->nc, d->H, d->W, left, right, fscale, cam_words, scratch);
  if (const int rc = launch_status(who)) return rc;
  hipLaunchKernelGGL(splat_kernel<1>, dim3((unsigned)pb), dim3(NT), 0, s, d->xyz, d->xyz_ld, d->xyz_dtype, d->rgb, d->rgb_ld,
                     d->rgb_dtype, d->N, d->cams, d->nc, d->H, d->W, left, right, fscale, cam_words, scratch);
  if (const int rc = launch_status(who)) return rc;
  hipLaunchKernelGGL(resolve_kernel, dim3((unsigned)cdiv(plane * d->nc, NT)), dim3(NT), 0, s, (const u64*)scratch, d->nc, d->H, d->W,
                     fscale, cam_words, d->img, d->img_cs, d->img_ld, d->weights, d->weights_cs, d->weights_ld, d->status);
  return launch_status(who);
}

extern "C" int gcd_render_fill_resize_f32(const float* img, int64_t img_ld, int H, int W, int k, double sigma, float* out,
                                          int64_t out_cs, int64_t out_rs, int64_t out_xs, int Hp, int Wp, double scale, double offset,
                                          void* scratch, int64_t scratch_bytes, void* stream) {
  const char* who = "gcd_render_fill_resize_f32";
  GCD_CHECK_ARG(img && out, "%s: null pointer (img and out are required)", who);
  if (const int rc = check_image(who, 1, H, W)) return rc;
  if (const int rc = check_image(who, 1, Hp, Wp)) return rc;
  GCD_CHECK_ARG(k >= 1 && k <= GCD_RENDER_MAX_KERNEL && (k & 1), "%s: kernel_size=%d: odd, 1 to %d", who, k, GCD_RENDER_MAX_KERNEL);
  GCD_CHECK_ARG(sigma > 0.0 && sigma < INFINITY, "%s: sigma=%g must be positive and finite", who, sigma);
  const int halo = k / 2 > 1 ? k / 2 : 1;
  GCD_CHECK_ARG(H > halo && W > halo, "%s: H=%d W=%d: reflect padding by %d needs more than %d pixels a side", who, H, W, halo, halo);
  GCD_CHECK_ARG(img_ld >= (int64_t)W * 3, "%s: img_ld=%lld: rows overlap (W=%d)", who, (long long)img_ld, W);
  const int64_t need = gcd_render_fill_scratch_bytes(H, W);
  GCD_CHECK_ARG(scratch && scratch_bytes >= need, "%s: scratch too small: %lld bytes given, %lld needed", who,
                (long long)(scratch ? scratch_bytes : 0), (long long)need);
  GCD_CHECK_ARG(((uintptr_t)scratch & 7u) == 0, "%s: scratch must be 8-byte aligned", who);
  Taps taps;
  double sum = 0.0;
  for (int j = 0; j < GCD_RENDER_MAX_KERNEL; ++j) taps.w[j] = 0.0;
  for (int j = 0; j < k; ++j) {
    const double x = (k == 1) ? 0.0 : -0.5 * (k - 1) + (double)j;
    taps.w[j] = exp(-0.5 * (x / sigma) * (x / sigma));
    sum += taps.w[j];
  }
  for (int j = 0; j < k; ++j) taps.w[j] /= sum;
  const double e1 = exp(-0.5 * (1.0 / 0.6) * (1.0 / 0.6));
  const double g0 = 1.0 / (1.0 + 2.0 * e1), g1 = e1 / (1.0 + 2.0 * e1);
  const int tiles_x = (int)cdiv(W, TW), tiles_y = (int)cdiv(H, TH);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(fill_kernel, dim3((unsigned)(tiles_x * tiles_y)), dim3(NT), 0, s, img, img_ld, H, W, k, taps, tiles_x,
                     (double*)scratch);
  if (const int rc = launch_status(who)) return rc;
  hipLaunchKernelGGL(resize_kernel, dim3((unsigned)cdiv(3 * (int64_t)Hp * Wp, NT)), dim3(NT), 0, s, (const double*)scratch, H, W, g0, g1,
                     out, out_cs, out_rs, out_xs, Hp, Wp, scale, offset);
  return launch_status(who);
}
