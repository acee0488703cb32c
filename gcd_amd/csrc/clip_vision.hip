// clip_vision.hip — libgcd_amd_clip.so: the kernels of the CLIP ViT image tower that libgcd_amd.so does not have.
// C ABI: include/gcd_amd_clip.h.
//
// gcd_clip_preprocess: one workgroup per (image, channel, output row).  The antialias blur and the bicubic resize are
// both separable and linear, so the row is produced in two steps: (1) every input column of the output row's 4 bicubic
// source rows, each blurred along y, goes to LDS as fp32 (one coalesced pass over 4 * ky input rows); (2) every output
// pixel takes its 4 bicubic source columns, each blurred along x, from that LDS row.  Source coordinates and tap weights
// are evaluated in fp64 (the fp32 coordinate rounding of torch's kernel is the largest error of a float32 chain).
//
// gcd_clip_attn_f16: one workgroup of 4 waves per (image, head) and query split.  K (row-major, 80 wide) and V
// (transposed, so that 4 consecutive keys of one channel are one 8-byte read) of the whole sequence are staged in LDS
// once; every wave then owns 16-query tiles.  Scores are computed transposed, S^T = K Q^T (v_mfma_f32_16x16x32_f16 with
// K as the A operand, the contraction 80 = 32 + 32 + 16 with the last step's upper lanes fed zeros), so that a lane
// holds 4 keys of ONE query per 16-key tile: the whole row of scores of a query lives in the registers of 4 lanes, the
// softmax is a plain two-pass one (no running maximum), and the probabilities are already in the A-operand layout of
// P V — the contraction index of an MFMA is a label, and V is read from LDS under the same key permutation.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gcd_amd_clip.h"

static thread_local char g_err[512] = "";
static void gcd_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* gcd_clip_last_error(void) { return g_err; }
extern "C" int gcd_clip_abi_version(void) { return GCD_AMD_CLIP_ABI_VERSION; }

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
typedef f16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int NT = 256;

// ---------------------------------------------------------------------------------------------------- preprocess
struct Taps {
  float w[4];
  int i[4];
};

// torch's upsample_bicubic2d, align_corners = True: A = -0.75, taps at floor(src) - 1 .. + 2, indices clamped
__device__ __forceinline__ Taps bicubic_taps(int dst, int in, int out) {
  const double scale = out > 1 ? (double)(in - 1) / (double)(out - 1) : 0.0;
  const double src = scale * dst;
  const double fl = floor(src);
  const double t = src - fl;
  const int i0 = (int)fl;
  const double A = -0.75;
  const double x0 = t + 1.0, x1 = t, x2 = 1.0 - t, x3 = 2.0 - t;
  Taps r;
  r.w[0] = (float)(((A * x0 - 5.0 * A) * x0 + 8.0 * A) * x0 - 4.0 * A);
  r.w[1] = (float)(((A + 2.0) * x1 - (A + 3.0)) * x1 * x1 + 1.0);
  r.w[2] = (float)(((A + 2.0) * x2 - (A + 3.0)) * x2 * x2 + 1.0);
  r.w[3] = (float)(((A * x3 - 5.0 * A) * x3 + 8.0 * A) * x3 - 4.0 * A);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int idx = i0 - 1 + j;
    idx = idx < 0 ? 0 : idx;
    idx = idx > in - 1 ? in - 1 : idx;
    r.i[j] = idx;
  }
  return r;
}

__device__ __forceinline__ int reflect_index(int i, int n) {
  i = i < 0 ? -i : i;
  return i > n - 1 ? 2 * (n - 1) - i : i;
}

// normalised Gaussian taps exp(-t^2 / (2 sigma^2)), t = j - k / 2, into g[0..k)
__device__ __forceinline__ void gaussian_taps(float* g, int k, double sigma, int tid) {
  if (tid < k) {
    double sum = 0.0;
    for (int j = 0; j < k; ++j) {
      const double t = (double)(j - k / 2);
      sum += exp(-(t * t) / (2.0 * sigma * sigma));
    }
    const double t = (double)(tid - k / 2);
    g[tid] = (float)(exp(-(t * t) / (2.0 * sigma * sigma)) / sum);
  }
}

__global__ __launch_bounds__(NT) void preprocess_kernel(const float* __restrict__ x, int64_t sn, int64_t sc, int64_t sh,
                                                        int64_t sw, int H, int W, int S, int P, int ky, int kx, double sy,
                                                        double sx, const float* __restrict__ mean,
                                                        const float* __restrict__ stdv, f16* __restrict__ patches, int Kp,
                                                        float* __restrict__ img32) {
  extern __shared__ float rowbuf[];            // [W]: the output row's source, blurred and interpolated along y
  __shared__ float gy[GCD_CLIP_MAX_BLUR], gx[GCD_CLIP_MAX_BLUR];
  const int tid = threadIdx.x;
  const int oy = blockIdx.x % S;
  const int c = (blockIdx.x / S) % 3;
  const int img = blockIdx.x / (3 * S);
  gaussian_taps(gy, ky, sy, tid);
  gaussian_taps(gx, kx, sx, tid);
  __syncthreads();
  const float* __restrict__ plane = x + (int64_t)img * sn + (int64_t)c * sc;
  const Taps ty = bicubic_taps(oy, H, S);
  for (int col = tid; col < W; col += NT) {
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float b = 0.0f;
      for (int a = 0; a < ky; ++a) {
        const int row = reflect_index(ty.i[i] + a - ky / 2, H);
        b += gy[a] * plane[(int64_t)row * sh + (int64_t)col * sw];
      }
      acc += ty.w[i] * b;
    }
    rowbuf[col] = acc;
  }
  __syncthreads();
  const int G = S / P;
  const float mu = mean[c], sd = stdv[c];
  for (int ox = tid; ox < S; ox += NT) {
    const Taps tx = bicubic_taps(ox, W, S);
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float b = 0.0f;
      for (int a = 0; a < kx; ++a) b += gx[a] * rowbuf[reflect_index(tx.i[j] + a - kx / 2, W)];
      acc += tx.w[j] * b;
    }
    const float v = (float)((((double)acc + 1.0) * 0.5 - (double)mu) / (double)sd);      // one rounding
    if (img32) img32[(((int64_t)img * 3 + c) * S + oy) * S + ox] = v;
    const int64_t prow = (int64_t)img * G * G + (int64_t)(oy / P) * G + ox / P;
    patches[prow * Kp + c * P * P + (oy % P) * P + ox % P] = (f16)v;
  }
  // the pad columns of this row of patches: written once, by the block of (channel 0, first pixel row of the patch)
  const int pad = Kp - 3 * P * P;
  if (c == 0 && oy % P == 0 && pad > 0) {
    for (int i = tid; i < G * pad; i += NT) {
      const int64_t prow = (int64_t)img * G * G + (int64_t)(oy / P) * G + i / pad;
      patches[prow * Kp + 3 * P * P + i % pad] = (f16)0.0f;
    }
  }
}

// ---------------------------------------------------------------------------------------------- tokens + ln_pre
// sum of v over the workgroup in a fixed order; every thread gets the result
__device__ __forceinline__ float block_sum(float v, float* red) {
  const int tid = threadIdx.x;
  __syncthreads();                             // `red` may still be read from the previous call
  red[tid] = v;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(NT) void tokens_ln_pre_kernel(const float* __restrict__ patch, int64_t ldp,
                                                           const float* __restrict__ cls, const float* __restrict__ pos,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float eps, float* __restrict__ tok, int64_t ldo, int G2, int C) {
  extern __shared__ float z[];                 // [C]
  __shared__ float red[NT];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int s = (int)(row % (G2 + 1));
  const int64_t img = row / (G2 + 1);
  const float* __restrict__ src = s == 0 ? cls : patch + (img * G2 + (s - 1)) * ldp;
  const float* __restrict__ p = pos + (int64_t)s * C;
  float sum = 0.0f;
  for (int i = tid; i < C; i += NT) {
    const float v = src[i] + p[i];
    z[i] = v;
    sum += v;
  }
  const float mean = block_sum(sum, red) / (float)C;
  float sq = 0.0f;
  for (int i = tid; i < C; i += NT) {
    const float d = z[i] - mean;
    sq += d * d;
  }
  const float rstd = 1.0f / sqrtf(block_sum(sq, red) / (float)C + eps);
  for (int i = tid; i < C; i += NT) tok[row * ldo + i] = (z[i] - mean) * rstd * gamma[i] + beta[i];
}

// ------------------------------------------------------------------------------------------------- bias + GELU
__global__ __launch_bounds__(NT) void bias_gelu_kernel(const float* __restrict__ h, int64_t ldh, const float* __restrict__ bias,
                                                       f16* __restrict__ out, int64_t ldo, int64_t M, int N4) {
  const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (idx >= M * N4) return;
  const int64_t row = idx / N4;
  const int c4 = (int)(idx % N4) * 4;
  const f32x4 v = *(const f32x4*)(h + row * ldh + c4);
  const f32x4 b = *(const f32x4*)(bias + c4);
  f16x4 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float t = v[j] + b[j];
    r[j] = (f16)(0.5f * t * (1.0f + erff(t * 0.70710678118654752440f)));
  }
  *(f16x4*)(out + row * ldo + c4) = r;
}

// --------------------------------------------------------------------------------------------------- attention
constexpr int HD = GCD_CLIP_HEAD_DIM;          // 80
constexpr int KS = 88;                         // row stride of K in LDS (halves): 176 bytes, 16-byte aligned rows
constexpr int ATTN_WAVES = 4;             // 256 threads: the 18-tile kernel keeps 72 score registers per lane without spilling
constexpr int ATTN_NT = ATTN_WAVES * 64;

template <int MAXT>
constexpr int attn_lds_bytes() {
  return (MAXT * 16 * KS + HD * (MAXT * 16 + 8)) * 2;
}

template <int MAXT>   // 16-key tiles held per query (even): S <= 16 * MAXT
__global__ __launch_bounds__(ATTN_NT) void attn_kernel(const f16* __restrict__ qkv, int64_t ld, f16* __restrict__ out,
                                                       int64_t ldo, int S, int heads, float scale_log2) {
  static_assert(MAXT % 2 == 0, "P V contracts 32 keys per MFMA");
  constexpr int SP = MAXT * 16;                // keys in LDS (rows S .. SP - 1 are zeros)
  constexpr int VS = SP + 8;                   // row stride of V^T in LDS (halves)
  extern __shared__ __align__(16) unsigned char smem[];
  f16* Ks = (f16*)smem;                        // [SP][KS]
  f16* Vt = Ks + SP * KS;                      // [HD][VS]
  const int img = blockIdx.x / heads, h = blockIdx.x % heads;
  const int Wd = heads * HD;
  const f16* __restrict__ base = qkv + (int64_t)img * S * ld;

  for (int i = threadIdx.x; i < SP * (HD / 8); i += ATTN_NT) {
    const int key = i / (HD / 8), seg = i % (HD / 8);
    f16x8 kv = {0, 0, 0, 0, 0, 0, 0, 0}, vv = {0, 0, 0, 0, 0, 0, 0, 0};
    if (key < S) {
      const f16* rowp = base + (int64_t)key * ld + h * HD + seg * 8;
      kv = *(const f16x8*)(rowp + Wd);
      vv = *(const f16x8*)(rowp + 2 * Wd);
    }
    *(f16x8*)(Ks + key * KS + seg * 8) = kv;
#pragma unroll
    for (int e = 0; e < 8; ++e) Vt[(seg * 8 + e) * VS + key] = vv[e];
  }
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, g = lane >> 4;
  const int nqt = (S + 15) / 16;
  const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int qt = blockIdx.y * ATTN_WAVES + wave; qt < nqt; qt += ATTN_WAVES * gridDim.y) {
    // Q^T as the B operand: lane holds q[query r16][d = 32 kk + 8 g + j]; d >= 80 and queries past S are zeros
    const int q = qt * 16 + r16;
    f16x8 qf[3];
#pragma unroll
    for (int kk = 0; kk < 3; ++kk) {
      qf[kk] = zero8;
      if (q < S && (kk < 2 || g < 2)) qf[kk] = *(const f16x8*)(base + (int64_t)q * ld + h * HD + kk * 32 + g * 8);
    }
    // sc[t][r]: score of (key 16 t + 4 g + r, query r16)
    f32x4 sc[MAXT];
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
      f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int kk = 0; kk < 3; ++kk) {
        f16x8 kf = zero8;
        if (kk < 2 || g < 2) kf = *(const f16x8*)(Ks + (t * 16 + r16) * KS + kk * 32 + g * 8);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[kk], acc, 0, 0, 0);
      }
      sc[t] = acc;
    }
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < MAXT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float s = (t * 16 + 4 * g + r < S) ? sc[t][r] : -INFINITY;      // keys past S are masked
        sc[t][r] = s;
        m = fmaxf(m, s);
      }
    m = fmaxf(m, __shfl_xor(m, 16));
    m = fmaxf(m, __shfl_xor(m, 32));
    // probabilities, rounded to fp16 (what P V accumulates); the row sum is the sum of the rounded values
    float l = 0.0f;
#pragma unroll
    for (int t = 0; t < MAXT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = (float)(f16)exp2f((sc[t][r] - m) * scale_log2);
        sc[t][r] = p;
        l += p;
      }
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    // O = P V: contraction slot (g, j) of chunk c is key 32 c + 4 g + j (j < 4) or 32 c + 16 + 4 g + (j - 4)
    f32x4 o[HD / 16];
#pragma unroll
    for (int dt = 0; dt < HD / 16; ++dt) o[dt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int c = 0; c < MAXT / 2; ++c) {
      f16x8 pf;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        pf[r] = (f16)sc[2 * c][r];
        pf[4 + r] = (f16)sc[2 * c + 1][r];
      }
#pragma unroll
      for (int dt = 0; dt < HD / 16; ++dt) {
        const f16* vp = Vt + (dt * 16 + r16) * VS + c * 32 + 4 * g;
        const f16x4 v0 = *(const f16x4*)vp;
        const f16x4 v1 = *(const f16x4*)(vp + 16);
        const f16x8 vf = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pf, vf, o[dt], 0, 0, 0);
      }
    }
    // o[dt][r]: (query 4 g + r of the tile, channel 16 dt + r16); that query's row sum sits in lane 4 g + r
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float inv = 1.0f / __shfl(l, 4 * g + r);
      const int qrow = qt * 16 + 4 * g + r;
      if (qrow < S) {
        f16* op = out + ((int64_t)img * S + qrow) * ldo + h * HD + r16;
#pragma unroll
        for (int dt = 0; dt < HD / 16; ++dt) op[dt * 16] = (f16)(o[dt][r] * inv);
      }
    }
  }
}

template <int MAXT>
int attn_launch(const f16* qkv, int64_t ld, f16* out, int64_t ldo, int n, int S, int heads, float scale_log2,
                hipStream_t s) {
  constexpr int bytes = attn_lds_bytes<MAXT>();
  if (bytes > 64 * 1024)
    GCD_CHECK_HIP(hipFuncSetAttribute((const void*)attn_kernel<MAXT>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  const int nqt = (S + 15) / 16;
  const int rounds = (nqt + ATTN_WAVES - 1) / ATTN_WAVES;
  int64_t want = 512 / ((int64_t)n * heads);           // query splits: about two workgroups per CU when n * heads is small
  int split = (int)(want < 1 ? 1 : want > rounds ? rounds : want);
  hipLaunchKernelGGL(attn_kernel<MAXT>, dim3((unsigned)(n * heads), (unsigned)split), dim3(ATTN_NT), bytes, s, qkv, ld, out,
                     ldo, S, heads, scale_log2);
  GCD_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace

static int blur_taps(double factor, double* sigma) {
  const double s = (factor - 1.0) / 2.0 > 0.001 ? (factor - 1.0) / 2.0 : 0.001;
  const double w = 2.0 * 2.0 * s > 3.0 ? 2.0 * 2.0 * s : 3.0;
  int k = (int)w;
  if (k % 2 == 0) k += 1;
  *sigma = s;
  return k;
}

extern "C" int gcd_clip_preprocess(const float* x, int64_t sn, int64_t sc, int64_t sh, int64_t sw, int n, int H, int W,
                                   int S, int P, int antialias, const float* mean, const float* stdev, void* patches16,
                                   int Kp, float* img32, void* stream) {
  GCD_CHECK_ARG(x && mean && stdev && patches16, "gcd_clip_preprocess: null pointer");
  GCD_CHECK_ARG(n > 0 && H > 0 && W > 0 && S > 0 && P > 0, "gcd_clip_preprocess: empty problem n=%d H=%d W=%d S=%d P=%d",
                n, H, W, S, P);
  GCD_CHECK_ARG(S % P == 0 && S <= 4096, "gcd_clip_preprocess: S=%d must be a multiple of P=%d (and <= 4096)", S, P);
  GCD_CHECK_ARG(W <= GCD_CLIP_MAX_WIDTH, "gcd_clip_preprocess: W=%d exceeds %d", W, GCD_CLIP_MAX_WIDTH);
  GCD_CHECK_ARG(Kp % 32 == 0 && Kp >= 3 * P * P, "gcd_clip_preprocess: Kp=%d must be a multiple of 32 and >= 3 P P = %d",
                Kp, 3 * P * P);
  GCD_CHECK_ARG(((uintptr_t)x & 3) == 0 && ((uintptr_t)patches16 & 15) == 0 && ((uintptr_t)img32 & 3) == 0 &&
                    ((uintptr_t)mean & 3) == 0 && ((uintptr_t)stdev & 3) == 0,
                "gcd_clip_preprocess: misaligned pointer (x, img32, mean, std: 4 bytes; patches16: 16 bytes)");
  GCD_CHECK_ARG(sn >= 0 && sc >= 0 && sh >= 0 && sw >= 0 && (sw > 0 || W == 1) && (sh > 0 || H == 1),
                "gcd_clip_preprocess: strides (%lld, %lld, %lld, %lld) must be non-negative element strides",
                (long long)sn, (long long)sc, (long long)sh, (long long)sw);
  int ky = 1, kx = 1;
  double sy = 1.0, sx = 1.0;
  const double fy = (double)H / S, fx = (double)W / S;
  if (antialias && (fy > fx ? fy : fx) > 1.0) {
    ky = blur_taps(fy, &sy);
    kx = blur_taps(fx, &sx);
  }
  GCD_CHECK_ARG(ky <= GCD_CLIP_MAX_BLUR && kx <= GCD_CLIP_MAX_BLUR, "gcd_clip_preprocess: antialias kernel (%d, %d) exceeds %d",
                ky, kx, GCD_CLIP_MAX_BLUR);
  GCD_CHECK_ARG(H > ky / 2 && W > kx / 2,
                "gcd_clip_preprocess: reflect padding needs H=%d > %d and W=%d > %d (half the antialias kernel)", H, ky / 2,
                W, kx / 2);
  const int64_t blocks = (int64_t)n * 3 * S;
  GCD_CHECK_ARG(blocks < (1ll << 31), "gcd_clip_preprocess: grid too large");
  hipLaunchKernelGGL(preprocess_kernel, dim3((unsigned)blocks), dim3(NT), (size_t)W * sizeof(float), (hipStream_t)stream, x,
                     sn, sc, sh, sw, H, W, S, P, ky, kx, sy, sx, mean, stdev, (f16*)patches16, Kp, img32);
  GCD_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int gcd_clip_tokens_ln_pre(const float* patch, int64_t ldp, const float* cls, const float* pos,
                                      const float* gamma, const float* beta, float eps, float* tok, int64_t ldo, int n,
                                      int G2, int C, void* stream) {
  GCD_CHECK_ARG(patch && cls && pos && gamma && beta && tok, "gcd_clip_tokens_ln_pre: null pointer");
  GCD_CHECK_ARG(n > 0 && G2 > 0 && C > 0, "gcd_clip_tokens_ln_pre: empty problem n=%d G2=%d C=%d", n, G2, C);
  GCD_CHECK_ARG(C <= GCD_CLIP_MAX_MODEL_WIDTH, "gcd_clip_tokens_ln_pre: C=%d exceeds %d", C, GCD_CLIP_MAX_MODEL_WIDTH);
  GCD_CHECK_ARG(ldp >= C && ldo >= C, "gcd_clip_tokens_ln_pre: row strides (%lld, %lld) below C=%d", (long long)ldp,
                (long long)ldo, C);
  GCD_CHECK_ARG((((uintptr_t)patch | (uintptr_t)cls | (uintptr_t)pos | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)tok) & 3) == 0,
                "gcd_clip_tokens_ln_pre: misaligned pointer (4 bytes)");
  GCD_CHECK_ARG(eps >= 0.0f, "gcd_clip_tokens_ln_pre: eps=%g", (double)eps);
  const int64_t rows = (int64_t)n * (G2 + 1);
  GCD_CHECK_ARG(rows < (1ll << 31), "gcd_clip_tokens_ln_pre: grid too large");
  hipLaunchKernelGGL(tokens_ln_pre_kernel, dim3((unsigned)rows), dim3(NT), (size_t)C * sizeof(float), (hipStream_t)stream,
                     patch, ldp, cls, pos, gamma, beta, eps, tok, ldo, G2, C);
  GCD_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int gcd_clip_attn_f16(const void* qkv, int64_t ld, void* out, int64_t ldo, int n, int S, int heads,
                                 int q_prescaled, void* stream) {
  GCD_CHECK_ARG(qkv && out, "gcd_clip_attn_f16: null pointer");
  GCD_CHECK_ARG(n > 0 && S > 0 && heads > 0, "gcd_clip_attn_f16: empty problem n=%d S=%d heads=%d", n, S, heads);
  GCD_CHECK_ARG(S <= GCD_CLIP_ATTN_MAX_S, "gcd_clip_attn_f16: S=%d exceeds %d keys (K and V of one head live in LDS)", S,
                GCD_CLIP_ATTN_MAX_S);
  GCD_CHECK_ARG(heads <= 4096 && (int64_t)n * heads < (1ll << 31), "gcd_clip_attn_f16: grid too large");
  GCD_CHECK_ARG(ld % 8 == 0 && ld >= 3 * (int64_t)heads * HD && ((uintptr_t)qkv & 15) == 0,
                "gcd_clip_attn_f16: qkv needs 16-byte aligned rows of at least 3 * heads * 80 columns (ld=%lld; the head "
                "dim is 80)", (long long)ld);
  GCD_CHECK_ARG(ldo >= (int64_t)heads * HD && ((uintptr_t)out & 1) == 0, "gcd_clip_attn_f16: ldo=%lld below heads * 80",
                (long long)ldo);
  const float log2e = 1.4426950408889634f;
  const float scale_log2 = q_prescaled ? 1.0f : log2e / sqrtf((float)HD);
  hipStream_t s = (hipStream_t)stream;
  if (S <= 32) return attn_launch<2>((const f16*)qkv, ld, (f16*)out, ldo, n, S, heads, scale_log2, s);
  if (S <= 96) return attn_launch<6>((const f16*)qkv, ld, (f16*)out, ldo, n, S, heads, scale_log2, s);
  return attn_launch<GCD_CLIP_ATTN_MAX_S / 16>((const f16*)qkv, ld, (f16*)out, ldo, n, S, heads, scale_log2, s);
}

extern "C" int gcd_clip_bias_gelu_f16(const float* h, int64_t ldh, const float* bias, void* out16, int64_t ldo, int64_t M,
                                      int N, void* stream) {
  GCD_CHECK_ARG(h && bias && out16, "gcd_clip_bias_gelu_f16: null pointer");
  GCD_CHECK_ARG(M > 0 && N > 0, "gcd_clip_bias_gelu_f16: empty problem M=%lld N=%d", (long long)M, N);
  GCD_CHECK_ARG(N % 4 == 0 && ldh % 4 == 0 && ldo % 4 == 0 && ldh >= N && ldo >= N,
                "gcd_clip_bias_gelu_f16: N=%d, ldh=%lld, ldo=%lld must be multiples of 4, the strides at least N", N,
                (long long)ldh, (long long)ldo);
  GCD_CHECK_ARG(((uintptr_t)h & 15) == 0 && ((uintptr_t)bias & 15) == 0 && ((uintptr_t)out16 & 7) == 0,
                "gcd_clip_bias_gelu_f16: misaligned pointer (h, bias: 16 bytes; out16: 8 bytes)");
  const int64_t blocks = (M * (N / 4) + NT - 1) / NT;
  GCD_CHECK_ARG(blocks < (1ll << 31), "gcd_clip_bias_gelu_f16: grid too large");
  hipLaunchKernelGGL(bias_gelu_kernel, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, h, ldh, bias, (f16*)out16,
                     ldo, M, N / 4);
  GCD_CHECK_HIP(hipGetLastError());
  return 0;
}
