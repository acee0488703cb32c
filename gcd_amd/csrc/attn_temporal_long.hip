// attn_temporal_long.hip — temporal self-attention over clips of up to 64 frames (head dim 64, softmax scale 1/8).
//
// The T <= 16 kernels of attention.hip / backward.hip hold one problem (clip, pixel, head) in ONE 16 x 16 MFMA tile
// (forward) or in 19 KB of fp32 LDS (backward).  Here a problem spans nb = ceil(T / 16) <= 4 key and query blocks of
// 16 frames; the two entries take the argument lists of gcd_attn_temporal_f16 / gcd_attn_temporal_bwd and the host
// dispatches T = 17..64 to them (T <= 16 keeps the old kernels, bit for bit).
//
//  * gcd_attn_temporal_long_f16: one problem per wave, attn_temporal_mfma_kernel generalised over nb blocks.  The
//    q|k|v fragments of all blocks are loaded once (16-byte row pieces straight into the MFMA A / B layouts); V goes
//    through a wave-private LDS tile of nb x 16 rows for the one transposed read.  Per query block qb:
//      S^T(kb, qb) = K_kb Q_qb^T    2 x v_mfma_f32_16x16x32_f16 per key block, [key 4 (l >> 4) + e][query l & 15];
//      softmax                      nb x 4 scores per lane + v_permlane16_swap / v_permlane32_swap (as the T <= 16 kernel);
//      O^T_qb = sum_kb V_kb^T P^T   P as fp16 hi + lo (no new rounding); two key blocks per v_mfma_f32_16x16x32_f16
//                                   (the k slot order of the pair is (block, 4 (l >> 4) + e) on both operands; an odd
//                                   last block is paired with zeros).
//    Rows >= T load a clamped (valid) row and are masked.
//  * gcd_attn_temporal_long_bwd: one problem per wave (one wave per workgroup).  q, k, v (fp16) and dO (fp32, never
//    rounded) go to wave-private LDS once; the products run on MFMA tiles in the orientation [query][key]:
//      pass A (per query block): S = Q K^T (f16 MFMA), dP = dO V^T (exact-fp32 v_mfma_f32_16x16x4_f32), the row
//      statistics (max, 1 / sum, D = rowsum(P o dP)) over 16-lane shuffles, dS = P o (dP - D) * scale and
//      dQ = dS K (dS transposed through a 1 KB LDS tile; K read from LDS in the accumulator layout);
//      pass B (per key block): S, dP recomputed, dV = P^T dO and dK = dS^T Q with the P / dS accumulator tiles as the
//      A operand of v_mfma_f32_16x16x4_f32 (the k index is the tile's row = the query).
#include "common.h"

#define TL_ROW 144   // bytes per fp16 row (64 channels) in LDS: 128 + 16 pad
#define TL_GROW 68   // floats per fp32 dO row in LDS: 64 + 4 pad

// ------------------------------------------------------------------------------------------------ forward
template <int NB>
__global__ __launch_bounds__(256) void attn_temporal_long_kernel(const f16* __restrict__ qkv, int64_t ld,
                                                                 f16* __restrict__ out, int64_t ldo, int nprob,
                                                                 int T, int HW, int heads) {
  __shared__ __attribute__((aligned(16))) char vs_all[4 * NB * 16 * TL_ROW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  char* const vs = vs_all + wave * NB * 16 * TL_ROW;
  const int r15 = lane & 15, q = lane >> 4;
  const int C = heads * 64;
  const float cs = 0.125f * 1.4426950408889634f;   // 1 / sqrt(64) in exp2 units
  for (int pid = (int)blockIdx.x * 4 + wave; pid < nprob; pid += (int)gridDim.x * 4) {
    const int h = pid % heads;
    const int rest = pid / heads;
    const int s = rest % HW, b = rest / HW;
    const int64_t row0 = (int64_t)b * T * HW + s;
    // ---- q|k|v rows 16 kb + (l & 15) (clamped to T - 1), channels 8 (l >> 4) .. + 7 and + 32 ----
    f16x8 kf[NB][2], qf[NB][2], vf[NB][2];
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) {
      const int t = 16 * kb + r15;
      const int fr = t < T ? t : T - 1;
      const f16* src = qkv + (row0 + (int64_t)fr * HW) * ld + h * 64 + 8 * q;
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2) {
        qf[kb][k2] = *(const f16x8*)(src + 32 * k2);
        kf[kb][k2] = *(const f16x8*)(src + C + 32 * k2);
        vf[kb][k2] = *(const f16x8*)(src + 2 * C + 32 * k2);
      }
    }
    // ---- V rows -> the wave's LDS tile; V^T fragments back: va[kb][cb][e] = V[16 kb + 4 q + e][16 cb + r15] ----
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) {
      *(f16x8*)(vs + (16 * kb + r15) * TL_ROW + 16 * q) = vf[kb][0];
      *(f16x8*)(vs + (16 * kb + r15) * TL_ROW + 64 + 16 * q) = vf[kb][1];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    f16x4 va[NB][4];
#pragma unroll
    for (int kb = 0; kb < NB; ++kb)
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          va[kb][cb][e] = *(const f16*)(vs + (16 * kb + 4 * q + e) * TL_ROW + (16 * cb + r15) * 2);
    // the tile's reads are done before the next problem's V rows overwrite it
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __builtin_amdgcn_wave_barrier();

#pragma unroll
    for (int qb = 0; qb < NB; ++qb) {
      // ---- S^T(kb, qb) = K_kb Q_qb^T ----
      f32x4 st[NB];
#pragma unroll
      for (int kb = 0; kb < NB; ++kb) {
        st[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
        st[kb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[kb][0], qf[qb][0], st[kb], 0, 0, 0);
        st[kb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[kb][1], qf[qb][1], st[kb], 0, 0, 0);
      }
      // ---- softmax of query 16 qb + r15 over the keys 16 kb + 4 q + e ----
      float mx = -INFINITY;
#pragma unroll
      for (int kb = 0; kb < NB; ++kb)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (kb == NB - 1 && 16 * kb + 4 * q + e >= T) st[kb][e] = -INFINITY;   // (16 (NB - 1) < T <= 16 NB)
          mx = fmaxf(mx, st[kb][e]);
        }
      {
        const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
        mx = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
        const auto c = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
        mx = fmaxf(__uint_as_float(c[0]), __uint_as_float(c[1]));
      }
      float l = 0.f;
#pragma unroll
      for (int kb = 0; kb < NB; ++kb)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          st[kb][e] = __builtin_amdgcn_exp2f((st[kb][e] - mx) * cs);   // exp2(-inf) = 0 for the masked keys
          l += st[kb][e];
        }
      {
        const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(l), __float_as_uint(l), false, false);
        l = __uint_as_float(a[0]) + __uint_as_float(a[1]);
        const auto c = __builtin_amdgcn_permlane32_swap(__float_as_uint(l), __float_as_uint(l), false, false);
        l = __uint_as_float(c[0]) + __uint_as_float(c[1]);
      }
      const float inv = 1.0f / l;
      f16x4 phi[NB], plo[NB];
#pragma unroll
      for (int kb = 0; kb < NB; ++kb)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float pv = st[kb][e] * inv;
          phi[kb][e] = (f16)pv;
          plo[kb][e] = (f16)(pv - (float)phi[kb][e]);
        }
      // ---- O^T_qb = sum_kb V_kb^T P^T(kb, qb), 16 channels at a time ----
      const int tq = 16 * qb + r15;
      f16* const dst = out + (row0 + (int64_t)tq * HW) * ldo + h * 64 + 4 * q;
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        // (an odd last block is paired with zeros: one MFMA shape on the accumulator chain)
#pragma unroll
        for (int kb = 0; kb < NB; kb += 2) {
          const f16x4 z = {};
          const f16x8 a8 = __builtin_shufflevector(va[kb][cb], kb + 1 < NB ? va[kb + 1][cb] : z, 0, 1, 2, 3, 4, 5, 6, 7);
          const f16x8 h8 = __builtin_shufflevector(phi[kb], kb + 1 < NB ? phi[kb + 1] : z, 0, 1, 2, 3, 4, 5, 6, 7);
          const f16x8 l8 = __builtin_shufflevector(plo[kb], kb + 1 < NB ? plo[kb + 1] : z, 0, 1, 2, 3, 4, 5, 6, 7);
          o = __builtin_amdgcn_mfma_f32_16x16x32_f16(a8, h8, o, 0, 0, 0);
          o = __builtin_amdgcn_mfma_f32_16x16x32_f16(a8, l8, o, 0, 0, 0);
        }
        if (tq < T) {
          f16x4 ov;
#pragma unroll
          for (int e = 0; e < 4; ++e) ov[e] = (f16)o[e];
          *(f16x4*)(dst + 16 * cb) = ov;
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ backward
// Fragments read from the wave's LDS copy of a problem (rows = frames, zero past T):
//   natural layout     lane (g = l >> 4, r = l & 15) holds row 16 blk + r, channels of chunk g;
//   accumulator layout lane (g, r) holds rows 16 blk + 4 g + e (e = 0..3), channel 16 cb + r.
struct TlBwdSmem {
  char* qs;    // fp16 [R][TL_ROW bytes]
  char* ks;
  char* vs;
  float* gs;   // fp32 [R][TL_GROW]
};

// S(qb, kb) = Q_qb K_kb^T and dP(qb, kb) = dO_qb V_kb^T as [query 16 qb + 4 g + e][key 16 kb + r].  S: the
// k order of the f16 MFMA is channel 32 k2 + 8 g + j on both operands; dP: step i of the fp32 MFMA takes channel
// 16 g + i on both operands.
__device__ __forceinline__ void tl_bwd_tiles(const TlBwdSmem& sm, int qb, int kb, int g, int r, f32x4& s,
                                             f32x4& dp) {
  const char* qrow = sm.qs + (16 * qb + r) * TL_ROW;
  const char* krow = sm.ks + (16 * kb + r) * TL_ROW;
  s = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k2 = 0; k2 < 2; ++k2)
    s = __builtin_amdgcn_mfma_f32_16x16x32_f16(*(const f16x8*)(qrow + 64 * k2 + 16 * g),
                                               *(const f16x8*)(krow + 64 * k2 + 16 * g), s, 0, 0, 0);
  const float* grow = sm.gs + (16 * qb + r) * TL_GROW + 16 * g;
  const char* vrow = sm.vs + (16 * kb + r) * TL_ROW + 32 * g;
  dp = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i8 = 0; i8 < 2; ++i8) {
    const f16x8 v8 = *(const f16x8*)(vrow + 16 * i8);
    const f32x4 g0 = *(const f32x4*)(grow + 8 * i8);
    const f32x4 g1 = *(const f32x4*)(grow + 8 * i8 + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) dp = __builtin_amdgcn_mfma_f32_16x16x4f32(g0[j], (float)v8[j], dp, 0, 0, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) dp = __builtin_amdgcn_mfma_f32_16x16x4f32(g1[j], (float)v8[4 + j], dp, 0, 0, 0);
  }
}

// sum / max over the 16 lanes of a row group (lanes with the same l >> 4)
__device__ __forceinline__ float tl_row_sum(float v) {
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ float tl_row_max(float v) {
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) v = fmaxf(v, __shfl_xor(v, m));
  return v;
}

template <int NB>
__global__ __launch_bounds__(64) void attn_temporal_long_bwd_kernel(const f16* __restrict__ qkv, int64_t ld,
                                                                    const float* __restrict__ dO, int64_t lddo,
                                                                    float* __restrict__ dqkv, int64_t lddq,
                                                                    int nprob, int T, int HW, int heads,
                                                                    float scale) {
  constexpr int R = NB * 16;
  __shared__ __attribute__((aligned(16))) char qs[R * TL_ROW], ks[R * TL_ROW], vs[R * TL_ROW];
  __shared__ __attribute__((aligned(16))) float gs[R * TL_GROW];
  __shared__ float xs[16 * 17];                     // dS tile transpose
  __shared__ float st_m[R], st_inv[R], st_d[R];     // row statistics: max * cs, 1 / sum, D
  const TlBwdSmem sm{qs, ks, vs, gs};
  const int lane = threadIdx.x, g = lane >> 4, r = lane & 15;
  const int C = heads * 64;
  const float cs = scale * 1.4426950408889634f;
  for (int pid = (int)blockIdx.x; pid < nprob; pid += (int)gridDim.x) {
    const int h = pid % heads;
    const int rest = pid / heads;
    const int s = rest % HW, b = rest / HW;
    const int64_t row0 = (int64_t)b * T * HW + s;
    // ---- the problem -> LDS (rows >= T zero) ----
#pragma unroll
    for (int tb = 0; tb < NB; ++tb) {
      const int t = 16 * tb + r;
      const int fr = t < T ? t : T - 1;
      const int64_t row = row0 + (int64_t)fr * HW;
      const f16* src = qkv + row * ld + h * 64 + 8 * g;
      const float* gsrc = dO + row * lddo + h * 64 + 16 * g;
      f16x8 q8[2], k8[2], v8[2];
      f32x4 g4[4];
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2) {
        q8[k2] = *(const f16x8*)(src + 32 * k2);
        k8[k2] = *(const f16x8*)(src + C + 32 * k2);
        v8[k2] = *(const f16x8*)(src + 2 * C + 32 * k2);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) g4[i] = *(const f32x4*)(gsrc + 4 * i);
      if (t >= T) {
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) q8[k2] = k8[k2] = v8[k2] = f16x8{};
#pragma unroll
        for (int i = 0; i < 4; ++i) g4[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2) {
        *(f16x8*)(qs + t * TL_ROW + 64 * k2 + 16 * g) = q8[k2];
        *(f16x8*)(ks + t * TL_ROW + 64 * k2 + 16 * g) = k8[k2];
        *(f16x8*)(vs + t * TL_ROW + 64 * k2 + 16 * g) = v8[k2];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) *(f32x4*)(gs + t * TL_GROW + 16 * g + 4 * i) = g4[i];
    }
    __syncthreads();

    // ---- pass A: per query block, row statistics and dQ ----
    for (int qb = 0; qb < NB; ++qb) {
      f32x4 sv[NB], dp[NB];
#pragma unroll
      for (int kb = 0; kb < NB; ++kb) tl_bwd_tiles(sm, qb, kb, g, r, sv[kb], dp[kb]);
      float m[4], inv[4], D[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < NB; ++kb) {
          if (kb == NB - 1 && 16 * kb + r >= T) sv[kb][e] = -INFINITY;   // (16 (NB - 1) < T <= 16 NB)
          mx = fmaxf(mx, sv[kb][e]);
        }
        m[e] = tl_row_max(mx) * cs;
        float l = 0.f;
#pragma unroll
        for (int kb = 0; kb < NB; ++kb) l += __builtin_amdgcn_exp2f(sv[kb][e] * cs - m[e]);
        inv[e] = 1.0f / tl_row_sum(l);
        float d = 0.f;
#pragma unroll
        for (int kb = 0; kb < NB; ++kb) {
          sv[kb][e] = __builtin_amdgcn_exp2f(sv[kb][e] * cs - m[e]) * inv[e];   // P
          d = fmaf(sv[kb][e], dp[kb][e], d);
        }
        D[e] = tl_row_sum(d);
#pragma unroll
        for (int kb = 0; kb < NB; ++kb) dp[kb][e] = sv[kb][e] * (dp[kb][e] - D[e]) * scale;   // dS
      }
      if (r == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          st_m[16 * qb + 4 * g + e] = m[e];
          st_inv[16 * qb + 4 * g + e] = inv[e];
          st_d[16 * qb + 4 * g + e] = D[e];
        }
      }
      // dQ(qb, cb) = sum_kb dS(qb, kb) K(kb, cb): A = dS[query r][key 4 g + i] (the tile transposed), B = K in the
      // accumulator layout; out [query 16 qb + 4 g + e][channel 16 cb + r]
      f32x4 dq[4];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) dq[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kb = 0; kb < NB; ++kb) {
#pragma unroll
        for (int e = 0; e < 4; ++e) xs[(4 * g + e) * 17 + r] = dp[kb][e];
        __syncthreads();
        float a[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = xs[r * 17 + 4 * g + i];
        __syncthreads();
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float kv = (float)*(const f16*)(ks + (16 * kb + 4 * g + i) * TL_ROW + (16 * cb + r) * 2);
            dq[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], kv, dq[cb], 0, 0, 0);
          }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int t = 16 * qb + 4 * g + e;
        if (t < T) {
          float* dst = dqkv + (row0 + (int64_t)t * HW) * lddq + h * 64 + r;
#pragma unroll
          for (int cb = 0; cb < 4; ++cb) dst[16 * cb] = dq[cb][e];
        }
      }
    }
    __syncthreads();   // row statistics visible to every lane

    // ---- pass B: per key block, dK and dV ----
    for (int kb = 0; kb < NB; ++kb) {
      f32x4 dk[4], dv[4];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) dk[cb] = dv[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
      const bool kvalid = 16 * kb + r < T;
      for (int qb = 0; qb < NB; ++qb) {
        f32x4 sv, dp;
        tl_bwd_tiles(sm, qb, kb, g, r, sv, dp);
        float p[4], dsv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int t = 16 * qb + 4 * g + e;
          p[e] = kvalid ? __builtin_amdgcn_exp2f(sv[e] * cs - st_m[t]) * st_inv[t] : 0.f;
          dsv[e] = p[e] * (dp[e] - st_d[t]) * scale;
        }
        // dV(kb, cb) += P^T dO, dK(kb, cb) += dS^T Q: A = the [query 4 g + e][key r] tile (k = query),
        // B = dO / Q in the accumulator layout; out [key 16 kb + 4 g + e][channel 16 cb + r]
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int t = 16 * qb + 4 * g + e;
            const float go = gs[t * TL_GROW + 16 * cb + r];
            const float qv = (float)*(const f16*)(qs + t * TL_ROW + (16 * cb + r) * 2);
            dv[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[e], go, dv[cb], 0, 0, 0);
            dk[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(dsv[e], qv, dk[cb], 0, 0, 0);
          }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int t = 16 * kb + 4 * g + e;
        if (t < T) {
          float* dst = dqkv + (row0 + (int64_t)t * HW) * lddq + h * 64 + r;
#pragma unroll
          for (int cb = 0; cb < 4; ++cb) {
            dst[C + 16 * cb] = dk[cb][e];
            dst[2 * C + 16 * cb] = dv[cb][e];
          }
        }
      }
    }
    __syncthreads();   // the LDS copy is read to the end before the next problem overwrites it
  }
}

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" int gcd_attn_temporal_long_f16(const void* qkv, int64_t ld, void* out, int64_t ldo, int clips, int T,
                                          int HW, int heads, void* stream) {
  GCD_CHECK_ARG(qkv && out, "gcd_attn_temporal_long_f16: null pointer");
  GCD_CHECK_ARG(clips > 0 && HW > 0 && heads > 0, "gcd_attn_temporal_long_f16: empty problem");
  GCD_CHECK_ARG(T >= 1 && T <= 64, "gcd_attn_temporal_long_f16: T=%d (supported: 1..64 frames)", T);
  GCD_CHECK_ARG(ld % 8 == 0 && ld >= 3 * heads * 64 && ldo % 4 == 0 && ldo >= heads * 64 &&
                    ((uintptr_t)qkv & 15) == 0 && ((uintptr_t)out & 7) == 0,
                "gcd_attn_temporal_long_f16: ld=%lld ldo=%lld (ld a multiple of 8 >= 3C, ldo a multiple of 4 >= C, "
                "16-byte aligned q|k|v)", (long long)ld, (long long)ldo);
  const int64_t nprob = (int64_t)clips * HW * heads;
  GCD_CHECK_ARG(nprob < (1ll << 31) - 8192, "gcd_attn_temporal_long_f16: %lld problems", (long long)nprob);
  // 4 problems per workgroup; at most 2048 workgroups walk the problems (8 per CU)
  int64_t blocks = (nprob + 3) / 4;
  if (blocks > 2048) blocks = 2048;
  const hipStream_t st = (hipStream_t)stream;
  const f16* a = (const f16*)qkv;
  f16* o = (f16*)out;
  const int np = (int)nprob;
  switch ((T + 15) / 16) {
    case 1: hipLaunchKernelGGL(attn_temporal_long_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, a, ld, o, ldo, np, T, HW, heads); break;
    case 2: hipLaunchKernelGGL(attn_temporal_long_kernel<2>, dim3((unsigned)blocks), dim3(256), 0, st, a, ld, o, ldo, np, T, HW, heads); break;
    case 3: hipLaunchKernelGGL(attn_temporal_long_kernel<3>, dim3((unsigned)blocks), dim3(256), 0, st, a, ld, o, ldo, np, T, HW, heads); break;
    default: hipLaunchKernelGGL(attn_temporal_long_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, st, a, ld, o, ldo, np, T, HW, heads); break;
  }
  GCD_CHECK_LAUNCH();
  return 0;
}

extern "C" int gcd_attn_temporal_long_bwd(const void* qkv16, int64_t ld, const float* dO, int64_t lddo, float* dqkv,
                                          int64_t lddq, int clips, int T, int HW, int heads, void* stream) {
  GCD_CHECK_ARG(qkv16 && dO && dqkv, "gcd_attn_temporal_long_bwd: null pointer");
  GCD_CHECK_ARG(clips > 0 && HW > 0 && heads > 0, "gcd_attn_temporal_long_bwd: empty problem");
  GCD_CHECK_ARG(T >= 1 && T <= 64, "gcd_attn_temporal_long_bwd: T=%d (supported: 1..64 frames)", T);
  GCD_CHECK_ARG(ld % 8 == 0 && ld >= 3 * heads * 64 && lddo % 4 == 0 && lddo >= heads * 64 &&
                    lddq >= 3 * heads * 64 && ((uintptr_t)qkv16 & 15) == 0 && ((uintptr_t)dO & 15) == 0,
                "gcd_attn_temporal_long_bwd: ld=%lld lddo=%lld lddq=%lld (ld a multiple of 8 >= 3C, lddo a multiple "
                "of 4 >= C, lddq >= 3C, 16-byte aligned q|k|v and dO)", (long long)ld, (long long)lddo,
                (long long)lddq);
  const int64_t nprob = (int64_t)clips * HW * heads;
  GCD_CHECK_ARG(nprob < (1ll << 31), "gcd_attn_temporal_long_bwd: %lld problems", (long long)nprob);
  // one problem per workgroup (one wave); at most 2048 workgroups walk the problems
  const int64_t blocks = nprob < 2048 ? nprob : 2048;
  const hipStream_t st = (hipStream_t)stream;
  const f16* a = (const f16*)qkv16;
  const int np = (int)nprob;
  switch ((T + 15) / 16) {
    case 1: hipLaunchKernelGGL(attn_temporal_long_bwd_kernel<1>, dim3((unsigned)blocks), dim3(64), 0, st, a, ld, dO, lddo, dqkv, lddq, np, T, HW, heads, 0.125f); break;
    case 2: hipLaunchKernelGGL(attn_temporal_long_bwd_kernel<2>, dim3((unsigned)blocks), dim3(64), 0, st, a, ld, dO, lddo, dqkv, lddq, np, T, HW, heads, 0.125f); break;
    case 3: hipLaunchKernelGGL(attn_temporal_long_bwd_kernel<3>, dim3((unsigned)blocks), dim3(64), 0, st, a, ld, dO, lddo, dqkv, lddq, np, T, HW, heads, 0.125f); break;
    default: hipLaunchKernelGGL(attn_temporal_long_bwd_kernel<4>, dim3((unsigned)blocks), dim3(64), 0, st, a, ld, dO, lddo, dqkv, lddq, np, T, HW, heads, 0.125f); break;
  }
  GCD_CHECK_LAUNCH();
  return 0;
}
