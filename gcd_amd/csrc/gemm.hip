// gemm.hip — fp16 x fp16 -> fp32 MFMA GEMM family for gfx950 (MI355X).
//
// One kernel template serves every contraction of the VideoUNet forward (81 % of the step's
// FLOPs): nn.Linear, Conv2d 3x3 (stride 1/2, optional fused nearest-x2 upsample),
// Conv2d 1x1 and the (3,1,1) temporal Conv3d, all as (implicit) GEMMs over token-major fp16
// activations:   out[m, n] = epilogue( sum_k A(m, k) * W[n, k] ).
//
// CDNA4 mapping
//   * 256-thread workgroup = 4 waves (2x2), block tile BM x BN (128x128 or 128x160 — every channel
//     count of the SVD UNet is a multiple of 320, so 160 divides all N), K step 64.
//   * A and W tiles go HBM/L2 -> LDS with global_load_lds_dwordx4 (LDS-DMA, no VGPR round trip).
//     The LDS image is lane-linear, so the bank swizzle is applied to the per-lane *source* chunk
//     and undone with the same XOR on the ds_read_b128 side (lds_tile_off).
//   * The A address generator is the implicit-GEMM gather: each lane owns BM/32 tile rows for the
//     whole K loop and re-derives (tap, dy, dx | dt) only when the K step crosses a tap boundary;
//     out-of-image taps read a device zero page instead of branching around the DMA.
//   * v_mfma_f32_16x16x32_f16 with the operands swapped (W is the "A" operand): the accumulator
//     layout then gives every lane 4 consecutive output channels of one token, so bias, residual
//     and output accesses are 16-byte vectors.
//   * Double-buffered LDS, one barrier per K step: wait(tile k) -> barrier -> issue DMA(tile k+1)
//     -> MFMA(tile k).
//   * blockIdx -> tile mapping is XCD-aware: the 8 XCDs each own a contiguous range of tiles and
//     sweep N fastest, so an A row-panel is fetched from HBM once and re-read from that XCD's L2.
//   * Epilogue fuses bias, per-frame vectors (timestep embedding / collapsed 1-key cross-attention),
//     up to two fp32 residual streams with AlphaBlender scaling, GEGLU, and the fp16 down-cast.
#include "gemm_common.h"


typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// BF16: the two operands are bfloat16 instead of fp16 (gcd_gemm_desc.operand_bf16; PLAIN mode, fp32
// output): the same 16-bit staging, swizzle and fragment reads, v_mfma_f32_16x16x32_bf16 instead of
// ..._f16 — same shape, same rate on gfx950; bf16 buys exponent range (gradients without loss scaling),
// not speed, and costs 3 mantissa bits.
template <int BM, int BN, int WM, int WN, int MODE, bool BF16 = false>
__global__ __launch_bounds__(256, 2) void gemm_f16_kernel(const GemmK p) {
  constexpr int TM = WM / 16, TN = WN / 16;
  constexpr int WAVES_N = BN / WN;
  static_assert((BM / WM) * (BN / WN) == 4, "4 waves per workgroup");
  constexpr int A_ROUNDS = BM / 32, W_ROUNDS = BN / 32;
  constexpr int A_BYTES = BM * 128, W_BYTES = BN * 128, STAGE_BYTES = A_BYTES + W_BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wave = t >> 6;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;

  // ---- XCD-aware tile assignment (bijective for any grid size) ----
  int tile_m, tile_n;
  {
    const int nblk = gridDim.x, bid = blockIdx.x;
    const int q = nblk >> 3, r = nblk & 7;
    const int xcd = bid & 7, idx = bid >> 3;
    const int L = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    tile_m = L / p.tiles_n;
    tile_n = L - tile_m * p.tiles_n;
  }
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  // ---- per-thread staging bookkeeping ----
  const int prow = t >> 3;                              // tile row within a staging round
  const int cl = (t & 7) ^ ((prow >> 1) & 7);           // logical 16-B chunk this lane fetches

  int64_t a_off[A_ROUNDS];   // PLAIN: element offset of the row; conv modes: see below
  int a_y[A_ROUNDS], a_x[A_ROUNDS];
  bool a_ok[A_ROUNDS];
#pragma unroll
  for (int i = 0; i < A_ROUNDS; ++i) {
    const int m = m0 + prow + 32 * i;
    a_ok[i] = m < p.M;
    if (MODE == GCD_GEMM_PLAIN) {
      const int mc = a_ok[i] ? m : p.M - 1;
      a_off[i] = (int64_t)mc * p.lda + cl * 8;
      a_y[i] = a_x[i] = 0;
    } else if (MODE == GCD_GEMM_CONV3X3) {
      const int hw = p.Ho * p.Wo;
      const int n = m / hw;
      const int rem = m - n * hw;
      a_y[i] = rem / p.Wo;
      a_x[i] = rem - a_y[i] * p.Wo;
      a_off[i] = (int64_t)n * p.Hi * p.Wi;              // frame base, in pixels
    } else {  // TEMPORAL3
      const int fr = m / p.HW;
      a_y[i] = fr % p.T;                                 // frame index within its clip
      a_x[i] = 0;
      a_off[i] = (int64_t)m;                             // row index
    }
  }
  int64_t w_off[W_ROUNDS];
#pragma unroll
  for (int i = 0; i < W_ROUNDS; ++i) {
    int n = n0 + prow + 32 * i;
    n = n < p.N ? n : p.N - 1;
    w_off[i] = (int64_t)n * p.K + cl * 8;
  }

  // K-step state for the conv address generators (block-uniform)
  int tap = 0, c0 = 0;

  auto stage = [&](int k0, int buf) {
    char* As = smem + buf * STAGE_BYTES;
    char* Ws = As + A_BYTES;
    int dy = 0, dx = 0;
    if (MODE == GCD_GEMM_CONV3X3) {
      dy = tap / 3 - 1;
      dx = tap - (tap / 3) * 3 - 1;
    } else if (MODE == GCD_GEMM_TEMPORAL3) {
      dy = tap - 1;
    }
#pragma unroll
    for (int i = 0; i < A_ROUNDS; ++i) {
      const f16* src;
      if (MODE == GCD_GEMM_PLAIN) {
        src = p.A + a_off[i] + k0;
      } else if (MODE == GCD_GEMM_CONV3X3) {
        int iy, ix;
        bool ok = a_ok[i];
        if (p.up) {
          const int uy = a_y[i] + dy, ux = a_x[i] + dx;
          ok = ok && uy >= 0 && uy < p.Ho && ux >= 0 && ux < p.Wo;
          iy = uy >> 1;
          ix = ux >> 1;
        } else {
          iy = a_y[i] * p.stride + dy + p.asym;
          ix = a_x[i] * p.stride + dx + p.asym;
          ok = ok && iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi;
        }
        src = ok ? p.A + (a_off[i] + (int64_t)iy * p.Wi + ix) * p.lda + c0 + cl * 8
                 : p.zero + cl * 8;
      } else {
        const int tt = a_y[i] + dy;
        const bool ok = a_ok[i] && tt >= 0 && tt < p.T;
        src = ok ? p.A + (a_off[i] + (int64_t)dy * p.HW) * p.lda + c0 + cl * 8 : p.zero + cl * 8;
      }
      glds16(src, As + (i * 256 + wave * 64) * 16);
    }
#pragma unroll
    for (int i = 0; i < W_ROUNDS; ++i) glds16(p.W + w_off[i] + k0, Ws + (i * 256 + wave * 64) * 16);
    // advance the tap state to the next K step
    if (MODE != GCD_GEMM_PLAIN) {
      c0 += 64;
      if (c0 >= p.Cin) {
        c0 = 0;
        ++tap;
      }
    }
  };

  f32x4 acc[TN][TM];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nk = p.K >> 6;
  stage(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // my DMA pieces of tile kt have landed
    __syncthreads();                                    // ... and everybody else's; tile kt-1 is consumed
    if (kt + 1 < nk) stage((kt + 1) << 6, buf ^ 1);
    const char* As = smem + buf * STAGE_BYTES;
    const char* Ws = As + A_BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int chunk = ks * 4 + (lane >> 4);
      f16x8 af[TM], wf[TN];
#pragma unroll
      for (int j = 0; j < TM; ++j)
        af[j] = *(const f16x8*)(As + lds_tile_off(wm * WM + j * 16 + (lane & 15), chunk));
#pragma unroll
      for (int i = 0; i < TN; ++i)
        wf[i] = *(const f16x8*)(Ws + lds_tile_off(wn * WN + i * 16 + (lane & 15), chunk));
#pragma unroll
      for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j)
          if constexpr (BF16)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf[i]),
                                                                __builtin_bit_cast(bf16x8, af[j]), acc[i][j], 0, 0, 0);
          else
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[i], af[j], acc[i][j], 0, 0, 0);
    }
  }

  // ---- epilogue: lane holds out[m][nb .. nb+3] for (i = n-tile, j = m-tile) ----
  // Bias vectors are loaded once, and the residual vectors of m-tile j + 1 are requested before the
  // stores of m-tile j are issued: the output may alias the residual, so written naively every load
  // would wait (vmcnt(0)) for the previous store as well (see gemm_common.h).
  const int nq = (lane >> 4) * 4;
  if (p.out_kind != GCD_OUT_GEGLU) {
    f32x4 bv[TN];
#pragma unroll
    for (int i = 0; i < TN; ++i) {
      const int n = n0 + wn * WN + i * 16 + nq;
      bv[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (p.bias && n < p.N) bv[i] = *(const f32x4*)(p.bias + n);
    }
    f32x4 q1[2][TN], q2[2][TN];
    auto fetch = [&](int j, int slot) {
      int m = m0 + wm * WM + j * 16 + (lane & 15);
      m = m < p.M ? m : p.M - 1;
#pragma unroll
      for (int i = 0; i < TN; ++i) {
        int n = n0 + wn * WN + i * 16 + nq;
        n = n < p.N ? n : p.N - 4;
        if (p.R1) q1[slot][i] = *(const f32x4*)(p.R1 + (int64_t)m * p.ldr1 + n);
        if (p.R2) q2[slot][i] = *(const f32x4*)(p.R2 + (int64_t)m * p.ldr2 + n);
      }
    };
    if (p.R1 || p.R2) fetch(0, 0);
#pragma unroll
    for (int j = 0; j < TM; ++j) {
      const int m = m0 + wm * WM + j * 16 + (lane & 15);
      const int mc = m < p.M ? m : p.M - 1;
      float sa = p.s_acc, sr1 = p.s_r1, sr2 = p.s_r2;
      if (p.frame_alpha) {
        const float al = p.frame_alpha[mc / p.rows_per_alpha];
        sa = 1.0f - al;
        sr2 = al;
        if (p.r1_blend) sr1 *= 1.0f - al;
      }
      const float* rv = p.rowvec ? p.rowvec + (int64_t)(mc / p.rows_per_vec) * p.ld_rowvec : nullptr;
      f32x4 v[TN];
#pragma unroll
      for (int i = 0; i < TN; ++i) {
        int n = n0 + wn * WN + i * 16 + nq;
        n = n < p.N ? n : p.N - 4;
        v[i] = acc[i][j] + bv[i];
        if (rv) v[i] += *(const f32x4*)(rv + n);
        v[i] *= sa;
        if (p.R1) v[i] += sr1 * q1[j & 1][i];
        if (p.R2) v[i] += sr2 * q2[j & 1][i];
      }
      if ((p.R1 || p.R2) && j + 1 < TM) fetch(j + 1, (j + 1) & 1);
      if (m < p.M) {
#pragma unroll
        for (int i = 0; i < TN; ++i) {
          const int n = n0 + wn * WN + i * 16 + nq;
          if (n >= p.N) continue;
          if (p.out_kind == GCD_OUT_F32) {
            *(f32x4*)((float*)p.out + (int64_t)m * p.ldo + n) = v[i];
          } else {
            f16x4 o;
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = (f16)v[i][r];
            *(f16x4*)((f16*)p.out + (int64_t)m * p.ldo + n) = o;
          }
        }
      }
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < TM; ++j) {
    const int m = m0 + wm * WM + j * 16 + (lane & 15);
    if (m >= p.M) continue;
    if constexpr ((TN % 2) == 0) {
#pragma unroll
      for (int i = 0; i < TN; i += 2) {
        const int nt = n0 + wn * WN + i * 16;      // value rows nt.., gate rows nt+16..
        if (nt >= p.N) continue;
        f32x4 a = acc[i][j], g = acc[i + 1][j];
        if (p.bias) {
          a += *(const f32x4*)(p.bias + nt + nq);
          g += *(const f32x4*)(p.bias + nt + 16 + nq);
        }
        f16x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = (f16)(a[r] * gelu_fast(g[r]));
        *(f16x4*)((f16*)p.out + (int64_t)m * p.ldo + (nt >> 1) + nq) = o;
      }
    }
  }
}

template <int BM, int BN, int WM, int WN, int MODE, bool BF16 = false>
static int launch_gemm(const GemmK& k, hipStream_t s) {
  constexpr int smem = 2 * (BM + BN) * 128;
  static GcdPerDeviceOnce attr_once;
  auto fn = gemm_f16_kernel<BM, BN, WM, WN, MODE, BF16>;
  GCD_CHECK_HIP(attr_once.opt_in((const void*)fn, smem));
  GemmK kk = k;
  kk.tiles_m = (k.M + BM - 1) / BM;
  kk.tiles_n = (k.N + BN - 1) / BN;
  const int64_t nblk = (int64_t)kk.tiles_m * kk.tiles_n;
  GCD_CHECK_ARG(nblk > 0 && nblk < (1ll << 31), "gcd_gemm_f16: bad grid %lld", (long long)nblk);
  hipLaunchKernelGGL(fn, dim3((unsigned)nblk), dim3(256), smem, s, kk);
  GCD_CHECK_LAUNCH();
  return 0;
}

template <int MODE>
static int dispatch_tile(const GemmK& k, hipStream_t s) {
  bool use160;
  if (k.out_kind == GCD_OUT_GEGLU) {
    use160 = false;
  } else {
    const int pad128 = (k.N + 127) / 128 * 128, pad160 = (k.N + 159) / 160 * 160;
    use160 = pad160 <= pad128;
  }
  // few 128-row tiles (the 9 x 16 bottleneck level: M = 4032): 64-row tiles double the number of
  // workgroups so that two are resident per CU
  const int64_t tiles128 = (int64_t)((k.M + 127) / 128) * ((k.N + 159) / 160);
  const int impl = gcd_tune_get(GCD_TUNE_GEMM_IMPL);
  if constexpr (MODE == GCD_GEMM_PLAIN) {
    if (k.operand_bf16) {   // validated by gcd_gemm_f16: PLAIN mode, fp32 output
      if (use160 && ((tiles128 <= 320 && impl != 5) || impl == 6))
        return launch_gemm<64, 160, 32, 80, MODE, true>(k, s);
      if (use160) return launch_gemm<128, 160, 64, 80, MODE, true>(k, s);
      return launch_gemm<128, 128, 64, 64, MODE, true>(k, s);
    }
  }
  if (use160 && ((tiles128 <= 320 && impl != 5) || impl == 6)) return launch_gemm<64, 160, 32, 80, MODE>(k, s);
  if (use160) return launch_gemm<128, 160, 64, 80, MODE>(k, s);
  return launch_gemm<128, 128, 64, 64, MODE>(k, s);
}

// Conditions under which EVERY tile of the launch takes the row-major fp32 fast epilogue of the
// ping-pong kernel, the only one that produces column statistics: full 256 x 320 tiles, fp32 output,
// at most one residual, no fused LayerNorm, per-frame vectors / blend factors constant over a tile.
static bool colstats_shape_ok(const gcd_gemm_desc* d) {
  if (d->out_kind != GCD_OUT_F32 || d->R2 || d->ln_out16) return false;
  // the phase form of the x2 up-convolution: a wave's 64 low-res tokens must lie in one frame (gemm_p8.hip, P8_CONV_UP2)
  if (d->mode == GCD_GEMM_CONV3X3 && d->upsample == 2)
    return d->N % 320 == 0 && d->Hi > 0 && d->Wi > 0 && ((int64_t)d->Hi * d->Wi) % 64 == 0 && !d->R1 && !d->rowvec &&
           !d->frame_alpha;
  if (d->M % 256 != 0 || d->N % 320 != 0) return false;
  if (d->rowvec && d->rows_per_vec % 256 != 0) return false;
  if (d->frame_alpha && d->rows_per_alpha % 256 != 0) return false;
  return true;
}

// 256 x 320 tiles of a launch on the tile kernels.  The phase form of the x2 up-convolution (upsample == 2) runs four
// phase tiles per 256 LOW-RES tokens.
static int64_t pp_tiles(const gcd_gemm_desc* d) {
  const int64_t tn = (d->N + 319) / 320;
  if (d->mode == GCD_GEMM_CONV3X3 && d->upsample == 2) return 4 * (((int64_t)d->M / 4 + 255) / 256) * tn;
  return (int64_t)((d->M + 255) / 256) * tn;
}

// Implicit-GEMM geometry of a descriptor (conv3x3: pad 1 / stride 1-2 / fused x2 upsample /
// asymmetric pad; temporal3: clips of T frames x HW tokens).  0 = fine, else the error is set.
static int validate_geometry(const gcd_gemm_desc* d) {
  switch (d->mode) {
    case GCD_GEMM_PLAIN:
      return 0;
    case GCD_GEMM_CONV3X3:
      GCD_CHECK_ARG(d->zero_page, "gcd_gemm_f16: conv mode needs a zero page");
      if (d->upsample == 2) {   // four 2 x 2 phase convolutions: W [4][N][4 Cin] (packing.pack_conv3x3_up_phases)
        GCD_CHECK_ARG(d->Cin > 0 && d->Cin % 64 == 0 && d->K == 4 * d->Cin,
                      "gcd_gemm_f16: upsample=2 (phase form) needs Cin %% 64 == 0 and K == 4*Cin (Cin=%d K=%d)",
                      d->Cin, d->K);
        GCD_CHECK_ARG(d->stride == 1 && d->Hi > 0 && d->Wi > 0 && d->Ho == 2 * d->Hi && d->Wo == 2 * d->Wi &&
                          !d->asym_pad && d->M % (d->Ho * d->Wo) == 0,
                      "gcd_gemm_f16: upsample=2 needs Ho=2Hi, Wo=2Wi, stride 1 and M = frames*Ho*Wo");
        GCD_CHECK_ARG(d->Wi % 8 == 0, "gcd_gemm_f16: upsample=2 (phase form) needs Wi %% 8 == 0 (Wi=%d)", d->Wi);
        GCD_CHECK_ARG(d->out_kind == GCD_OUT_F32 && !d->R1 && !d->R2 && !d->rowvec && !d->frame_alpha &&
                          !d->operand_bf16,
                      "gcd_gemm_f16: upsample=2 (phase form) writes fp32 rows + bias only: no residual, per-frame "
                      "vector, blend, fp16 / GEGLU output or bf16 operands");
        return 0;
      }
      GCD_CHECK_ARG(d->Cin > 0 && d->Cin % 32 == 0 && d->K == 9 * d->Cin,
                    "gcd_gemm_f16: conv3x3 needs Cin %% 32 == 0 and K == 9*Cin (Cin=%d K=%d)",
                    d->Cin, d->K);
      GCD_CHECK_ARG(d->stride == 1 || d->stride == 2, "gcd_gemm_f16: stride %d", d->stride);
      GCD_CHECK_ARG(d->Ho > 0 && d->Wo > 0 && d->M % (d->Ho * d->Wo) == 0,
                    "gcd_gemm_f16: M=%d is not frames*Ho*Wo (%dx%d)", d->M, d->Ho, d->Wo);
      if (d->upsample)
        GCD_CHECK_ARG(d->stride == 1 && d->Ho == 2 * d->Hi && d->Wo == 2 * d->Wi,
                      "gcd_gemm_f16: fused upsample needs Ho=2Hi, Wo=2Wi, stride 1");
      else if (d->asym_pad)
        GCD_CHECK_ARG(d->stride == 2 && d->Ho == d->Hi / 2 && d->Wo == d->Wi / 2,
                      "gcd_gemm_f16: asym_pad needs stride 2 and Ho = Hi/2, Wo = Wi/2 (%dx%d -> %dx%d)",
                      d->Hi, d->Wi, d->Ho, d->Wo);
      else
        GCD_CHECK_ARG(d->Ho == (d->Hi - 1) / d->stride + 1 && d->Wo == (d->Wi - 1) / d->stride + 1,
                      "gcd_gemm_f16: conv3x3 pad-1 geometry mismatch (%dx%d -> %dx%d, stride %d)",
                      d->Hi, d->Wi, d->Ho, d->Wo, d->stride);
      return 0;
    case GCD_GEMM_TEMPORAL3:
      GCD_CHECK_ARG(d->zero_page, "gcd_gemm_f16: temporal mode needs a zero page");
      GCD_CHECK_ARG(d->Cin > 0 && d->Cin % 32 == 0 && d->K == 3 * d->Cin,
                    "gcd_gemm_f16: temporal3 needs Cin %% 32 == 0 and K == 3*Cin");
      GCD_CHECK_ARG(d->T > 0 && d->HW > 0 && d->M % (d->T * d->HW) == 0,
                    "gcd_gemm_f16: M=%d is not clips*T*HW (T=%d HW=%d)", d->M, d->T, d->HW);
      return 0;
    default:
      gcd_set_error("gcd_gemm_f16: unknown mode %d", d->mode);
      return 2;
  }
}

extern "C" int gcd_gemm_f16(const gcd_gemm_desc* d, void* stream) {
  GCD_CHECK_ARG(d != nullptr, "gcd_gemm_f16: null descriptor");
  GCD_CHECK_ARG(d->A && d->W && d->out, "gcd_gemm_f16: null operand");
  GCD_CHECK_ARG(d->M > 0 && d->N > 0 && d->K > 0, "gcd_gemm_f16: empty problem M=%d N=%d K=%d",
                d->M, d->N, d->K);
  GCD_CHECK_ARG(d->K % 32 == 0, "gcd_gemm_f16: K=%d must be a multiple of 32", d->K);
  GCD_CHECK_ARG(d->N % 16 == 0, "gcd_gemm_f16: N=%d must be a multiple of 16", d->N);
  GCD_CHECK_ARG(d->lda % 8 == 0, "gcd_gemm_f16: lda=%lld must be a multiple of 8 (16-B rows)",
                (long long)d->lda);
  GCD_CHECK_ARG(((uintptr_t)d->A & 15) == 0 && ((uintptr_t)d->W & 15) == 0 &&
                    ((uintptr_t)d->out & 15) == 0,
                "gcd_gemm_f16: operands must be 16-byte aligned");
  GCD_CHECK_ARG(d->out_kind >= GCD_OUT_F32 && d->out_kind <= GCD_OUT_GEGLU,
                "gcd_gemm_f16: bad out_kind %d", d->out_kind);
  if (d->out_kind == GCD_OUT_GEGLU) {
    GCD_CHECK_ARG(d->N % 32 == 0, "gcd_gemm_f16: GEGLU needs N %% 32 == 0 (N=%d)", d->N);
    GCD_CHECK_ARG(!d->R1 && !d->R2 && !d->rowvec, "gcd_gemm_f16: GEGLU takes bias only");
    GCD_CHECK_ARG(d->ldo % 4 == 0, "gcd_gemm_f16: ldo must be a multiple of 4");
  } else {
    GCD_CHECK_ARG(d->ldo % 4 == 0, "gcd_gemm_f16: ldo must be a multiple of 4");
  }
  if (d->rowvec)
    GCD_CHECK_ARG(d->rows_per_vec > 0 && d->ld_rowvec % 4 == 0, "gcd_gemm_f16: bad rowvec geometry");
  if (d->R1) GCD_CHECK_ARG(d->ldr1 % 4 == 0, "gcd_gemm_f16: ldr1 must be a multiple of 4");
  if (d->R2) GCD_CHECK_ARG(d->ldr2 % 4 == 0, "gcd_gemm_f16: ldr2 must be a multiple of 4");
  if (d->frame_alpha) GCD_CHECK_ARG(d->rows_per_alpha > 0, "gcd_gemm_f16: rows_per_alpha <= 0");

  GemmK k;
  k.A = (const f16*)d->A;
  k.W = (const f16*)d->W;
  k.out = d->out;
  k.lda = d->lda;
  k.ldo = d->ldo;
  k.M = d->M;
  k.N = d->N;
  k.K = d->K;
  k.Cin = d->Cin;
  k.Hi = d->Hi;
  k.Wi = d->Wi;
  k.Ho = d->Ho;
  k.Wo = d->Wo;
  k.stride = d->stride;
  k.up = d->upsample;
  k.asym = d->asym_pad ? 1 : 0;
  k.T = d->T;
  k.HW = d->HW;
  k.bias = d->bias;
  k.rowvec = d->rowvec;
  k.ld_rowvec = d->ld_rowvec;
  k.rows_per_vec = d->rows_per_vec;
  k.R1 = d->R1;
  k.ldr1 = d->ldr1;
  k.R2 = d->R2;
  k.ldr2 = d->ldr2;
  k.s_acc = d->s_acc;
  k.s_r1 = d->s_r1;
  k.s_r2 = d->s_r2;
  k.frame_alpha = d->frame_alpha;
  k.rows_per_alpha = d->rows_per_alpha;
  k.r1_blend = d->r1_blend;
  k.out_kind = d->out_kind;
  k.zero = (const f16*)d->zero_page;
  k.tiles_m = k.tiles_n = 0;
  k.ln_out = (f16*)d->ln_out16;
  k.ld_ln_out = d->ld_ln_out;
  k.ln_gamma = d->ln_gamma;
  k.ln_beta = d->ln_beta;
  k.ln_eps = d->ln_eps;
  k.ln_rows_per_vec = d->ln_rows_per_vec;
  k.ln_addvec = d->ln_addvec;
  k.ld_ln_addvec = d->ld_ln_addvec;
  k.ln_sum_out = d->ln_sum_out;
  k.ld_ln_sum = d->ld_ln_sum;
  k.splitk = 1;
  k.split_stride = 0;
  k.colstats = d->colstats;
  k.out_blocked = d->out_blocked ? 1 : 0;
  k.a_blocked = d->a_blocked ? 1 : 0;
  k.operand_bf16 = d->operand_bf16 ? 1 : 0;
  k.sched = d->sched & 1;
  hipStream_t s = (hipStream_t)stream;

  // kernel choice: the 256 x 320 ping-pong kernel whenever the grid fills most of the chip with
  // its (large) tiles, the general 128-row kernel otherwise.  GCD_TUNE_GEMM_IMPL overrides.
  const int impl = gcd_tune_get(GCD_TUNE_GEMM_IMPL);
  bool use_pp = false;
  if (impl != 1 && impl != 5 && impl != 6 && gcd_gemm_pp_supported(k, d->mode)) {
    const int64_t tiles = pp_tiles(d);
    int min_tiles = gcd_tune_get(GCD_TUNE_PP_MIN_TILES);
    if (min_tiles <= 0) min_tiles = (d->sched & 2) ? 128 : 192;   // sched bit 1: the caller's shapes pay from 128 tiles
    use_pp = (impl >= 2 && impl != 7) || ((impl == 0 || impl == 7) && tiles >= min_tiles && d->N >= 160);
    // K (or the channels per tap) a multiple of 32 but not of 64: only the ping-pong kernel's 32-deep
    // sub-tiles can walk it
    if (d->K % 64 != 0 || (d->mode != GCD_GEMM_PLAIN && d->Cin % 64 != 0)) use_pp = true;
  }
  if (d->operand_bf16) {
    GCD_CHECK_ARG(d->out_kind == GCD_OUT_F32 && !d->ln_out16 && !d->colstats && !d->out_blocked && !d->a_blocked,
                  "gcd_gemm_f16: bf16 operands are implemented for fp32 output, without fused LayerNorm / "
                  "colstats / blocked layouts");
    // every mode on the ping-pong kernel; the general 128-row kernel carries PLAIN-mode bf16 instantiations
    // only (small problems, K %% 64 == 0)
    if (!use_pp) {
      if (d->mode != GCD_GEMM_PLAIN || d->K % 64 != 0) {
        GCD_CHECK_ARG(gcd_gemm_pp_supported(k, d->mode) && impl != 1 && impl != 5 && impl != 6,
                      "gcd_gemm_f16: bf16 operands with mode %d / K=%d need the ping-pong kernel, which the "
                      "shape or GCD_TUNE_GEMM_IMPL=%d rules out", d->mode, d->K, impl);
        use_pp = true;
      }
    }
  }
#ifndef GCD_ABLATION_BUILD
  // Round 5: the fused LayerNorm in the producer's epilogue and the tile-blocked GEGLU hidden layout were built, are
  // bit-correct, and measured slower / neutral: they live in the ablation build
  // (python -m gcd_amd.csrc.build --ablation), not in the product library.
  GCD_CHECK_ARG(!d->ln_out16 && !d->out_blocked && !d->a_blocked,
                "gcd_gemm_f16: ln_out16 / out_blocked / a_blocked are compiled into the ablation build only");
#endif
  if (d->ln_out16) {
    GCD_CHECK_ARG(use_pp && d->N == 320 && d->out_kind == GCD_OUT_F32 && d->ln_gamma && d->ln_beta &&
                      d->ld_ln_out % 4 == 0 && ((uintptr_t)d->ln_out16 & 7) == 0,
                  "gcd_gemm_f16: fused LayerNorm needs N == 320, fp32 out, gamma / beta and a shape "
                  "the ping-pong kernel takes (M=%d N=%d; see gcd_gemm_ln_fusable)", d->M, d->N);
    if (d->ln_addvec)
      GCD_CHECK_ARG(d->ln_rows_per_vec > 0 && d->ld_ln_addvec % 4 == 0 &&
                        (!d->ln_sum_out || d->ld_ln_sum % 4 == 0),
                    "gcd_gemm_f16: bad fused-LayerNorm addvec geometry");
  }
  GCD_CHECK_ARG(use_pp || (d->K % 64 == 0 && (d->mode == GCD_GEMM_PLAIN || d->Cin % 64 == 0)),
                "gcd_gemm_f16: K=%d (Cin=%d) needs the ping-pong kernel, which the shape or "
                "GCD_TUNE_GEMM_IMPL=%d rules out", d->K, d->Cin, impl);

  if (d->colstats)
    GCD_CHECK_ARG(use_pp && colstats_shape_ok(d) && ((uintptr_t)d->colstats & 15) == 0,
                  "gcd_gemm_f16: colstats cannot be honoured for this descriptor (M=%d N=%d; see "
                  "gcd_gemm_colstats_supported)", d->M, d->N);

  if (d->out_blocked)
    GCD_CHECK_ARG(use_pp && d->out_kind == GCD_OUT_GEGLU && d->M % 256 == 0 && d->N % 320 == 0,
                  "gcd_gemm_f16: out_blocked needs a GEGLU output, M %% 256 == 0, N %% 320 == 0 and the "
                  "ping-pong kernel (M=%d N=%d)", d->M, d->N);
  if (d->a_blocked)
    GCD_CHECK_ARG(use_pp && d->mode == GCD_GEMM_PLAIN && d->M % 256 == 0 && d->K % 160 == 0 &&
                      !d->colstats && !d->ln_out16,
                  "gcd_gemm_f16: a_blocked needs PLAIN mode, M %% 256 == 0, K %% 160 == 0, no colstats / "
                  "fused LayerNorm and the ping-pong kernel (M=%d K=%d)", d->M, d->K);

  // mode-specific geometry, checked BEFORE any kernel choice (split-K included): a malformed conv /
  // temporal descriptor must come back as an argument error, never reach a gather
  if (const int rc = validate_geometry(d)) return rc;

  // The phase form of the x2 up-convolution exists on the 8-phase 256 x 320 tile kernel only: a shape or knob that
  // would send it elsewhere (the general kernel, the ring kernel, split-K over few tiles) is an argument error.
  if (d->mode == GCD_GEMM_CONV3X3 && d->upsample == 2) {
    GCD_CHECK_ARG(use_pp && impl != 3 && gcd_gemm_p8_supported(k, d->mode),
                  "gcd_gemm_f16: upsample=2 (phase form) needs the 8-phase 256x320 tile kernel, which the shape "
                  "(%lld tiles: the automatic choice takes the general kernel or split-K) or GCD_TUNE_GEMM_IMPL=%d "
                  "rules out", (long long)pp_tiles(d), impl);
    return gcd_gemm_pp_launch(k, d->mode, s);
  }

  // N == 16: the UNet's output head (320 -> 4, padded).  GCD_TUNE_GEMM_IMPL = 1 keeps it on the general kernel (tests).
  if (impl == 0 && gcd_conv3x3_narrow_supported(k, d->mode)) return gcd_conv3x3_narrow_launch(k, s);

  // split-K: few 256x320 tiles (<= 96 of 256 CUs) and a long K — the 3x3 convs of the 9x16 level
  if (d->workspace && !d->ln_out16 && !d->colstats && !d->a_blocked &&
      d->out_kind != GCD_OUT_GEGLU &&
      (impl == 0 || impl == 7) &&
      gcd_gemm_pp_supported(k, d->mode) && d->N >= 160 && d->N % 4 == 0) {
    const int64_t tiles = (int64_t)((d->M + 255) / 256) * ((d->N + 319) / 320);
    int splitk = (int)(256 / tiles);
    if (tiles <= 32 && d->K >= 4096 && (d->sched & 2)) {
      // a handful of tiles and a very long K: the weight gradients of the fine-tune step (dW = dY^T X, the
      // contraction runs over the tokens: K >= 43 008).  Up to 32 K slices of at least 640, as many as the scratch
      // holds.  Only for callers that ask for it (gcd_gemm_desc.sched bit 1, set by the fine-tune step's GEMMs): the
      // sampler's few-tile launches keep the 2-4-way split they were measured with.
      if (splitk > 32) splitk = 32;
      while (splitk > 1 && (d->K / splitk < 640 || d->workspace_bytes < (int64_t)splitk * d->M * d->N * 4)) --splitk;
      if (splitk >= 2 && ((uintptr_t)d->workspace & 15) == 0)
        return gcd_gemm_pp_launch_splitk(k, d->mode, splitk, (float*)d->workspace, s);
    } else {
      if (splitk > 4) splitk = 4;
      if (tiles <= 96 && splitk >= 2 && d->K / splitk >= 1920 &&
          d->workspace_bytes >= (int64_t)splitk * d->M * d->N * 4 && ((uintptr_t)d->workspace & 15) == 0) {
        return gcd_gemm_pp_launch_splitk(k, d->mode, splitk, (float*)d->workspace, s);
      }
    }
  }

  switch (d->mode) {
    case GCD_GEMM_PLAIN:
      if (use_pp) return gcd_gemm_pp_launch(k, d->mode, s);
      return dispatch_tile<GCD_GEMM_PLAIN>(k, s);
    case GCD_GEMM_CONV3X3:
      if (use_pp) return gcd_gemm_pp_launch(k, d->mode, s);
      return dispatch_tile<GCD_GEMM_CONV3X3>(k, s);
    default:   // GCD_GEMM_TEMPORAL3 (validate_geometry rejected anything else)
      if (use_pp) return gcd_gemm_pp_launch(k, d->mode, s);
      return dispatch_tile<GCD_GEMM_TEMPORAL3>(k, s);
  }
}

extern "C" int gcd_gemm_colstats_supported(const gcd_gemm_desc* d) {
  if (!d || d->M <= 0 || d->N <= 0 || d->K <= 0 || d->K % 32 != 0 || !colstats_shape_ok(d)) return 0;
  if (d->mode != GCD_GEMM_PLAIN && (d->Cin <= 0 || d->Cin % 32 != 0)) return 0;
  const int impl = gcd_tune_get(GCD_TUNE_GEMM_IMPL);
  if (impl == 1 || impl == 5 || impl == 6) return 0;          // general kernel forced
  const bool up2 = d->mode == GCD_GEMM_CONV3X3 && d->upsample == 2;
  if (up2 && (d->Cin % 64 != 0 || d->K != 4 * d->Cin || d->Wi % 8 != 0 || impl == 3)) return 0;
  const int64_t tiles = up2 ? pp_tiles(d) : (int64_t)(d->M / 256) * (d->N / 320);
  int min_tiles = gcd_tune_get(GCD_TUNE_PP_MIN_TILES);
  if (min_tiles <= 0) min_tiles = (d->sched & 2) ? 128 : 192;
  if ((impl == 0 || impl == 7) && tiles < min_tiles) return 0;      // automatic choice: general kernel / split-K
  return 1;
}

extern "C" int gcd_gemm_hidden_blocked_supported(int M, int N_geglu, int N_out) {
#ifndef GCD_ABLATION_BUILD
  (void)M, (void)N_geglu, (void)N_out;
  return 0;      // ablation build only (see gcd_gemm_f16)
#endif
  if (M <= 0 || M % 256 != 0 || N_geglu <= 0 || N_geglu % 320 != 0 || N_out < 160 || N_out % 16 != 0) return 0;
  const int impl = gcd_tune_get(GCD_TUNE_GEMM_IMPL);
  if (impl == 1 || impl == 5 || impl == 6) return 0;          // general kernel forced
  if (impl == 0 || impl == 7) {                                // automatic choice: both grids must be large
    const int64_t t1 = (int64_t)(M / 256) * (N_geglu / 320), t2 = (int64_t)(M / 256) * ((N_out + 319) / 320);
    if (t1 < 192 || t2 < 192) return 0;
  }
  return 1;
}

extern "C" int gcd_gemm_ln_fusable(int M, int N, int K, int mode) {
#ifndef GCD_ABLATION_BUILD
  (void)M, (void)N, (void)K, (void)mode;
  return 0;      // ablation build only (see gcd_gemm_f16)
#endif
  if (N != 320 || K <= 0 || K % 32 != 0 || M <= 0) return 0;
  const int impl = gcd_tune_get(GCD_TUNE_GEMM_IMPL);
  if (impl == 1 || impl == 5 || impl == 6) return 0;
  const int64_t tiles = (int64_t)((M + 255) / 256);
  (void)mode;
  return (impl >= 2 || tiles >= 192) ? 1 : 0;
}
