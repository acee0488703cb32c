// train_optim.hip — the device-resident optimizer step of libgcd_amd_train.so.  C ABI: include/gcd_amd_train_optim.h.
//
// Two passes over one device table of (p, g, m, v, ema, n, chunk0) and a 64-byte state block between them:
//   pass 1  gradstat: workgroup b owns chunk b (16 K elements of one tensor, the granule of adam_multi_kernel), sums the
//           squares of g * grad_scale and WRITES the sum to slot b of the caller's scratch — a plain vector store, nothing to
//           zero first.  Then the ordered fold, one workgroup: thread t adds slots t, t + 1024, ... in index order in fp64,
//           the 1024 sums go through a fixed binary tree in fp64.  One thread then decides everything a step depends on
//           (found_inf, grad_norm, clip_coef, the gradient factor, the loss scale of the next step, the step count, the
//           bias corrections, the EMA decay) and stores it in the state block.
//   pass 2  apply: one streaming pass, 28 B per parameter (36 B with an EMA shadow); reads the state block; on found_inf
//           p, m and v are not even loaded.
// The grids are functions of the element counts alone, so the order of every sum is fixed and the result is a function
// of (inputs, shapes).  No read-modify-write reduction anywhere in this file.  All HBM-bound: 16-byte accesses where every
// base of a tensor allows, two vectors per operand in flight per thread, a scalar loop for the tail and for views whose
// base is not 16-byte aligned.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gcd_amd_train_optim.h"
#include "train_common.h"

typedef __attribute__((ext_vector_type(4))) float f32x4;

namespace {

constexpr int CHUNK = GCD_OPTIM_CHUNK;
constexpr int FOLD_THREADS = 1024;

struct ApplyArgs {
  float b1, omb1, b2, omb2, eps, wd;
  int decoupled, use_ema;
};

// the tensor that owns chunk `c`: the last entry whose chunk0 <= c (uniform over the workgroup: scalar loads)
__device__ __forceinline__ int find_tensor(const gcd_optim_tensor* __restrict__ tab, int n, int c) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].chunk0 <= c) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ---------------------------------------------------------------------------------------------------------------------
// pass 1a: one slot per chunk
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gradstat_partial_kernel(const gcd_optim_tensor* __restrict__ tab, int n_tensors,
                                                               float gscale, float* __restrict__ slots) {
  __shared__ float red[4];
  const int t = find_tensor(tab, n_tensors, (int)blockIdx.x);
  const float* __restrict__ g = tab[t].g;
  const int64_t n = tab[t].n;
  const int64_t i0 = (int64_t)((int)blockIdx.x - tab[t].chunk0) * CHUNK;
  const int64_t i1 = i0 + CHUNK < n ? i0 + CHUNK : n;
  float s = 0.f;
  if (g != nullptr && i0 < i1) {
    int64_t i = i0;
    if (((uintptr_t)g & 15) == 0) {
      const int nv = (int)((i1 - i0) >> 2);
      int k = threadIdx.x;
      for (; k + 768 < nv; k += 1024) {
        f32x4 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = *(const f32x4*)(g + i0 + 4 * (int64_t)(k + 256 * u));
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float y = x[u][e] * gscale;
            s = fmaf(y, y, s);
          }
      }
      for (; k < nv; k += 256) {
        const f32x4 x = *(const f32x4*)(g + i0 + 4 * (int64_t)k);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float y = x[e] * gscale;
          s = fmaf(y, y, s);
        }
      }
      i = i0 + 4 * (int64_t)nv;
    }
    for (i += threadIdx.x; i < i1; i += 256) {
      const float y = g[i] * gscale;
      s = fmaf(y, y, s);
    }
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) slots[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// what one thread decides after the sum (or without one): everything pass 2 reads
__device__ void advance_state(gcd_optim_state* __restrict__ st, const gcd_optim_config c, bool have_total, double total) {
  const float ls = st->loss_scale;
  int step = st->step;
  bool found = false;
  float gnorm = -1.f, clip = 1.f;
  if (have_total) {
    found = !isfinite(total);
    gnorm = (float)(sqrt(total) / (double)ls);
    if (c.max_norm > 0.f) clip = fminf(1.0f, c.max_norm / (gnorm + 1e-6f));
    if (found) clip = 0.f;
  }
  if (found) {
    st->skipped_total += 1;
    if (c.dynamic_scale) {
      st->loss_scale = ls * c.backoff_factor;
      st->growth_tracker = 0;
    }
  } else {
    step += 1;
    st->step = step;
    if (c.dynamic_scale) {
      const int tr = st->growth_tracker + 1;
      if (tr >= c.growth_interval) {
        st->loss_scale = ls * c.growth_factor;
        st->growth_tracker = 0;
      } else {
        st->growth_tracker = tr;
      }
    }
  }
  st->found_inf = found ? 1 : 0;
  st->grad_norm = gnorm;
  st->clip_coef = clip;
  st->gfactor = c.grad_scale / ls * clip;
  const double s = (double)(step > 0 ? step : 1);
  st->bc1 = (float)(1.0 - pow(c.beta1, s));
  st->bc2_sqrt = (float)sqrt(1.0 - pow(c.beta2, s));
}

// LitEma.forward's decay: the count's home is c.ema_count when given
__device__ void advance_ema(gcd_optim_state* __restrict__ st, const gcd_optim_config c) {
  int n = c.ema_count != nullptr ? *c.ema_count : st->ema_num_updates;
  float decay = c.ema_decay;
  if (n >= 0) {
    n += 1;
    decay = fminf(decay, (float)(1 + n) / (float)(10 + n));
  }
  st->ema_num_updates = n;
  if (c.ema_count != nullptr) *c.ema_count = n;
  st->ema_omd = 1.0f - decay;
}

// ---------------------------------------------------------------------------------------------------------------------
// pass 1b: the ordered fold, one workgroup
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FOLD_THREADS) void gradstat_fold_kernel(const float* __restrict__ slots, int64_t nslots,
                                                                     gcd_optim_state* __restrict__ st,
                                                                     const gcd_optim_config c) {
  __shared__ double red[FOLD_THREADS];
  double s = 0.0;
  int64_t k = threadIdx.x;
  for (; k + 7 * FOLD_THREADS < nslots; k += 8 * FOLD_THREADS) {
    float x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = slots[k + (int64_t)u * FOLD_THREADS];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += (double)x[u];
  }
  for (; k < nslots; k += FOLD_THREADS) s += (double)slots[k];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = FOLD_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    advance_state(st, c, true, red[0]);
    if (c.use_ema) advance_ema(st, c);
  }
}

__global__ void advance_kernel(gcd_optim_state* __restrict__ st, const gcd_optim_config c, int optimizer, int ema) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    if (optimizer) advance_state(st, c, false, 0.0);
    if (ema) advance_ema(st, c);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// pass 2
// ---------------------------------------------------------------------------------------------------------------------
template <bool ADAM, bool EMA>
__device__ __forceinline__ void apply_chunk(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                            float* __restrict__ v, float* __restrict__ ema, int64_t i0, int64_t i1,
                                            const ApplyArgs a, float gf, float stepsz, float bc2s, float keep, float omd) {
  auto upd = [&](float& pi, float gi, float& mi, float& vi, float& ei) {
    if (ADAM) {
      gi *= gf;
      if (a.decoupled) pi *= keep;                      // torch.optim.AdamW: p.mul_(1 - lr * weight_decay)
      else if (a.wd != 0.f) gi = fmaf(a.wd, pi, gi);    // torch.optim.Adam: grad.add(p, alpha=weight_decay)
      mi = fmaf(a.b1, mi, a.omb1 * gi);
      vi = fmaf(a.b2, vi, a.omb2 * gi * gi);
      pi -= stepsz * (mi / (sqrtf(vi) / bc2s + a.eps));
    }
    if (EMA) ei = __fsub_rn(ei, __fmul_rn(omd, __fsub_rn(ei, pi)));      // LitEma: shadow.sub_(omd * (shadow - p))
  };
  uintptr_t bases = (uintptr_t)p;
  if (ADAM) bases |= (uintptr_t)g | (uintptr_t)m | (uintptr_t)v;
  if (EMA) bases |= (uintptr_t)ema;
  int64_t i = i0;
  if ((bases & 15) == 0) {
    const int nv = (int)((i1 - i0) >> 2);
#pragma unroll 2
    for (int k = threadIdx.x; k < nv; k += 256) {
      const int64_t j = i0 + 4 * (int64_t)k;
      f32x4 pv = *(const f32x4*)(p + j), gv, mv, vv, ev;
      if (ADAM) {
        gv = *(const f32x4*)(g + j);
        mv = *(const f32x4*)(m + j);
        vv = *(const f32x4*)(v + j);
      }
      if (EMA) ev = *(const f32x4*)(ema + j);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = pv[e], ge = ADAM ? gv[e] : 0.f, me = ADAM ? mv[e] : 0.f, ve = ADAM ? vv[e] : 0.f, ee = EMA ? ev[e] : 0.f;
        upd(pe, ge, me, ve, ee);
        pv[e] = pe;
        if (ADAM) {
          mv[e] = me;
          vv[e] = ve;
        }
        if (EMA) ev[e] = ee;
      }
      if (ADAM) {
        *(f32x4*)(p + j) = pv;
        *(f32x4*)(m + j) = mv;
        *(f32x4*)(v + j) = vv;
      }
      if (EMA) *(f32x4*)(ema + j) = ev;
    }
    i = i0 + 4 * (int64_t)nv;
  }
  for (i += threadIdx.x; i < i1; i += 256) {
    float pe = p[i], ge = 0.f, me = 0.f, ve = 0.f, ee = 0.f;
    if (ADAM) {
      ge = g[i];
      me = m[i];
      ve = v[i];
    }
    if (EMA) ee = ema[i];
    upd(pe, ge, me, ve, ee);
    if (ADAM) {
      p[i] = pe;
      m[i] = me;
      v[i] = ve;
    }
    if (EMA) ema[i] = ee;
  }
}

__global__ __launch_bounds__(256) void apply_kernel(const gcd_optim_tensor* __restrict__ tab, int n_tensors,
                                                    const gcd_optim_state* __restrict__ st, const ApplyArgs a,
                                                    int optimizer) {
  const int t = find_tensor(tab, n_tensors, (int)blockIdx.x);
  const gcd_optim_tensor e = tab[t];
  const int64_t i0 = (int64_t)((int)blockIdx.x - e.chunk0) * CHUNK;
  const int64_t i1 = i0 + CHUNK < e.n ? i0 + CHUNK : e.n;
  if (i0 >= i1) return;
  const bool adam = optimizer && e.g != nullptr && st->found_inf == 0;
  const bool ema = a.use_ema && e.ema != nullptr;
  const float lr = st->lr, gf = st->gfactor, bc2s = st->bc2_sqrt, omd = st->ema_omd;
  const float stepsz = lr / st->bc1;
  const float keep = 1.0f - lr * a.wd;
  if (adam && ema) apply_chunk<true, true>(e.p, e.g, e.m, e.v, e.ema, i0, i1, a, gf, stepsz, bc2s, keep, omd);
  else if (adam) apply_chunk<true, false>(e.p, e.g, e.m, e.v, nullptr, i0, i1, a, gf, stepsz, bc2s, keep, omd);
  else if (ema) apply_chunk<false, true>(e.p, nullptr, nullptr, nullptr, e.ema, i0, i1, a, gf, stepsz, bc2s, keep, omd);
}

int check_common(const char* what, const void* table, int n_tensors, int64_t total_chunks, const gcd_optim_config* cfg,
                 const void* state) {
  CHECK_ARG(table && cfg && state, "%s: null table, config or state", what);
  CHECK_ARG(((uintptr_t)table & 7) == 0 && ((uintptr_t)state & 15) == 0,
            "%s: the table must be 8-byte and the state block 16-byte aligned", what);
  CHECK_ARG(n_tensors >= 1, "%s: empty table (n_tensors %d)", what, n_tensors);
  CHECK_ARG(total_chunks >= n_tensors && total_chunks < (1ll << 30),
            "%s: total_chunks %lld for %d tensors (every tensor has at least one chunk; at most 2^30)", what,
            (long long)total_chunks, n_tensors);
  return 0;
}

int check_config(const char* what, const gcd_optim_config* c) {
  CHECK_ARG(c->beta1 >= 0.0 && c->beta1 < 1.0 && c->beta2 >= 0.0 && c->beta2 < 1.0,
            "%s: betas (%g, %g) must lie in [0, 1)", what, c->beta1, c->beta2);
  CHECK_ARG(c->eps >= 0.0 && c->weight_decay >= 0.0, "%s: eps %g and weight_decay %g must not be negative", what, c->eps,
            c->weight_decay);
  CHECK_ARG(isfinite(c->grad_scale) && c->grad_scale != 0.f, "%s: grad_scale must be finite and non-zero", what);
  CHECK_ARG(!c->dynamic_scale || (c->growth_factor > 1.f && c->backoff_factor > 0.f && c->backoff_factor < 1.f &&
                                  c->growth_interval >= 1),
            "%s: dynamic scaling needs growth_factor > 1, 0 < backoff_factor < 1, growth_interval >= 1", what);
  CHECK_ARG(!c->use_ema || (c->ema_decay >= 0.f && c->ema_decay <= 1.f), "%s: ema_decay %g must lie in [0, 1]", what,
            c->ema_decay);
  return 0;
}

}  // namespace

extern "C" int64_t gcd_optim_gradstat_scratch_floats(int64_t total_chunks) {
  return total_chunks >= 1 && total_chunks < (1ll << 30) ? total_chunks : 0;
}

extern "C" int gcd_optim_gradstat(const gcd_optim_tensor* table_dev, int n_tensors, int64_t total_chunks,
                                  const gcd_optim_config* cfg, gcd_optim_state* state_dev, float* scratch,
                                  int64_t scratch_floats, void* stream) {
  if (int rc = check_common("gcd_optim_gradstat", table_dev, n_tensors, total_chunks, cfg, state_dev)) return rc;
  if (int rc = check_config("gcd_optim_gradstat", cfg)) return rc;
  CHECK_ARG(scratch && scratch_floats >= total_chunks && ((uintptr_t)scratch & 15) == 0,
            "gcd_optim_gradstat: scratch of %lld floats, need %lld (gcd_optim_gradstat_scratch_floats), 16-byte aligned",
            (long long)scratch_floats, (long long)total_chunks);
  hipLaunchKernelGGL(gradstat_partial_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, table_dev,
                     n_tensors, cfg->grad_scale, scratch);
  CHECK_LAUNCH("gcd_optim_gradstat");
  hipLaunchKernelGGL(gradstat_fold_kernel, dim3(1), dim3(FOLD_THREADS), 0, (hipStream_t)stream, (const float*)scratch,
                     total_chunks, state_dev, *cfg);
  CHECK_LAUNCH("gcd_optim_gradstat (fold)");
  return 0;
}

extern "C" int gcd_optim_advance(const gcd_optim_config* cfg, gcd_optim_state* state_dev, void* stream) {
  CHECK_ARG(cfg && state_dev && ((uintptr_t)state_dev & 15) == 0,
            "gcd_optim_advance: null config or state, or a state block that is not 16-byte aligned");
  if (int rc = check_config("gcd_optim_advance", cfg)) return rc;
  hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state_dev, *cfg, 1, cfg->use_ema);
  CHECK_LAUNCH("gcd_optim_advance");
  return 0;
}

static ApplyArgs apply_args(const gcd_optim_config* c) {
  ApplyArgs a;
  a.b1 = (float)c->beta1;
  a.omb1 = (float)(1.0 - c->beta1);
  a.b2 = (float)c->beta2;
  a.omb2 = (float)(1.0 - c->beta2);
  a.eps = (float)c->eps;
  a.wd = (float)c->weight_decay;
  a.decoupled = c->decoupled && c->weight_decay != 0.0;
  a.use_ema = c->use_ema;
  return a;
}

extern "C" int gcd_optim_apply(const gcd_optim_tensor* table_dev, int n_tensors, int64_t total_chunks,
                               const gcd_optim_config* cfg, gcd_optim_state* state_dev, void* stream) {
  if (int rc = check_common("gcd_optim_apply", table_dev, n_tensors, total_chunks, cfg, state_dev)) return rc;
  if (int rc = check_config("gcd_optim_apply", cfg)) return rc;
  hipLaunchKernelGGL(apply_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, table_dev, n_tensors,
                     (const gcd_optim_state*)state_dev, apply_args(cfg), 1);
  CHECK_LAUNCH("gcd_optim_apply");
  return 0;
}

extern "C" int gcd_ema_update(const gcd_optim_tensor* table_dev, int n_tensors, int64_t total_chunks,
                              const gcd_optim_config* cfg, gcd_optim_state* state_dev, void* stream) {
  if (int rc = check_common("gcd_ema_update", table_dev, n_tensors, total_chunks, cfg, state_dev)) return rc;
  CHECK_ARG(cfg->use_ema && cfg->ema_decay >= 0.f && cfg->ema_decay <= 1.f,
            "gcd_ema_update: use_ema must be set and ema_decay %g must lie in [0, 1]", cfg->ema_decay);
  hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state_dev, *cfg, 0, 1);
  CHECK_LAUNCH("gcd_ema_update (advance)");
  hipLaunchKernelGGL(apply_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, table_dev, n_tensors,
                     (const gcd_optim_state*)state_dev, apply_args(cfg), 0);
  CHECK_LAUNCH("gcd_ema_update");
  return 0;
}
