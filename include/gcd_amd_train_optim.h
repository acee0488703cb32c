/* gcd_amd_train_optim.h — the device-resident optimizer step of gcd_amd/libgcd_amd_train.so (gcd_amd/csrc/train_optim.hip).
 *
 * One reduction pass over the gradients, one fused update pass over the parameters, and a small state block in device
 * memory between them, so that nothing about a step is decided on the host: the step count, the learning rate, the loss
 * scale, "was a gradient non-finite", the clip coefficient and the EMA update count all live in `gcd_optim_state`.
 *   gcd_optim_gradstat   pass 1: per 16 K-element chunk the sum of squares of g * grad_scale, written to the chunk's own slot
 *                        of `scratch`; then a fold launch of one workgroup: found_inf, grad_norm, clip_coef, the factor
 *                        pass 2 multiplies the gradients by, torch.amp.GradScaler's update rule, the step count and the
 *                        bias corrections;
 *   gcd_optim_advance    what takes the fold's place when neither clipping nor dynamic loss scaling is on;
 *   gcd_optim_apply      pass 2: Adam / AdamW on the unscaled, clipped gradient and, from the freshly updated p, the EMA;
 *   gcd_ema_update       the EMA part alone (LitEma.forward outside the optimizer).
 * Every sum has a fixed order (derived from the element counts alone) and no entry uses a read-modify-write reduction:
 * results are bit-reproducible.  Same rules as gcd_amd_train.h: raw device pointers, the caller's hipStream_t, no
 * allocation, no synchronisation; status 0 / non-zero and a message in gcd_train_last_error. */
#ifndef GCD_AMD_TRAIN_OPTIM_H
#define GCD_AMD_TRAIN_OPTIM_H
#include <stdint.h>

#include "gcd_amd_train.h"
#ifdef __cplusplus
extern "C" {
#endif

#define GCD_OPTIM_CHUNK 16384 /* elements per workgroup: the granule of gcd_adam_step_multi */

/* The state block: 64 bytes of DEVICE memory, fp32 / int32 only, 16-byte aligned.  The caller initialises step (0), lr,
 * loss_scale (1 when unused), growth_tracker (0), skipped_total (0) and ema_num_updates (0, or -1 for a fixed decay);
 * the kernels own the rest. */
typedef struct gcd_optim_state {
  int32_t step;            /* optimizer steps taken (torch's state['step']); not advanced by a skipped step */
  float lr;                /* read by pass 2 */
  float loss_scale;        /* the scale the NEXT loss is multiplied by */
  int32_t growth_tracker;  /* consecutive finite steps since the last change of loss_scale */
  int32_t found_inf;       /* last step: 1 = the sum of squares was not finite, the step was skipped */
  float grad_norm;         /* last step: l2 norm of the unscaled gradients before clipping; -1 when pass 1 did not run */
  float clip_coef;         /* last step: min(1, max_norm / (grad_norm + 1e-6)); 1 when clipping is off */
  int32_t skipped_total;   /* skipped steps so far */
  int32_t ema_num_updates; /* LitEma.num_updates; -1 = use the fixed decay */
  float gfactor;           /* for pass 2: grad_scale / loss_scale * clip_coef */
  float bc1;               /* for pass 2: 1 - beta1^step */
  float bc2_sqrt;          /* for pass 2: sqrt(1 - beta2^step) */
  float ema_omd;           /* for pass 2: 1 - decay of this update */
  int32_t reserved[3];
} gcd_optim_state;

/* One tensor of the device table.  g == NULL: a parameter the graph never reached (EMA part only); ema == NULL: no shadow.
 * chunk0 = sum of ceil(n / GCD_OPTIM_CHUNK) over the tensors before it; n >= 1. */
typedef struct gcd_optim_tensor {
  float* p;
  const float* g;
  float* m;
  float* v;
  float* ema;
  int64_t n;
  int32_t chunk0;
  int32_t reserved;
} gcd_optim_tensor;

/* Hyper-parameters: HOST memory, read during the call. */
typedef struct gcd_optim_config {
  double beta1, beta2, eps, weight_decay;
  float grad_scale;        /* multiplies every gradient (undoes a static scale, 1 / world size) */
  float max_norm;          /* > 0: clip the global l2 norm (torch.nn.utils.clip_grad_norm_); <= 0: off */
  float growth_factor, backoff_factor; /* torch.amp.GradScaler */
  float ema_decay;
  int32_t growth_interval;
  int32_t dynamic_scale;   /* 1: update loss_scale by GradScaler's rule */
  int32_t decoupled;       /* 1: AdamW (p *= 1 - lr wd); 0: Adam (g += wd p) */
  int32_t use_ema;         /* 1: tensors with an ema pointer get the EMA update, ema_num_updates advances */
  int32_t reserved;
  int32_t* ema_count;      /* optional DEVICE int32 that holds the EMA update count (LitEma's num_updates buffer): when
                              given it is the count's home — read, advanced, written back — and the state block's field
                              is a copy of it */
} gcd_optim_config;

/* Pass 1.  scratch: >= gcd_optim_gradstat_scratch_floats(total_chunks) floats (= total_chunks), 16-byte aligned; written
 * before it is read.  total_chunks = the table's chunk count (the grid), n_tensors >= 1.  Two launches. */
int64_t gcd_optim_gradstat_scratch_floats(int64_t total_chunks);
int gcd_optim_gradstat(const gcd_optim_tensor* table_dev, int n_tensors, int64_t total_chunks, const gcd_optim_config* cfg,
                       gcd_optim_state* state_dev, float* scratch, int64_t scratch_floats, void* stream);

/* The state advance without a reduction: found_inf = 0, grad_norm = -1, clip_coef = 1, step + 1.  One launch. */
int gcd_optim_advance(const gcd_optim_config* cfg, gcd_optim_state* state_dev, void* stream);

/* Pass 2, after gcd_optim_gradstat or gcd_optim_advance on the same stream.  One launch.  On found_inf p, m and v keep
 * their bits; the EMA moves all the same. */
int gcd_optim_apply(const gcd_optim_tensor* table_dev, int n_tensors, int64_t total_chunks, const gcd_optim_config* cfg,
                    gcd_optim_state* state_dev, void* stream);

/* ema -= (1 - d) (ema - p) over the table's tensors that have an ema pointer; advances the update count first
 * (d = min(decay, (1 + n) / (10 + n)) unless the count is -1).  Two launches. */
int gcd_ema_update(const gcd_optim_tensor* table_dev, int n_tensors, int64_t total_chunks, const gcd_optim_config* cfg,
                   gcd_optim_state* state_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
