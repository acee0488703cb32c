/* gcd_amd_loss.h — gcd_amd/libgcd_amd_loss.so (gcd_amd/csrc/loss.hip): the fine-tune loss on the device
 * (gcd_amd/loss_device.py; the `hip` loss engine of gcd_amd/training.py): the ParallelDomain class weight map, the
 * annealed top-fraction focal loss with the EDM weighting, and its gradient with respect to the model output.
 *
 * A library of its own (gcd_amd/csrc/build.py LIBRARIES, gcd_amd/_lib_loss.py): include/gcd_amd.h and its ABI version do not
 * change.  Same rules as gcd_amd.h: raw device pointers, the caller's hipStream_t, no allocation, no synchronisation;
 * every argument is checked before anything is launched, and a non-zero status comes with a message in
 * gcd_loss_last_error().  Every payload element of every output is stored by every call.  There is no floating-point
 * atomic and no workgroup reads what another one wrote: a frame is one workgroup, its sums are fp64 in a fixed order, so
 * a result is bit-identical from call to call and a frame's values cannot reach another frame's. */
#ifndef GCD_AMD_LOSS_H
#define GCD_AMD_LOSS_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCD_AMD_LOSS_ABI_VERSION 1
/* most rows of a class table (the kernel argument holds the table) */
#define GCD_LOSS_MAX_CLASSES 16
/* most frames per call (BT) */
#define GCD_LOSS_MAX_BT 65535
/* most elements per frame (C * H * W) of the focal loss: counts stay exact in int32 and in fp32 */
#define GCD_LOSS_MAX_N 16777216
/* widest weight map (Wl): one workgroup holds a latent row's per-class counts, Wl x GCD_LOSS_MAX_CLASSES int32, in LDS */
#define GCD_LOSS_MAX_MAP_W 512
/* loss_type */
#define GCD_LOSS_L2 0
#define GCD_LOSS_L1 1

int gcd_loss_abi_version(void);
const char* gcd_loss_last_error(void);

/* gt_rgb: fp32 [BT, 3, Hp, Wp], contiguous (semantic-map frames in [-1, 1]).  classes: fp32 [ncls, 4] in HOST memory, read
 * during the call: (r, g, b, weight - 1) per class, colours on the [-1, 1] range; 1 <= ncls <= GCD_LOSS_MAX_CLASSES.
 * wmap: fp32 [BT, 1, Hl, Wl], 1 <= Hl <= Hp, 1 <= Wl <= Wp, Wl <= GCD_LOSS_MAX_MAP_W.
 *   match_c(y, x) = ((|gt[0] - r_c| + |gt[1] - g_c|) + |gt[2] - b_c|) / 3 < 0.02        (fp32, each operation rounded)
 *   wmap[i, j]    = sum_c fp32(count of match_c over the bin / pixels of the bin) * (weight_c - 1)
 * summed in class order, every product and sum rounded to fp32 on its own.  The bin of (i, j) is torch's
 * F.interpolate(mode="area"): rows floor(i Hp / Hl) .. ceil((i + 1) Hp / Hl) - 1, columns by the same rule (the 8 x 8
 * square when Hp = 8 Hl; neighbouring bins share a row / column otherwise).  The counts are integers: no rounding
 * depends on the order in which the pixels are visited.  One workgroup per (frame, latent row). */
int gcd_loss_class_map(const float* gt_rgb, int BT, int Hp, int Wp, const float* classes, int ncls, float* wmap, int Hl,
                       int Wl, void* stream);

/* out, tgt: fp32 [BT, C, H, W] contiguous, n = C * H * W <= GCD_LOSS_MAX_N, HW = H * W divides n; w: fp32 [BT];
 * wmap: fp32 [BT, 1, H, W] (values >= 0) or null; loss_type GCD_LOSS_L2 / GCD_LOSS_L1; 0 <= keep <= n.
 * Per frame f and element e (wmap read at e mod HW), in fp32 as torch forms them:
 *   diff = out - tgt;  raw = diff^2 | |diff|;  rb = raw * wmap;  all = raw + 0.5 * rb            (rb = 0 without wmap)
 * and then in fp64, each sum in a fixed order:
 *   mean_all = sum(all) / n;  bias_mean = sum(rb) / n
 *   keep == 0:  loss[f] = (mean_all + 0.5 bias_mean) * w[f]
 *   keep >= 1:  tau = the keep-th largest value of all (exact: a three-pass radix select over the fp32 bit patterns,
 *               11 + 11 + 9 bits, integer LDS histograms; nothing is sorted);  quota = keep - #{all > tau} >= 1
 *               top_mean = (sum_{all > tau} all + quota * tau) / keep
 *               loss[f] = (0.9 top_mean + 0.1 mean_all + 0.5 bias_mean) * w[f]
 * loss: fp32 [BT].  state: int32 [BT, 2] = (bit pattern of tau, quota) per frame, (0, 0) when keep == 0: what
 * gcd_loss_focal_bwd needs.  A non-finite value makes its own frame's loss non-finite and touches no other frame. */
int gcd_loss_focal_fwd(const float* out, const float* tgt, const float* w, const float* wmap, int BT, int n, int HW,
                       int loss_type, int keep, float* loss, int32_t* state, void* stream);

/* The gradient of sum_f g[f] * loss[f] with respect to `out`.  g: fp32 [BT]; state: what gcd_loss_focal_fwd wrote for the
 * same operands and the same keep; dout: fp32 [BT, C, H, W], every element stored.  In fp64, rounded once:
 *   dout[e] = g[f] w[f] ((0.9 / keep * sel(e) + 0.1 / n) (1 + 0.5 wmap) + 0.5 wmap / n) draw
 *   draw    = 2 diff | sign(diff) (0 at 0);   keep == 0: 1 / n in place of (0.9 / keep * sel + 0.1 / n)
 *   sel(e)  = 1 for all > tau; among all == tau, 1 for the `quota` lowest flat indices e of the frame; else 0
 * so exactly `keep` elements of a frame are selected.  tgt, w and wmap get no gradient. */
int gcd_loss_focal_bwd(const float* out, const float* tgt, const float* w, const float* wmap, const float* g,
                       const int32_t* state, int BT, int n, int HW, int loss_type, int keep, float* dout, void* stream);

#ifdef __cplusplus
}
#endif
#endif
