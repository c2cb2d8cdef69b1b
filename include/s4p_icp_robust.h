/* s4p_icp_robust.h -- robust ICP in libsuper4pcs_icp.so: trimmed ICP and the Huber and Tukey M-estimators, for both metrics,
 * next to the entry points of s4p_icp.h and s4p_icp_plane.h (same context, target grid, normals and correspondences).
 * DESIGN.md section "Robust ICP".
 *
 * Residual key of a matched pair j (the correspondences of s4p_icp_correspondences):
 *  - point metric: u_j = d2_j, the float of the correspondence contract;
 *  - plane metric: u_j = fl(r_j^2), r_j computed in double as in s4p_icp_plane.h.  A pair whose normal is zero has no key: it
 *    carries no plane term (weight 0 in the plane loss) and counts in entries [0] and [1] as in s4p_icp_plane_sums.
 *  M = the number of keyed pairs.  u_(k) = the exact k-th smallest key (1 <= k <= M), selected on the device over the key
 *  bits (radix select, integer atomics only): bit-exact and independent of the visiting order.
 *
 * Weights (computed in double):
 *  - TRIMMED: k = min(M, max(1, ceil(trim_fraction * n_Q))); w = 1 iff u <= u_(k), else 0.  Every pair tied with the
 *    threshold is kept, so more than k pairs may carry weight 1.
 *  - HUBER, TUKEY: scale s = `scale` when > 0; otherwise s = max(1.4826 sqrt(u_(ceil(M/2))), s_min) with
 *    s_min = 1e-6 max_distance (the MAD about zero; s_min keeps an exact fit from zeroing every Tukey weight).
 *    With cs = c s and cs2 = cs cs:  HUBER  w = 1 if u <= cs2, else cs / sqrt(u);
 *                                    TUKEY  w = (1 - u / cs2)^2 if u < cs2, else 0.
 *
 * Weighted sums: the layouts of s4p_icp.h (S4P_ICP_NSUMS) and s4p_icp_plane.h (S4P_ICP_PLANE_NSUMS) with every keyed pair's
 * terms multiplied by w_j in double, in the same lane order and the same fixed-order reduction as s4p_icp_sums /
 * s4p_icp_plane_sums: with every weight equal to 1 the sums are bit-identical to those.  One exception: plane entry [2] is
 * the count of pairs with w > 0 and a nonzero normal, so s4p_icp_solve_plane's degeneracy rule still works on a count.
 * s4p_icp_solve and s4p_icp_solve_plane apply unchanged.
 *
 * Info (S4P_ICP_ROBUST_NINFO doubles): [0] M, [1] k (TRIMMED: k; HUBER / TUKEY with an estimated scale: ceil(M/2); else 0),
 * [2] the bits of u_(k) as an unsigned integer (0 when k == 0), [3] s (0 for TRIMMED), [4] the count of matched pairs with
 * w > 0 (a pair without a key counts), [5] sum w (== sums[0]), [6], [7] 0.
 */
#ifndef S4P_ICP_ROBUST_H_
#define S4P_ICP_ROBUST_H_

#include "s4p_icp.h"
#include "s4p_icp_plane.h"

#ifdef __cplusplus
extern "C" {
#endif

#define S4P_ICP_LOSS_TRIMMED 1
#define S4P_ICP_LOSS_HUBER 2
#define S4P_ICP_LOSS_TUKEY 3

#define S4P_ICP_METRIC_POINT 0
#define S4P_ICP_METRIC_PLANE 1

#define S4P_ICP_ROBUST_NINFO 8
#define S4P_ICP_HUBER_C 1.345
#define S4P_ICP_TUKEY_C 4.685

typedef struct s4p_icp_robust {
  int32_t loss;                    /* S4P_ICP_LOSS_* */
  int32_t reserved0;
  double trim_fraction;            /* TRIMMED: xi in (0, 1] */
  double scale;                    /* HUBER / TUKEY: > 0 fixed, <= 0 estimated on the device */
  double c;                        /* HUBER / TUKEY tuning constant, > 0 */
  double reserved[4];
} s4p_icp_robust;

/* loss, trim_fraction 1, scale 0 (estimated), c = S4P_ICP_HUBER_C / S4P_ICP_TUKEY_C (0 for TRIMMED), reserved 0 */
void s4p_icp_robust_defaults(s4p_icp_robust* r, int32_t loss);

/* stage call, centred frame, float T (16, row-major, last row ignored): the weighted sums of `metric` (S4P_ICP_NSUMS or
 * S4P_ICP_PLANE_NSUMS doubles) and info (S4P_ICP_ROBUST_NINFO doubles, may be null) */
int32_t s4p_icp_robust_sums(s4p_icp_ctx* h, const float* T16_centred, int32_t metric, const s4p_icp_robust* robust, double* sums,
                            double* info);

/* As s4p_icp_refine / s4p_icp_refine_plane on the weighted sums: rmse_k = sqrt(sum w d2 / sum w); n_corr and history_n are
 * the count with w > 0; TOO_FEW when that count < min_correspondences (point metric: or sum w < 1, which s4p_icp_solve
 * rejects); DEGENERATE as s4p_icp_refine_plane.  info_out (may be null): the final pass's info. */
int32_t s4p_icp_refine_robust(s4p_icp_ctx* h, const s4p_icp_params* params, int32_t metric, const s4p_icp_robust* robust,
                              double* T16_inout, s4p_icp_result* result, double* info_out);

#ifdef __cplusplus
}
#endif
#endif
