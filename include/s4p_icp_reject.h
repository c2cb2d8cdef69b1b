/* s4p_icp_reject.h -- correspondence rejection in libsuper4pcs_icp.so: a reciprocity filter and a normal-angle filter on
 * the pairs of s4p_icp_correspondences, next to the entry points of s4p_icp.h, s4p_icp_plane.h, s4p_icp_robust.h,
 * s4p_icp_gicp.h and s4p_icp_color.h (same context, same target grid, same forward search).  DESIGN.md section
 * "Correspondence rejection".
 *
 * The rejection is a state of the context (s4p_icp_set_rejection; off by default).  While it is off nothing changes: no
 * kernel of this header is launched and every result of the other headers keeps its bits.  While it is on, every sums stage
 * call (s4p_icp_sums, s4p_icp_plane_sums, s4p_icp_robust_sums, s4p_icp_gicp_sums, s4p_icp_color_sums) and every refine entry
 * point sees a rejected pair as unmatched: n_corr, fitness, history_n, the trim rank's M (the rank itself stays
 * ceil(trim_fraction * n_Q)) and the median scale are over the survivors.  s4p_icp_correspondences stays the raw one-way
 * search.  The plain point and plane sums under rejection are the weighted sums of s4p_icp_robust.h with every weight 1,
 * which have s4p_icp_sums' / s4p_icp_plane_sums' bits on the same pairs.
 *
 * For a float T in the centred frame, c(j) is the correspondence of s4p_icp.h (unchanged).  A pair (j, c(j)) goes through
 * the normal test first and, if it passes, the reciprocity test.
 *
 * Normal test (normal_mode 1 or 2).  np: the stored target normal of c(j) (s4p_icp_plane.h); nq: the stored source normal j
 * (s4p_icp_gicp.h); R: the linear part of the float T as doubles; all in double, no fused multiply-add:
 *   nh_a = (R_a0 * nq_0 + R_a1 * nq_1) + R_a2 * nq_2            (s4p_icp_gicp.h's rotation, not renormalised)
 *   c    = (np_0 * nh_0 + np_1 * nh_1) + np_2 * nh_2
 * The pair is kept when np or nq is (0, 0, 0) (no information: the generalized metric's convention), else when
 * |c| >= normal_cos (mode 1, unoriented normals) or c >= normal_cos (mode 2, oriented normals).  It needs target normals
 * (uploaded or estimated) and source normals (s4p_icp_set_source_normals); a pass without one of them returns
 * S4P_ICP_ERR_STATE, as the generalized metric does.
 *
 * Reciprocity test (reciprocal 1).  T is taken as rigid; the reverse map is T- = [M^T | t-] with M^T the transposed float
 * entries of T's linear part (exact) and, computed on the host with m, t the float entries of T as doubles,
 *   t-_a = float(-((m_0a * t_0 + m_1a * t_1) + m_2a * t_2)).
 * For a target point p'_i: p~ = T- p'_i in float (k_apply's order); r(i) is the source index j with the least
 * d2(p~, q'_j) = dx * dx + (dy * dy + dz * dz) (float) among d2 <= fl(d * d), ties to the smallest uploaded source index,
 * -1 if there is none.  The pair (j, c(j)) is kept iff r(c(j)) == j.  Consequences:
 *  - of two identical source points only the one with the lower index can be kept;
 *  - a pair whose forward d2 sits on the bound fl(d * d) may fail backwards through rounding (p~ is rounded, and T is
 *    only rigid up to rounding).  That is part of the contract: the reverse search is stated, not "symmetric".
 *
 * s4p_icp_rejection: per source point j in the uploaded order, why[j] = 0 kept, 1 unmatched, 2 rejected by the normal test,
 * 3 rejected by the reciprocity test; idx[j] = c(j) when kept, else -1; d2[j] = the forward float d2 when kept, else 0.
 * With the rejection off it reports the one-way search (why 0 / 1).
 * s4p_icp_rejection_counts: of the last pass that ran with the rejection on (any stage call, s4p_icp_rejection, or the
 * final pass of a refine): counts[0] matched one-way, [1] rejected by normals, [2] rejected by reciprocity, [3] kept;
 * [0] == [1] + [2] + [3].  Zeros before any such pass.
 *
 * The source grid of the reverse search is built once, when a pass first needs it after s4p_icp_set_source,
 * s4p_icp_set_target (the frame and d belong to the target) or s4p_icp_set_rejection; never inside a refine loop.
 */
#ifndef S4P_ICP_REJECT_H_
#define S4P_ICP_REJECT_H_

#include "s4p_icp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define S4P_ICP_REJECT_NORMALS_OFF 0
#define S4P_ICP_REJECT_NORMALS_UNORIENTED 1   /* |c| >= normal_cos, normal_cos in [0, 1] */
#define S4P_ICP_REJECT_NORMALS_ORIENTED 2     /* c >= normal_cos, normal_cos in [-1, 1] */

#define S4P_ICP_WHY_KEPT 0
#define S4P_ICP_WHY_UNMATCHED 1
#define S4P_ICP_WHY_NORMALS 2
#define S4P_ICP_WHY_RECIPROCITY 3

typedef struct s4p_icp_reject {
  int32_t reciprocal;     /* 0 / 1 */
  int32_t normal_mode;    /* S4P_ICP_REJECT_NORMALS_* */
  double normal_cos;      /* cosine of the largest accepted angle; ignored when normal_mode is 0 */
  double reserved[4];
} s4p_icp_reject;

void s4p_icp_reject_defaults(s4p_icp_reject* r);                          /* everything off */
/* null: off.  S4P_ICP_ERR_BAD_ARG for a flag or mode outside its values, or a cosine outside the mode's range (NaN included) */
int32_t s4p_icp_set_rejection(s4p_icp_ctx* h, const s4p_icp_reject* r);
/* stage call, centred frame, float T (16, row-major, last row ignored); n_Q entries each, host */
int32_t s4p_icp_rejection(s4p_icp_ctx* h, const float* T16_centred, int32_t* idx, float* d2, int32_t* why);
int32_t s4p_icp_rejection_counts(const s4p_icp_ctx* h, int64_t counts[4]);

#ifdef __cplusplus
}
#endif
#endif
