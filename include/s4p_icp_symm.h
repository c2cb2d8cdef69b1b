/* s4p_icp_symm.h -- symmetric ICP (Rusinkiewicz, "A Symmetric Objective Function for ICP", SIGGRAPH 2019) in
 * libsuper4pcs_icp.so, next to the entry points of s4p_icp.h, s4p_icp_plane.h and s4p_icp_gicp.h (same context, same target
 * grid, same normals, same correspondences).  DESIGN.md section "Symmetric ICP".
 *
 * The pair's offset is measured along the sum of both normals and both clouds are rotated half-way: exact whenever the pair
 * lies on a common second-order patch, not only on a common plane.
 *
 * Normals: target normals as in s4p_icp_plane.h, source normals as in s4p_icp_gicp.h (s4p_icp_set_source_normals is used as
 * it is; s4p_icp_set_source invalidates them).  A symmetric call without source normals, or without target normals, returns
 * S4P_ICP_ERR_STATE.
 *
 * Symmetric sums (S4P_ICP_SYMM_NSUMS doubles, the layout of S4P_ICP_PLANE_NSUMS) over the pairs of s4p_icp_correspondences.
 * Per pair, all in double, no fused multiply-add: u = q^ = T q' (k_apply's order, float, widened), v = the winner p'
 * (widened), its stored normal np, the stored source normal m, and with T's linear part as doubles
 *   nh_a  = (T_a0 * m_0 + T_a1 * m_1) + T_a2 * m_2                            (s4p_icp_gicp.h's expression, not renormalised)
 *   dot   = (np_0 * nh_0 + np_1 * nh_1) + np_2 * nh_2
 *   n_a   = np_a - nh_a  if dot < 0,  else  np_a + nh_a                       (both normals on one side: estimated normals
 *                                                                              carry an arbitrary sign; n is not normalised)
 * The pair carries a term iff some component of n is nonzero (a zero target normal with a nonzero source normal does; two
 * zero normals do not, and the pair then counts in [0] and [1] only, as in s4p_icp_plane_sums).  With a term:
 *   e_a = v_a - u_a,   h_a = u_a + v_a
 *   a_0 = h_1 * n_2 - h_2 * n_1,   a_1 = h_2 * n_0 - h_0 * n_2,   a_2 = h_0 * n_1 - h_1 * n_0                  (a = h x n)
 *   r   = (e_0 * n_0 + e_1 * n_1) + e_2 * n_2
 *   J   = (a_0, a_1, a_2, n_0, n_1, n_2)
 *   [0] n, [1] sum d2 (the contract's float d2), [2] the count of pairs with a term, [3] sum r * r,
 *   [4..24] upper triangle of sum J J^T, row-major (s4p_icp_plane.h's order), each term J_u * J_v,
 *   [25..30] sum J_u * r.
 * Point-to-plane is the same shape with a = q^ x np and n = np.
 *
 * s4p_icp_solve_symmetric (host, no device): the 6x6 system goes through s4p_icp_solve_plane's path (the [2] >= 6 test, the
 * balance of the rotation block, the eigenvalue-ratio test at 1e-10, the Cholesky solve; S4P_ICP_ERR_DEGENERATE where
 * s4p_icp_solve_plane returns it) and gives x = (a~, t~).  Then, in this order,
 *   m2 = (a~_0 * a~_0 + a~_1 * a~_1) + a~_2 * a~_2,   c = 1 / sqrt(1 + m2),   k = (c * c) / (1 + c),   K = [a~]x
 *   Rh_rs = ((r == s ? 1 : 0) + c * K_rs) + k * (a~_r * a~_s - (r == s ? m2 : 0))
 *           (the rotation by atan |a~| about a~: no trigonometry, no division at |a~| = 0)
 *   t'_r  = c * t~_r
 *   dT    = [Rh Rh | Rh t'],  (Rh Rh)_rs = (Rh_r0 * Rh_0s + Rh_r1 * Rh_1s) + Rh_r2 * Rh_2s,
 *                             (Rh t')_r  = (Rh_r0 * t'_0 + Rh_r1 * t'_1) + Rh_r2 * t'_2.
 *
 * Out of scope: robust losses (s4p_icp_robust.h refuses any metric but point and plane) and the batch (s4p_icp_batch.h
 * likewise).  Correspondence rejection (s4p_icp_reject.h) holds for this metric as for every other.
 */
#ifndef S4P_ICP_SYMM_H_
#define S4P_ICP_SYMM_H_

#include "s4p_icp_gicp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define S4P_ICP_SYMM_NSUMS S4P_ICP_PLANE_NSUMS

/* stage call, centred frame, float T (16, row-major, last row ignored) */
int32_t s4p_icp_symm_sums(s4p_icp_ctx* h, const float* T16_centred, double* sums);

/* host only: the step of the symmetric sums, dT (16, row-major) mapping q^ towards p' */
int32_t s4p_icp_solve_symmetric(const double* sums, double* dT16);

/* As s4p_icp_refine_plane with the symmetric sums and s4p_icp_solve_symmetric (TOO_FEW, DEGENERATE, the final pass and
 * order_source as there).  The reported and convergence quantity stays rmse = sqrt(sum d2 / n), comparable across metrics; it
 * need not fall monotonically under this metric. */
int32_t s4p_icp_refine_symm(s4p_icp_ctx* h, const s4p_icp_params* params, double* T16_inout, s4p_icp_result* result);

#ifdef __cplusplus
}
#endif
#endif
