/* s4p_icp_plane.h -- point-to-plane ICP in libsuper4pcs_icp.so, next to the point-to-point entry points of s4p_icp.h
 * (same context, same target grid, same correspondences).  DESIGN.md section "Point-to-plane ICP".
 *
 * Target normals:
 *  - s4p_icp_set_target_normals[_device]: one normal per target point, in the uploaded order; each is normalised in double
 *    and rounded to float, a zero or non-finite normal is stored as (0, 0, 0).
 *  - s4p_icp_estimate_normals: for target i, N(i) = { j : d2(p'_i, p'_j) <= fl(r*r) } (d2 as in the correspondence
 *    contract, i itself included).  |N(i)| < min_neighbours gives a zero normal; otherwise, with e_j = p'_j - p'_i and
 *    k = |N(i)| in double, C = sum e e^T / k - m m^T (m = sum e / k) and the normal is the unit eigenvector of C's smallest
 *    eigenvalue (cyclic Jacobi in double, first on ties), signed so that its component of largest magnitude (the first of
 *    equal ones) is positive, rounded to float.  Requires 0 < r <= max_distance and min_neighbours >= 3.
 *  - s4p_icp_set_target invalidates the normals; a plane call without normals returns S4P_ICP_ERR_STATE.
 *
 * Plane sums (S4P_ICP_PLANE_NSUMS doubles) over the pairs of s4p_icp_correspondences, with q^ = T q' (k_apply's order), the
 * winner p' and its normal nrm, all in double: a = [q^ x nrm ; nrm], r = (p' - q^) . nrm.
 *   [0] n, [1] sum d2, [2] n_plane (pairs whose normal is nonzero), [3] sum r^2,
 *   [4..24] upper triangle of A = sum a a^T (row-major), [25..30] b = sum a r.
 * A pair whose normal is zero counts in n and sum d2 only.
 */
#ifndef S4P_ICP_PLANE_H_
#define S4P_ICP_PLANE_H_

#include "s4p_icp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define S4P_ICP_ERR_DEGENERATE (-8)
#define S4P_ICP_PLANE_NSUMS 31

/* s4p_icp_result.status of s4p_icp_refine_plane, in addition to those of s4p_icp.h */
#define S4P_ICP_DEGENERATE 3         /* the plane system was degenerate (s4p_icp_solve_plane): T_k kept */

/* host (float32) or device SoA, n == the target's count */
int32_t s4p_icp_set_target_normals(s4p_icp_ctx* h, const float* nx, const float* ny, const float* nz, int64_t n);
int32_t s4p_icp_set_target_normals_device(s4p_icp_ctx* h, const float* nx, const float* ny, const float* nz, int64_t n);
int32_t s4p_icp_estimate_normals(s4p_icp_ctx* h, float radius, int32_t min_neighbours);
/* host SoA, n_P entries each, in the uploaded target order */
int32_t s4p_icp_target_normals(s4p_icp_ctx* h, float* nx, float* ny, float* nz);

/* stage call, centred frame, float T (16, row-major, last row ignored) */
int32_t s4p_icp_plane_sums(s4p_icp_ctx* h, const float* T16_centred, double* sums);

/* Solves A x = b for x = (omega, t); dT = [Rodrigues(omega) | t] (row-major 4x4).  Host only; needs no device.
 * S4P_ICP_ERR_DEGENERATE when n_plane < 6 or A is not safely positive definite: with s = sqrt(tr A_tt / tr A_ww), the
 * block-balanced B = D A D, D = diag(s, s, s, 1, 1, 1), must have lambda_min(B) > 1e-10 lambda_max(B). */
int32_t s4p_icp_solve_plane(const double* sums, double* dT16);

/* As s4p_icp_refine, minimising point-to-plane distances; status S4P_ICP_DEGENERATE stops the loop and keeps T_k. */
int32_t s4p_icp_refine_plane(s4p_icp_ctx* h, const s4p_icp_params* params, double* T16_inout, s4p_icp_result* result);

#ifdef __cplusplus
}
#endif
#endif
