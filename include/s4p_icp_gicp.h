/* s4p_icp_gicp.h -- generalized (plane-to-plane) ICP in libsuper4pcs_icp.so, next to the entry points of s4p_icp.h and
 * s4p_icp_plane.h (same context, same target grid, same correspondences).  DESIGN.md section "Generalized ICP".
 *
 * Source normals:
 *  - s4p_icp_set_source_normals[_device]: one normal per source point, in the uploaded order and in the frame of the source
 *    as uploaded; each is normalised in double and rounded to float, a zero or non-finite normal is stored as (0, 0, 0)
 *    (the rule of s4p_icp_set_target_normals; the _device entry point copies to the host first, so both store the same bits).
 *  - s4p_icp_set_source invalidates them; a generalized call without source normals, or without target normals
 *    (s4p_icp_plane.h), returns S4P_ICP_ERR_STATE.
 *
 * Generalized sums (S4P_ICP_GICP_NSUMS doubles, the layout of S4P_ICP_PLANE_NSUMS) over the pairs of
 * s4p_icp_correspondences.  Per pair, all in double, no fused multiply-add: q^ = T q' (k_apply's order, float), the winner
 * p', its stored normal np, the stored source normal nq, k = 1 - epsilon, and with R the linear part of the float T as doubles
 *   nh_a  = (R_a0 * nq_0 + R_a1 * nq_1) + R_a2 * nq_2                         (not renormalised)
 *   S_ab  = (D_ab - k * (np_a * np_b)) - k * (nh_a * nh_b),  D = 2 I           (a <= b; S symmetric)
 *           i.e. S = C(np) + C(nh) with C(n) = I - (1 - epsilon) n n^T; a zero normal gives C = I by the same expression
 *   c00 = S11 * S22 - S12 * S12    c01 = S02 * S12 - S01 * S22    c02 = S01 * S12 - S02 * S11
 *   c11 = S00 * S22 - S02 * S02    c12 = S01 * S02 - S00 * S12    c22 = S00 * S11 - S01 * S01
 *   det = (S00 * c00 + S01 * c01) + S02 * c02,   M_ab = c_ab / det             (M = S^-1, symmetric)
 *   r_a = p'_a - q^_a,   g_a = (M_a0 * r_0 + M_a1 * r_1) + M_a2 * r_2
 *   B_0c = q^_1 * M_2c - q^_2 * M_1c,  B_1c = q^_2 * M_0c - q^_0 * M_2c,  B_2c = q^_0 * M_1c - q^_1 * M_0c     (B = [q^]x M)
 *   W_a0 = q^_1 * B_a2 - q^_2 * B_a1,  W_a1 = q^_2 * B_a0 - q^_0 * B_a2,  W_a2 = q^_0 * B_a1 - q^_1 * B_a0     (W = B [q^]x^T)
 *   h = (q^_1 * g_2 - q^_2 * g_1,  q^_2 * g_0 - q^_0 * g_2,  q^_0 * g_1 - q^_1 * g_0)                          (h = q^ x g)
 * With J = [-[q^]x | I]:  J^T M J = [W B; B^T M],  J^T g = [h; g].
 *   [0] n, [1] sum d2 (the contract's float d2), [2] n again (every pair carries a term),
 *   [3] sum (r_0 * g_0 + r_1 * g_1) + r_2 * g_2,
 *   [4..24] upper triangle of A = sum J^T M J, row-major: W00 W01 W02 B00 B01 B02 | W11 W12 B10 B11 B12 | W22 B20 B21 B22 |
 *           M00 M01 M02 | M11 M12 | M22,
 *   [25..30] b = sum [h ; g].
 * Point-to-plane is the special case M = np np^T of the same expressions.  s4p_icp_solve_plane solves these sums unchanged.
 * epsilon must be in [1e-6, 1]: S is then positive definite (eigenvalues in [2 epsilon - 2e-7, 2] for float-unit normals).
 */
#ifndef S4P_ICP_GICP_H_
#define S4P_ICP_GICP_H_

#include "s4p_icp_plane.h"

#ifdef __cplusplus
extern "C" {
#endif

#define S4P_ICP_GICP_NSUMS S4P_ICP_PLANE_NSUMS
#define S4P_ICP_GICP_EPSILON 1e-3       /* the usual choice (PCL's gicp_epsilon) */
#define S4P_ICP_GICP_EPSILON_MIN 1e-6
#define S4P_ICP_GICP_EPSILON_MAX 1.0

/* host (float32) or device SoA, n == the source's count */
int32_t s4p_icp_set_source_normals(s4p_icp_ctx* h, const float* nx, const float* ny, const float* nz, int64_t n);
int32_t s4p_icp_set_source_normals_device(s4p_icp_ctx* h, const float* nx, const float* ny, const float* nz, int64_t n);
/* host SoA, n_Q entries each, in the uploaded source order */
int32_t s4p_icp_source_normals(s4p_icp_ctx* h, float* nx, float* ny, float* nz);

/* stage call, centred frame, float T (16, row-major, last row ignored) */
int32_t s4p_icp_gicp_sums(s4p_icp_ctx* h, const float* T16_centred, double epsilon, double* sums);

/* As s4p_icp_refine_plane with the generalized sums and s4p_icp_solve_plane.  The reported and convergence quantity stays
 * rmse = sqrt(sum d2 / n), comparable across metrics; it need not fall monotonically under this metric. */
int32_t s4p_icp_refine_gicp(s4p_icp_ctx* h, const s4p_icp_params* params, double epsilon, double* T16_inout, s4p_icp_result* result);

#ifdef __cplusplus
}
#endif
#endif
