/* s4p_icp_color.h -- coloured ICP (Park, Zhou, Koltun: "Colored Point Cloud Registration Revisited", ICCV 2017) in
 * libsuper4pcs_icp.so, next to the entry points of s4p_icp.h and s4p_icp_plane.h (same context, same target grid, same
 * correspondences: nearest in geometry only).  DESIGN.md section "Coloured ICP".
 *
 * The library works on one scalar per point, an intensity (a grey value of rgb, a LiDAR reflectance): the layers above
 * turn colour into it.
 *
 * Intensities:
 *  - s4p_icp_set_target_intensity[_device] / s4p_icp_set_source_intensity[_device]: one float per point, in the uploaded
 *    order, stored as given; n must be the cloud's count and every value finite, else S4P_ICP_ERR_BAD_ARG.  The _device
 *    entry points copy to the host first, so both store the same bits.
 *  - s4p_icp_set_source invalidates the source intensity.  s4p_icp_set_target invalidates the target intensity and the
 *    gradients.  Every call that replaces the target normals (s4p_icp_set_target_normals[_device],
 *    s4p_icp_estimate_normals) or the target intensity invalidates the gradients.
 *
 * Gradients, s4p_icp_estimate_color_gradients(h, r, min_neighbours): needs target normals and target intensity (else
 * S4P_ICP_ERR_STATE), 0 < r <= max_distance and min_neighbours >= 4 (else S4P_ICP_ERR_BAD_ARG).  For target i with the
 * stored normal n and intensity I_i, N(i) = { j : d2(p'_i, p'_j) <= fl(r*r) } is s4p_icp_estimate_normals' neighbourhood
 * (float d2 of the correspondence contract, i itself included), k = |N(i)|.  All in double, no fused multiply-add, the
 * neighbours in the order of the walk over the grid (27 cells in the order of s4p_icp_estimate_normals, each cell's
 * points in their stored order); per neighbour j
 *   e_a = p'_j,a - p'_i,a,   en = (e_0 * n_0 + e_1 * n_1) + e_2 * n_2,   u_a = e_a - en * n_a,   dI = I_j - I_i
 *   S_ab += u_a * u_b  (a <= b),   b_a += u_a * dI
 * then
 *   tr = (S_00 + S_11) + S_22,   A_ab = S_ab + tr * (n_a * n_b)               (A = S + tr(S) n n^T: the row that keeps
 *                                                                              g in the tangent plane, at the scale of S)
 *   c00 = A11 * A22 - A12 * A12    c01 = A02 * A12 - A01 * A22    c02 = A01 * A12 - A02 * A11
 *   c11 = A00 * A22 - A02 * A02    c12 = A01 * A02 - A00 * A12    c22 = A00 * A11 - A01 * A01
 *   det = (A00 * c00 + A01 * c01) + A02 * c02
 *   g_a = ((c_a0 * b_0 + c_a1 * b_1) + c_a2 * b_2) / det,   rounded to float                     (g = A^-1 b, c symmetric)
 * The gradient is (0, 0, 0) when k < min_neighbours, when the normal is zero, or when lambda_min(A) <= 1e-6 lambda_max(A)
 * (eigenvalues by the cyclic Jacobi of s4p_icp_estimate_normals, in double).  Two calls give the same bits.
 * s4p_icp_target_color_gradients returns them in the uploaded target order.
 *
 * Colour sums (S4P_ICP_COLOR_NSUMS doubles, the layout of S4P_ICP_PLANE_NSUMS) over the pairs of s4p_icp_correspondences.
 * Per pair whose stored target normal n is nonzero, all in double, no fused multiply-add: q^ = T q' (k_apply's order,
 * float), the winner p', its gradient g and intensity I_p, the source point's intensity I_q, wg = lambda, wc = 1 - lambda
 *   r_a  = p'_a - q^_a,   s = (r_0 * n_0 + r_1 * n_1) + r_2 * n_2
 *   aG   = (q^_1 * n_2 - q^_2 * n_1,  q^_2 * n_0 - q^_0 * n_2,  q^_0 * n_1 - q^_1 * n_0,  n_0, n_1, n_2)
 *   gn   = (g_0 * n_0 + g_1 * n_1) + g_2 * n_2,   gp_a = g_a - gn * n_a                                  (g in the plane)
 *   rC   = ((I_q - I_p) + ((g_0 * r_0 + g_1 * r_1) + g_2 * r_2)) - s * gn
 *          i.e. I_q minus the first-order intensity of the target at q^'s projection onto the tangent plane
 *   aC   = (q^_1 * gp_2 - q^_2 * gp_1,  q^_2 * gp_0 - q^_0 * gp_2,  q^_0 * gp_1 - q^_1 * gp_0,  gp_0, gp_1, gp_2)
 *   [0] n, [1] sum d2 (the contract's float d2), [2] the number of pairs that carry a term (nonzero normal),
 *   [3] sum wg * (s * s) + wc * (rC * rC),
 *   [4..24] upper triangle of sum wg * (aG_u * aG_v) + wc * (aC_u * aC_v), row-major,
 *   [25..30] sum wg * (aG_u * s) + wc * (aC_u * rC).
 * A pair whose normal is zero counts in [0] and [1] only.  A zero gradient takes part through the same expressions
 * (aC = 0, rC = I_q - I_p).  lambda must be in [0, 1].  At lambda = 1 the entries [2..30] are point-to-plane's.
 * s4p_icp_solve_plane solves these sums unchanged.  A colour call without target normals, target intensity, gradients or
 * source intensity returns S4P_ICP_ERR_STATE.  Robust losses (s4p_icp_robust.h) do not cover this metric.
 */
#ifndef S4P_ICP_COLOR_H_
#define S4P_ICP_COLOR_H_

#include "s4p_icp_plane.h"

#ifdef __cplusplus
extern "C" {
#endif

#define S4P_ICP_COLOR_NSUMS S4P_ICP_PLANE_NSUMS
#define S4P_ICP_COLOR_LAMBDA 0.968      /* the weight of the geometric term (Open3D's lambda_geometric) */
#define S4P_ICP_COLOR_MIN_NEIGHBOURS 4  /* the smallest min_neighbours of s4p_icp_estimate_color_gradients */
#define S4P_ICP_COLOR_GATE 1e-6         /* gradient 0 when lambda_min(A) <= gate * lambda_max(A) */

/* host (float32) or device, n == the cloud's count, every value finite */
int32_t s4p_icp_set_target_intensity(s4p_icp_ctx* h, const float* intensity, int64_t n);
int32_t s4p_icp_set_target_intensity_device(s4p_icp_ctx* h, const float* intensity, int64_t n);
int32_t s4p_icp_set_source_intensity(s4p_icp_ctx* h, const float* intensity, int64_t n);
int32_t s4p_icp_set_source_intensity_device(s4p_icp_ctx* h, const float* intensity, int64_t n);

int32_t s4p_icp_estimate_color_gradients(s4p_icp_ctx* h, float radius, int32_t min_neighbours);
/* host SoA, n_P entries each, in the uploaded target order */
int32_t s4p_icp_target_color_gradients(s4p_icp_ctx* h, float* gx, float* gy, float* gz);

/* stage call, centred frame, float T (16, row-major, last row ignored) */
int32_t s4p_icp_color_sums(s4p_icp_ctx* h, const float* T16_centred, double lambda, double* sums);

/* As s4p_icp_refine_plane with the colour sums and s4p_icp_solve_plane.  The reported and convergence quantity stays
 * rmse = sqrt(sum d2 / n), comparable across metrics; it need not fall monotonically under this metric. */
int32_t s4p_icp_refine_color(s4p_icp_ctx* h, const s4p_icp_params* params, double lambda, double* T16_inout, s4p_icp_result* result);

#ifdef __cplusplus
}
#endif
#endif
