/* s4p_icp_info.h -- the information matrix of a pairwise pose in libsuper4pcs_icp.so, next to the entry points of s4p_icp.h
 * (same context, same target grid, same correspondences).  DESIGN.md section "Multiway registration".
 *
 * How well the matched pairs constrain a pose: the 6x6 matrix Lambda = sum G^T G over the matched target points p, with
 * G = [-[p]x | I], so that xi^T Lambda xi is, to second order, the summed squared displacement of those points under a small
 * twist xi = (omega, v) applied on the left in the target's caller frame (p -> p + omega x p + v).  It is the weight of the
 * pair's edge in a pose graph (s4p_icp_posegraph.h).
 *
 * Information sums (S4P_ICP_INFO_NSUMS doubles) over the matched pairs of s4p_icp_correspondences for T (a pair the rejection
 * state of s4p_icp_reject.h removes is unmatched here too), with p' the winner's centred float target point, widened:
 *   [0]      n
 *   [1]      sum d2          (the contract's float d2, widened)
 *   [2..4]   sum p'_a
 *   [5..10]  sum p'_a * p'_b, upper triangle in the order xx, xy, xz, yy, yz, zz; each product of two floats in double (exact)
 * No float or double atomics; the lane order and the fixed-order reduction of the other sums: two calls return identical bits.
 *
 * s4p_icp_information: one pass for float(T in the centred frame) (s4p_icp_refine's conversion), then on the host in double,
 * no fused multiply-add, with c = the frame of s4p_icp_frame widened, s = [2..4], C = [5..10] and p = double(p') + double(c):
 *   S_a   = s_a + n * c_a                                                            (sum p)
 *   P_ab  = (C_ab + (s_a * c_b + c_a * s_b)) + n * (c_a * c_b)     for a <= b        (sum p p^T, the binomial expansion)
 *   tr    = (P_00 + P_11) + P_22
 *   M_ab  = (a == b ? tr - P_aa : -P_ab)                                             (sum |p|^2 I - p p^T)
 *   Lambda = [[M, [S]x], [-[S]x, n I]], row-major 6x6, the rotation block first (the (a, n) order of the plane sums' J), with
 *            [S]x = [[0, -S_2, S_1], [S_2, 0, -S_0], [-S_1, S_0, 0]]
 *   rmse  = sqrt([1] / n)
 * n == 0: info36, n_corr and rmse are all zero and the call returns S4P_ICP_OK.
 *
 * Both calls need a target and a source, else S4P_ICP_ERR_STATE; normals only where the rejection state needs them.
 */
#ifndef S4P_ICP_INFO_H_
#define S4P_ICP_INFO_H_

#include "s4p_icp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define S4P_ICP_INFO_NSUMS 11

/* stage call, centred frame, float T (16, row-major, last row ignored) */
int32_t s4p_icp_information_sums(s4p_icp_ctx* h, const float* T16_centred, double* sums);

/* host only, no device: the order of operations above on 11 sums and the frame c (3 floats, s4p_icp_frame's); info36
 * row-major; n_corr and rmse may be null.  S4P_ICP_ERR_BAD_ARG for a null sums, c3 or info36. */
int32_t s4p_icp_information_from_sums(const double* sums, const float* c3, double* info36, int64_t* n_corr, double* rmse);

/* T (16 doubles, row-major) in the caller's frame; info36 row-major; n_corr and rmse may be null */
int32_t s4p_icp_information(s4p_icp_ctx* h, const double* T16, double* info36, int64_t* n_corr, double* rmse);

#ifdef __cplusplus
}
#endif
#endif
