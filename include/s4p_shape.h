/* s4p_shape.h -- radius-neighbourhood normals and surface variation in libsuper4pcs_normals.so, on an MI355X (gfx950).  The
 * functions work on an s4p_normals_ctx (include/s4p_normals.h) after s4p_normals_set_cloud[_device], on its cloud X (n
 * points), its stream and its work memory.  No CPU fallback.  The entry points carry the prefix s4p_shape_: the older
 * prefixes stay the closed sets their headers declare.
 *
 * s4p_normals_estimate takes at most 32 neighbours, and its radius only trims that list; here the neighbourhood is every
 * point within the radius, hundreds or thousands of them on a dense scan, and the eigenvalues of its covariance come back
 * with the normal.
 *
 * Contract ("Radius normals"), written so that the result is unique: the moments are sums of
 * integers, which have no order, so no walk order, no grid and no order of the device's work can change a bit of the
 * output, and a restatement on the CPU gives the same bits.  fl() is rounding to float; "double" steps are IEEE double
 * without contraction.
 *  - Neighbourhood of a query q: N(q) = { j : d2(q, j) <= fl(r*r) }, the product in float; d2 is that of s4p_cluster.h,
 *    dx*dx + (dy*dy + dz*dz) in float with dx = fl(x_j - q_x), no contraction.  A cloud point that is its own query
 *    counts, and so do its duplicates.  count = |N(q)|, exact.
 *  - Quantised offsets.  With E = ilogb(r) and s = 18 - E, r 2^s lies in [2^18, 2^19).  For every neighbour and
 *    coordinate a, u_a = rint(double(e_a) 2^s) as an integer, e_a being the very float difference d2 used (dx, dy, dz); the
 *    product is exact and ties go to even.  |u_a| <= 2^19 + 1 for every neighbour (section 34 derives it).  The resolution
 *    is r 2^-18.
 *  - Moments: S_a = sum u_a and Q_ab = sum u_a u_b (xx, xy, xz, yy, yz, zz) over N(q), as 64-bit integers.  The sums cannot
 *    wrap while count <= 2^24 (|Q_ab| <= 2^24 (2^19 + 1)^2 < 2^63); above that they are defined modulo 2^64 and mean
 *    nothing.  Nothing tests for it: a query with more than 2^24 neighbours within r costs count tests per query, and no
 *    such call finishes in a time anyone waits for.
 *  - Covariance, in double: k = double(count), m_a = double(S_a) / k, C_ab = double(Q_ab) / k - m_a m_b, the conversions of
 *    the integers rounding to nearest even, as s4p_normals.h computes a covariance; trace = (C00 + C11) + C22.
 *  - Degenerate rows: the normal is (0, 0, 0) and the eigenvalues are (0, 0, 0) when count < max(3, min_neighbours), when
 *    the trace is not > 0, or when the query has a coordinate that is not finite (its count is then 0 as well).
 *  - Normal: otherwise the cyclic Jacobi of s4p_normals.h on C; the eigenvector of the first smallest of the three diagonal
 *    entries, divided by its length sqrt((v0 v0 + v1 v1) + v2 v2), negated when its component of largest magnitude (the
 *    first of those on a tie, as s4p_normals.h) is negative, rounded to float.
 *  - Eigenvalues: the three diagonal entries as Jacobi leaves them, not clamped (a tiny negative value stays), sorted
 *    descending, each scaled by 2^(-2s) with ldexp in double and then rounded to float: l1 >= l2 >= l3 in the cloud's
 *    squared units.  Surface variation ("curvature") is l3 / (l1 + l2 + l3).
 *      normal  float[3 rows], interleaved as in s4p_normals.h; required
 *      eig     float[3 rows], l1, l2, l3 per row; may be null
 *      count   int32[rows]; may be null
 *    rows = n for s4p_shape_estimate (the cloud's own points, in the caller's order) and m for s4p_shape_estimate_at (the
 *    query positions qx, qy, qz, in the caller's order).
 *  - Host forms read and write host memory, _device forms memory of the context's device.  Two calls give the same bits;
 *    host and device forms give the same bits.  A call leaves the context's cloud and grid as they were.
 *
 * Limits.  Refused with S4P_NORMALS_ERR_BAD_ARG: a radius that is not finite, is <= 0 or whose float square is not finite
 * and normal (the rule of s4p_cluster.h: fl(r*r) >= 2^-126); min_neighbours < 1; a null normal; null query pointers with
 * m > 0; m outside [0, 2^31 - 2].  With m = 0 the call returns S4P_NORMALS_OK and touches nothing.  With
 * S4P_NORMALS_ERR_STATE: a call before set_cloud.  s4p_normals_last_error has the message.
 */
#ifndef S4P_SHAPE_H_
#define S4P_SHAPE_H_

#include <stdint.h>

#include "s4p_normals.h"

#ifdef __cplusplus
extern "C" {
#endif

int32_t s4p_shape_estimate(s4p_normals_ctx* h, float radius, int32_t min_neighbours, float* normal, float* eig, int32_t* count);
int32_t s4p_shape_estimate_device(s4p_normals_ctx* h, float radius, int32_t min_neighbours, float* normal, float* eig, int32_t* count);

int32_t s4p_shape_estimate_at(s4p_normals_ctx* h, const float* qx, const float* qy, const float* qz, int64_t m, float radius,
                              int32_t min_neighbours, float* normal, float* eig, int32_t* count);
int32_t s4p_shape_estimate_at_device(s4p_normals_ctx* h, const float* qx, const float* qy, const float* qz, int64_t m, float radius,
                                     int32_t min_neighbours, float* normal, float* eig, int32_t* count);

#ifdef __cplusplus
}
#endif
#endif
