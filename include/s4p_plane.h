/* s4p_plane.h -- RANSAC plane segmentation in libsuper4pcs_normals.so, on an MI355X (gfx950).  The functions work on an
 * s4p_normals_ctx (include/s4p_normals.h) after s4p_normals_set_cloud[_device], on its cloud X (n points), its stream and its
 * work memory.  No CPU fallback.  The entry points carry the prefix s4p_plane_: the older prefixes stay the closed sets their
 * headers declare.
 *
 * Contract ("Plane segmentation"), written so that the result is unique: every step below is defined by
 * the cloud, the exclude mask and the four options alone, every sum has one order, and a restatement on the CPU gives the
 * same bits.  fl() is rounding to float; "double" steps are IEEE double without contraction.
 *  - Alive points: those whose exclude[i] is 0, in ascending index order; exclude may be null, then every point is alive.
 *    Their number is m, reported as alive.  An excluded point is never sampled, counted or marked.  exclude lets several
 *    planes be peeled off one uploaded cloud: pass the union of the masks found so far.
 *  - Frame: c_k = fl(fl(0.5 lo_k) + fl(0.5 hi_k)) from the context's bounds lo, hi of the whole cloud (excluded points
 *    included), reported as centre, and x' = fl(x - c) in float, per coordinate.  Every residual is measured on x': a cloud
 *    at coordinates around 1e4 is as exact as one at the origin.
 *  - Candidate t (0 <= t < trials) takes its three sample positions from the elements 3t, 3t + 1, 3t + 2 of the splitmix64
 *    stream started at state seed (element k is mix(seed + (k + 1) 0x9E3779B97F4A7C15), mix being splitmix64's finaliser).
 *    An element u is mapped to the position floor(u m / 2^64) of the alive list.  The plane is computed in double from the
 *    three centred points a, b, c converted to double:
 *      e1 = b - a, e2 = c - a;  w = e1 x e2 with w0 = e1y e2z - e1z e2y, w1 = e1z e2x - e1x e2z, w2 = e1x e2y - e1y e2x, every
 *      product and the difference rounded once;  l2 = (w0 w0 + w1 w1) + w2 w2;  s = sqrt(l2);  v = (w0 / s, w1 / s, w2 / s);
 *      the sign rule: with a_k = |v_k|, the lead is v0 when a0 >= a1 and a0 >= a2, else v1 when a1 >= a2, else v2; when the
 *      lead is negative v is negated (the largest component is positive);
 *      n = float(v), d' = float(-((v0 a0 + v1 a1) + v2 a2)).
 *    A candidate is invalid when m < 3, when two of its positions are equal, when a centred sample has a non-finite
 *    coordinate, or when l2 is 0 or not finite.  An invalid candidate counts 0 and can never win.  valid_trials is the
 *    number of valid candidates.
 *  - Residual of a point against a plane (n, d'): r = fmaf(n0, x', fmaf(n1, y', fmaf(n2, z', d'))), three fused
 *    multiply-adds in float.  The point is an inlier when |r| <= distance.  A point whose centred coordinates are not
 *    finite is never an inlier (its r is not finite).
 *  - Winner: the valid candidate with the largest inlier count over the alive points; ties go to the smallest t.  trial
 *    is its t, or -1 when there is none (m < 3, or every candidate invalid): then inliers is 0, normal, d and d_centred are
 *    0, inlier is all zeros and the call returns S4P_NORMALS_OK.
 *  - Refit, repeated refine times on the current plane's inliers i_0 < i_1 < ... < i_(k-1) (ascending index):
 *      S = sum x' (3 doubles) and Q = sum x' x'^T (xx, xy, xz, yy, yz, zz; 6 doubles), products of the coordinates converted
 *      to double.  Two-level order: the list is cut into blocks of S4P_PLANE_SUM_BLOCK consecutive positions; every block is
 *      summed from zero in ascending position, and the block sums are then added from zero in ascending block order.
 *      mean = S / k, C_ab = Q_ab / k - mean_a mean_b, trace = (C00 + C11) + C22, as s4p_normals.h computes a covariance;
 *      the cyclic Jacobi of that library on C; the eigenvector of the smallest eigenvalue (the first smallest of the three
 *      diagonal entries), divided by its length sqrt((v0 v0 + v1 v1) + v2 v2), then the sign rule above;
 *      n = float(v), d' = float(-((v0 mean0 + v1 mean1) + v2 mean2)).  The inliers are then recounted against the new plane
 *      over all alive points.
 *      With k < 3 or a trace <= 0 the previous plane stays and the loop ends.
 *  - Output.  inliers and inlier (uint8[n], the caller's order, 0 or 1) are those of the final plane; normal = n (the sign
 *    rule holds for every plane above), d_centred = d', and d = float(double(d') - ((double(n0) c0 + double(n1) c1) +
 *    double(n2) c2)) with c converted to double, so that n . x + d = 0 in the caller's frame.  The mask is defined by the
 *    centred residual above, not by normal and d evaluated in float on the caller's coordinates, which loses the digits the
 *    centring keeps.
 *  - Host form: exclude and inlier in host memory; _device form: in memory of the context's device.  result is host memory
 *    in both.  Two calls give the same bits; host and device forms give the same bits.  A call leaves the context's cloud
 *    and grid as they were.
 *
 * Limits.  Refused with S4P_NORMALS_ERR_BAD_ARG: a null options, result or inlier; a distance that is not finite or is < 0
 * (0 is allowed); trials outside [1, S4P_PLANE_MAX_TRIALS]; refine outside [0, S4P_PLANE_MAX_REFINE].  With
 * S4P_NORMALS_ERR_STATE: a call before set_cloud.  s4p_normals_last_error has the message.
 */
#ifndef S4P_PLANE_H_
#define S4P_PLANE_H_

#include <stdint.h>

#include "s4p_normals.h"

#ifdef __cplusplus
extern "C" {
#endif

#define S4P_PLANE_MAX_TRIALS (1 << 20)
#define S4P_PLANE_MAX_REFINE 16
#define S4P_PLANE_SUM_BLOCK 128

typedef struct s4p_plane_options {
  float distance;
  int32_t trials;
  uint64_t seed;
  int32_t refine;
} s4p_plane_options;

typedef struct s4p_plane_result {
  float normal[3];
  float d;               /* n . x + d = 0 in the caller's frame */
  float centre[3];
  float d_centred;       /* the frame and the offset the inlier test uses */
  int64_t inliers;
  int64_t alive;
  int32_t trial;
  int32_t valid_trials;
} s4p_plane_result;

int32_t s4p_plane_segment(s4p_normals_ctx* h, const s4p_plane_options* options, const uint8_t* exclude, s4p_plane_result* result,
                          uint8_t* inlier);
int32_t s4p_plane_segment_device(s4p_normals_ctx* h, const s4p_plane_options* options, const uint8_t* exclude, s4p_plane_result* result,
                                 uint8_t* inlier);

#ifdef __cplusplus
}
#endif
#endif
