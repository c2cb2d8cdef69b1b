/* s4p_feature.h -- Fast Point Feature Histograms (Rusu, Blodow, Beetz, ICRA 2009) and a feature-space matcher in
 * libsuper4pcs_normals.so, on an MI355X (gfx950).  The functions work on an s4p_normals_ctx (include/s4p_normals.h), on its
 * stream and its work memory.  No CPU fallback.  The entry points carry the prefix s4p_feature_: the older prefixes stay
 * the closed sets their headers declare.
 *
 * Contract ("Descriptors"), written so that the result is unique.  A histogram is a sum of integers,
 * which have no order, so no walk order, no grid and no order of the device's work can change a bit of the output, and a
 * restatement on the CPU gives the same bits.  fl() is rounding to float; every float step is IEEE single without
 * contraction, and the only functions are sqrtf, floorf, fminf and the division; a three-term dot product a.b is
 * (a0 b0 + a1 b1) + a2 b2 everywhere.
 *
 * s4p_feature_fpfh[_device](h, normals, radius, fpfh, count), after s4p_normals_set_cloud[_device], on the cloud X (n points):
 *      normals  float[3 n], interleaved as in s4p_normals.h, the caller's: expected of unit length and CONSISTENTLY ORIENTED
 *               (s4p_orient_consistent).  With normals of arbitrary sign (as s4p_normals_estimate and s4p_shape_estimate
 *               return them) the descriptor is defined just the same and is useless for matching.  required
 *      radius   the rules of s4p_shape.h
 *      fpfh     uint16[33 n]: three groups of eleven bins (alpha, phi, theta), every value in [0, 4096].  required
 *      count    int32[n]: c_i below.  may be null
 *  - Valid point i: its three coordinates are finite, its normal is finite and (nx nx + ny ny) + nz nz > 0.
 *  - Pairs of a valid i: every valid j with 0 < d2(i, j) <= fl(r*r); d2 and the float differences dx, dy, dz of
 *    d = p_j - p_i are exactly those of s4p_cluster.h (dx*dx + (dy*dy + dz*dz)).  The point itself and its duplicates
 *    (d2 = 0) do not pair.  A point that is not valid has no pairs.
 *  - Darboux frame of a pair (PCL's computePairFeatures): len = sqrtf(d2), a_i = n_i . d, a_j = n_j . d.  When
 *    |a_i| >= |a_j| the source s is i, the target t is j and e = d; otherwise s = j, t = i and e = -d.  a_s = n_s . e (of
 *    the negated vector in the second case), phi = a_s / len.  v = e x n_s, that is (e1 n2 - e2 n1, e2 n0 - e0 n2,
 *    e0 n1 - e1 n0); |v| = sqrtf(v . v); when |v| > 0 does not hold the pair is SKIPPED.  v = v / |v| by components,
 *    w = n_s x v, alpha = v . n_t, x = n_s . n_t, y = w . n_t.
 *  - Bins.  For f = alpha and f = phi: t = 11 * ((f + 1) * 0.5); the bin is 0 when t >= 1 does not hold (a NaN included),
 *    10 when t >= 10, and int(floorf(t)) otherwise: min(10, max(0, floor(11 (f + 1) / 2))).
 *    theta is the angle of (x, y), binned uniformly over [-pi, pi) without atan2, against the ten boundary directions
 *    S4P_FEATURE_THETA_BOUNDS below, (bx_k, by_k) = fl(cos beta_k), fl(sin beta_k), beta_k = -pi + 2 pi k / 11, k = 1 .. 10:
 *    c_k = fl(fl(bx_k * y) - fl(by_k * x)) and
 *        bin = sum_{k = 1..5} [y >= 0 or c_k >= 0] + sum_{k = 6..10} [y >= 0 and c_k >= 0].
 *    (A boundary of the lower half plane lies below every vector with y >= 0; otherwise boundary and vector lie in one
 *    half plane, less than pi apart, and the cross product's sign decides.)  The table is part of the contract.
 *  - SPFH.  H_i[33] counts the accepted (not skipped) pairs of i in 32 bits, one count per group and pair; c_i is their
 *    number.  S_i[b] = (H_i[b] 2^15) / c_i in integer division (the product in 64 bits), at most 2^15; all zeros when i is
 *    not valid or c_i = 0.  c_i < 2^32 is presumed: a point with more pairs costs that many per call.
 *  - Weights.  q_ij = int(fminf(fl(64 * fl(fl(r*r) / d2)), 65536)): PCL's 1 / d2 in steps of 1 / 64 at the rim, saturated
 *    for neighbours nearer than r / 32; q in [64, 2^16].
 *  - FPFH.  A_i[b] = sum q_ij S_j[b] over ALL pairs of i, skipped or not, as 64-bit integers (below 2^31 per pair and
 *    group: no wrap below 2^32 pairs).  For each group of eleven bins T = sum of A over the group, and
 *    F[b] = uint16(floor((double(A[b]) / double(T)) * 4096.0)), 0 when T = 0.  A row is all zeros exactly when the point is
 *    not valid or none of its pairs j has c_j > 0.  A plane with one normal puts every pair into bins 5, 16 and 27.
 *  - Host forms read and write host memory, _device forms memory of the context's device.  Two calls give the same bits;
 *    host and device forms give the same bits.  A call leaves the context's cloud and grid as they were.
 *  - Refusals: S4P_NORMALS_ERR_BAD_ARG for a radius s4p_shape.h refuses, a null normals, a null fpfh;
 *    S4P_NORMALS_ERR_STATE before set_cloud.
 *
 * s4p_feature_match[_device](h, fa, m, fb, n, mutual, idx, dist), on any created context, with or without a cloud:
 *      fa, fb   uint16[33 m], uint16[33 n]: two descriptor tables, every value at most S4P_FEATURE_MAX
 *      idx      int32[m].  required when m > 0
 *      dist     int32[m].  may be null
 *  - D(a, b) = sum over the 33 bins of (fa[a][k] - fb[b][k])^2, exact in int32 (33 * 2^24 < 2^30).
 *  - A row is usable when it is not all zeros.  best_B(a) is the usable row b of B with the smallest (D(a, b), b);
 *    best_A(b) the usable row a of A with the smallest (D(a, b), a).
 *  - idx[a] = best_B(a) and dist[a] = that D; both are -1 when row a is not usable, when B has no usable row, or when
 *    mutual != 0 and best_A(idx[a]) != a.
 *  - Refusals: S4P_NORMALS_ERR_BAD_ARG for a value above S4P_FEATURE_MAX in either table (nothing is written), for m or n
 *    outside [0, 2^31 - 2], for a null fa or idx with m > 0 and a null fb with n > 0.  With m = 0 the call returns
 *    S4P_NORMALS_OK and touches nothing.  With n = 0 every idx and dist is -1.
 * s4p_normals_last_error has the message.
 */
#ifndef S4P_FEATURE_H_
#define S4P_FEATURE_H_

#include <stdint.h>

#include "s4p_normals.h"

#define S4P_FEATURE_BINS 33       /* three groups of eleven */
#define S4P_FEATURE_MAX 4096      /* the largest value of a descriptor */

/* (fl(cos beta_k), fl(sin beta_k)), beta_k = -pi + 2 pi k / 11, k = 1 .. 10 */
#define S4P_FEATURE_THETA_BOUNDS                                                                                    \
  {                                                                                                                 \
    {-0.841253519f, -0.540640831f}, {-0.415415019f, -0.909631968f}, {0.142314836f, -0.989821434f},                  \
    {0.654860735f, -0.755749583f}, {0.959492981f, -0.281732559f}, {0.959492981f, 0.281732559f},                     \
    {0.654860735f, 0.755749583f}, {0.142314836f, 0.989821434f}, {-0.415415019f, 0.909631968f},                      \
    {-0.841253519f, 0.540640831f}                                                                                   \
  }

#ifdef __cplusplus
extern "C" {
#endif

int32_t s4p_feature_fpfh(s4p_normals_ctx* h, const float* normals, float radius, uint16_t* fpfh, int32_t* count);
int32_t s4p_feature_fpfh_device(s4p_normals_ctx* h, const float* normals, float radius, uint16_t* fpfh, int32_t* count);

int32_t s4p_feature_match(s4p_normals_ctx* h, const uint16_t* fa, int64_t m, const uint16_t* fb, int64_t n, int32_t mutual, int32_t* idx,
                          int32_t* dist);
int32_t s4p_feature_match_device(s4p_normals_ctx* h, const uint16_t* fa, int64_t m, const uint16_t* fb, int64_t n, int32_t mutual,
                                 int32_t* idx, int32_t* dist);

#ifdef __cplusplus
}
#endif
#endif
