/* s4p_knn.h -- k-nearest-neighbour queries and outlier removal in libsuper4pcs_normals.so, on an MI355X (gfx950).  The
 * functions work on an s4p_normals_ctx (include/s4p_normals.h) after s4p_normals_set_cloud[_device]: the same cloud X, the
 * same grid, the same search.  No CPU fallback.
 *
 * Contract (DESIGN.md section "Neighbour queries and outlier removal"):
 *  - d2(q, j) = dx*dx + (dy*dy + dz*dz) in float, dx = fl(x_j - q_x); neighbours are ordered lexicographically by
 *    (d2, index), ties to the smaller index, as in s4p_normals.h.  A radius > 0 bounds the search at d2 <= fl(r*r); a
 *    radius <= 0 is unbounded.
 *  - Lists (s4p_knn_search: the cloud's own points are the queries, m = n; s4p_knn_search_at: m caller queries, SoA):
 *      idx  int32[m * k], row-major, row i = the neighbours of query i in ascending (d2, index) order, padded with -1
 *      d2   float[m * k], the neighbours' d2, padded with +inf
 *      cnt  int32[m], the number of neighbours found (may be null)
 *    exclude_self = 1 (self form only) leaves out the one candidate whose index is the query's own index and nothing else:
 *    a duplicate of the point stays, at d2 = 0.  A non-finite query gets cnt = 0 (all -1, all +inf).
 *  - Statistical outlier removal (s4p_outliers_statistical).  For each point j the list with exclude_self = 1 and an
 *    unbounded radius, so cnt_j = min(k, n - 1); m_j = (sum of sqrt((double)d2) over the list in ascending order, in
 *    double) / cnt_j, and m_j = 0 when cnt_j = 0.  mu = sum m_j / n; sigma^2 = sum (m_j - mu)^2 / (n - 1), 0 for n < 2; both
 *    sums in double in a fixed order (per-workgroup partial rows, then a fixed-order final kernel; no float or double
 *    atomics).  t = mu + std_ratio * sigma; keep_j = (m_j <= t).
 *      mean_dist  double[n], m_j (may be null)
 *      keep       uint8[n], 1 = kept
 *      stats      n, mu, sigma, t and the number kept (may be null)
 *  - Radius outlier removal (s4p_outliers_radius): keep_j = 1 exactly when the search with the radius, k = min_neighbours
 *    and exclude_self = 1 fills all k slots, that is when at least min_neighbours other points lie within the radius.
 *  - Host forms read and write host memory, _device forms memory of the context's device (stats is host memory in both).
 *    Two calls give the same bits; host and device forms give the same bits.
 *
 * Limits (S4P_NORMALS_ERR_BAD_ARG outside them; S4P_NORMALS_ERR_STATE before set_cloud): 1 <= k <= 32; radius finite (<= 0:
 * unbounded) for the lists; 0 <= m <= 2^31 - 2; std_ratio finite and >= 0; for radius removal radius finite and > 0 and
 * 1 <= min_neighbours <= 32; non-null idx, d2 and keep (and queries when m > 0).  Error codes and s4p_normals_last_error
 * as in s4p_normals.h.  The lists are exactly the k smallest (d2, index) for every cloud that set_cloud accepts: it refuses
 * a cloud whose planned cell edge is below 2^-43, where neighbours' d2 becomes subnormal (s4p_normals.h, Limits).
 */
#ifndef S4P_KNN_H_
#define S4P_KNN_H_

#include <stdint.h>

#include "s4p_normals.h"

#ifdef __cplusplus
extern "C" {
#endif

#define S4P_KNN_MIN_K 1
#define S4P_KNN_MAX_K 32

typedef struct s4p_outliers_stats {
  int64_t n;
  double mean;                     /* mu */
  double stddev;                   /* sigma */
  double threshold;                /* t = mu + std_ratio * sigma */
  int64_t kept;
} s4p_outliers_stats;

int32_t s4p_knn_search(s4p_normals_ctx* h, int32_t k, float radius, int32_t exclude_self, int32_t* idx, float* d2, int32_t* cnt);
int32_t s4p_knn_search_device(s4p_normals_ctx* h, int32_t k, float radius, int32_t exclude_self, int32_t* idx, float* d2,
                              int32_t* cnt);

int32_t s4p_knn_search_at(s4p_normals_ctx* h, const float* qx, const float* qy, const float* qz, int64_t m, int32_t k,
                          float radius, int32_t* idx, float* d2, int32_t* cnt);
int32_t s4p_knn_search_at_device(s4p_normals_ctx* h, const float* qx, const float* qy, const float* qz, int64_t m, int32_t k,
                                 float radius, int32_t* idx, float* d2, int32_t* cnt);

int32_t s4p_outliers_statistical(s4p_normals_ctx* h, int32_t k, double std_ratio, double* mean_dist, uint8_t* keep,
                                 s4p_outliers_stats* stats);
int32_t s4p_outliers_statistical_device(s4p_normals_ctx* h, int32_t k, double std_ratio, double* mean_dist, uint8_t* keep,
                                        s4p_outliers_stats* stats);

int32_t s4p_outliers_radius(s4p_normals_ctx* h, float radius, int32_t min_neighbours, uint8_t* keep);
int32_t s4p_outliers_radius_device(s4p_normals_ctx* h, float radius, int32_t min_neighbours, uint8_t* keep);

#ifdef __cplusplus
}
#endif
#endif
