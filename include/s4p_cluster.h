/* s4p_cluster.h -- density clustering (DBSCAN) and fixed-radius density in libsuper4pcs_normals.so, on an MI355X (gfx950).
 * The functions work on an s4p_normals_ctx (include/s4p_normals.h) after s4p_normals_set_cloud[_device], on its cloud X (n
 * points), its stream and its work memory.  No CPU fallback.  The entry points carry the prefix s4p_cluster_: the older
 * prefixes stay the closed sets their headers declare.
 *
 * Contract ("Density clustering"), written so that the result is unique: every set below is defined
 * by the cloud and the two parameters alone, so no order of the device's atomics can change a bit of the output, and a
 * restatement on the CPU (a grid, a union-find, a ranking) gives the same arrays.
 *  - Neighbourhood: j is a neighbour of i when d2(i, j) <= fl(eps*eps), the product in float; d2 is that of s4p_knn.h,
 *    dx*dx + (dy*dy + dz*dz) in float with dx = fl(x_j - x_i), no contraction: the same bits for (i, j) and (j, i).  The
 *    point itself and its duplicates count.
 *  - Density: count_i = the number of neighbours of i, i included (so count_i >= 1).
 *  - Core: i is a core point when count_i >= min_points.
 *  - Cluster: a connected component of the graph whose vertices are the core points and whose edges join neighbours.
 *  - Border: a point that is not core and has at least one core neighbour.  It joins the cluster of its nearest core
 *    neighbour under the order (bits of d2, index): the only place where classical DBSCAN depends on the visiting order.
 *  - Noise: every other point; label -1.
 *  - Labels: clusters are numbered 0 .. C - 1 in ascending order of their smallest core index.
 *      label  int32[n], the cluster of every point, -1 for noise
 *      kind   uint8[n], S4P_CLUSTER_NOISE / _BORDER / _CORE (may be null)
 *      stats  the numbers of core, border and noise points and of clusters (may be null; host memory in both forms)
 *  - s4p_cluster_density writes count int32[n], the exact count_i with radius in the place of eps.
 *  - Host forms read and write host memory, _device forms memory of the context's device.  Two calls give the same bits;
 *    host and device forms give the same bits.  A call leaves the context's cloud and grid as they were.
 *
 * Limits.  Refused with S4P_NORMALS_ERR_BAD_ARG: eps or radius that is not finite, is <= 0 or whose float square is not
 * finite and normal (fl(eps*eps) >= FLT_MIN = 2^-126, so eps above about 1.1e-19: a subnormal or zero square cannot bound
 * float distances); min_points < 1; a null label or count.  The cloud's scale is limited by set_cloud (s4p_normals.h).
 * With S4P_NORMALS_ERR_STATE: a call before set_cloud.  S4P_CLUSTER_ERR_INTERNAL: a bounded loop of the device path ran
 * out, which the bound's derivation excludes; the call returns instead of spinning.  s4p_normals_last_error has the
 * message.
 */
#ifndef S4P_CLUSTER_H_
#define S4P_CLUSTER_H_

#include <stdint.h>

#include "s4p_normals.h"

#ifdef __cplusplus
extern "C" {
#endif

#define S4P_CLUSTER_NOISE 0
#define S4P_CLUSTER_BORDER 1
#define S4P_CLUSTER_CORE 2

#define S4P_CLUSTER_ERR_INTERNAL (-8)

typedef struct s4p_cluster_stats {
  int64_t core;
  int64_t border;
  int64_t noise;
  int64_t clusters;
} s4p_cluster_stats;

int32_t s4p_cluster_dbscan(s4p_normals_ctx* h, float eps, int32_t min_points, int32_t* label, uint8_t* kind, s4p_cluster_stats* stats);
int32_t s4p_cluster_dbscan_device(s4p_normals_ctx* h, float eps, int32_t min_points, int32_t* label, uint8_t* kind,
                                  s4p_cluster_stats* stats);

int32_t s4p_cluster_density(s4p_normals_ctx* h, float radius, int32_t* count);
int32_t s4p_cluster_density_device(s4p_normals_ctx* h, float radius, int32_t* count);

#ifdef __cplusplus
}
#endif
#endif
