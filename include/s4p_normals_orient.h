/* s4p_normals_orient.h -- consistent orientation of normals in libsuper4pcs_normals.so, on an MI355X (gfx950).  The functions
 * work on an s4p_normals_ctx (include/s4p_normals.h) after s4p_normals_set_cloud[_device]: the same cloud X, the same grid,
 * the same search as include/s4p_knn.h.  No CPU fallback.  The entry points carry the prefix s4p_orient_: the prefix
 * s4p_normals_ stays the closed set that s4p_normals.h declares.
 *
 * Contract ("Normal orientation"), written so that the result is unique: the minimum spanning forest
 * under a strict total order is unique, so no order of the device's atomics can change a bit of the output, and a
 * restatement on the CPU (Kruskal, then a walk of the tree) gives the same signs.
 *  - Inputs: the context's cloud X (n points) and normals float[3 n], interleaved as s4p_normals_estimate writes them.  Point
 *    i is a vertex when its three components are finite and not all zero.  A point that is no vertex -- the normal (0, 0, 0),
 *    or one with a non-finite component, which is treated as a zero normal -- keeps its bits, is never flipped and gets
 *    component = -1.
 *  - Lists: N(i) = the list of s4p_knn_search with exclude_self = 1: the k nearest other points in (d2, index) order,
 *    1 <= k <= 32, bounded by radius as there (<= 0: unbounded).
 *  - Edges: the undirected edge {i, j} exists when j is in N(i) or i is in N(j), and both are vertices.  With
 *      d = nx*nx' + (ny*ny' + nz*nz')   in float, no contraction (the same bits for (i, j) and (j, i)),
 *      t = 1 - |d| in float,  w = t if t > 0, else 0   (so a NaN d gives w = 0),
 *      f = (d < 0), the flip bit,
 *    edges are ordered strictly by (the bits of w, min(i, j), max(i, j)).
 *  - Tree: the minimum spanning forest of that graph under that order; one tree per connected component.
 *  - Anchor of a component:
 *      S4P_ORIENT_VIEWPOINT, viewpoint v: the vertex with the smallest (d2(v, x), index), d2 as in s4p_knn.h with q = v;
 *        its direction is g = fl(v - x).
 *      S4P_ORIENT_OUTWARD: c = 0.5f * (lo + hi) per axis in float, lo / hi the cloud's bounds; the vertex with the largest
 *        d2(c, x), ties to the smaller index; its direction is g = fl(x - c).
 *    The anchor is flipped exactly when nx*gx + (ny*gy + nz*gz) < 0 in float.  (The vertex nearest to the viewpoint faces it,
 *    the vertex farthest from the centre faces away from it: exact for the extreme points of convex shapes, a heuristic
 *    otherwise.)
 *  - Result: vertex i is flipped exactly when (flip of its anchor) XOR (the XOR of f along the tree path from the anchor to
 *    i) is 1.  A flip negates the three floats: every output bit pattern is the input's or its negation.
 *      normals    rewritten in place
 *      flipped    uint8[n], 1 = negated (may be null)
 *      component  int32[n], the index of the component's anchor, -1 for a point that is no vertex (may be null)
 *      stats      counts, the Boruvka rounds that merged components and the most pointer-jump launches one round took
 *                 (may be null; host memory in both forms)
 *  - s4p_orient_towards: no graph, no k.  Vertex i is flipped exactly when nx*gx + (ny*gy + nz*gz) < 0 in float with
 *    g = fl(v - x_i); a point that is no vertex keeps its bits.
 *  - Host forms read and write host memory, _device forms memory of the context's device (viewpoint and stats are host
 *    memory in both).  Two calls give the same bits; host and device forms give the same bits.
 *
 * Refused with S4P_NORMALS_ERR_BAD_ARG: k outside 1..32, a non-finite radius, a mode that is neither of the two, a null or
 * non-finite viewpoint (towards, and consistent in viewpoint mode), null normals; with S4P_NORMALS_ERR_STATE: a call before
 * set_cloud.  S4P_ORIENT_ERR_INTERNAL: a bounded loop of the device path (32 rounds, 32 pointer-jump launches per round) ran
 * out, which the contract's order excludes; the call returns instead of spinning.  s4p_normals_last_error has the message.
 */
#ifndef S4P_NORMALS_ORIENT_H_
#define S4P_NORMALS_ORIENT_H_

#include <stdint.h>

#include "s4p_knn.h"
#include "s4p_normals.h"

#ifdef __cplusplus
extern "C" {
#endif

#define S4P_ORIENT_OUTWARD 0
#define S4P_ORIENT_VIEWPOINT 1

#define S4P_ORIENT_ERR_INTERNAL (-8)

#define S4P_ORIENT_MAX_ROUNDS 32
#define S4P_ORIENT_MAX_JUMPS 32

typedef struct s4p_orient_stats {
  int64_t vertices;                /* points with a usable normal */
  int64_t components;              /* trees of the forest = anchors */
  int64_t flipped;                 /* normals negated */
  int32_t rounds;                  /* Boruvka rounds that merged at least two components */
  int32_t max_jumps;               /* the most pointer-jump launches in one round */
} s4p_orient_stats;

int32_t s4p_orient_consistent(s4p_normals_ctx* h, int32_t k, float radius, int32_t mode, const float* viewpoint, float* normals,
                              uint8_t* flipped, int32_t* component, s4p_orient_stats* stats);
int32_t s4p_orient_consistent_device(s4p_normals_ctx* h, int32_t k, float radius, int32_t mode, const float* viewpoint,
                                     float* normals, uint8_t* flipped, int32_t* component, s4p_orient_stats* stats);

int32_t s4p_orient_towards(s4p_normals_ctx* h, float* normals, const float* viewpoint, uint8_t* flipped);
int32_t s4p_orient_towards_device(s4p_normals_ctx* h, float* normals, const float* viewpoint, uint8_t* flipped);

#ifdef __cplusplus
}
#endif
#endif
