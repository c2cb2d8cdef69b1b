/* s4p_icp_batch.h -- batched multi-start ICP in libsuper4pcs_icp.so: B start poses of one source against one target, refined
 * side by side, and the rule that ranks the results.  DESIGN.md section "Batched multi-start ICP".
 *
 * A batch shares the context's target, its grid, the source and (plane) the target normals; only the transform differs from
 * pose to pose.  One launch covers every pose that is still iterating (grid: source workgroups x active poses), so B
 * refinements of a source too small to fill the device alone run in the time of few.
 *
 * Sums.  Row b of s4p_icp_sums_batch holds the bits of s4p_icp_sums (S4P_ICP_METRIC_POINT, S4P_ICP_NSUMS = 17 doubles per
 * row) or s4p_icp_plane_sums (S4P_ICP_METRIC_PLANE, S4P_ICP_PLANE_NSUMS = 31 per row) called with transform b: the same
 * workgroups in x, the same lane for every source point, the same expressions per lane, the same reduction order.
 *
 * Refine.  Pose b runs the state machine of s4p_icp_refine / s4p_icp_refine_plane, comparison for comparison: too few
 * correspondences, the solve (for plane: S4P_ICP_DEGENERATE), the rel_tol stop (from the second iteration on), the
 * max_iterations stop, the final pass.  A pose that stops leaves the launches; the final pass is one launch over all B.
 *  - params->icp.order_source = 0: T16_inout[b] and every byte of results[b] equal what the single call returns for start b
 *    with order_source = 0.
 *  - params->icp.order_source = 1 (default): the source is ordered once, by the cell of its image under start 0.  Pose 0
 *    equals the single call with order_source = 1 bit for bit; the other poses differ from their order_source = 0 results
 *    only through the order in which the double sums are added.
 *
 * Ranking (s4p_icp_rank_batch, and `order` of s4p_icp_refine_batch): n_corr descending, then rmse ascending, then the index
 * ascending; poses with n_corr = 0 come last, by index.  order[0] is the best pose.
 *
 * Refused, each with the code the single calls use: B outside 1..S4P_ICP_BATCH_MAX, a null pointer, a metric other than
 * point or plane (S4P_ICP_ERR_BAD_ARG); target or source missing, plane without target normals, correspondence rejection
 * switched on (S4P_ICP_ERR_STATE: the batch has no split pass).
 *
 * Out of scope: robust losses, generalized and coloured ICP have no batch form; refine those start by start.
 */
#ifndef S4P_ICP_BATCH_H_
#define S4P_ICP_BATCH_H_

#include "s4p_icp.h"
#include "s4p_icp_plane.h"
#include "s4p_icp_robust.h"      /* S4P_ICP_METRIC_POINT, S4P_ICP_METRIC_PLANE */

#ifdef __cplusplus
extern "C" {
#endif

#define S4P_ICP_BATCH_MAX 64

typedef struct s4p_icp_batch_params {
  s4p_icp_params icp;     /* as s4p_icp_refine; order_source: see above */
  int32_t metric;         /* S4P_ICP_METRIC_POINT | S4P_ICP_METRIC_PLANE */
  int32_t reserved;
} s4p_icp_batch_params;

/* stage call, centred frame: B float transforms (B * 16, row-major, last rows ignored) -> B rows of sums (17 per row for
 * point, 31 for plane), over the source as uploaded */
int32_t s4p_icp_sums_batch(s4p_icp_ctx* h, int32_t metric, int32_t B, const float* T16_centred, double* sums);

/* B starts in, B refined transforms out (caller frame, double, B * 16); results[B]; order[B] may be null.  params may be
 * null (defaults). */
int32_t s4p_icp_refine_batch(s4p_icp_ctx* h, const s4p_icp_batch_params* params, int32_t B, double* T16_inout,
                             s4p_icp_result* results, int32_t* order);

/* Host only, needs no device (like s4p_icp_solve): the ranking rule above. */
int32_t s4p_icp_rank_batch(const s4p_icp_result* results, int32_t B, int32_t* order);

#ifdef __cplusplus
}
#endif
#endif
