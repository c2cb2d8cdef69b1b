/* s4p_icp_posegraph.h -- pose-graph optimisation with a line process (Choi, Zhou, Koltun, "Robust Reconstruction of Indoor
 * Scenes", CVPR 2015) in libsuper4pcs_icp.so.  Host only, double, no device needed (like s4p_icp_solve).  It reconciles the
 * pairwise poses of N scans into one frame and switches off the pairwise poses that contradict the rest (false loop
 * closures).  DESIGN.md section "Multiway registration".
 *
 * Nodes: X_i, 4x4 double, row-major, world <- scan i (rigid: the inverse is taken as [R^T | -R^T t]).
 * Edges: an edge e carries the scan indices source (s) and target (t), T_e mapping scan s onto scan t (the project's "T maps
 *   Q onto P": t is the target cloud, s the source), a 6x6 information matrix Lambda_e (s4p_icp_info.h; row-major, rotation
 *   block first) and the flag uncertain (0: an odometry edge, always on; 1: a loop closure the line process may switch off).
 * Residual:  E_e = X_t^-1 X_s T_e^-1,  r_e = (omega, v) with omega the rotation vector of E_e's rotation and v E_e's
 *   translation as it stands,  chi2_e = r_e^T Lambda_e r_e.
 * Cost:  F = sum_e l_e chi2_e + mu sum_{uncertain} (sqrt(l_e) - 1)^2,  l_e = 1 on certain edges and, on uncertain ones, the
 *   closed-form minimiser l_e = (mu / (mu + chi2_e))^2, so that over the poses
 *   F = sum_{certain} chi2_e + sum_{uncertain} mu chi2_e / (mu + chi2_e).
 *
 * s4p_icp_posegraph_optimize: Levenberg-Marquardt in double on the dense 6 (N - 1) system (every node but the reference, whose
 * pose is returned bit for bit), Cholesky solve.  A node moves by X_i <- X_i [Rodrigues(omega_i) | v_i].  The gradient is
 * the exact one of F (sum l_e J_e^T Lambda_e r_e); the matrix is sum l_e J_e^T Lambda_e J_e plus, on an uncertain edge with
 * chi2_e < mu / 3 (where it keeps the matrix positive), the second-order term of the robust kernel.  A step is kept when F
 * falls; the damping falls by 10 after a kept step and rises by 10 after a refused one.  A stage ends CONVERGED when a kept
 * step lowers F by at most rel_tol * F or when F is 0, STALLED when no step is kept up to the largest damping (F is at
 * its floor in double, as on a graph whose edges agree exactly), else at max_iterations linear solves.
 *   Stage 1 optimises all edges.  Uncertain edges with l_e < prune_threshold at its end are pruned.  Stage 2 re-optimises
 *   from the stage-1 poses without them (the line process stays on for the other uncertain edges).  If the graph without
 *   the pruned edges no longer connects every node to the reference, stage 2 is skipped: the stage-1 poses are returned and
 *   status is S4P_ICP_POSEGRAPH_STAGE2_SKIPPED.  Without a pruned edge there is no stage 2 (iterations[1] = 0).
 *   line_out (optional, n_edges doubles): each edge's last l_e (1 on certain edges; a pruned edge keeps its stage-1 value).
 *
 * S4P_ICP_ERR_BAD_ARG, poses untouched: null arguments, n_nodes < 1 or > S4P_ICP_POSEGRAPH_MAX_NODES, a reference out of
 * range, an edge index out of range or source == target, a non-finite entry of a pose, T_e or Lambda_e, a Lambda_e that is
 * not symmetric to 1e-9 of its largest entry, uncertain not 0 or 1, line_process_weight <= 0 (or not finite) with an
 * uncertain edge present, a node not connected to the reference, negative max_iterations / prune_threshold / rel_tol.
 */
#ifndef S4P_ICP_POSEGRAPH_H_
#define S4P_ICP_POSEGRAPH_H_

#include "s4p_icp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define S4P_ICP_POSEGRAPH_MAX_NODES 256

#define S4P_ICP_POSEGRAPH_MAX_ITERATIONS 0
#define S4P_ICP_POSEGRAPH_CONVERGED 1
#define S4P_ICP_POSEGRAPH_STAGE2_SKIPPED 2   /* stage 1 ended (either way); pruning would disconnect the graph */
#define S4P_ICP_POSEGRAPH_STALLED 3          /* no step lowered F up to the largest damping: F is at its floor in double */

typedef struct s4p_icp_posegraph_edge {
  int32_t source, target;
  int32_t uncertain, reserved;
  double T[16];        /* row-major, maps scan `source` onto scan `target` */
  double info[36];     /* row-major, rotation block first */
} s4p_icp_posegraph_edge;

typedef struct s4p_icp_posegraph_params {
  int32_t max_iterations;        /* per stage; default 100 */
  int32_t reference;             /* the node that stays; default 0 */
  double line_process_weight;    /* mu > 0, required when any edge is uncertain; default 0 */
  double prune_threshold;        /* default 0.25 */
  double rel_tol;                /* default 1e-12, on the relative decrease of F */
  double reserved[3];
} s4p_icp_posegraph_params;

typedef struct s4p_icp_posegraph_result {
  int32_t iterations[2];         /* linear solves per stage */
  int32_t status;                /* S4P_ICP_POSEGRAPH_*: of the last stage that ran */
  int32_t n_pruned;
  double cost_start, cost_end;   /* F over all edges before stage 1; F over the edges of the last stage at its end */
  double reserved[4];
} s4p_icp_posegraph_result;

void s4p_icp_posegraph_default_params(s4p_icp_posegraph_params* p);

/* F for the poses (n_nodes x 16 doubles); chi2_out (optional): n_edges doubles.  Returns NaN for a bad argument (null,
 * index out of range, mu <= 0 with an uncertain edge). */
double s4p_icp_posegraph_cost(int32_t n_nodes, const double* poses, int32_t n_edges, const s4p_icp_posegraph_edge* edges,
                              double mu, double* chi2_out);

int32_t s4p_icp_posegraph_optimize(int32_t n_nodes, double* poses_inout, int32_t n_edges, const s4p_icp_posegraph_edge* edges,
                                   const s4p_icp_posegraph_params* params, double* line_out, s4p_icp_posegraph_result* result);

#ifdef __cplusplus
}
#endif
#endif
