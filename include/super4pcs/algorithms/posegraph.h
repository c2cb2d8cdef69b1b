// OptimizePoseGraph: pose-graph optimisation with a line process (Choi, Zhou, Koltun, CVPR 2015) through the C ABI of
// libsuper4pcs_icp.so (include/s4p_icp_posegraph.h): host only, needs no device.  It reconciles the pairwise poses of N
// scans and switches off the ones that contradict the rest.  Link with -lsuper4pcs_icp.  Plain row-major doubles: the same
// header with and without Eigen.
//
//   PoseGraph g;
//   g.poses = poses0;                                   // world <- scan i
//   g.edges.push_back(edge);                            // T maps scan `source` onto scan `target`, info from ICPInformation
//   PoseGraphOptions o; o.max_distance = 4 * delta;     // sets the line-process weight by the default rule
//   PoseGraphResult r = OptimizePoseGraph(&g, o);       // g.poses optimised; r.line[k]: edge k's line value
#ifndef S4P_FACADE_POSEGRAPH_H_
#define S4P_FACADE_POSEGRAPH_H_

#include <array>
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "s4p_icp_posegraph.h"

namespace GlobalRegistration {

using Pose = std::array<double, 16>;           // 4x4, row-major

inline Pose IdentityPose() { return Pose{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}}; }

struct PoseGraphEdge {
  int source = 0, target = 0;
  bool uncertain = false;                      // a loop closure the line process may switch off
  Pose T = IdentityPose();                     // maps scan `source` onto scan `target`
  std::array<double, 36> info{};               // row-major, rotation block first
};

struct PoseGraph {
  std::vector<Pose> poses;                     // world <- scan i
  std::vector<PoseGraphEdge> edges;
};

struct PoseGraphOptions {
  int max_iterations = 100;                    // linear solves per stage
  int reference = 0;                           // the node whose pose stays, bit for bit
  // mu.  <= 0: preference * max_distance^2 * mean over the uncertain edges of info[3][3] (the matched count): an edge is
  // switched off when its matched points disagree by about max_distance on average; that rule needs max_distance > 0
  double line_process_weight = -1.0;
  double preference = 1.0;
  double max_distance = -1.0;
  double prune_threshold = 0.25;
  double rel_tol = 1e-12;
};

struct PoseGraphResult {
  int iterations[2] = {0, 0};
  int status = 0;                              // S4P_ICP_POSEGRAPH_MAX_ITERATIONS / _CONVERGED / _STAGE2_SKIPPED / _STALLED
  int n_pruned = 0;
  double cost_start = 0.0, cost_end = 0.0;
  double line_process_weight = 0.0;            // the mu that was used
  std::vector<double> line;                    // per edge: its last line value (1 on certain edges)
};

// mu of the default rule (0 without an uncertain edge)
inline double DefaultLineProcessWeight(const PoseGraph& g, double max_distance, double preference = 1.0) {
  double sum = 0.0;
  size_t n = 0;
  for (const PoseGraphEdge& e : g.edges)
    if (e.uncertain) { sum += e.info[21]; ++n; }
  if (n == 0) return 0.0;
  return preference * (max_distance * max_distance) * (sum / double(n));
}

// Optimises g->poses in place.  Throws std::invalid_argument for what include/s4p_icp_posegraph.h refuses (the poses stay
// as they were) and when an edge is uncertain and neither line_process_weight nor max_distance is given.
inline PoseGraphResult OptimizePoseGraph(PoseGraph* g, const PoseGraphOptions& options = PoseGraphOptions()) {
  if (g == nullptr || g->poses.empty()) throw std::invalid_argument("OptimizePoseGraph: no nodes");
  bool any = false;
  for (const PoseGraphEdge& e : g->edges) any = any || e.uncertain;
  double mu = options.line_process_weight;
  if (!(mu > 0.0)) {
    if (any && !(options.max_distance > 0.0))
      throw std::invalid_argument("OptimizePoseGraph: line_process_weight or max_distance is required with an uncertain edge");
    mu = any ? DefaultLineProcessWeight(*g, options.max_distance, options.preference) : 0.0;
  }
  std::vector<s4p_icp_posegraph_edge> edges(g->edges.size() ? g->edges.size() : 1);
  for (size_t k = 0; k < g->edges.size(); ++k) {
    const PoseGraphEdge& e = g->edges[k];
    edges[k].source = e.source; edges[k].target = e.target; edges[k].uncertain = e.uncertain ? 1 : 0; edges[k].reserved = 0;
    for (int a = 0; a < 16; ++a) edges[k].T[a] = e.T[size_t(a)];
    for (int a = 0; a < 36; ++a) edges[k].info[a] = e.info[size_t(a)];
  }
  s4p_icp_posegraph_params p;
  s4p_icp_posegraph_default_params(&p);
  p.max_iterations = options.max_iterations;
  p.reference = options.reference;
  p.line_process_weight = mu;
  p.prune_threshold = options.prune_threshold;
  p.rel_tol = options.rel_tol;
  std::vector<double> poses(16 * g->poses.size());
  for (size_t i = 0; i < g->poses.size(); ++i) for (size_t a = 0; a < 16; ++a) poses[16 * i + a] = g->poses[i][a];
  PoseGraphResult out;
  out.line.assign(g->edges.size() ? g->edges.size() : 1, 1.0);
  s4p_icp_posegraph_result r;
  const int32_t rc = s4p_icp_posegraph_optimize(int32_t(g->poses.size()), poses.data(), int32_t(g->edges.size()), edges.data(), &p,
                                                out.line.data(), &r);
  if (rc != S4P_ICP_OK) throw std::invalid_argument("OptimizePoseGraph: bad argument (include/s4p_icp_posegraph.h lists them)");
  out.line.resize(g->edges.size());
  for (size_t i = 0; i < g->poses.size(); ++i) for (size_t a = 0; a < 16; ++a) g->poses[i][a] = poses[16 * i + a];
  out.iterations[0] = r.iterations[0]; out.iterations[1] = r.iterations[1];
  out.status = r.status; out.n_pruned = r.n_pruned; out.cost_start = r.cost_start; out.cost_end = r.cost_end;
  out.line_process_weight = mu;
  return out;
}

}  // namespace GlobalRegistration
#endif
