// RegisterMultiway: N scans into one frame on the MI355X.  Pairwise ICP refinement and its information matrix per pair of
// scans (RefineICP's and ICPInformation's calls of libsuper4pcs_icp.so, on one context per run), then OptimizePoseGraph
// (algorithms/posegraph.h).  It makes the calls of super4pcs_amd.multiway.register_multiway in its order, so that both
// return the same poses.  Link with -lsuper4pcs_icp.  Builds with and without Eigen.
//
// For each target i: one s4p_icp_set_target, plus normals estimated on the device within icp.normal_radius (<= 0:
// max_distance) when the metric needs them.  For each source j > i of the pairs (default: all): s4p_icp_set_source, the
// refine of icp.metric from poses[i]^-1 poses[j], s4p_icp_information at the refined pose.  j = i + 1 gives a certain edge
// (fewer than icp.min_correspondences matches: std::runtime_error); any other pair an uncertain edge when its fitness >=
// min_fitness, and no edge below.  The clouds' own normals are not read: target normals are estimated, and the generalized
// and symmetric metrics take the 16-nearest-neighbour normals of each source.  ICPMetric::Colored and the robust losses are
// refused (std::invalid_argument): a list of scans carries no colours, and the pairwise poses feed a robust graph already.
// The rejection flags of icp hold for every refine and information pass.
//
//   std::vector<Pose> poses = poses0;                   // world <- scan i, from the caller's pairwise runs
//   MultiwayOptions o; o.icp.max_distance = 4 * delta; o.icp.metric = ICPMetric::PointToPlane;
//   MultiwayReport rep = RegisterMultiway(scans, &poses, o);
#ifndef S4P_FACADE_MULTIWAY_H_
#define S4P_FACADE_MULTIWAY_H_

#include <algorithm>
#include <utility>

#include "super4pcs/algorithms/icp_information.h"
#include "super4pcs/algorithms/posegraph.h"

namespace GlobalRegistration {

struct MultiwayOptions {
  ICPOptions icp;                              // max_distance is required; metric PointToPlane is the usual choice
  double min_fitness = 0.3;
  std::vector<std::pair<int, int>> pairs;      // (i, j), i < j; empty: all pairs.  Every (i, i + 1) must be there
  PoseGraphOptions graph;                      // max_distance <= 0: icp.max_distance
};

struct MultiwayEdgeReport {
  int source = 0, target = 0;
  bool uncertain = false;
  int64_t n = 0;
  double rmse = 0.0, fitness = 0.0, l = 1.0;
};

struct MultiwayReport {
  PoseGraph graph;                             // the optimised poses and the edges that were built
  std::vector<MultiwayEdgeReport> edges;
  PoseGraphResult optimize;
};

namespace detail {

// [R^T | -R^T t], term by term
inline Pose rigid_inverse(const Pose& X) {
  Pose o = IdentityPose();
  for (size_t r = 0; r < 3; ++r) {
    for (size_t c = 0; c < 3; ++c) o[4 * r + c] = X[4 * c + r];
    o[4 * r + 3] = -((X[r] * X[3] + X[4 + r] * X[7]) + X[8 + r] * X[11]);
  }
  return o;
}

// A B in the facade's one order (detail::icp_product16)
inline Pose pose_product(const Pose& A, const Pose& B) {
  Pose o;
  icp_product16(A.data(), B.data(), o.data());
  return o;
}

}  // namespace detail

// poses: in, the start (world <- scan i; null entries are not allowed, pass identities for "unknown"); out, the optimised
// poses.  Throws std::invalid_argument for fewer than two scans, a poses vector of another length, a bad pair, a metric or
// loss it refuses; std::runtime_error when there is no device or a certain edge has too few correspondences.
inline MultiwayReport RegisterMultiway(const std::vector<std::vector<Point3D>>& scans, std::vector<Pose>* poses,
                                       const MultiwayOptions& options) {
  const int N = int(scans.size());
  if (N < 2) throw std::invalid_argument("RegisterMultiway: at least two scans");
  if (N > S4P_ICP_POSEGRAPH_MAX_NODES) throw std::invalid_argument("RegisterMultiway: more scans than S4P_ICP_POSEGRAPH_MAX_NODES");
  if (poses == nullptr || int(poses->size()) != N) throw std::invalid_argument("RegisterMultiway: one pose per scan");
  for (const auto& s : scans) if (s.empty()) throw std::invalid_argument("RegisterMultiway: empty cloud");
  const ICPOptions& icp = options.icp;
  if (icp.metric == ICPMetric::Colored) throw std::invalid_argument("RegisterMultiway: the coloured metric is not supported");
  if (icp.loss != ICPLoss::None) throw std::invalid_argument("RegisterMultiway: robust losses are not supported");
  std::vector<std::pair<int, int>> pairs = options.pairs;
  if (pairs.empty())
    for (int i = 0; i < N; ++i) for (int j = i + 1; j < N; ++j) pairs.emplace_back(i, j);
  for (const auto& pr : pairs)
    if (!(0 <= pr.first && pr.first < pr.second && pr.second < N)) throw std::invalid_argument("RegisterMultiway: pairs are (i, j) with 0 <= i < j < N");
  for (int i = 0; i + 1 < N; ++i)
    if (std::find(pairs.begin(), pairs.end(), std::make_pair(i, i + 1)) == pairs.end())
      throw std::invalid_argument("RegisterMultiway: pairs must hold every (i, i + 1)");
  s4p_icp_reject rej;                              // the angle is checked before a device is asked for (RefineICP: after)
  const bool reject = detail::icp_rejection(icp, &rej, "RegisterMultiway");
  const bool pair_normals = icp.metric == ICPMetric::Generalized || icp.metric == ICPMetric::Symmetric || icp.normal_angle_deg >= 0;
  const bool target_normals = pair_normals || icp.metric == ICPMetric::PointToPlane;
  const int min_corr = icp.min_correspondences > 1 ? icp.min_correspondences : 1;
  MultiwayReport rep;
  rep.graph.poses = *poses;
  const detail::IcpHandle H("RegisterMultiway", icp.device);
  if (reject) H.check(s4p_icp_set_rejection(H.h, &rej));
  std::vector<std::vector<float>> src_normals(static_cast<size_t>(N));         // 3 n floats per source that needs them, filled once
  for (int i = 0; i + 1 < N; ++i) {
    std::vector<int> sources;
    for (const auto& pr : pairs) if (pr.first == i) sources.push_back(pr.second);
    if (sources.empty()) continue;
    std::sort(sources.begin(), sources.end());
    std::vector<float> p[3];
    detail::cloud_soa(scans[size_t(i)], p);
    detail::icp_set_target(H, p, icp.max_distance);
    // a scan's own normals are never read: always estimated here, and always the cached knn estimate for a source
    if (target_normals) H.check(s4p_icp_estimate_normals(H.h, float(detail::icp_normal_radius(icp)), 6));
    const Pose Xi_inv = detail::rigid_inverse((*poses)[size_t(i)]);
    for (int j : sources) {
      std::vector<float> q[3];
      detail::cloud_soa(scans[size_t(j)], q);
      detail::icp_set_source(H, q);
      if (pair_normals) {
        std::vector<float>& est = src_normals[size_t(j)];
        if (est.empty()) detail::icp_knn_normals(q, 16, icp.device, &est);
        detail::icp_set_knn_normals(H, est);
      }
      Pose T = detail::pose_product(Xi_inv, (*poses)[size_t(j)]);
      const s4p_icp_result r = detail::icp_refine(H, icp, T.data());
      PoseGraphEdge e;
      int64_t n = 0;
      double rmse = 0.0;
      H.check(s4p_icp_information(H.h, T.data(), e.info.data(), &n, &rmse));
      const bool certain = j == i + 1;
      if (certain && n < int64_t(min_corr))
        throw std::runtime_error("RegisterMultiway: scans " + std::to_string(i) + " and " + std::to_string(j) + " share " +
                                 std::to_string(n) + " correspondences (fewer than " + std::to_string(min_corr) + ")");
      if (!certain && !(r.fitness >= options.min_fitness && n >= 1)) continue;
      e.source = j; e.target = i; e.uncertain = !certain; e.T = T;
      rep.graph.edges.push_back(e);
      MultiwayEdgeReport er;
      er.source = j; er.target = i; er.uncertain = !certain; er.n = n; er.rmse = rmse; er.fitness = r.fitness;
      rep.edges.push_back(er);
    }
  }
  PoseGraphOptions g = options.graph;
  if (!(g.max_distance > 0.0)) g.max_distance = icp.max_distance;
  rep.optimize = OptimizePoseGraph(&rep.graph, g);
  for (size_t k = 0; k < rep.edges.size(); ++k) rep.edges[k].l = rep.optimize.line[k];
  *poses = rep.graph.poses;
  return rep;
}

}  // namespace GlobalRegistration
#endif
