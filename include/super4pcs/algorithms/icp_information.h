// ICPInformation: the 6x6 information matrix of a pairwise pose on the MI355X (include/s4p_icp_info.h): Lambda = sum G^T G,
// G = [-[p]x | I], over the points p of P that the points of Q match under T within options.max_distance.  It is the
// weight of the pair's edge in a pose graph (algorithms/posegraph.h).  Link with -lsuper4pcs_icp.  Builds with and without
// Eigen: the pose and the matrix are plain row-major doubles.
//
// Q is in its own frame and T (16 doubles, row-major) maps Q onto P; after RefineICP, which leaves Q moved, pass the moved Q
// and the identity.  Of ICPOptions it reads max_distance, device, normal_radius and the rejection flags (reciprocal,
// normal_angle_deg, normals_oriented; algorithms/icp.h).  With normal_angle_deg >= 0 the normals of both clouds are needed:
// P's own when every point of P has a nonzero one, else estimated on the device within normal_radius; Q's own (in Q's frame:
// the library rotates them with T) when every point has a nonzero one, else the 16-nearest-neighbour normals of Q.
//
//   double info[36]; int64_t n; double rmse;
//   ICPInformation(P, Q, T, icp, info, &n, &rmse);
#ifndef S4P_FACADE_ICP_INFORMATION_H_
#define S4P_FACADE_ICP_INFORMATION_H_

#include "s4p_icp_info.h"
#include "super4pcs/algorithms/icp.h"

namespace GlobalRegistration {

// info36: row-major, rotation block first; n and rmse may be null.  Throws std::invalid_argument for an empty cloud or a
// null T / info36, std::runtime_error when there is no device (no CPU fallback) or the library refuses an argument.
inline void ICPInformation(const std::vector<Point3D>& P, const std::vector<Point3D>& Q, const double* T16, const ICPOptions& options,
                           double* info36, int64_t* n = nullptr, double* rmse = nullptr) {
  if (P.empty() || Q.empty()) throw std::invalid_argument("ICPInformation: empty cloud");
  if (!T16 || !info36) throw std::invalid_argument("ICPInformation: null transformation or matrix");
  s4p_icp_reject rej;                              // the angle is checked before a device is asked for (RefineICP: after)
  const bool reject = detail::icp_rejection(options, &rej, "ICPInformation");
  const detail::IcpHandle H("ICPInformation", options.device);
  std::vector<float> p[3], q[3];
  detail::cloud_soa(P, p);
  detail::cloud_soa(Q, q);
  detail::icp_set_target(H, p, options.max_distance);
  detail::icp_set_source(H, q);
  if (options.normal_angle_deg >= 0) {
    detail::icp_target_normals(H, P, options);
    detail::icp_source_normals(H, Q, q, options.device, nullptr);      // unrotated: the library rotates them with T16
  }
  if (reject) H.check(s4p_icp_set_rejection(H.h, &rej));
  H.check(s4p_icp_information(H.h, T16, info36, n, rmse));
}

// The facade's matrix type for T (its entries widened to double).
inline void ICPInformation(const std::vector<Point3D>& P, const std::vector<Point3D>& Q, const Match4PCSBase::MatrixType& T,
                           const ICPOptions& options, double* info36, int64_t* n = nullptr, double* rmse = nullptr) {
  double T16[16];
  detail::icp_to16(T, T16);
  ICPInformation(P, Q, T16, options, info36, n, rmse);
}

}  // namespace GlobalRegistration
#endif
