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

namespace detail {

struct IcpHandle {
  s4p_icp_ctx* h = nullptr;
  const char* who;
  explicit IcpHandle(const char* w, int device) : who(w) {
    if (s4p_icp_create(device, &h) != S4P_ICP_OK) throw std::runtime_error(std::string(who) + " (MI355X): " + s4p_icp_last_error(nullptr));
  }
  IcpHandle(const IcpHandle&) = delete;
  IcpHandle& operator=(const IcpHandle&) = delete;
  ~IcpHandle() { s4p_icp_destroy(h); }
  void check(int32_t rc) const {
    if (rc != S4P_ICP_OK) throw std::runtime_error(std::string(who) + " (MI355X): " + s4p_icp_last_error(h));
  }
};

inline void icp_soa(const std::vector<Point3D>& pts, std::vector<float> (&c)[3]) {
  for (int k = 0; k < 3; ++k) c[k].resize(pts.size());
  for (size_t i = 0; i < pts.size(); ++i) { c[0][i] = pts[i].x(); c[1][i] = pts[i].y(); c[2][i] = pts[i].z(); }
}

// the cloud's own normals as SoA when every point has a nonzero one
inline bool icp_own_normals(const std::vector<Point3D>& pts, std::vector<float> (&n)[3]) {
  for (const Point3D& pt : pts) {
    const auto& nv = pt.normal();
    if (!(nv(0) != 0 || nv(1) != 0 || nv(2) != 0)) return false;
  }
  for (int k = 0; k < 3; ++k) n[k].resize(pts.size());
  for (size_t i = 0; i < pts.size(); ++i) for (int k = 0; k < 3; ++k) n[k][i] = float(pts[i].normal()(k));
  return true;
}

// RefineICP's translation of the rejection flags
inline bool icp_rejection(const ICPOptions& o, s4p_icp_reject* rej, const char* who) {
  const bool by_normals = o.normal_angle_deg >= 0;
  if (by_normals && !(o.normal_angle_deg <= (o.normals_oriented ? 180.0 : 90.0)))
    throw std::invalid_argument(std::string(who) + ": normal_angle_deg must be at most 90 (oriented normals: 180)");
  s4p_icp_reject_defaults(rej);
  rej->reciprocal = o.reciprocal ? 1 : 0;
  if (by_normals) {
    rej->normal_mode = o.normals_oriented ? S4P_ICP_REJECT_NORMALS_ORIENTED : S4P_ICP_REJECT_NORMALS_UNORIENTED;
    const double c = std::cos(o.normal_angle_deg * (3.14159265358979323846 / 180.0));
    const double lo = o.normals_oriented ? -1.0 : 0.0;
    rej->normal_cos = c < lo ? lo : (c > 1.0 ? 1.0 : c);
  }
  return o.reciprocal || by_normals;
}

}  // namespace detail

// info36: row-major, rotation block first; n and rmse may be null.  Throws std::invalid_argument for an empty cloud or a
// null T / info36, std::runtime_error when there is no device (no CPU fallback) or the library refuses an argument.
inline void ICPInformation(const std::vector<Point3D>& P, const std::vector<Point3D>& Q, const double* T16, const ICPOptions& options,
                           double* info36, int64_t* n = nullptr, double* rmse = nullptr) {
  if (P.empty() || Q.empty()) throw std::invalid_argument("ICPInformation: empty cloud");
  if (!T16 || !info36) throw std::invalid_argument("ICPInformation: null transformation or matrix");
  s4p_icp_reject rej;
  const bool reject = detail::icp_rejection(options, &rej, "ICPInformation");
  detail::IcpHandle H("ICPInformation", options.device);
  std::vector<float> p[3], q[3];
  detail::icp_soa(P, p);
  detail::icp_soa(Q, q);
  H.check(s4p_icp_set_target(H.h, p[0].data(), p[1].data(), p[2].data(), int64_t(P.size()), float(options.max_distance)));
  H.check(s4p_icp_set_source(H.h, q[0].data(), q[1].data(), q[2].data(), int64_t(Q.size())));
  if (options.normal_angle_deg >= 0) {
    std::vector<float> nv[3];
    if (detail::icp_own_normals(P, nv)) {
      H.check(s4p_icp_set_target_normals(H.h, nv[0].data(), nv[1].data(), nv[2].data(), int64_t(P.size())));
    } else {
      const double r = options.normal_radius > 0 ? options.normal_radius : options.max_distance;
      H.check(s4p_icp_estimate_normals(H.h, float(r), 6));
    }
    if (!detail::icp_own_normals(Q, nv)) {
      std::vector<float> est;
      detail::icp_knn_normals(q, 16, options.device, &est);
      for (int k = 0; k < 3; ++k) nv[k].resize(Q.size());
      for (size_t i = 0; i < Q.size(); ++i) for (int k = 0; k < 3; ++k) nv[k][i] = est[3 * i + k];
    }
    H.check(s4p_icp_set_source_normals(H.h, nv[0].data(), nv[1].data(), nv[2].data(), int64_t(Q.size())));
  }
  if (reject) H.check(s4p_icp_set_rejection(H.h, &rej));
  H.check(s4p_icp_information(H.h, T16, info36, n, rmse));
}

// The facade's matrix type for T (its entries widened to double).
inline void ICPInformation(const std::vector<Point3D>& P, const std::vector<Point3D>& Q, const Match4PCSBase::MatrixType& T,
                           const ICPOptions& options, double* info36, int64_t* n = nullptr, double* rmse = nullptr) {
  double T16[16];
  for (int a = 0; a < 4; ++a) for (int b = 0; b < 4; ++b) T16[4 * a + b] = double(T(a, b));
  ICPInformation(P, Q, T16, options, info36, n, rmse);
}

}  // namespace GlobalRegistration
#endif
