// EstimateNormals: k-nearest-neighbour normals of a whole cloud on the MI355X, through the C ABI of libsuper4pcs_normals.so
// (include/s4p_normals.h).  The matcher's pair filter (Match4PCSOptions::max_normal_difference, -a) and point-to-plane ICP
// (ICPMetric::PointToPlane) read Point3D::normal(); this fills it for clouds that carry none.
// Link with -lsuper4pcs_normals.  Builds with and without Eigen, like the rest of the facade.
//
//   NormalEstimationOptions nopt;  nopt.k = 16;
//   EstimateNormals(P, nopt);  EstimateNormals(Q, nopt);      // then options.max_normal_difference filters on them
//
// OrientNormals: one consistent sign per surface for normals the points already carry (include/s4p_normals_orient.h): the
// estimates' sign is arbitrary, and the oriented mode of ICP's normal-angle filter (ICPOptions::normals_oriented) needs
// normals that point out of the surface on both clouds.
//
//   NormalOrientationOptions oopt;  oopt.k = 8;               // outward; or oopt.use_viewpoint = true, oopt.viewpoint = ...
//   OrientNormals(P, oopt);  OrientNormals(Q, oopt);
#ifndef S4P_FACADE_NORMALS_H_
#define S4P_FACADE_NORMALS_H_

#include <cstdint>
#include <stdexcept>
#include <vector>

#include "s4p_normals_orient.h"
#include "super4pcs/algorithms/normals_handle.h"

namespace GlobalRegistration {

struct NormalEstimationOptions {
  int k = 16;                       // neighbours, 3..32 (the point itself included)
  double radius = -1;               // > 0: only neighbours within radius ("hybrid"); <= 0: unbounded
  int device = 0;
};

// Sets every point's normal() (Point3D::set_normal) to its estimated, unoriented normal; (0, 0, 0), "no normal", where
// fewer than 3 neighbours qualify or they all coincide.  Replaces any normal the points had.  Throws std::runtime_error
// when there is no device (no CPU fallback) and std::invalid_argument when an option is outside its limits.
inline void EstimateNormals(std::vector<Point3D>& cloud, const NormalEstimationOptions& options) {
  if (cloud.empty()) return;
  if (options.k < S4P_NORMALS_MIN_K || options.k > S4P_NORMALS_MAX_K) throw std::invalid_argument("EstimateNormals: k must be in [3, 32]");
  if (!(options.radius == options.radius) || options.radius > 3.0e38) throw std::invalid_argument("EstimateNormals: radius must be finite");
  const detail::NormalsHandle H("EstimateNormals", options.device);
  H.set_cloud(cloud);
  std::vector<float> out(3 * cloud.size());
  H.check(s4p_normals_estimate(H.h, options.k, float(options.radius), out.data()));
  for (size_t i = 0; i < cloud.size(); ++i) {
    cloud[i].set_normal(Point3D::VectorType(out[3 * i], out[3 * i + 1], out[3 * i + 2]));
  }
}

struct NormalOrientationOptions {
  int k = 8;                        // neighbours of the graph, 1..32 (the point itself excluded)
  double radius = -1;               // > 0: only neighbours within radius; <= 0: unbounded
  bool use_viewpoint = false;       // false: outward, away from the centre of the cloud's bounds
  double viewpoint[3] = {0, 0, 0};  // use_viewpoint: the anchor of every connected component faces this position
  int device = 0;
};

// Negates the normal() of every point that the contract of include/s4p_normals_orient.h flips: signs spread from an anchor
// per connected component of the k-nearest-neighbour graph along the minimum spanning tree of 1 - |n . n'|.  Points without
// a normal, (0, 0, 0), keep it.  A flipped point gets set_normal(-n): Point3D renormalises, which gives the negation of
// set_normal(n); the other points are not touched.  Returns the number of points flipped.  Throws as EstimateNormals does.
inline size_t OrientNormals(std::vector<Point3D>& cloud, const NormalOrientationOptions& options) {
  if (cloud.empty()) return 0;
  if (options.k < S4P_KNN_MIN_K || options.k > S4P_KNN_MAX_K) throw std::invalid_argument("OrientNormals: k must be in [1, 32]");
  if (!(options.radius == options.radius) || options.radius > 3.0e38) throw std::invalid_argument("OrientNormals: radius must be finite");
  float v[3] = {0.f, 0.f, 0.f};
  for (int a = 0; a < 3 && options.use_viewpoint; ++a) {
    if (!(options.viewpoint[a] == options.viewpoint[a]) || options.viewpoint[a] > 3.0e38 || options.viewpoint[a] < -3.0e38)
      throw std::invalid_argument("OrientNormals: the viewpoint must be finite");
    v[a] = float(options.viewpoint[a]);
  }
  const detail::NormalsHandle H("OrientNormals", options.device);
  const size_t n = cloud.size();
  std::vector<float> nrm(3 * n);
  for (size_t i = 0; i < n; ++i) for (int a = 0; a < 3; ++a) nrm[3 * i + a] = cloud[i].normal()(a);
  H.set_cloud(cloud);
  std::vector<uint8_t> flipped(n);
  H.check(s4p_orient_consistent(H.h, options.k, float(options.radius), options.use_viewpoint ? S4P_ORIENT_VIEWPOINT : S4P_ORIENT_OUTWARD,
                                v, nrm.data(), flipped.data(), nullptr, nullptr));
  size_t count = 0;
  for (size_t i = 0; i < n; ++i) {
    if (!flipped[i]) continue;
    cloud[i].set_normal(Point3D::VectorType(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]));
    ++count;
  }
  return count;
}

}  // namespace GlobalRegistration
#endif
