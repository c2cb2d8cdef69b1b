// EstimateNormalsRadius: normals of a whole cloud from every point within a radius, and the surface variation of each
// neighbourhood, on the MI355X, through the C ABI of libsuper4pcs_normals.so (include/s4p_shape.h).  EstimateNormals
// (algorithms/normals.h) takes at most 32 neighbours; on a dense, noisy scan those lie inside the noise and the normals that
// -a, --icp-normal-angle and the gicp and symmetric metrics read are noise too.  A radius of a few noise widths takes hundreds
// of neighbours and gives the surface's normal without thinning the cloud first.
// Link with -lsuper4pcs_normals.  Builds with and without Eigen, like the rest of the facade.
//
//   RadiusNormalOptions ropt;  ropt.radius = 0.02;
//   std::vector<float> curvature;
//   EstimateNormalsRadius(P, ropt, &curvature);      // P[i].normal() set; curvature[i] = l3 / (l1 + l2 + l3), 0 on a plane
#ifndef S4P_FACADE_SHAPE_H_
#define S4P_FACADE_SHAPE_H_

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "s4p_shape.h"
#include "super4pcs/algorithms/normals_handle.h"

namespace GlobalRegistration {

struct RadiusNormalOptions {
  double radius = -1;               // every point within it is a neighbour, the point itself included: finite, > 0
  int min_neighbours = 3;           // a point with fewer neighbours (or fewer than 3) gets no normal; >= 1
  int device = 0;
};

// Sets every point's normal() (Point3D::set_normal) to the unoriented normal of its neighbourhood; (0, 0, 0), "no normal",
// where fewer than max(3, options.min_neighbours) points lie within the radius or they all coincide.  Replaces any normal the
// points had.  curvature, when given, gets one surface variation per point: l3 / (l1 + l2 + l3) of the eigenvalues
// l1 >= l2 >= l3 of the neighbourhood's covariance, in float as written; 0 where the sum is not > 0.  Returns the number of
// points that got no normal.  Throws std::runtime_error when there is no device (no CPU fallback) and std::invalid_argument
// when an option is outside its limits.
inline size_t EstimateNormalsRadius(std::vector<Point3D>& cloud, const RadiusNormalOptions& options, std::vector<float>* curvature = nullptr) {
  if (!(options.radius > 0) || options.radius > 1.8e19 || !(float(options.radius) > 0.f))
    throw std::invalid_argument("EstimateNormalsRadius: radius must be finite and > 0, with a square that fits a float");
  if (options.min_neighbours < 1) throw std::invalid_argument("EstimateNormalsRadius: min_neighbours must be at least 1");
  if (curvature) curvature->clear();
  if (cloud.empty()) return 0;
  const detail::NormalsHandle H("EstimateNormalsRadius", options.device);
  H.set_cloud(cloud);
  const size_t n = cloud.size();
  std::vector<float> nrm(3 * n), eig(curvature ? 3 * n : 0);
  H.check(s4p_shape_estimate(H.h, float(options.radius), options.min_neighbours, nrm.data(), curvature ? eig.data() : nullptr, nullptr));
  size_t none = 0;
  for (size_t i = 0; i < n; ++i) {
    cloud[i].set_normal(Point3D::VectorType(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]));
    if (nrm[3 * i] == 0.f && nrm[3 * i + 1] == 0.f && nrm[3 * i + 2] == 0.f) ++none;
  }
  if (curvature) {
    curvature->resize(n);
    for (size_t i = 0; i < n; ++i) {
      const float total = (eig[3 * i] + eig[3 * i + 1]) + eig[3 * i + 2];
      (*curvature)[i] = total > 0.f ? eig[3 * i + 2] / total : 0.f;
    }
  }
  return none;
}

}  // namespace GlobalRegistration
#endif
