// SegmentPlane / RemovePlanes: RANSAC plane segmentation of a whole cloud on the MI355X, through the C ABI of
// libsuper4pcs_normals.so (include/s4p_plane.h).  On a scanned scene the ground carries a large share of the points: density
// clustering joins the scene through it, and a registration can slide along it.  RemovePlanes takes the dominant planes out
// so that the structure above them is what the next step sees.
// Link with -lsuper4pcs_normals.  Builds with and without Eigen, like the rest of the facade.
//
//   PlaneOptions popt;  popt.distance = 0.15;
//   std::vector<uint8_t> inlier;
//   const PlaneModel g = SegmentPlane(P, popt, inlier);           // g.normal . x + g.d = 0; inlier[i] = 1 on the plane
//   RemovePlanes(P, popt);                                        // P = the cloud without its dominant plane
#ifndef S4P_FACADE_PLANE_H_
#define S4P_FACADE_PLANE_H_

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "s4p_plane.h"
#include "super4pcs/algorithms/normals_handle.h"

namespace GlobalRegistration {

struct PlaneOptions {
  double distance = -1;             // a point within this distance of the plane is an inlier: finite, >= 0
  int trials = 1024;                // RANSAC candidates; 1 .. 2^20
  uint64_t seed = 0;                // of the sample stream; plane p of RemovePlanes uses seed + p
  int refine = 1;                   // least-squares refits on the inliers; 0 .. 16
  int count = 1;                    // RemovePlanes: how many planes go; >= 1
  int min_inliers = 3;              // RemovePlanes: stop at the first plane with fewer inliers; >= 1
  int device = 0;
};

struct PlaneModel {
  float normal[3] = {0.f, 0.f, 0.f};      // unit, the component of largest magnitude positive; zero when no plane was found
  float d = 0.f;                          // normal . x + d = 0
  size_t inliers = 0;
  bool found = false;
};

namespace detail {
inline void plane_check_options(const char* who, const PlaneOptions& o) {
  if (!(o.distance >= 0) || !(o.distance <= 3.4028234e38))
    throw std::invalid_argument(std::string(who) + ": distance must be finite and >= 0");
  if (o.trials < 1 || o.trials > S4P_PLANE_MAX_TRIALS) throw std::invalid_argument(std::string(who) + ": trials must be in [1, 2^20]");
  if (o.refine < 0 || o.refine > S4P_PLANE_MAX_REFINE) throw std::invalid_argument(std::string(who) + ": refine must be in [0, 16]");
  if (o.count < 1) throw std::invalid_argument(std::string(who) + ": count must be at least 1");
  if (o.min_inliers < 1) throw std::invalid_argument(std::string(who) + ": min_inliers must be at least 1");
}

// one call on a context that holds the cloud: plane p with the seed seed + p, without the points of exclude (null: none)
inline PlaneModel plane_segment(const NormalsHandle& H, const PlaneOptions& o, int p, const uint8_t* exclude, uint8_t* inlier) {
  s4p_plane_options so{};
  so.distance = float(o.distance);
  so.trials = o.trials;
  so.seed = o.seed + uint64_t(p);
  so.refine = o.refine;
  s4p_plane_result r{};
  H.check(s4p_plane_segment(H.h, &so, exclude, &r, inlier));
  PlaneModel m;
  m.found = r.trial >= 0;
  for (int a = 0; a < 3; ++a) m.normal[a] = r.normal[a];
  m.d = r.d;
  m.inliers = size_t(r.inliers);
  return m;
}
}  // namespace detail

// The dominant plane of the cloud and its inlier mask (one byte per point, 1 = within options.distance of the plane; the
// mask is the library's, defined in its centred frame).  found is false, and the mask all zero, when no three sampled points
// spanned a plane.  Throws std::runtime_error when there is no device (no CPU fallback) and std::invalid_argument when an
// option is outside its limits.
inline PlaneModel SegmentPlane(const std::vector<Point3D>& cloud, const PlaneOptions& options, std::vector<uint8_t>& inlier) {
  detail::plane_check_options("SegmentPlane", options);
  inlier.clear();
  if (cloud.empty()) return PlaneModel();
  const detail::NormalsHandle H("SegmentPlane", options.device);
  H.set_cloud(cloud);
  inlier.resize(cloud.size());
  return detail::plane_segment(H, options, 0, nullptr, inlier.data());
}

// Peels the options.count dominant planes off the cloud on one upload (plane p is found on the points the planes before it
// left, and the peeling stops at the first plane with fewer than options.min_inliers inliers) and erases their points in
// place, keeping the order of the remaining points and their normals and colours; returns how many it removed.  kept, when
// given, gets one byte per point of the input cloud (1 = kept); planes, when given, the planes that were removed.
inline size_t RemovePlanes(std::vector<Point3D>& cloud, const PlaneOptions& options, std::vector<uint8_t>* kept = nullptr,
                           std::vector<PlaneModel>* planes = nullptr) {
  detail::plane_check_options("RemovePlanes", options);
  if (kept) kept->clear();
  if (planes) planes->clear();
  if (cloud.empty()) return 0;
  std::vector<uint8_t> gone(cloud.size(), 0), inlier(cloud.size());
  {
    const detail::NormalsHandle H("RemovePlanes", options.device);
    H.set_cloud(cloud);
    for (int p = 0; p < options.count; ++p) {
      const PlaneModel m = detail::plane_segment(H, options, p, p ? gone.data() : nullptr, inlier.data());
      if (!m.found || m.inliers < size_t(options.min_inliers)) break;
      for (size_t i = 0; i < cloud.size(); ++i) gone[i] |= inlier[i];
      if (planes) planes->push_back(m);
    }
  }
  size_t w = 0;
  for (size_t i = 0; i < cloud.size(); ++i) {
    if (gone[i]) continue;
    if (w != i) cloud[w] = std::move(cloud[i]);
    ++w;
  }
  const size_t removed = cloud.size() - w;
  cloud.resize(w);
  if (kept) {
    for (uint8_t& g : gone) g = g ? 0 : 1;
    *kept = std::move(gone);
  }
  return removed;
}

}  // namespace GlobalRegistration
#endif
