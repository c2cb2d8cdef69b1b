// What the facade functions on libsuper4pcs_normals.so share (EstimateNormals, OrientNormals, RemoveOutliers,
// VoxelDownsample, ClusterDBSCAN, SegmentPlane, EstimateNormalsRadius, ComputeFPFH, MatchFeatures): the context that lives for one call, and a cloud's positions as three columns.  algorithms/icp.h takes
// cloud_soa from here too; it never names NormalsHandle, so a program that links -lsuper4pcs_icp alone still links.
#ifndef S4P_FACADE_NORMALS_HANDLE_H_
#define S4P_FACADE_NORMALS_HANDLE_H_

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "s4p_normals.h"
#include "super4pcs/shared4pcs.h"

namespace GlobalRegistration {
namespace detail {

inline void cloud_soa(const std::vector<Point3D>& pts, std::vector<float> (&c)[3]) {
  for (int k = 0; k < 3; ++k) c[k].resize(pts.size());
  for (size_t i = 0; i < pts.size(); ++i) { c[0][i] = pts[i].x(); c[1][i] = pts[i].y(); c[2][i] = pts[i].z(); }
}

// One s4p_normals context; every message starts with "<who> (MI355X): ".
struct NormalsHandle {
  s4p_normals_ctx* h = nullptr;
  const char* who;
  NormalsHandle(const char* w, int device) : who(w) {
    if (s4p_normals_create(device, &h) != S4P_NORMALS_OK) throw std::runtime_error(std::string(who) + " (MI355X): " + s4p_normals_last_error(nullptr));
  }
  NormalsHandle(const NormalsHandle&) = delete;
  NormalsHandle& operator=(const NormalsHandle&) = delete;
  ~NormalsHandle() { s4p_normals_destroy(h); }
  void check(int32_t rc) const {
    if (rc != S4P_NORMALS_OK) throw std::runtime_error(std::string(who) + " (MI355X): " + s4p_normals_last_error(h));
  }
  void set_cloud(const std::vector<Point3D>& cloud) const {
    std::vector<float> c[3];
    cloud_soa(cloud, c);
    check(s4p_normals_set_cloud(h, c[0].data(), c[1].data(), c[2].data(), int64_t(cloud.size())));
  }
};

}  // namespace detail
}  // namespace GlobalRegistration
#endif
