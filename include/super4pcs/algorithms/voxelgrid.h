// VoxelDownsample: voxel-grid downsampling of a whole cloud on the MI355X, through the C ABI of libsuper4pcs_normals.so
// (include/s4p_voxel.h).  Scans of millions of points are thinned to one point per occupied voxel -- the mean of its members --
// before normals, outlier removal or ICP; RefineICPMultiScale (algorithms/icp_multiscale.h) builds its coarse levels with it.
// Link with -lsuper4pcs_normals.  Builds with and without Eigen, like the rest of the facade.
//
//   VoxelGridOptions vopt;  vopt.voxel_size = 0.01;
//   VoxelDownsample(P, vopt);  VoxelDownsample(Q, vopt);      // the lattice is anchored at the origin: both clouds share it
#ifndef S4P_FACADE_VOXELGRID_H_
#define S4P_FACADE_VOXELGRID_H_

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "s4p_voxel.h"
#include "super4pcs/algorithms/normals_handle.h"

namespace GlobalRegistration {

struct VoxelGridOptions {
  double voxel_size = -1;           // required: finite and > 0
  int device = 0;
};

// Replaces the cloud by the means of its occupied voxels, in ascending (iz, iy, ix) of the voxel floor(x / voxel_size), and
// returns how many points remain.  Points with a non-finite coordinate are dropped.  Normals are carried only when every
// point has a nonzero one: they are averaged and passed through Point3D::set_normal (a zero mean stays zero).  rgb is
// carried, averaged, when every point has one (rgb()[0] >= 0).  voxel_of, when given, gets the output row of every input
// point, -1 for a dropped one.  Throws std::runtime_error when there is no device (no CPU fallback) and
// std::invalid_argument when an option is outside its limits.
inline size_t VoxelDownsample(std::vector<Point3D>& cloud, const VoxelGridOptions& options, std::vector<int>* voxel_of = nullptr) {
  if (!(options.voxel_size > 0) || options.voxel_size > 3.0e38 || !(float(options.voxel_size) > 0.f))
    throw std::invalid_argument("VoxelDownsample: voxel_size must be finite and > 0");
  if (voxel_of) voxel_of->clear();
  if (cloud.empty()) return 0;
  const detail::NormalsHandle H("VoxelDownsample", options.device);
  const size_t n = cloud.size();
  bool normals = true, colours = true;
  for (const Point3D& pt : cloud) {
    const auto& nv = pt.normal();
    if (!(nv(0) != 0 || nv(1) != 0 || nv(2) != 0)) normals = false;
    if (!(pt.rgb()(0) >= 0)) colours = false;
  }
  const int nattr = (normals ? 3 : 0) + (colours ? 3 : 0);
  const int rgb_at = normals ? 3 : 0;
  std::vector<float> c[3], attr(n * size_t(nattr));
  detail::cloud_soa(cloud, c);
  for (size_t i = 0; i < n; ++i) {
    if (normals) for (int k = 0; k < 3; ++k) attr[i * nattr + k] = float(cloud[i].normal()(k));
    if (colours) for (int k = 0; k < 3; ++k) attr[i * nattr + rgb_at + k] = float(cloud[i].rgb()(k));
  }
  std::vector<float> xyz(3 * n), out_attr(n * size_t(nattr));
  std::vector<int32_t> vof(voxel_of ? n : 0);
  int64_t m = 0;
  H.check(s4p_voxel_downsample(H.h, c[0].data(), c[1].data(), c[2].data(), int64_t(n), float(options.voxel_size),
                               nattr ? attr.data() : nullptr, nattr, xyz.data(), nattr ? out_attr.data() : nullptr, nullptr,
                               voxel_of ? vof.data() : nullptr, &m));
  std::vector<Point3D> out;
  out.reserve(size_t(m));
  for (size_t r = 0; r < size_t(m); ++r) {
    Point3D pt(xyz[3 * r], xyz[3 * r + 1], xyz[3 * r + 2]);
    const float* a = out_attr.data() + r * size_t(nattr);
    if (normals) pt.set_normal(Point3D::VectorType(a[0], a[1], a[2]));
    if (colours) pt.set_rgb(Point3D::VectorType(a[rgb_at], a[rgb_at + 1], a[rgb_at + 2]));
    out.push_back(pt);
  }
  cloud.swap(out);
  if (voxel_of) voxel_of->assign(vof.begin(), vof.end());
  return size_t(m);
}

}  // namespace GlobalRegistration
#endif
