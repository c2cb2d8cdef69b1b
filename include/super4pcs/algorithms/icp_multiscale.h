// RefineICPMultiScale: coarse-to-fine ICP on the MI355X as a composition of VoxelDownsample (algorithms/voxelgrid.h) and the
// existing RefineICP (algorithms/icp.h), once per level.  A large correspondence distance widens ICP's basin but is
// expensive on the full-resolution target; here the large distances run on voxel-downsampled pairs and the full resolution
// last, from a pose that is already close.  icp.h and ICPOptions are unchanged.
// Link with -lsuper4pcs_icp -lsuper4pcs_normals.  Builds with and without Eigen, like the rest of the facade.
//
// Unlike RefineICP, Q is taken in its own frame, as read, NOT moved by `transformation`: every level downsamples Q itself, so
// the coarse clouds do not depend on the pose.  After ComputeTransformation (which moves Q) pass a copy made before it:
//
//   std::vector<Point3D> Q0 = Q;
//   matcher.ComputeTransformation(P, &Q, mat);
//   std::vector<ICPLevel> levels = {{0.04, 0.12, 30}, {0.01, 0.03, 30}, {0, 0.008, 30}};
//   RefineICPMultiScale(P, &Q0, mat, ICPOptions(), levels);      // mat refined; Q0 moved by it
//
// Order of operations (tests restate it): level l takes copies of P and Q, downsampled at voxel_size > 0 (normals and colours
// carried as VoxelDownsample does), moves the copy of Q by the current transformation in float,
// x' = ((m00 * x + m01 * y) + m02 * z) + m03, and calls RefineICP on the pair with the level's max_distance and
// max_iterations, which sets transformation <- dT * transformation.  At the end the full Q is moved once, in the same order.
#ifndef S4P_FACADE_ICP_MULTISCALE_H_
#define S4P_FACADE_ICP_MULTISCALE_H_

#include <stdexcept>
#include <vector>

#include "super4pcs/algorithms/icp.h"
#include "super4pcs/algorithms/voxelgrid.h"

namespace GlobalRegistration {

struct ICPLevel {
  double voxel_size = 0;            // > 0: both clouds downsampled at this size; 0: the clouds as given
  double max_distance = -1;         // required (> 0); max(d, 3 * voxel_size) is the usual choice
  int max_iterations = 30;
};

namespace detail {

// pts moved by the float matrix m in k_apply's rounding order; normals and colours stay as they are
inline void icp_move_points(std::vector<Point3D>& pts, Match4PCSBase::MatrixRef m) {
  using Scalar = Match4PCSBase::Scalar;
  Scalar a[3][4];
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) a[r][c] = m(r, c);
  for (Point3D& p : pts) {
    const Scalar x = p.x(), y = p.y(), z = p.z();
    Scalar o[3];
    for (int r = 0; r < 3; ++r) {
      const Scalar s0 = a[r][0] * x, s1 = a[r][1] * y, s2 = a[r][2] * z;      // one product, one sum at a time: no fusing
      const Scalar t0 = s0 + s1;
      const Scalar t1 = t0 + s2;
      o[r] = t1 + a[r][3];
    }
    p.x() = o[0]; p.y() = o[1]; p.z() = o[2];
  }
}

}  // namespace detail

// Levels run in the order given, coarse to fine: voxel sizes must be non-increasing (0 counted as smallest).  options gives
// everything but max_distance and max_iterations, which come from the level.  Returns the last level's fitness; results,
// when given, gets one ICPResult per level.  Throws as RefineICP and VoxelDownsample do, and std::invalid_argument for an
// empty or ill-ordered level list.
inline float RefineICPMultiScale(const std::vector<Point3D>& P, std::vector<Point3D>* Q, Match4PCSBase::MatrixRef transformation,
                                 const ICPOptions& options, const std::vector<ICPLevel>& levels,
                                 std::vector<ICPResult>* results = nullptr) {
  if (Q == nullptr || P.empty() || Q->empty()) throw std::invalid_argument("RefineICPMultiScale: empty cloud");
  if (levels.empty()) throw std::invalid_argument("RefineICPMultiScale: no levels");
  for (size_t l = 0; l < levels.size(); ++l) {
    const double v = levels[l].voxel_size;
    if (!(v >= 0) || v > 3.0e38) throw std::invalid_argument("RefineICPMultiScale: voxel sizes must be finite and >= 0");
    if (l > 0 && v > levels[l - 1].voxel_size)
      throw std::invalid_argument("RefineICPMultiScale: voxel sizes must be non-increasing (coarse to fine, 0 counted as smallest)");
    if (!(levels[l].max_distance > 0)) throw std::invalid_argument("RefineICPMultiScale: every level needs a max_distance > 0");
  }
  if (results) results->clear();
  float fitness = 0.f;
  std::vector<Point3D> Pl, Ql0;                   // the level's clouds before the move; kept while the voxel size repeats
  double have = -1.0;
  for (const ICPLevel& level : levels) {
    if (level.voxel_size != have) {
      Pl = P;
      Ql0 = *Q;
      if (level.voxel_size > 0) {
        VoxelGridOptions vopt;
        vopt.voxel_size = level.voxel_size;
        vopt.device = options.device;
        VoxelDownsample(Pl, vopt);
        VoxelDownsample(Ql0, vopt);
      }
      have = level.voxel_size;
    }
    std::vector<Point3D> Ql = Ql0;
    detail::icp_move_points(Ql, transformation);
    ICPOptions lopt = options;
    lopt.max_distance = level.max_distance;
    lopt.max_iterations = level.max_iterations;
    ICPResult res;
    fitness = RefineICP(Pl, &Ql, transformation, lopt, &res);
    if (results) results->push_back(res);
  }
  detail::icp_move_points(*Q, transformation);
  return fitness;
}

}  // namespace GlobalRegistration
#endif
