// ComputeFPFH and MatchFeatures: Fast Point Feature Histograms of a whole cloud from its points' normals, and the mutual
// nearest neighbours of two descriptor tables, on the MI355X, through the C ABI of libsuper4pcs_normals.so
// (include/s4p_feature.h).  The normals must be CONSISTENTLY ORIENTED (OrientNormals of algorithms/normals.h after
// EstimateNormals or EstimateNormalsRadius): with normals of arbitrary sign the descriptors of one surface differ between two
// clouds and the matches are noise.
// Link with -lsuper4pcs_normals.  Builds with and without Eigen, like the rest of the facade.
//
//   FPFHOptions fopt;  fopt.radius = 0.08;
//   std::vector<std::array<uint16_t, 33>> FP, FQ;
//   ComputeFPFH(P, fopt, FP);  ComputeFPFH(Q, fopt, FQ);      // every value in [0, 4096]; a row of zeros: no descriptor
//   std::vector<std::pair<int, int>> matches;
//   MatchFeatures(FP, FQ, true, matches);                     // (index in P, index in Q), ascending in P
#ifndef S4P_FACADE_FEATURES_H_
#define S4P_FACADE_FEATURES_H_

#include <array>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <utility>
#include <vector>

#include "s4p_feature.h"
#include "super4pcs/algorithms/normals_handle.h"

namespace GlobalRegistration {

struct FPFHOptions {
  double radius = -1;               // every other point within it is a neighbour: finite, > 0
  int device = 0;
};

using FPFHRow = std::array<uint16_t, S4P_FEATURE_BINS>;

// out[i] is the descriptor of points[i] from the points' positions and normal()s: three groups of eleven bins, each group
// summing to at most 4096.  A row is all zeros where the point has no normal (a zero or non-finite one) or no neighbour with
// one.  Returns the number of such rows.  Throws std::runtime_error when there is no device (no CPU fallback) and
// std::invalid_argument when the radius is outside its limits.
inline size_t ComputeFPFH(const std::vector<Point3D>& points, const FPFHOptions& options, std::vector<FPFHRow>& out) {
  if (!(options.radius > 0) || options.radius > 1.8e19 || !(float(options.radius) > 0.f))
    throw std::invalid_argument("ComputeFPFH: radius must be finite and > 0, with a square that fits a float");
  out.clear();
  if (points.empty()) return 0;
  const detail::NormalsHandle H("ComputeFPFH", options.device);
  H.set_cloud(points);
  const size_t n = points.size();
  std::vector<float> nrm(3 * n);
  for (size_t i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) nrm[3 * i + a] = float(points[i].normal()(a));
  out.resize(n);
  static_assert(sizeof(FPFHRow) == S4P_FEATURE_BINS * sizeof(uint16_t), "rows are contiguous");
  H.check(s4p_feature_fpfh(H.h, nrm.data(), float(options.radius), out[0].data(), nullptr));
  size_t none = 0;
  for (const FPFHRow& row : out) {
    bool any = false;
    for (uint16_t v : row) any |= v != 0;
    if (!any) ++none;
  }
  return none;
}

// out gets (index in a, index in b) for every row of a that found a partner, in ascending index of a: the row of b with the
// smallest (squared distance, index) among the rows of b that are not all zeros; with mutual only where the row of a is that
// row's best in turn.  Returns the number of pairs.  Throws std::runtime_error when there is no device or a value exceeds 4096.
inline size_t MatchFeatures(const std::vector<FPFHRow>& a, const std::vector<FPFHRow>& b, bool mutual, std::vector<std::pair<int, int>>& out,
                            int device = 0) {
  out.clear();
  if (a.empty()) return 0;
  const detail::NormalsHandle H("MatchFeatures", device);
  std::vector<int32_t> idx(a.size());
  H.check(s4p_feature_match(H.h, a[0].data(), int64_t(a.size()), b.empty() ? nullptr : b[0].data(), int64_t(b.size()), mutual ? 1 : 0,
                            idx.data(), nullptr));
  for (size_t i = 0; i < idx.size(); ++i)
    if (idx[i] >= 0) out.emplace_back(int(i), int(idx[i]));
  return out.size();
}

}  // namespace GlobalRegistration
#endif
