// RemoveOutliers: statistical or radius outlier removal of a whole cloud on the MI355X, through the C ABI of
// libsuper4pcs_normals.so (include/s4p_knn.h).  Generalized and coloured ICP take no robust loss, and a normal or a matched
// pair taken on a stray return is wrong in a way no later stage repairs: filter the clouds first.
// Link with -lsuper4pcs_normals.  Builds with and without Eigen, like the rest of the facade.
//
//   OutlierRemovalOptions oopt;                  // statistical: k = 16, std_ratio = 2
//   RemoveOutliers(P, oopt);  RemoveOutliers(Q, oopt);
//   oopt.radius = 0.05;  oopt.min_neighbours = 4;   // radius: at least 4 other points within 0.05
#ifndef S4P_FACADE_OUTLIERS_H_
#define S4P_FACADE_OUTLIERS_H_

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <utility>
#include <vector>

#include "s4p_knn.h"
#include "super4pcs/algorithms/normals_handle.h"

namespace GlobalRegistration {

struct OutlierRemovalOptions {
  int k = 16;                       // statistical: neighbours per point, 1..32 (the point itself not counted)
  double std_ratio = 2.0;           // statistical: keep m_j <= mu + std_ratio * sigma; finite, >= 0
  double radius = -1;               // radius filter: > 0, with min_neighbours > 0
  int min_neighbours = 0;           // 0: the statistical filter; 1..32: the radius filter
  int device = 0;
};

// Erases the outliers in place, keeping the order of the remaining points and their normals and colours, and returns how
// many it removed.  kept, when given, gets one byte per point of the input cloud (1 = kept).  min_neighbours == 0 selects
// the statistical filter (k, std_ratio); radius > 0 && min_neighbours > 0 the radius filter.  Throws std::runtime_error
// when there is no device (no CPU fallback) and std::invalid_argument when an option is outside its limits.
inline size_t RemoveOutliers(std::vector<Point3D>& cloud, const OutlierRemovalOptions& options, std::vector<uint8_t>* kept = nullptr) {
  const bool statistical = options.min_neighbours == 0;
  if (statistical) {
    if (options.k < S4P_KNN_MIN_K || options.k > S4P_KNN_MAX_K) throw std::invalid_argument("RemoveOutliers: k must be in [1, 32]");
    if (!(options.std_ratio >= 0) || options.std_ratio > 1.0e300) throw std::invalid_argument("RemoveOutliers: std_ratio must be finite and >= 0");
  } else {
    if (options.min_neighbours < S4P_KNN_MIN_K || options.min_neighbours > S4P_KNN_MAX_K)
      throw std::invalid_argument("RemoveOutliers: min_neighbours must be 0 (statistical) or in [1, 32]");
    if (!(options.radius > 0) || options.radius > 3.0e38) throw std::invalid_argument("RemoveOutliers: the radius filter needs a finite radius > 0");
  }
  if (kept) kept->clear();
  if (cloud.empty()) return 0;
  const detail::NormalsHandle H("RemoveOutliers", options.device);
  H.set_cloud(cloud);
  std::vector<uint8_t> keep(cloud.size());
  if (statistical) H.check(s4p_outliers_statistical(H.h, options.k, options.std_ratio, nullptr, keep.data(), nullptr));
  else H.check(s4p_outliers_radius(H.h, float(options.radius), options.min_neighbours, keep.data()));
  size_t w = 0;
  for (size_t i = 0; i < cloud.size(); ++i) {
    if (!keep[i]) continue;
    if (w != i) cloud[w] = std::move(cloud[i]);
    ++w;
  }
  const size_t removed = cloud.size() - w;
  cloud.resize(w);
  if (kept) *kept = std::move(keep);
  return removed;
}

}  // namespace GlobalRegistration
#endif
