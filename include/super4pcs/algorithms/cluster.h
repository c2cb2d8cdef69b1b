// ClusterDBSCAN / KeepLargestClusters: density clustering of a whole cloud on the MI355X, through the C ABI of
// libsuper4pcs_normals.so (include/s4p_cluster.h).  The statistical filter keeps a dense fragment away from the surface (a
// second object, a floating patch): it is as dense as the surface.  The matcher then spends bases on it and ICP matches into
// it; KeepLargestClusters takes the cloud apart and keeps the surface.
// Link with -lsuper4pcs_normals.  Builds with and without Eigen, like the rest of the facade.
//
//   ClusterOptions copt;  copt.eps = 0.03;  copt.min_points = 4;
//   std::vector<int32_t> labels;
//   const size_t clusters = ClusterDBSCAN(P, copt, labels);      // labels[i] in 0 .. clusters - 1, or -1: noise
//   KeepLargestClusters(P, copt);                                 // P = its largest cluster
#ifndef S4P_FACADE_CLUSTER_H_
#define S4P_FACADE_CLUSTER_H_

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "s4p_cluster.h"
#include "super4pcs/algorithms/normals_handle.h"

namespace GlobalRegistration {

struct ClusterOptions {
  double eps = -1;                  // the neighbourhood radius: finite, > 0
  int min_points = 10;              // a core point has at least this many points within eps, itself included; >= 1
  int keep = 1;                     // KeepLargestClusters: how many clusters stay; >= 1
  int min_size = 1;                 // KeepLargestClusters: a cluster that stays has at least this many points; >= 1
  int device = 0;
};

namespace detail {
inline void cluster_check_options(const char* who, const ClusterOptions& o) {
  if (!(o.eps > 0) || o.eps > 1.8e19) throw std::invalid_argument(std::string(who) + ": eps must be finite and > 0, with a square that fits a float");
  if (o.min_points < 1) throw std::invalid_argument(std::string(who) + ": min_points must be at least 1");
  if (o.keep < 1) throw std::invalid_argument(std::string(who) + ": keep must be at least 1");
  if (o.min_size < 1) throw std::invalid_argument(std::string(who) + ": min_size must be at least 1");
}
}  // namespace detail

// labels[i] = the cluster of point i, numbered from 0 in ascending order of the clusters' smallest core index, or -1 for
// noise; returns the number of clusters.  Throws std::runtime_error when there is no device (no CPU fallback) and
// std::invalid_argument when an option is outside its limits.
inline size_t ClusterDBSCAN(const std::vector<Point3D>& cloud, const ClusterOptions& options, std::vector<int32_t>& labels) {
  detail::cluster_check_options("ClusterDBSCAN", options);
  labels.clear();
  if (cloud.empty()) return 0;
  const detail::NormalsHandle H("ClusterDBSCAN", options.device);
  H.set_cloud(cloud);
  labels.resize(cloud.size());
  s4p_cluster_stats st{};
  H.check(s4p_cluster_dbscan(H.h, float(options.eps), options.min_points, labels.data(), nullptr, &st));
  return size_t(st.clusters);
}

// Keeps the options.keep largest clusters that have at least options.min_size points (ties in size go to the smaller
// label) and erases every other point in place, keeping the order of the remaining points and their normals and colours;
// returns how many it removed.  kept, when given, gets one byte per point of the input cloud (1 = kept).
inline size_t KeepLargestClusters(std::vector<Point3D>& cloud, const ClusterOptions& options, std::vector<uint8_t>* kept = nullptr) {
  detail::cluster_check_options("KeepLargestClusters", options);
  if (kept) kept->clear();
  if (cloud.empty()) return 0;
  std::vector<int32_t> labels;
  const size_t clusters = ClusterDBSCAN(cloud, options, labels);
  std::vector<size_t> size(clusters, 0);
  for (int32_t l : labels)
    if (l >= 0) ++size[size_t(l)];
  std::vector<int32_t> order;
  for (size_t c = 0; c < clusters; ++c)
    if (size[c] >= size_t(options.min_size)) order.push_back(int32_t(c));
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return size[size_t(a)] > size[size_t(b)]; });
  if (order.size() > size_t(options.keep)) order.resize(size_t(options.keep));
  std::vector<uint8_t> chosen(clusters, 0);
  for (int32_t c : order) chosen[size_t(c)] = 1;
  std::vector<uint8_t> keep(cloud.size());
  size_t w = 0;
  for (size_t i = 0; i < cloud.size(); ++i) {
    keep[i] = labels[i] >= 0 && chosen[size_t(labels[i])] ? 1 : 0;
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
