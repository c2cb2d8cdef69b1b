// External application of the facade's clustering (tests/test_cluster_host.py compiles it, tests/test_gpu_cluster.py runs it).
//   cluster_app P.xyz eps min_points keep min_size          (text file: "x y z" per line)
// Prints "clusters <count>", one label line per input point (ClusterDBSCAN), then "removed <count>", one "0" / "1" line per
// input point (the kept mask of KeepLargestClusters), then one "x y z nx r" line (%.9g) per remaining point: every point
// gets the normal (1, 0, 0) and its input index as the red channel before the calls, so the caller sees that normals and
// colours moved with the points.
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <vector>

#include "super4pcs/algorithms/cluster.h"

using namespace GlobalRegistration;

int main(int argc, char** argv) {
  if (argc < 6) return 2;
  std::vector<Point3D> pts;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  float x, y, z;
  while (std::fscanf(f, "%f %f %f", &x, &y, &z) == 3) {
    pts.emplace_back(x, y, z);
    pts.back().set_normal(Point3D::VectorType(float(pts.size()), 0.f, 0.f));       // normalised to (1, 0, 0)
    pts.back().set_rgb(Point3D::VectorType(float(pts.size() - 1), 0.f, 0.f));
  }
  std::fclose(f);
  ClusterOptions opt;
  opt.eps = std::atof(argv[2]);
  opt.min_points = std::atoi(argv[3]);
  opt.keep = std::atoi(argv[4]);
  opt.min_size = std::atoi(argv[5]);
  std::vector<int32_t> labels;
  std::vector<uint8_t> kept;
  size_t clusters = 0, removed = 0;
  try {
    clusters = ClusterDBSCAN(pts, opt, labels);
    removed = KeepLargestClusters(pts, opt, &kept);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  std::printf("clusters %zu\n", clusters);
  for (int32_t l : labels) std::printf("%d\n", int(l));
  std::printf("removed %zu\n", removed);
  for (uint8_t k : kept) std::printf("%d\n", int(k));
  for (const Point3D& p : pts) std::printf("%.9g %.9g %.9g %.9g %.9g\n", p.x(), p.y(), p.z(), p.normal()(0), p.rgb()(0));
  return 0;
}
