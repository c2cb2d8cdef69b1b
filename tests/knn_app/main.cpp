// External application of the facade's outlier removal (tests/test_knn_host.py compiles it, tests/test_gpu_outliers.py runs it).
//   knn_app P.xyz stat k std_ratio          (text file: "x y z" per line)
//   knn_app P.xyz radius r min_neighbours
// Prints "removed <count>", one "0" / "1" line per input point (the kept mask), then one "x y z nx r" line (%.9g) per
// remaining point: every point gets the normal (1, 0, 0) and its input index as the red channel before the call, so the
// caller sees that normals and colours moved with the points.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <vector>

#include "super4pcs/algorithms/outliers.h"

using namespace GlobalRegistration;

int main(int argc, char** argv) {
  if (argc < 5) return 2;
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
  OutlierRemovalOptions opt;
  if (!std::strcmp(argv[2], "stat")) {
    opt.k = std::atoi(argv[3]);
    opt.std_ratio = std::atof(argv[4]);
  } else {
    opt.radius = std::atof(argv[3]);
    opt.min_neighbours = std::atoi(argv[4]);
  }
  std::vector<uint8_t> kept;
  size_t removed = 0;
  try {
    removed = RemoveOutliers(pts, opt, &kept);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  std::printf("removed %zu\n", removed);
  for (uint8_t k : kept) std::printf("%d\n", int(k));
  for (const Point3D& p : pts) std::printf("%.9g %.9g %.9g %.9g %.9g\n", p.x(), p.y(), p.z(), p.normal()(0), p.rgb()(0));
  return 0;
}
