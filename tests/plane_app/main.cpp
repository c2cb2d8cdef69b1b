// External application of the facade's plane segmentation (tests/test_plane_host.py compiles it, tests/test_gpu_plane.py runs
// it).
//   plane_app P.xyz distance trials refine count          (text file: "x y z" per line)
// Prints "plane n0 n1 n2 d" (%.9g) and "inliers <count>", one "0" / "1" line per input point (the inlier mask of
// SegmentPlane), then "removed <count> planes <count>" of RemovePlanes and one "x y z nx r" line (%.9g) per remaining point:
// every point gets the normal (1, 0, 0) and its input index as the red channel before the calls, so the caller sees that
// normals and colours moved with the points.
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <vector>

#include "super4pcs/algorithms/plane.h"

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
  PlaneOptions opt;
  opt.distance = std::atof(argv[2]);
  opt.trials = std::atoi(argv[3]);
  opt.refine = std::atoi(argv[4]);
  opt.count = std::atoi(argv[5]);
  std::vector<uint8_t> inlier;
  std::vector<PlaneModel> planes;
  PlaneModel m;
  size_t removed = 0;
  try {
    m = SegmentPlane(pts, opt, inlier);
    removed = RemovePlanes(pts, opt, nullptr, &planes);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  std::printf("plane %.9g %.9g %.9g %.9g\n", m.normal[0], m.normal[1], m.normal[2], m.d);
  std::printf("inliers %zu\n", m.inliers);
  for (uint8_t k : inlier) std::printf("%d\n", int(k));
  std::printf("removed %zu planes %zu\n", removed, planes.size());
  for (const Point3D& p : pts) std::printf("%.9g %.9g %.9g %.9g %.9g\n", p.x(), p.y(), p.z(), p.normal()(0), p.rgb()(0));
  return 0;
}
