// External application of the facade's normal estimation (tests/test_normals_host.py compiles it, tests/test_gpu_normals.py
// runs it).
//   normals_app P.xyz k [radius]    (text file: "x y z" per line)
// Prints one "nx ny nz" line (%.9g) per point: Point3D::normal() after EstimateNormals.
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <vector>

#include "super4pcs/algorithms/normals.h"

using namespace GlobalRegistration;

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  std::vector<Point3D> pts;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  float x, y, z;
  while (std::fscanf(f, "%f %f %f", &x, &y, &z) == 3) pts.emplace_back(x, y, z);
  std::fclose(f);
  NormalEstimationOptions opt;
  opt.k = std::atoi(argv[2]);
  if (argc > 3) opt.radius = std::atof(argv[3]);
  try {
    EstimateNormals(pts, opt);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  for (const Point3D& p : pts) std::printf("%.9g %.9g %.9g\n", p.normal()(0), p.normal()(1), p.normal()(2));
  return 0;
}
