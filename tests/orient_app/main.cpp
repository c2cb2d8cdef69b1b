// External application of the facade's normal orientation (tests/test_orient_host.py compiles it,
// tests/test_gpu_normals_orient.py runs it).
//   orient_app PN.txt k radius [vx vy vz]    (text file: "x y z nx ny nz" per line; radius <= 0: unbounded)
// Prints "flipped <count>" and then one "nx ny nz" line (%.9g) per point: Point3D::normal() after OrientNormals.  The
// normals enter through Point3D::set_normal, which renormalises them.
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <vector>

#include "super4pcs/algorithms/normals.h"

using namespace GlobalRegistration;

int main(int argc, char** argv) {
  if (argc != 4 && argc != 7) return 2;
  std::vector<Point3D> pts;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  float x, y, z, nx, ny, nz;
  while (std::fscanf(f, "%f %f %f %f %f %f", &x, &y, &z, &nx, &ny, &nz) == 6) {
    pts.emplace_back(x, y, z);
    pts.back().set_normal(Point3D::VectorType(nx, ny, nz));
  }
  std::fclose(f);
  NormalOrientationOptions opt;
  opt.k = std::atoi(argv[2]);
  opt.radius = std::atof(argv[3]);
  if (argc == 7) {
    opt.use_viewpoint = true;
    for (int a = 0; a < 3; ++a) opt.viewpoint[a] = std::atof(argv[4 + a]);
  }
  size_t flipped = 0;
  try {
    flipped = OrientNormals(pts, opt);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  std::printf("flipped %zu\n", flipped);
  for (const Point3D& p : pts) std::printf("%.9g %.9g %.9g\n", p.normal()(0), p.normal()(1), p.normal()(2));
  return 0;
}
