// External application of the facade's voxel-grid downsampling (tests/test_voxel_host.py compiles it, tests/test_gpu_voxel.py
// runs it).
//   voxel_app P.txt voxel_size plain          (text file: "x y z" per line)
//   voxel_app P.txt voxel_size attrs          (text file: "x y z nx ny nz r g b" per line: normals and colours set)
// Prints "m <count>", one line per input point (its output row, -1 if dropped), then one "x y z nx ny nz r g b" line (%.9g)
// per remaining point.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <vector>

#include "super4pcs/algorithms/voxelgrid.h"

using namespace GlobalRegistration;

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const bool attrs = !std::strcmp(argv[3], "attrs");
  std::vector<Point3D> pts;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  float v[9];
  for (;;) {
    int got = 0;
    for (int k = 0; k < (attrs ? 9 : 3); ++k) got += std::fscanf(f, "%f", &v[k]) == 1;
    if (got != (attrs ? 9 : 3)) break;
    pts.emplace_back(v[0], v[1], v[2]);
    if (attrs) {
      pts.back().set_normal(Point3D::VectorType(v[3], v[4], v[5]));
      pts.back().set_rgb(Point3D::VectorType(v[6], v[7], v[8]));
    }
  }
  std::fclose(f);
  VoxelGridOptions opt;
  opt.voxel_size = std::atof(argv[2]);
  std::vector<int> voxel_of;
  size_t m = 0;
  try {
    m = VoxelDownsample(pts, opt, &voxel_of);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  std::printf("m %zu\n", m);
  for (int r : voxel_of) std::printf("%d\n", r);
  for (const Point3D& p : pts)
    std::printf("%.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", p.x(), p.y(), p.z(), p.normal()(0), p.normal()(1), p.normal()(2),
                p.rgb()(0), p.rgb()(1), p.rgb()(2));
  return 0;
}
