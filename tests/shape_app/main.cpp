// External application of the facade's radius normals (include/super4pcs/algorithms/shape.h on libsuper4pcs_normals.so;
// tests/test_shape_host.py compiles it and runs its refusals, tests/test_gpu_shape.py its results).  A text file, one
// "x y z" per line; every number is printed as %.9g.
//   shape P.xyz radius min_neighbours [plain]   -> "none <count>" (the points without a normal), then "nx ny nz curvature" per
//                                                  point (EstimateNormalsRadius); with plain no curvature is asked for and
//                                                  the lines are "nx ny nz"
// Exit status 2 for usage or an unreadable file, 1 after the exception's text.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <vector>

#include "super4pcs/algorithms/shape.h"

using namespace GlobalRegistration;

int main(int argc, char** argv) {
  if (argc < 5 || std::strcmp(argv[1], "shape")) return 2;
  FILE* f = std::fopen(argv[2], "r");
  if (!f) return 2;
  std::vector<Point3D> pts;
  float v[3];
  while (std::fscanf(f, "%f %f %f", &v[0], &v[1], &v[2]) == 3) pts.emplace_back(v[0], v[1], v[2]);
  std::fclose(f);
  const bool plain = argc > 5 && !std::strcmp(argv[5], "plain");
  try {
    RadiusNormalOptions opt;
    opt.radius = std::atof(argv[3]);
    opt.min_neighbours = std::atoi(argv[4]);
    std::vector<float> curvature;
    const size_t none = EstimateNormalsRadius(pts, opt, plain ? nullptr : &curvature);
    std::printf("none %zu\n", none);
    for (size_t i = 0; i < pts.size(); ++i) {
      std::printf("%.9g %.9g %.9g", pts[i].normal()(0), pts[i].normal()(1), pts[i].normal()(2));
      if (!plain) std::printf(" %.9g", curvature[i]);
      std::printf("\n");
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
