// External application of the facade's multi-scale ICP (tests/test_voxel_host.py compiles it, tests/test_gpu_icp_multiscale.py
// runs it).
//   icp_multiscale_app P.xyz Q.xyz T0.txt metric v:d:it [v:d:it ...]
// P.xyz, Q.xyz: one "x y z" per line, Q in its own frame; T0.txt: 16 numbers, the start pose row-major; metric: point, plane
// (normals estimated by RefineICP) or huber (point with the Huber loss).
// Prints the refined 4x4 (%.9g, row-major), one "level" line per level (iterations, status, n_corr, rmse and fitness as
// %.17g), then one "x y z" line (%.9g) per point of the moved Q.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <vector>

#include "super4pcs/algorithms/icp_multiscale.h"

using namespace GlobalRegistration;

static std::vector<Point3D> load(const char* path) {
  std::vector<Point3D> out;
  FILE* f = std::fopen(path, "r");
  if (!f) return out;
  float x, y, z;
  while (std::fscanf(f, "%f %f %f", &x, &y, &z) == 3) out.emplace_back(x, y, z);
  std::fclose(f);
  return out;
}

int main(int argc, char** argv) {
  if (argc < 6) return 2;
  std::vector<Point3D> P = load(argv[1]), Q = load(argv[2]);
  Match4PCSBase::MatrixType M = Match4PCSBase::MatrixType::Identity();
  FILE* f = std::fopen(argv[3], "r");
  if (!f) return 3;
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      float v;
      if (std::fscanf(f, "%f", &v) != 1) return 3;
      M(r, c) = v;
    }
  std::fclose(f);
  ICPOptions opt;
  if (!std::strcmp(argv[4], "plane")) opt.metric = ICPMetric::PointToPlane;
  if (!std::strcmp(argv[4], "huber")) opt.loss = ICPLoss::Huber;
  std::vector<ICPLevel> levels;
  for (int a = 5; a < argc; ++a) {
    ICPLevel level;
    if (std::sscanf(argv[a], "%lf:%lf:%d", &level.voxel_size, &level.max_distance, &level.max_iterations) != 3) return 2;
    levels.push_back(level);
  }
  std::vector<ICPResult> res;
  try {
    RefineICPMultiScale(P, &Q, M, opt, levels, &res);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  std::printf("refined");
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) std::printf(" %.9g", double(M(r, c)));
  std::printf("\n");
  for (const ICPResult& r : res)
    std::printf("level %d %d %lld %.17g %.17g\n", r.iterations, r.status, (long long)r.n_corr, r.rmse, r.fitness);
  for (const Point3D& p : Q) std::printf("%.9g %.9g %.9g\n", p.x(), p.y(), p.z());
  return 0;
}
