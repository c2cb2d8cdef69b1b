// External application of the facade's pair rejection: MatchSuper4PCS, then RefineICP with ICPOptions::reciprocal and
// ICPOptions::normal_angle_deg (tests/test_gpu_icp_reject.py).  Links -lsuper4pcs_amd and -lsuper4pcs_icp only.
//   icp_reject_app P.xyz Q.xyz delta overlap samples metric reciprocal angle_deg
//     metric: point | plane | gicp; reciprocal: 0 | 1; angle_deg < 0: no normal test
//     (text files: "x y z" or "x y z nx ny nz" per line)
// A cloud's normals are used when every line of its file has them, else RefineICP estimates them.  Prints the
// registration's and the refined 4x4 (%.9g, row-major) and the refinement's statistics.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <vector>

#include "super4pcs/algorithms/icp.h"
#include "super4pcs/algorithms/super4pcs.h"

using namespace GlobalRegistration;

static std::vector<Point3D> load(const char* path) {
  std::vector<Point3D> out;
  FILE* f = std::fopen(path, "r");
  if (!f) return out;
  char line[512];
  while (std::fgets(line, sizeof line, f)) {
    float v[6];
    const int k = std::sscanf(line, "%f %f %f %f %f %f", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5]);
    if (k < 3) continue;
    out.emplace_back(v[0], v[1], v[2]);
    if (k == 6) out.back().set_normal(Point3D::VectorType(v[3], v[4], v[5]));
  }
  std::fclose(f);
  return out;
}

static void print(const char* what, const Match4PCSBase::MatrixType& M) {
  std::printf("%s", what);
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) std::printf(" %.9g", double(M(r, c)));
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 9) return 2;
  std::vector<Point3D> P = load(argv[1]), Q = load(argv[2]);
  if (P.empty() || Q.empty()) return 3;
  Match4PCSOptions opt;
  if (!opt.configureOverlap(float(std::atof(argv[4])))) return 4;
  opt.delta = float(std::atof(argv[3]));
  opt.sample_size = size_t(std::atoi(argv[5]));
  opt.max_time_seconds = 1000;
  try {
    Utils::Logger logger(Utils::NoLog);
    MatchSuper4PCS matcher(opt, logger);
    Match4PCSBase::MatrixType M = Match4PCSBase::MatrixType::Identity();
    matcher.ComputeTransformation(P, &Q, M);
    print("registered", M);
    ICPOptions icp;
    icp.max_distance = 4.0 * opt.delta;
    icp.metric = !std::strcmp(argv[6], "gicp") ? ICPMetric::Generalized
                 : (!std::strcmp(argv[6], "plane") ? ICPMetric::PointToPlane : ICPMetric::PointToPoint);
    icp.reciprocal = std::atoi(argv[7]) != 0;
    icp.normal_angle_deg = std::atof(argv[8]);
    ICPResult res;
    const float fit = RefineICP(P, &Q, M, icp, &res);
    print("refined", M);
    std::printf("icp iterations %d status %d n_corr %lld rmse %.9g fitness %.9g\n", res.iterations, res.status,
                (long long)res.n_corr, res.rmse, double(fit));
  } catch (const std::exception& e) {
    std::printf("error: %s\n", e.what());
    return 1;
  }
  return 0;
}
