// External application of the facade's symmetric ICP path: MatchSuper4PCS, then RefineICP with ICPMetric::Symmetric
// (tests/test_gpu_icp_symm.py, tests/test_icp_symm_host.py).  Links -lsuper4pcs_amd and -lsuper4pcs_icp only.
//   icp_symm_app P.xyz Q.xyz delta overlap samples [iterations]    (text files: "x y z" or "x y z nx ny nz" per line)
//   icp_symm_app P.xyz Q.xyz delta overlap samples iterations huber|batch
// A cloud's normals are used when every line of its file has them, else RefineICP estimates them.  Prints the
// registration's and the refined 4x4 (%.9g, row-major) and the refinement's statistics.  With a seventh argument no
// registration runs: RefineICP with a Huber loss, or RefineICPBatch, is called with the symmetric metric and must refuse it
// before it asks for a device ("refused: ..." and exit status 0; anything else exits with 5).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <stdexcept>
#include <vector>

#include "super4pcs/algorithms/icp.h"
#include "super4pcs/algorithms/icp_batch.h"
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
  if (argc < 6) return 2;
  std::vector<Point3D> P = load(argv[1]), Q = load(argv[2]);
  if (P.empty() || Q.empty()) return 3;
  Match4PCSOptions opt;
  if (!opt.configureOverlap(float(std::atof(argv[4])))) return 4;
  opt.delta = float(std::atof(argv[3]));
  opt.sample_size = size_t(std::atoi(argv[5]));
  opt.max_time_seconds = 1000;
  ICPOptions icp;
  icp.max_distance = 4.0 * opt.delta;
  icp.metric = ICPMetric::Symmetric;
  if (argc > 6) icp.max_iterations = std::atoi(argv[6]);
  Match4PCSBase::MatrixType M = Match4PCSBase::MatrixType::Identity();
  if (argc > 7) {
    try {
      if (!std::strcmp(argv[7], "huber")) {
        icp.loss = ICPLoss::Huber;
        RefineICP(P, &Q, M, icp);
      } else {
        RefineICPBatch(P, &Q, std::vector<Match4PCSBase::MatrixType>(2, M), icp);
      }
    } catch (const std::invalid_argument& e) {
      std::printf("refused: %s\n", e.what());
      return 0;
    } catch (const std::exception& e) {
      std::printf("error: %s\n", e.what());
    }
    return 5;
  }
  try {
    Utils::Logger logger(Utils::NoLog);
    MatchSuper4PCS matcher(opt, logger);
    matcher.ComputeTransformation(P, &Q, M);
    print("registered", M);
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
