// External application of the facade's ICP paths: MatchSuper4PCS, then RefineICP on the same clouds with the ICPOptions the
// flags set (tests/apps.py; the hippo tests of tests/test_gpu_icp*.py and tests/test_icp_symm_host.py).  Links
// -lsuper4pcs_amd and -lsuper4pcs_icp only: RefineICP binds the normals library at run time.
//   icp_facade_app P.xyz Q.xyz delta overlap samples [options]    (text files: "x y z" or "x y z a b c" per line)
//     --metric point|plane|gicp|symmetric|color      --loss trimmed|huber|tukey      --trim-fraction F
//     --gicp-epsilon E      --color-lambda L      --reciprocal      --normal-angle-deg A      --max-iterations N
//     --rgb         a b c is the point's colour (0..255), not its normal
//     --identity    no registration: RefineICP starts from the identity (needs no device until RefineICP asks for one)
//     --batch       no registration: RefineICPBatch with two identity starts
// A cloud's normals (colours) are used when every line of its file has them.  Prints the registration's and the refined
// 4x4 (%.9g, row-major) and the refinement's statistics.  Exit status: 2 too few arguments or an unknown option, 3 an empty
// cloud, 4 a bad overlap, 5 after "invalid: ..." for std::invalid_argument, 1 after "error: ..." for any other exception.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <stdexcept>
#include <string>
#include <vector>

#include "super4pcs/algorithms/icp.h"
#include "super4pcs/algorithms/icp_batch.h"
#include "super4pcs/algorithms/super4pcs.h"

using namespace GlobalRegistration;

static std::vector<Point3D> load(const char* path, bool rgb) {
  std::vector<Point3D> out;
  FILE* f = std::fopen(path, "r");
  if (!f) return out;
  char line[512];
  while (std::fgets(line, sizeof line, f)) {
    float v[6];
    const int k = std::sscanf(line, "%f %f %f %f %f %f", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5]);
    if (k < 3) continue;
    out.emplace_back(v[0], v[1], v[2]);
    if (k == 6 && rgb) out.back().set_rgb(Point3D::VectorType(v[3], v[4], v[5]));
    if (k == 6 && !rgb) out.back().set_normal(Point3D::VectorType(v[3], v[4], v[5]));
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
  ICPOptions icp;
  bool rgb = false, identity = false, batch = false;
  for (int a = 6; a < argc; ++a) {
    const std::string o = argv[a];
    if (o == "--rgb") { rgb = true; continue; }
    if (o == "--identity") { identity = true; continue; }
    if (o == "--batch") { batch = true; continue; }
    if (o == "--reciprocal") { icp.reciprocal = true; continue; }
    if (++a == argc) return 2;                        // every other option takes a value
    const char* v = argv[a];
    if (o == "--metric")
      icp.metric = !std::strcmp(v, "plane") ? ICPMetric::PointToPlane : !std::strcmp(v, "gicp") ? ICPMetric::Generalized
                   : !std::strcmp(v, "symmetric") ? ICPMetric::Symmetric : !std::strcmp(v, "color") ? ICPMetric::Colored
                                                                                                   : ICPMetric::PointToPoint;
    else if (o == "--loss")
      icp.loss = !std::strcmp(v, "trimmed") ? ICPLoss::Trimmed : (!std::strcmp(v, "huber") ? ICPLoss::Huber : ICPLoss::Tukey);
    else if (o == "--trim-fraction") icp.trim_fraction = std::atof(v);
    else if (o == "--gicp-epsilon") icp.gicp_epsilon = std::atof(v);
    else if (o == "--color-lambda") icp.color_lambda = std::atof(v);
    else if (o == "--normal-angle-deg") icp.normal_angle_deg = std::atof(v);
    else if (o == "--max-iterations") icp.max_iterations = std::atoi(v);
    else return 2;
  }
  std::vector<Point3D> P = load(argv[1], rgb), Q = load(argv[2], rgb);
  if (P.empty() || Q.empty()) return 3;
  Match4PCSOptions opt;
  if (!opt.configureOverlap(float(std::atof(argv[4])))) return 4;
  opt.delta = float(std::atof(argv[3]));
  opt.sample_size = size_t(std::atoi(argv[5]));
  opt.max_time_seconds = 1000;
  icp.max_distance = 4.0 * opt.delta;
  try {
    Match4PCSBase::MatrixType M = Match4PCSBase::MatrixType::Identity();
    if (batch) {
      const auto best = RefineICPBatch(P, &Q, std::vector<Match4PCSBase::MatrixType>(2, M), icp);
      print("refined", best.first);
      std::printf("batch best %d\n", best.second);
      return 0;
    }
    if (!identity) {
      Utils::Logger logger(Utils::NoLog);
      MatchSuper4PCS matcher(opt, logger);
      matcher.ComputeTransformation(P, &Q, M);
    }
    print("registered", M);
    ICPResult res;
    const float fit = RefineICP(P, &Q, M, icp, &res);
    print("refined", M);
    std::printf("icp iterations %d status %d n_corr %lld rmse %.9g fitness %.9g\n", res.iterations, res.status,
                (long long)res.n_corr, res.rmse, double(fit));
  } catch (const std::invalid_argument& e) {
    std::printf("invalid: %s\n", e.what());
    return 5;
  } catch (const std::exception& e) {
    std::printf("error: %s\n", e.what());
    return 1;
  }
  return 0;
}
