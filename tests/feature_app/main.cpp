// External application of the facade's descriptors (include/super4pcs/algorithms/features.h on libsuper4pcs_normals.so;
// tests/test_features_host.py compiles it and runs its refusals, tests/test_gpu_features.py its results).  Text files, one
// "x y z nx ny nz" per line.
//   fpfh P.xyzn radius                  -> "none <count>" (the rows that are all zeros), then the 33 values of every row
//   match P.xyzn Q.xyzn radius mutual   -> "matches <count>", then "a b" per pair (ComputeFPFH of both, MatchFeatures)
// Exit status 2 for usage or an unreadable file, 1 after the exception's text.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <vector>

#include "super4pcs/algorithms/features.h"

using namespace GlobalRegistration;

static bool read_cloud(const char* path, std::vector<Point3D>& pts) {
  FILE* f = std::fopen(path, "r");
  if (!f) return false;
  float v[6];
  while (std::fscanf(f, "%f %f %f %f %f %f", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5]) == 6) {
    pts.emplace_back(v[0], v[1], v[2]);
    // set_normal renormalises in float: the tests give the Python path the normals renormalised the same way
    pts.back().set_normal(Point3D::VectorType(v[3], v[4], v[5]));
  }
  std::fclose(f);
  return true;
}

int main(int argc, char** argv) {
  const bool fpfh = argc == 4 && !std::strcmp(argv[1], "fpfh"), match = argc == 6 && !std::strcmp(argv[1], "match");
  if (!fpfh && !match) return 2;
  std::vector<Point3D> P, Q;
  if (!read_cloud(argv[2], P) || (match && !read_cloud(argv[3], Q))) return 2;
  try {
    FPFHOptions opt;
    opt.radius = std::atof(argv[match ? 4 : 3]);
    std::vector<FPFHRow> FP, FQ;
    const size_t none = ComputeFPFH(P, opt, FP);
    if (fpfh) {
      std::printf("none %zu\n", none);
      for (const FPFHRow& row : FP) {
        for (size_t k = 0; k < row.size(); ++k) std::printf(k ? " %u" : "%u", unsigned(row[k]));
        std::printf("\n");
      }
      return 0;
    }
    ComputeFPFH(Q, opt, FQ);
    std::vector<std::pair<int, int>> pairs;
    MatchFeatures(FP, FQ, std::atoi(argv[5]) != 0, pairs);
    std::printf("matches %zu\n", pairs.size());
    for (const auto& p : pairs) std::printf("%d %d\n", p.first, p.second);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
