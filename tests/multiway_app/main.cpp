// External application of the facade's multiway path (tests/test_gpu_multiway.py): RegisterMultiway on N scans from poses
// read from a file, and ICPInformation of scan 1 against scan 0 at a pose read from a file.  Links -lsuper4pcs_amd and
// -lsuper4pcs_icp (tests/apps.py).
//   multiway_app poses.txt max_distance min_fitness scan0.xyz scan1.xyz ...   (poses.txt: N + 1 lines of 16 numbers: the N
//                start poses, world <- scan i, row-major, then T for the information of scan 1 onto scan 0)
//     --metric gicp   RegisterMultiway with ICPMetric::Generalized (default: PointToPlane)
//     --check      no device: OptimizePoseGraph on the chain built from the poses file (edges i + 1 -> i that agree with the
//                  poses, unit information), prints its status
// Prints "pose i" + 16 numbers per scan, "edge source target uncertain n rmse fitness l" per edge, "graph iterations a b
// status s pruned p", and "info" + 36 numbers + n + rmse, every double as %.17g.  Exit status: 2 too few arguments, 3 an
// unreadable file, 5 after "invalid: ..." for std::invalid_argument, 1 after "error: ..." for any other exception.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <stdexcept>
#include <vector>

#include "super4pcs/algorithms/multiway.h"

using namespace GlobalRegistration;

static std::vector<Point3D> load(const char* path) {
  std::vector<Point3D> out;
  FILE* f = std::fopen(path, "r");
  if (!f) return out;
  char line[512];
  while (std::fgets(line, sizeof line, f)) {
    float v[3];
    if (std::sscanf(line, "%f %f %f", &v[0], &v[1], &v[2]) == 3) out.emplace_back(v[0], v[1], v[2]);
  }
  std::fclose(f);
  return out;
}

static std::vector<Pose> load_poses(const char* path) {
  std::vector<Pose> out;
  FILE* f = std::fopen(path, "r");
  if (!f) return out;
  for (;;) {
    Pose X;
    int k = 0;
    while (k < 16 && std::fscanf(f, "%lf", &X[size_t(k)]) == 1) ++k;
    if (k < 16) break;
    out.push_back(X);
  }
  std::fclose(f);
  return out;
}

static void print16(const char* what, int i, const double* v, int count) {
  std::printf("%s %d", what, i);
  for (int k = 0; k < count; ++k) std::printf(" %.17g", v[k]);
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  bool check = false, gicp = false;
  std::vector<const char*> files;
  for (int a = 4; a < argc; ++a) {
    if (!std::strcmp(argv[a], "--check")) check = true;
    else if (!std::strcmp(argv[a], "--metric") && a + 1 < argc) gicp = !std::strcmp(argv[++a], "gicp");
    else files.push_back(argv[a]);
  }
  std::vector<Pose> poses = load_poses(argv[1]);
  if (poses.size() < 2) return 3;
  try {
    if (check) {
      const Pose T = poses.back();
      poses.pop_back();
      PoseGraph g;
      g.poses = poses;
      for (size_t i = 0; i + 1 < poses.size(); ++i) {
        PoseGraphEdge e;
        e.source = int(i + 1); e.target = int(i);
        e.T = detail::pose_product(detail::rigid_inverse(poses[i]), poses[i + 1]);
        for (size_t a = 0; a < 6; ++a) e.info[7 * a] = 1.0;
        g.edges.push_back(e);
      }
      g.poses.back() = detail::pose_product(g.poses.back(), T);       // off the chain: the optimiser brings it back
      const PoseGraphResult r = OptimizePoseGraph(&g);
      std::printf("graph iterations %d %d status %d pruned %d cost %.17g %.17g\n", r.iterations[0], r.iterations[1], r.status, r.n_pruned,
                  r.cost_start, r.cost_end);
      for (size_t i = 0; i < g.poses.size(); ++i) { print16("pose", int(i), g.poses[i].data(), 16); std::printf("\n"); }
      PoseGraphEdge bad;
      bad.source = bad.target = 0;
      g.edges.push_back(bad);
      OptimizePoseGraph(&g);                                          // source == target: std::invalid_argument
      return 0;
    }
    if (files.size() + 1 != poses.size()) return 2;
    std::vector<std::vector<Point3D>> scans;
    for (const char* f : files) {
      scans.push_back(load(f));
      if (scans.back().empty()) return 3;
    }
    const Pose T = poses.back();
    poses.pop_back();
    MultiwayOptions o;
    o.icp.max_distance = std::atof(argv[2]);
    o.icp.metric = gicp ? ICPMetric::Generalized : ICPMetric::PointToPlane;
    o.min_fitness = std::atof(argv[3]);
    const MultiwayReport rep = RegisterMultiway(scans, &poses, o);
    for (size_t i = 0; i < poses.size(); ++i) { print16("pose", int(i), poses[i].data(), 16); std::printf("\n"); }
    for (const MultiwayEdgeReport& e : rep.edges)
      std::printf("edge %d %d %d %lld %.17g %.17g %.17g\n", e.source, e.target, e.uncertain ? 1 : 0, (long long)e.n, e.rmse, e.fitness, e.l);
    std::printf("graph iterations %d %d status %d pruned %d cost %.17g %.17g\n", rep.optimize.iterations[0], rep.optimize.iterations[1],
                rep.optimize.status, rep.optimize.n_pruned, rep.optimize.cost_start, rep.optimize.cost_end);
    double info[36], rmse = 0.0;
    int64_t n = 0;
    ICPOptions io;
    io.max_distance = o.icp.max_distance;
    ICPInformation(scans[0], scans[1], T.data(), io, info, &n, &rmse);
    print16("info", int(n), info, 36);
    std::printf(" %.17g\n", rmse);
  } catch (const std::invalid_argument& e) {
    std::printf("invalid: %s\n", e.what());
    return 5;
  } catch (const std::exception& e) {
    std::printf("error: %s\n", e.what());
    return 1;
  }
  return 0;
}
