// External application of the facade's cleaning calls on libsuper4pcs_normals.so (tests/normals_suite.py compiles it; the host
// modules run its refusals, the GPU modules its results, tests/golden/make_facade_parity_golden.py its printed lines).  Text
// files, one point per line; every number is printed as %.9g.
//   normals  P.xyz k [radius]                       "x y z"             -> "nx ny nz" per point (EstimateNormals)
//   outliers P.xyz stat k std_ratio                 "x y z", tagged     -> "removed <count>", the kept mask, "x y z nx r" per
//   outliers P.xyz radius r min_neighbours                                 remaining point (RemoveOutliers)
//   voxel    P.txt voxel_size plain|attrs           "x y z" or "x y z nx ny nz r g b"
//                                                   -> "m <count>", every input point's output row (-1 if dropped),
//                                                      "x y z nx ny nz r g b" per remaining point (VoxelDownsample)
//   orient   PN.txt k radius [vx vy vz]             "x y z nx ny nz"; radius <= 0: unbounded
//                                                   -> "flipped <count>", "nx ny nz" per point (OrientNormals)
//   cluster  P.xyz eps min_points keep min_size     "x y z", tagged     -> "clusters <count>", every point's label
//                                                      (ClusterDBSCAN), "removed <count>", the kept mask, "x y z nx r" per
//                                                      remaining point (KeepLargestClusters)
//   plane    P.xyz distance trials refine count     "x y z", tagged     -> "plane n0 n1 n2 d", "inliers <count>", the inlier
//                                                      mask (SegmentPlane), "removed <count> planes <count>", "x y z nx r" per
//                                                      remaining point (RemovePlanes)
// A mask is one "0" / "1" line per input point.  Tagged: every point gets the normal (1, 0, 0) and its input index as the red
// channel before the calls, so the caller sees that normals and colours moved with the points.  Normals read from a file enter
// through Point3D::set_normal, which renormalises them.  Exit status 2 for usage or an unreadable file, 1 after the exception's
// text.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <initializer_list>
#include <vector>

#include "super4pcs/algorithms/cluster.h"
#include "super4pcs/algorithms/normals.h"
#include "super4pcs/algorithms/outliers.h"
#include "super4pcs/algorithms/plane.h"
#include "super4pcs/algorithms/voxelgrid.h"

using namespace GlobalRegistration;
using Points = std::vector<Point3D>;

struct Usage {};

// `columns` numbers per line: 3 (position), 6 (and a normal) or 9 (and a colour); stops at the first incomplete line.
static Points read_points(const char* path, int columns, bool tagged = false) {
  FILE* f = std::fopen(path, "r");
  if (!f) throw Usage();
  Points pts;
  float v[9];
  for (;;) {
    int got = 0;
    for (int k = 0; k < columns; ++k) got += std::fscanf(f, "%f", &v[k]) == 1;
    if (got != columns) break;
    pts.emplace_back(v[0], v[1], v[2]);
    if (columns >= 6) pts.back().set_normal(Point3D::VectorType(v[3], v[4], v[5]));
    if (columns >= 9) pts.back().set_rgb(Point3D::VectorType(v[6], v[7], v[8]));
    if (tagged) {
      pts.back().set_normal(Point3D::VectorType(float(pts.size()), 0.f, 0.f));       // normalised to (1, 0, 0)
      pts.back().set_rgb(Point3D::VectorType(float(pts.size() - 1), 0.f, 0.f));
    }
  }
  std::fclose(f);
  return pts;
}

static void print_row(std::initializer_list<float> row) {
  const char* sep = "";
  for (float v : row) {
    std::printf("%s%.9g", sep, v);
    sep = " ";
  }
  std::printf("\n");
}

template <class T>
static void print_lines(const std::vector<T>& values) {
  for (T v : values) std::printf("%d\n", int(v));
}

static void print_normals(const Points& pts) {
  for (const Point3D& p : pts) print_row({p.normal()(0), p.normal()(1), p.normal()(2)});
}

static void print_tagged(const Points& pts) {
  for (const Point3D& p : pts) print_row({p.x(), p.y(), p.z(), p.normal()(0), p.rgb()(0)});
}

static void normals(int argc, char** argv) {
  if (argc < 3) throw Usage();
  Points pts = read_points(argv[1], 3);
  NormalEstimationOptions opt;
  opt.k = std::atoi(argv[2]);
  if (argc > 3) opt.radius = std::atof(argv[3]);
  EstimateNormals(pts, opt);
  print_normals(pts);
}

static void outliers(int argc, char** argv) {
  if (argc < 5) throw Usage();
  Points pts = read_points(argv[1], 3, true);
  OutlierRemovalOptions opt;
  if (!std::strcmp(argv[2], "stat")) {
    opt.k = std::atoi(argv[3]);
    opt.std_ratio = std::atof(argv[4]);
  } else {
    opt.radius = std::atof(argv[3]);
    opt.min_neighbours = std::atoi(argv[4]);
  }
  std::vector<uint8_t> kept;
  const size_t removed = RemoveOutliers(pts, opt, &kept);
  std::printf("removed %zu\n", removed);
  print_lines(kept);
  print_tagged(pts);
}

static void voxel(int argc, char** argv) {
  if (argc < 4) throw Usage();
  Points pts = read_points(argv[1], std::strcmp(argv[3], "attrs") ? 3 : 9);
  VoxelGridOptions opt;
  opt.voxel_size = std::atof(argv[2]);
  std::vector<int> voxel_of;
  const size_t m = VoxelDownsample(pts, opt, &voxel_of);
  std::printf("m %zu\n", m);
  print_lines(voxel_of);
  for (const Point3D& p : pts)
    print_row({p.x(), p.y(), p.z(), p.normal()(0), p.normal()(1), p.normal()(2), p.rgb()(0), p.rgb()(1), p.rgb()(2)});
}

static void orient(int argc, char** argv) {
  if (argc != 4 && argc != 7) throw Usage();
  Points pts = read_points(argv[1], 6);
  NormalOrientationOptions opt;
  opt.k = std::atoi(argv[2]);
  opt.radius = std::atof(argv[3]);
  if (argc == 7) {
    opt.use_viewpoint = true;
    for (int a = 0; a < 3; ++a) opt.viewpoint[a] = std::atof(argv[4 + a]);
  }
  const size_t flipped = OrientNormals(pts, opt);
  std::printf("flipped %zu\n", flipped);
  print_normals(pts);
}

static void cluster(int argc, char** argv) {
  if (argc < 6) throw Usage();
  Points pts = read_points(argv[1], 3, true);
  ClusterOptions opt;
  opt.eps = std::atof(argv[2]);
  opt.min_points = std::atoi(argv[3]);
  opt.keep = std::atoi(argv[4]);
  opt.min_size = std::atoi(argv[5]);
  std::vector<int32_t> labels;
  std::vector<uint8_t> kept;
  const size_t clusters = ClusterDBSCAN(pts, opt, labels);
  const size_t removed = KeepLargestClusters(pts, opt, &kept);
  std::printf("clusters %zu\n", clusters);
  print_lines(labels);
  std::printf("removed %zu\n", removed);
  print_lines(kept);
  print_tagged(pts);
}

static void plane(int argc, char** argv) {
  if (argc < 6) throw Usage();
  Points pts = read_points(argv[1], 3, true);
  PlaneOptions opt;
  opt.distance = std::atof(argv[2]);
  opt.trials = std::atoi(argv[3]);
  opt.refine = std::atoi(argv[4]);
  opt.count = std::atoi(argv[5]);
  std::vector<uint8_t> inlier;
  std::vector<PlaneModel> planes;
  const PlaneModel m = SegmentPlane(pts, opt, inlier);
  const size_t removed = RemovePlanes(pts, opt, nullptr, &planes);
  std::printf("plane ");
  print_row({m.normal[0], m.normal[1], m.normal[2], m.d});
  std::printf("inliers %zu\n", m.inliers);
  print_lines(inlier);
  std::printf("removed %zu planes %zu\n", removed, planes.size());
  print_tagged(pts);
}

int main(int argc, char** argv) {
  const struct { const char* word; void (*call)(int, char**); } calls[] = {
      {"normals", normals}, {"outliers", outliers}, {"voxel", voxel}, {"orient", orient}, {"cluster", cluster}, {"plane", plane}};
  try {
    for (const auto& c : calls)
      if (argc > 1 && !std::strcmp(argv[1], c.word)) {
        c.call(argc - 1, argv + 1);
        return 0;
      }
  } catch (const Usage&) {
    return 2;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 2;
}
