// Command-line surface of the Super4PCS program: a table of the flags the reference's binary understands
// (demos/demo-utils.h:119-162: -i -o -d -c -t -a -n -r -m -x --sampled1 --sampled2 -h), with its defaults
// (demo-utils.h:57-101), so that scripts written for it (scripts/run-example.sh:68) run unchanged.
#ifndef S4P_CLI_OPTIONS_H_
#define S4P_CLI_OPTIONS_H_

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <super4pcs/shared4pcs.h>

namespace s4p_cli {

struct Options {
  std::string first = "input1.obj", second = "input2.obj";   // -i P Q
  std::string registered;                                    // -r  second input after registration
  std::string matrix;                                        // -m  Polyworks matrix file
  std::string sampled[2];                                    // --sampled1 / --sampled2
  double overlap = 0.2, delta = 5.0, colour = -1, normal_deg = -1;
  int samples = 200, seconds = 10;
  bool legacy_4pcs = false;                                  // -x
  int icp_iterations = 0;                                    // --icp  ICP refinement after the registration (0: off)
  double icp_distance = -1;                                  // --icp-dist  (default 4 delta)
  bool icp_plane = false;                                    // --icp-metric point|plane|gicp|symmetric|color  (default point)
  bool icp_gicp = false;                                     //   gicp: generalized ICP, normals of both clouds
  bool icp_symm = false;                                     //   symmetric: symmetric ICP, normals of both clouds, no parameter
  bool icp_color = false;                                    //   color: coloured ICP, the colours of both clouds
  double icp_color_lambda = 0.968;                           // --icp-color-lambda l  (color; in [0, 1])
  bool icp_color_lambda_set = false;
  double icp_gicp_epsilon = 1e-3;                            // --icp-gicp-epsilon e  (gicp; in [1e-6, 1])
  bool icp_gicp_epsilon_set = false;
  double icp_normal_radius = -1;                             // --icp-normal-radius  (default: the ICP max distance)
  int icp_loss = 0;                                          // --icp-loss none|trimmed|huber|tukey  (0 1 2 3; default none)
  double icp_trim = -1;                                      // --icp-trim  (trimmed; default: the overlap -o)
  double icp_loss_scale = -1;                                // --icp-loss-scale  (huber / tukey; default: estimated)
  bool icp_trim_set = false, icp_loss_scale_set = false;
  bool icp_reciprocal = false;                               // --icp-reciprocal  keep reciprocal pairs only (needs --icp)
  double icp_normal_angle = -1;                              // --icp-normal-angle deg  reject pairs whose normals differ by more (needs --icp)
  bool icp_normal_angle_set = false;
  std::string icp_information;                               // --icp-information file  the refined pose's 6x6 information matrix (needs --icp)
  int normals_k = 0;                                         // --estimate-normals k  normals of both inputs on the device (0: off)
  double normals_radius = -1;                                // --estimate-normals-radius r  (default: unbounded)
  bool normals_radius_set = false;
  int orient_k = 0;                                          // --orient-normals k  consistent orientation of the estimated normals (0: off)
  bool orient_viewpoint_set = false;                         // --orient-viewpoint x,y,z  (needs --orient-normals; default: outward)
  double orient_viewpoint[3] = {0, 0, 0};
  int outliers_k = 0;                                        // --remove-outliers k  statistical outlier removal of both inputs (0: off)
  double outliers_std = 2.0;                                 // --remove-outliers-std ratio  (needs k)
  bool outliers_std_set = false;
  double voxel_size = -1;                                    // --voxel-size v  voxel-grid downsampling of both inputs (off)
  std::vector<double> icp_scales;                            // --icp-scales v1,v2,...  multi-scale ICP levels, coarse to fine (needs --icp)
  bool icp_scales_set = false;
  int icp_starts = 0;                                        // --icp-starts K  refine the matcher's K best distinct poses in one batch (needs --icp)
  bool icp_starts_set = false;
  double cluster_eps = -1;                                   // --cluster-eps e  keep the largest density clusters of both inputs (off)
  int cluster_min_points = 10;                               // --cluster-min-points m  (needs eps)
  int cluster_keep = 1;                                      // --cluster-keep K  (needs eps)
  bool cluster_min_points_set = false, cluster_keep_set = false;
  double remove_plane = -1;                                  // --remove-plane distance  remove the dominant planes of both inputs (off)
  int remove_plane_trials = 1024;                            // --remove-plane-trials T  (needs distance; 1 .. 2^20)
  int remove_plane_count = 1;                                // --remove-plane-count K  (needs distance)
  bool remove_plane_trials_set = false, remove_plane_count_set = false;
  double normals_within = -1;                                // --estimate-normals-within r  radius normals of both inputs on the device (off)
  int normals_min = 3;                                       // --estimate-normals-min m  (needs r)
  bool normals_min_set = false;
  bool bad_value = false;                                   // a flag's value does not parse
};

enum class Parse { Run, Help, Bad };

// One row per flag: how many values follow and where they go.
struct Flag {
  const char* name;
  int values;
  void (*store)(Options&, char** v);
};

inline const Flag* flag_table(size_t* n) {
  static const Flag table[] = {
      {"-i", 2, [](Options& o, char** v) { o.first = v[0]; o.second = v[1]; }},
      {"-o", 1, [](Options& o, char** v) { o.overlap = std::atof(v[0]); }},
      {"-d", 1, [](Options& o, char** v) { o.delta = std::atof(v[0]); }},
      {"-c", 1, [](Options& o, char** v) { o.colour = std::atof(v[0]); }},
      {"-t", 1, [](Options& o, char** v) { o.seconds = std::atoi(v[0]); }},
      {"-a", 1, [](Options& o, char** v) { o.normal_deg = std::atof(v[0]); }},
      {"-n", 1, [](Options& o, char** v) { o.samples = std::atoi(v[0]); }},
      {"-r", 1, [](Options& o, char** v) { o.registered = v[0]; }},
      {"-m", 1, [](Options& o, char** v) { o.matrix = v[0]; }},
      {"-x", 0, [](Options& o, char**) { o.legacy_4pcs = true; }},
      {"--sampled1", 1, [](Options& o, char** v) { o.sampled[0] = v[0]; }},
      {"--sampled2", 1, [](Options& o, char** v) { o.sampled[1] = v[0]; }},
      {"--icp", 1, [](Options& o, char** v) {
         char* end = nullptr;
         const long n = std::strtol(v[0], &end, 10);
         if (end == v[0] || *end != '\0' || n < 0 || n > 100000) o.bad_value = true; else o.icp_iterations = int(n);
       }},
      {"--icp-dist", 1, [](Options& o, char** v) {
         char* end = nullptr;
         const double d = std::strtod(v[0], &end);
         if (end == v[0] || *end != '\0' || !(d > 0)) o.bad_value = true; else o.icp_distance = d;
       }},
      {"--icp-metric", 1, [](Options& o, char** v) {
         o.icp_plane = o.icp_gicp = o.icp_symm = o.icp_color = false;
         if (!std::strcmp(v[0], "point")) {}
         else if (!std::strcmp(v[0], "plane")) o.icp_plane = true;
         else if (!std::strcmp(v[0], "gicp")) o.icp_gicp = true;
         else if (!std::strcmp(v[0], "symmetric")) o.icp_symm = true;
         else if (!std::strcmp(v[0], "color")) o.icp_color = true;
         else o.bad_value = true;
       }},
      {"--icp-color-lambda", 1, [](Options& o, char** v) {
         char* end = nullptr;
         const double l = std::strtod(v[0], &end);
         o.icp_color_lambda_set = true;
         if (end == v[0] || *end != '\0' || !(l >= 0) || !(l <= 1)) o.bad_value = true; else o.icp_color_lambda = l;
       }},
      {"--icp-gicp-epsilon", 1, [](Options& o, char** v) {
         char* end = nullptr;
         const double e = std::strtod(v[0], &end);
         o.icp_gicp_epsilon_set = true;
         if (end == v[0] || *end != '\0' || !(e >= 1e-6) || !(e <= 1)) o.bad_value = true; else o.icp_gicp_epsilon = e;
       }},
      {"--icp-normal-radius", 1, [](Options& o, char** v) {
         char* end = nullptr;
         const double r = std::strtod(v[0], &end);
         if (end == v[0] || *end != '\0' || !(r > 0) || !std::isfinite(r)) o.bad_value = true; else o.icp_normal_radius = r;
       }},
      {"--icp-loss", 1, [](Options& o, char** v) {
         static const char* names[] = {"none", "trimmed", "huber", "tukey"};
         int hit = -1;
         for (int k = 0; k < 4; ++k) if (!std::strcmp(v[0], names[k])) hit = k;
         if (hit < 0) o.bad_value = true; else o.icp_loss = hit;
       }},
      {"--icp-trim", 1, [](Options& o, char** v) {
         char* end = nullptr;
         const double t = std::strtod(v[0], &end);
         o.icp_trim_set = true;
         if (end == v[0] || *end != '\0' || !(t > 0) || !(t <= 1)) o.bad_value = true; else o.icp_trim = t;
       }},
      {"--icp-loss-scale", 1, [](Options& o, char** v) {
         char* end = nullptr;
         const double s = std::strtod(v[0], &end);
         o.icp_loss_scale_set = true;
         if (end == v[0] || *end != '\0' || !(s > 0) || !std::isfinite(s)) o.bad_value = true; else o.icp_loss_scale = s;
       }},
      {"--icp-reciprocal", 0, [](Options& o, char**) { o.icp_reciprocal = true; }},
      {"--icp-normal-angle", 1, [](Options& o, char** v) {
         char* end = nullptr;
         const double a = std::strtod(v[0], &end);
         o.icp_normal_angle_set = true;
         if (end == v[0] || *end != '\0' || !(a >= 0) || !(a <= 90)) o.bad_value = true; else o.icp_normal_angle = a;
       }},
      {"--icp-information", 1, [](Options& o, char** v) {
         o.icp_information = v[0];
         if (o.icp_information.empty()) o.bad_value = true;
       }},
      {"--estimate-normals", 1, [](Options& o, char** v) {
         char* end = nullptr;
         const long k = std::strtol(v[0], &end, 10);
         if (end == v[0] || *end != '\0' || k < 3 || k > 32) o.bad_value = true; else o.normals_k = int(k);
       }},
      {"--estimate-normals-radius", 1, [](Options& o, char** v) {
         char* end = nullptr;
         const double r = std::strtod(v[0], &end);
         o.normals_radius_set = true;
         if (end == v[0] || *end != '\0' || !(r > 0) || !(r < 3.0e38)) o.bad_value = true; else o.normals_radius = r;
       }},
      {"--orient-normals", 1, [](Options& o, char** v) {
         char* end = nullptr;
         const long k = std::strtol(v[0], &end, 10);
         if (end == v[0] || *end != '\0' || k < 1 || k > 32) o.bad_value = true; else o.orient_k = int(k);
       }},
      {"--orient-viewpoint", 1, [](Options& o, char** v) {
         // x,y,z: three finite numbers that fit a float
         o.orient_viewpoint_set = true;
         const char* p = v[0];
         for (int a = 0; a < 3; ++a) {
           char* end = nullptr;
           const double c = std::strtod(p, &end);
           if (end == p || *end != (a < 2 ? ',' : '\0') || !std::isfinite(c) || !(std::fabs(c) < 3.0e38)) { o.bad_value = true; return; }
           o.orient_viewpoint[a] = c;
           p = end + 1;
         }
       }},
      {"--remove-outliers", 1, [](Options& o, char** v) {
         char* end = nullptr;
         const long k = std::strtol(v[0], &end, 10);
         if (end == v[0] || *end != '\0' || k < 1 || k > 32) o.bad_value = true; else o.outliers_k = int(k);
       }},
      {"--remove-outliers-std", 1, [](Options& o, char** v) {
         char* end = nullptr;
         const double s = std::strtod(v[0], &end);
         o.outliers_std_set = true;
         if (end == v[0] || *end != '\0' || !(s >= 0) || !std::isfinite(s)) o.bad_value = true; else o.outliers_std = s;
       }},
      {"--voxel-size", 1, [](Options& o, char** v) {
         char* end = nullptr;
         const double s = std::strtod(v[0], &end);
         if (end == v[0] || *end != '\0' || !(s > 0) || !(s < 3.0e38) || !(float(s) > 0.f)) o.bad_value = true; else o.voxel_size = s;
       }},
      {"--icp-scales", 1, [](Options& o, char** v) {
         // v1,v2,...: at most 16 sizes, each > 0 and representable as a float, non-increasing; only the last may be 0
         o.icp_scales_set = true;
         o.icp_scales.clear();
         const char* p = v[0];
         for (;;) {
           char* end = nullptr;
           const double s = std::strtod(p, &end);
           const bool last = *end == '\0';
           if (end == p || (*end != ',' && !last) || !(s >= 0) || !(s < 3.0e38) || (s > 0 && !(float(s) > 0.f)) || (s == 0 && !last) ||
               (!o.icp_scales.empty() && s > o.icp_scales.back()) || o.icp_scales.size() >= 16) {
             o.bad_value = true;
             return;
           }
           o.icp_scales.push_back(s);
           if (last) return;
           p = end + 1;
         }
       }},
      {"--icp-starts", 1, [](Options& o, char** v) {
         char* end = nullptr;
         const long k = std::strtol(v[0], &end, 10);
         o.icp_starts_set = true;
         if (end == v[0] || *end != '\0' || k < 1 || k > 64) o.bad_value = true; else o.icp_starts = int(k);
       }},
      {"--cluster-eps", 1, [](Options& o, char** v) {
         // finite, > 0, and with a square that is a finite float
         char* end = nullptr;
         const double e = std::strtod(v[0], &end);
         if (end == v[0] || *end != '\0' || !(e > 0) || !(e < 1.8e19) || !(float(e) > 0.f)) o.bad_value = true; else o.cluster_eps = e;
       }},
      {"--cluster-min-points", 1, [](Options& o, char** v) {
         char* end = nullptr;
         const long m = std::strtol(v[0], &end, 10);
         o.cluster_min_points_set = true;
         if (end == v[0] || *end != '\0' || m < 1 || m > 2147483647L) o.bad_value = true; else o.cluster_min_points = int(m);
       }},
      {"--cluster-keep", 1, [](Options& o, char** v) {
         char* end = nullptr;
         const long k = std::strtol(v[0], &end, 10);
         o.cluster_keep_set = true;
         if (end == v[0] || *end != '\0' || k < 1 || k > 2147483647L) o.bad_value = true; else o.cluster_keep = int(k);
       }},
      {"--remove-plane", 1, [](Options& o, char** v) {
         // finite, >= 0, and a finite float
         char* end = nullptr;
         const double d = std::strtod(v[0], &end);
         if (end == v[0] || *end != '\0' || !(d >= 0) || !(d < 3.0e38)) o.bad_value = true; else o.remove_plane = d;
       }},
      {"--remove-plane-trials", 1, [](Options& o, char** v) {
         char* end = nullptr;
         const long t = std::strtol(v[0], &end, 10);
         o.remove_plane_trials_set = true;
         if (end == v[0] || *end != '\0' || t < 1 || t > 1048576L) o.bad_value = true; else o.remove_plane_trials = int(t);
       }},
      {"--remove-plane-count", 1, [](Options& o, char** v) {
         char* end = nullptr;
         const long k = std::strtol(v[0], &end, 10);
         o.remove_plane_count_set = true;
         if (end == v[0] || *end != '\0' || k < 1 || k > 2147483647L) o.bad_value = true; else o.remove_plane_count = int(k);
       }},
      {"--estimate-normals-within", 1, [](Options& o, char** v) {
         // finite, > 0, and with a square that is a finite float
         char* end = nullptr;
         const double r = std::strtod(v[0], &end);
         if (end == v[0] || *end != '\0' || !(r > 0) || !(r < 1.8e19) || !(float(r) > 0.f)) o.bad_value = true; else o.normals_within = r;
       }},
      {"--estimate-normals-min", 1, [](Options& o, char** v) {
         char* end = nullptr;
         const long m = std::strtol(v[0], &end, 10);
         o.normals_min_set = true;
         if (end == v[0] || *end != '\0' || m < 1 || m > 2147483647L) o.bad_value = true; else o.normals_min = int(m);
       }},
  };
  *n = sizeof(table) / sizeof(table[0]);
  return table;
}

inline Parse parse(Options& o, int argc, char** argv) {
  size_t nflags = 0;
  const Flag* table = flag_table(&nflags);
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "-h")) return Parse::Help;
    const Flag* hit = nullptr;
    for (size_t k = 0; k < nflags && !hit; ++k)
      if (!std::strcmp(argv[i], table[k].name)) hit = &table[k];
    if (!hit) {
      if (argv[i][0] == '-') { std::fputs("Unknown flag\n", stderr); return Parse::Bad; }
      continue;                                   // stray words are ignored, as the reference does
    }
    if (i + hit->values > argc - 1) return Parse::Bad;      // value(s) missing (the reference reads past argv here)
    hit->store(o, argv + i + 1);
    i += hit->values;
  }
  if (o.bad_value) return Parse::Bad;
  if (o.normals_radius_set && o.normals_k == 0) return Parse::Bad;    // the radius needs --estimate-normals
  if (o.outliers_std_set && o.outliers_k == 0) return Parse::Bad;      // the ratio needs --remove-outliers
  if (o.normals_k > 0 && o.normals_within > 0) return Parse::Bad;      // k neighbours or a radius neighbourhood, not both
  if (o.normals_min_set && !(o.normals_within > 0)) return Parse::Bad; // the minimum needs --estimate-normals-within
  if (o.orient_k > 0 && o.normals_k == 0 && !(o.normals_within > 0)) return Parse::Bad;    // --orient-normals needs --estimate-normals or -within
  if (o.orient_viewpoint_set && o.orient_k == 0) return Parse::Bad;    // --orient-viewpoint needs --orient-normals
  if ((o.cluster_min_points_set || o.cluster_keep_set) && !(o.cluster_eps > 0)) return Parse::Bad;    // both need --cluster-eps
  if ((o.remove_plane_trials_set || o.remove_plane_count_set) && !(o.remove_plane >= 0)) return Parse::Bad;    // both need --remove-plane
  if (o.icp_trim_set && o.icp_loss != 1) return Parse::Bad;            // --icp-trim needs --icp-loss trimmed
  if (o.icp_loss_scale_set && o.icp_loss < 2) return Parse::Bad;       // --icp-loss-scale needs huber or tukey
  if (o.icp_gicp && o.icp_loss != 0) return Parse::Bad;                // the generalized metric takes no loss
  if (o.icp_gicp_epsilon_set && !o.icp_gicp) return Parse::Bad;        // --icp-gicp-epsilon needs --icp-metric gicp
  if (o.icp_symm && o.icp_loss != 0) return Parse::Bad;                // the symmetric metric takes no loss
  if (o.icp_color && o.icp_loss != 0) return Parse::Bad;               // the coloured metric takes no loss
  if (o.icp_color_lambda_set && !o.icp_color) return Parse::Bad;       // --icp-color-lambda needs --icp-metric color
  if (o.icp_scales_set && o.icp_iterations == 0) return Parse::Bad;    // --icp-scales needs --icp
  if ((o.icp_reciprocal || o.icp_normal_angle_set) && o.icp_iterations == 0) return Parse::Bad;    // pair rejection needs --icp
  if (o.icp_starts_set && o.icp_iterations == 0) return Parse::Bad;    // --icp-starts needs --icp
  if (!o.icp_information.empty() && o.icp_iterations == 0) return Parse::Bad;    // --icp-information needs --icp
  // the batch refines point and plane only, without a loss and without pair rejection
  if (o.icp_starts_set && (o.icp_loss != 0 || o.icp_gicp || o.icp_symm || o.icp_color || o.icp_reciprocal || o.icp_normal_angle_set)) return Parse::Bad;
  // neither geometry nor matrix requested: write the registered geometry under the reference's default name
  if (o.registered.empty() && o.matrix.empty()) o.registered = "output.obj";
  return Parse::Run;
}

inline void usage(const Options& o, const char* prog, bool all) {
  std::fprintf(stderr, "\nUsage: %s -i input1 input2\n", prog);
  std::fprintf(stderr, "Parameter list:\n");
  std::fprintf(stderr, "\t[ -o overlap (%2.2f) ]\n\t[ -d delta (%2.2f) ]\n\t[ -n n_points (%d) ]\n", o.overlap, o.delta, o.samples);
  std::fprintf(stderr, "\t[ -a norm_diff (%f) ]\n\t[ -c max_color_diff (%f) ]\n\t[ -t max_time_seconds (%d) ]\n", o.normal_deg, o.colour, o.seconds);
  if (!all) return;
  std::fprintf(stderr, "\t[ -r result_file_name (%s) ]\n\t[ -m output matrix file (%s) ]\n", o.registered.c_str(), o.matrix.c_str());
  std::fprintf(stderr, "\t[ -x (legacy 4PCS: not available in this build) ]\n");
  std::fprintf(stderr, "\t[ --sampled1 file ] [ --sampled2 file ]  (sampled clouds)\n");
  std::fprintf(stderr, "\t[ --icp iterations (%d: off) ] [ --icp-dist max_distance (4 delta) ]  (ICP refinement)\n", o.icp_iterations);
  std::fprintf(stderr, "\t[ --icp-metric point|plane|gicp|symmetric|color (point) ] [ --icp-normal-radius r (max_distance) ]  (ICP metric)\n");
  std::fprintf(stderr, "\t[ --icp-gicp-epsilon e (gicp; 0.001, in [1e-6, 1]; gicp takes no --icp-loss) ]\n");
  std::fprintf(stderr, "\t    (symmetric: point-to-plane along the sum of both inputs' normals, obtained as for gicp; no parameter, no --icp-loss,\n");
  std::fprintf(stderr, "\t     no --icp-starts)\n");
  std::fprintf(stderr, "\t[ --icp-color-lambda l (color; 0.968, in [0, 1]: the weight of the geometric term; color needs coloured\n");
  std::fprintf(stderr, "\t    inputs and takes no --icp-loss) ]\n");
  std::fprintf(stderr, "\t[ --icp-loss none|trimmed|huber|tukey (none) ] [ --icp-trim fraction (trimmed; -o) ]\n");
  std::fprintf(stderr, "\t[ --icp-loss-scale s (huber, tukey; estimated) ]  (robust ICP)\n");
  std::fprintf(stderr, "\t[ --icp-reciprocal ] [ --icp-normal-angle deg (in [0, 90]; off) ]  (pair rejection, needs --icp, any metric and loss:\n");
  std::fprintf(stderr, "\t    keep a pair only when it is nearest in both directions / when its normals, up to sign, differ by at most deg)\n");
  std::fprintf(stderr, "\t[ --icp-information file (needs --icp: the final pose in double, its 6x6 information matrix over the matched points of\n");
  std::fprintf(stderr, "\t    input1, their count and the rmse; the edge of this pair in a pose graph) ]\n");
  std::fprintf(stderr, "\t[ --estimate-normals k (3..32; off) ] [ --estimate-normals-radius r (needs k; unbounded) ]\n");
  std::fprintf(stderr, "\t    (kNN normals of both inputs on the device, replacing the files' normals, before matching: -a filters on\n");
  std::fprintf(stderr, "\t     them and --icp-metric plane / gicp / symmetric / color use P's (gicp, symmetric: Q's too) when all are nonzero)\n");
  std::fprintf(stderr, "\t[ --remove-outliers k (1..32; off) ] [ --remove-outliers-std ratio (needs k; 2.0, >= 0) ]\n");
  std::fprintf(stderr, "\t    (statistical outlier removal of both inputs on the device, right after loading: a point is kept when the mean\n");
  std::fprintf(stderr, "\t     distance to its k nearest others is at most mean + ratio * stddev over the cloud; point sets only, -r writes\n");
  std::fprintf(stderr, "\t     the filtered input2)\n");
  std::fprintf(stderr, "\t[ --voxel-size v (> 0; off) ]\n");
  std::fprintf(stderr, "\t    (voxel-grid downsampling of both inputs on the device, after --remove-outliers and before --estimate-normals:\n");
  std::fprintf(stderr, "\t     one point per occupied voxel of edge v, the mean of its members; point sets only, -r writes the\n");
  std::fprintf(stderr, "\t     downsampled input2)\n");
  std::fprintf(stderr, "\t[ --icp-scales v1,v2,... (needs --icp; off) ]\n");
  std::fprintf(stderr, "\t    (multi-scale ICP: one level per voxel size, coarse to fine, non-increasing, the last may be 0 = the inputs as\n");
  std::fprintf(stderr, "\t     they are; level distance max(--icp-dist, 3 v), --icp iterations per level)\n");
  std::fprintf(stderr, "\t[ --icp-starts K (1..64, needs --icp; off) ]\n");
  std::fprintf(stderr, "\t    (multi-start ICP: the matcher's K best distinct poses, its own result first, refined in one batch; the one with\n");
  std::fprintf(stderr, "\t     the most correspondences on the full clouds, then the least rmse, is kept; --icp-metric point or plane only, no\n");
  std::fprintf(stderr, "\t     --icp-loss, no pair rejection; with --icp-scales the batch is the coarsest level)\n");
  std::fprintf(stderr, "\t[ --orient-normals k (1..32, needs --estimate-normals; off) ] [ --orient-viewpoint x,y,z (needs --orient-normals; outward) ]\n");
  std::fprintf(stderr, "\t    (one consistent sign for the estimated normals of each input, right after the estimation: signs spread over the\n");
  std::fprintf(stderr, "\t     graph of the k nearest neighbours from an anchor that faces away from the centre of the input's bounds, or faces\n");
  std::fprintf(stderr, "\t     the viewpoint, the same coordinates in each file's own frame: that suits scans taken from the origin; then\n");
  std::fprintf(stderr, "\t     --icp-normal-angle compares the normals with their sign, in [0, 90] degrees)\n");
  std::fprintf(stderr, "\t[ --cluster-eps e (> 0; off) ] [ --cluster-min-points m (needs e; 10, >= 1) ] [ --cluster-keep K (needs e; 1, >= 1) ]\n");
  std::fprintf(stderr, "\t    (density clustering of both inputs on the device, after --voxel-size and before --estimate-normals: a point with\n");
  std::fprintf(stderr, "\t     at least m points within e, itself included, is a core point, core points within e of each other share a\n");
  std::fprintf(stderr, "\t     cluster, and the K largest clusters stay: a dense fragment away from the surface goes, which\n");
  std::fprintf(stderr, "\t     --remove-outliers keeps; point sets only, -r writes the filtered input2)\n");
  std::fprintf(stderr, "\t[ --remove-plane d (>= 0; off) ] [ --remove-plane-trials T (needs d; 1024, 1..1048576) ] [ --remove-plane-count K (needs d; 1, >= 1) ]\n");
  std::fprintf(stderr, "\t    (RANSAC plane removal of both inputs on the device, after --voxel-size and before --cluster-eps: of T sampled\n");
  std::fprintf(stderr, "\t     planes the one with the most points within d wins, is refitted once to them by least squares and goes with\n");
  std::fprintf(stderr, "\t     them, K times: the ground of a scan, through which --cluster-eps would join the scene; point sets only, -r\n");
  std::fprintf(stderr, "\t     writes the filtered input2)\n");
  std::fprintf(stderr, "\t[ --estimate-normals-within r (> 0; off) ] [ --estimate-normals-min m (needs r; 3, >= 1) ]\n");
  std::fprintf(stderr, "\t    (radius normals of both inputs on the device, where --estimate-normals stands and instead of it: every point\n");
  std::fprintf(stderr, "\t     within r is a neighbour, hundreds on a dense scan where 32 lie inside the noise; a point with fewer than\n");
  std::fprintf(stderr, "\t     max(3, m) gets no normal; --orient-normals may follow)\n");
}

// false: the overlap / terminate-threshold pair is inconsistent (Match4PCSOptions::configureOverlap)
inline bool to_matcher_options(const Options& o, GlobalRegistration::Match4PCSOptions& m) {
  using Scalar = GlobalRegistration::Match4PCSOptions::Scalar;
  if (!m.configureOverlap(Scalar(o.overlap))) return false;
  m.delta = Scalar(o.delta);
  m.sample_size = size_t(o.samples);
  m.max_time_seconds = o.seconds;
  m.max_normal_difference = Scalar(o.normal_deg);
  m.max_color_distance = Scalar(o.colour);
  return true;
}

}  // namespace s4p_cli
#endif
