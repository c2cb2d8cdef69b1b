// Super4PCS, the command-line program, on the MI355X path.  Drop-in for the reference's binary
// (demos/Super4PCS/super4pcs_test.cc; usage in doc/Usage.md and scripts/run-example.sh:68): same flags, same files in
// and out (io/io.h), same exit statuses -- 254 (-2) usage / runtime error, 1 help or unknown flag, 253 (-3) bad
// options, 255 (-1) unreadable input.
//   Super4PCS -i P.obj Q.obj [-o overlap] [-d delta] [-n samples] [-t seconds] [-a normal_deg] [-c colour]
//             [-r registered_geometry] [-m polyworks_matrix] [--sampled1 file] [--sampled2 file]
//             [--icp iterations] [--icp-dist max_distance] [--icp-metric point|plane|gicp|symmetric|color] [--icp-normal-radius r]
//             [--icp-gicp-epsilon e] [--icp-color-lambda l]
//             [--icp-loss none|trimmed|huber|tukey] [--icp-trim fraction] [--icp-loss-scale s]
//             [--estimate-normals k] [--estimate-normals-radius r] [--orient-normals k] [--orient-viewpoint x,y,z]
//             [--remove-outliers k] [--remove-outliers-std ratio]
//             [--voxel-size v] [--icp-scales v1,v2,...] [--icp-starts K] [--icp-information file]
//             [--cluster-eps e] [--cluster-min-points m] [--cluster-keep K]
//             [--remove-plane d] [--remove-plane-trials T] [--remove-plane-count K]
//             [--estimate-normals-within r] [--estimate-normals-min m]
// --icp N refines the registration by point-to-point ICP on the full clouds (algorithms/icp.h) before -m / -r are written;
// with --icp-metric plane it minimises point-to-plane distances (P's normals, or normals estimated within r).
// With --icp-metric gicp it is generalized ICP (include/s4p_icp_gicp.h, covariance parameter --icp-gicp-epsilon): P's
// normals as for plane, Q's own when all are nonzero (after --estimate-normals they are), else estimated with k = 16; no --icp-loss.
// With --icp-metric symmetric it is symmetric ICP (include/s4p_icp_symm.h): point-to-plane along the sum of both normals, the
// normals of both inputs as for gicp; no parameter, no --icp-loss, no --icp-starts.
// With --icp-metric color it is coloured ICP (include/s4p_icp_color.h, weight of the geometric term --icp-color-lambda): P's
// normals as for plane, the colours of both inputs (a coloured PLY or a PTX), gradients within --icp-normal-radius; no --icp-loss.
// --icp-loss refines with a robust loss (include/s4p_icp_robust.h): trimmed keeps the --icp-trim fraction of |Q| (default
// the overlap -o) with the smallest residuals, huber / tukey reweight with --icp-loss-scale (default estimated on the device).
// --estimate-normals k gives both inputs k-nearest-neighbour normals (algorithms/normals.h, within r if given) before the
// matcher runs, replacing the normals read from the files for matching only (-r writes the files' own): -a then filters on
// them, and --icp-metric plane uses P's when all of them are nonzero.
// --orient-normals k (needs --estimate-normals) gives the estimated normals of each input one consistent sign
// (algorithms/normals.h, OrientNormals: include/s4p_normals_orient.h) right after the estimation: outward, or, with
// --orient-viewpoint x,y,z, facing that position, taken in each file's own coordinates (scans taken from the origin).  With it
// an --icp-normal-angle filter compares the normals with their sign (ICPOptions::normals_oriented).
// --remove-outliers k removes the statistical outliers of both inputs (algorithms/outliers.h: mean distance to the k nearest
// other points above mean + ratio * stddev, ratio --remove-outliers-std, default 2) right after loading, before
// --estimate-normals, the matcher and ICP; -r then writes the filtered, registered second input.  Faces index the vertex
// list, so an input with faces is refused (exit status 254).
// --voxel-size v replaces both inputs by the means of their occupied voxels of edge v (algorithms/voxelgrid.h) after
// --remove-outliers and before --estimate-normals, the matcher and ICP; normals and colours are averaged when every point
// has one; -r then writes the downsampled, registered second input.  An input with faces is refused (exit status 254).
// --cluster-eps e keeps the --cluster-keep K (default 1) largest density clusters of both inputs (algorithms/cluster.h:
// DBSCAN with the radius e and --cluster-min-points m, default 10) after --voxel-size, where the density is even and e is
// easiest to choose, and before --estimate-normals, the matcher and ICP: a dense fragment away from the surface goes, which
// --remove-outliers keeps; -r then writes the filtered, registered second input.  An input with faces, or one left with no
// cluster, is refused (exit status 254).
// --remove-plane d removes the --remove-plane-count K (default 1) dominant planes of both inputs (algorithms/plane.h: RANSAC with
// --remove-plane-trials T candidates, default 1024, inliers within d, one least-squares refit) after --voxel-size and before
// --cluster-eps, which would otherwise join a scanned scene through its ground; -r then writes the filtered, registered
// second input.  An input with faces, or one left with fewer than 3 points, is refused (exit status 254).
// --estimate-normals-within r gives both inputs radius normals (algorithms/shape.h: every point within r is a neighbour, a point
// with fewer than max(3, --estimate-normals-min m) gets none) at the place and in the stead of --estimate-normals, which takes at
// most 32 neighbours; the two together are a usage error, and --orient-normals may follow either.
// --icp-scales v1,v2,... (needs --icp) refines coarse to fine (algorithms/icp_multiscale.h): one level per voxel size, both
// inputs downsampled at it (the second in its own frame; 0, allowed last, takes them as they are), the level's distance
// max(--icp-dist, 3 v) and --icp iterations per level; every --icp-metric and --icp-loss applies to every level.
// --icp-starts K (needs --icp; K in 1..64) refines several start poses in one batch (algorithms/icp_batch.h): the matcher runs
// with a TopPoses(K, 10 degrees, 2 x the ICP distance) listener, its own result is start 0 and its other distinct candidates of
// greatest LCP follow; RefineICPBatch keeps the pose with the most correspondences on the full clouds (then the least rmse), so
// the outcome never has fewer correspondences than --icp alone.  Point and plane metrics only, no --icp-loss, no pair
// rejection.  With --icp-scales the batch runs on the coarsest level's clouds and the other levels follow from its pose.
// --icp-information file (needs --icp) writes, next to what -m writes, the final pose T (the printed matrix, widened to double),
// the 6x6 information matrix of algorithms/icp_information.h for the second input in its own frame under T (after
// --remove-outliers / --voxel-size; --icp-dist and the pair rejection flags hold), the matched count and the rmse, every number
// as %.17g: the edge of this pair in a pose graph (algorithms/posegraph.h), so that a graph can be assembled from pairwise runs.
// -x (the legacy 4PCS matcher, algorithms/4pcs.cc) is outside this library and is refused.
#include <cstdio>
#include <exception>
#include <stdexcept>
#include <string>
#include <vector>

#include "super4pcs/algorithms/cluster.h"
#include "super4pcs/algorithms/icp.h"
#include "super4pcs/algorithms/icp_batch.h"
#include "super4pcs/algorithms/icp_information.h"
#include "super4pcs/algorithms/icp_multiscale.h"
#include "super4pcs/algorithms/normals.h"
#include "super4pcs/algorithms/outliers.h"
#include "super4pcs/algorithms/plane.h"
#include "super4pcs/algorithms/shape.h"
#include "super4pcs/algorithms/super4pcs.h"
#include "super4pcs/algorithms/voxelgrid.h"
#include "super4pcs/io/io.h"
#include "super4pcs/utils/geometry.h"

#include "../cli_options.h"

namespace {

using namespace GlobalRegistration;

struct Mesh {                                    // everything IOManager returns for one file
  std::vector<Point3D> points;
  std::vector<IOManager::TexCoord> tex;
  std::vector<Point3D::VectorType> normals;
  std::vector<tripple> faces;
  std::vector<std::string> materials;

  bool load(IOManager& io, const std::string& path) {
    if (!io.ReadObject(path.c_str(), points, tex, normals, faces, materials)) return false;
    if (faces.empty()) Utils::CleanInvalidNormals(points, normals);   // point sets only: faces index the vertex list
    return true;
  }
  // a filter that erases points in place and reports which it kept: per-vertex normal and texture lists follow the vertices
  template <class Erase>
  size_t filtered(Erase erase) {
    const size_t before = points.size();
    std::vector<uint8_t> kept;
    const size_t removed = erase(points, &kept);
    compact(normals, kept, before);
    compact(tex, kept, before);
    return removed;
  }
  // a per-vertex list (one entry per point before the filter) without the entries of the removed points
  template <class List>
  static void compact(List& list, const std::vector<uint8_t>& kept, size_t before) {
    if (list.size() != before) return;
    size_t w = 0;
    for (size_t i = 0; i < before; ++i)
      if (kept[i]) list[w++] = list[i];
    list.resize(w);
  }
  // statistical outlier removal of the points
  size_t remove_outliers(const OutlierRemovalOptions& oopt) {
    return filtered([&](std::vector<Point3D>& pts, std::vector<uint8_t>* kept) { return RemoveOutliers(pts, oopt, kept); });
  }
  // the largest density clusters of the points
  size_t keep_clusters(const ClusterOptions& copt) {
    return filtered([&](std::vector<Point3D>& pts, std::vector<uint8_t>* kept) { return KeepLargestClusters(pts, copt, kept); });
  }
  // the points without their dominant planes
  size_t remove_planes(const PlaneOptions& popt) {
    return filtered([&](std::vector<Point3D>& pts, std::vector<uint8_t>* kept) { return RemovePlanes(pts, popt, kept); });
  }
  // voxel-grid downsampling of the points; the per-vertex normal list is rebuilt from the averaged normals when they were
  // carried (every point had one), the texture list does not survive
  size_t voxel_downsample(const VoxelGridOptions& vopt) {
    const size_t m = VoxelDownsample(points, vopt);
    bool carried = !points.empty() && normals.size() != 0;
    for (const Point3D& pt : points) carried = carried && (pt.normal()(0) != 0 || pt.normal()(1) != 0 || pt.normal()(2) != 0);
    normals.clear();
    if (carried) for (const Point3D& pt : points) normals.push_back(pt.normal());
    tex.clear();
    return m;
  }
  bool save(IOManager& io, const std::string& path) const {
    return io.WriteObject(path.c_str(), points, tex, normals, faces, materials);
  }
};

bool save_points(IOManager& io, const std::string& path, const std::vector<Point3D>& pts) {
  Mesh m;
  m.points = pts;
  return m.save(io, path);
}

// Progress and TopPoses together: one visitor for the matcher
struct ProgressAndPoses {
  const TopPoses* top;
  inline void operator()(float fraction, float best_lcp, Match4PCSBase::MatrixRef T) const {
    if (fraction < 0) { (*top)(fraction, best_lcp, T); return; }
    std::printf("done: %d%c best: %f                  \r", int(fraction * 100), '%', best_lcp);
    std::fflush(stdout);
  }
  constexpr bool needsGlobalTransformation() const { return true; }
};

// progress line while the matcher runs: one call per trial with the fraction done; per-candidate calls carry -1
struct Progress {
  inline void operator()(float fraction, float best_lcp, Match4PCSBase::MatrixRef) const {
    if (fraction < 0) return;
    std::printf("done: %d%c best: %f                  \r", int(fraction * 100), '%', best_lcp);
    std::fflush(stdout);
  }
  constexpr bool needsGlobalTransformation() const { return false; }
};

int run(const s4p_cli::Options& opt, const Utils::Logger& log) {
  Match4PCSOptions mopt;
  if (!s4p_cli::to_matcher_options(opt, mopt)) {
    log.Log<Utils::ErrorReport>("Invalid overlap configuration. ABORT");
    return -3;
  }
  if (opt.legacy_4pcs) {
    log.Log<Utils::ErrorReport>("-x: the legacy 4PCS matcher is not part of this library (Super4PCS only)");
    return -3;
  }
  IOManager io;
  Mesh P, Q;
  if (!P.load(io, opt.first)) { log.Log<Utils::ErrorReport>("Can't read input set1"); return -1; }
  if (!Q.load(io, opt.second)) { log.Log<Utils::ErrorReport>("Can't read input set2"); return -1; }

  Match4PCSBase::MatrixType mat = Match4PCSBase::MatrixType::Identity();
  float score = 0.f;
  if (opt.outliers_k > 0 && (!P.faces.empty() || !Q.faces.empty())) {
    log.Log<Utils::ErrorReport>("--remove-outliers: an input has faces; faces index the vertex list, so only point sets can be filtered");
    return -2;
  }
  if (opt.voxel_size > 0 && (!P.faces.empty() || !Q.faces.empty())) {
    log.Log<Utils::ErrorReport>("--voxel-size: an input has faces; faces index the vertex list, so only point sets can be downsampled");
    return -2;
  }
  if (opt.remove_plane >= 0 && (!P.faces.empty() || !Q.faces.empty())) {
    log.Log<Utils::ErrorReport>("--remove-plane: an input has faces; faces index the vertex list, so only point sets can be filtered");
    return -2;
  }
  if (opt.cluster_eps > 0 && (!P.faces.empty() || !Q.faces.empty())) {
    log.Log<Utils::ErrorReport>("--cluster-eps: an input has faces; faces index the vertex list, so only point sets can be filtered");
    return -2;
  }
  try {
    if (opt.outliers_k > 0) {
      OutlierRemovalOptions oopt;
      oopt.k = opt.outliers_k;
      oopt.std_ratio = opt.outliers_std;
      const size_t rp = P.remove_outliers(oopt), rq = Q.remove_outliers(oopt);
      log.Log<Utils::Verbose>("Removed outliers: k ", opt.outliers_k, ", ratio ", opt.outliers_std, ": ", rp, " of input1, ", rq, " of input2");
    }
    if (opt.voxel_size > 0) {
      VoxelGridOptions vopt;
      vopt.voxel_size = opt.voxel_size;
      const size_t np = P.points.size(), nq = Q.points.size();
      const size_t mp = P.voxel_downsample(vopt), mq = Q.voxel_downsample(vopt);
      log.Log<Utils::Verbose>("Voxel grid: edge ", opt.voxel_size, ": ", mp, " of ", np, " points of input1, ", mq, " of ", nq, " of input2");
    }
    if (opt.remove_plane >= 0) {
      PlaneOptions popt;
      popt.distance = opt.remove_plane;
      popt.trials = opt.remove_plane_trials;
      popt.count = opt.remove_plane_count;
      const size_t rp = P.remove_planes(popt), rq = Q.remove_planes(popt);
      log.Log<Utils::Verbose>("Removed planes: distance ", opt.remove_plane, ", trials ", opt.remove_plane_trials, ", count ", opt.remove_plane_count,
                              ": removed ", rp, " of input1, ", rq, " of input2");
      if (P.points.size() < 3 || Q.points.size() < 3)
        throw std::runtime_error(std::string("--remove-plane: fewer than 3 points are left of ") + (P.points.size() < 3 ? "input1" : "input2") +
                                 " at this distance; nothing is left to register");
    }
    if (opt.cluster_eps > 0) {
      ClusterOptions copt;
      copt.eps = opt.cluster_eps;
      copt.min_points = opt.cluster_min_points;
      copt.keep = opt.cluster_keep;
      const size_t rp = P.keep_clusters(copt), rq = Q.keep_clusters(copt);
      log.Log<Utils::Verbose>("Kept clusters: eps ", opt.cluster_eps, ", min points ", opt.cluster_min_points, ", keep ", opt.cluster_keep, ": removed ",
                              rp, " of input1, ", rq, " of input2");
      if (P.points.empty() || Q.points.empty())
        throw std::runtime_error(std::string("--cluster-eps: no cluster in ") + (P.points.empty() ? "input1" : "input2") +
                                 " at this eps and --cluster-min-points; nothing is left to register");
    }
    if (opt.normals_k > 0) {
      NormalEstimationOptions nopt;
      nopt.k = opt.normals_k;
      nopt.radius = opt.normals_radius;
      EstimateNormals(P.points, nopt);
      EstimateNormals(Q.points, nopt);
      log.Log<Utils::Verbose>("Estimated normals: k ", opt.normals_k, ", radius ", opt.normals_radius);
    }
    if (opt.normals_within > 0) {
      RadiusNormalOptions ropt;
      ropt.radius = opt.normals_within;
      ropt.min_neighbours = opt.normals_min;
      const size_t zp = EstimateNormalsRadius(P.points, ropt), zq = EstimateNormalsRadius(Q.points, ropt);
      log.Log<Utils::Verbose>("Estimated normals within radius ", opt.normals_within, ", min neighbours ", opt.normals_min, ": ", zp,
                              " points of input1 without a normal, ", zq, " of input2");
    }
    if (opt.orient_k > 0) {
      NormalOrientationOptions oopt;
      oopt.k = opt.orient_k;
      oopt.use_viewpoint = opt.orient_viewpoint_set;
      for (int a = 0; a < 3; ++a) oopt.viewpoint[a] = opt.orient_viewpoint[a];
      const size_t fp = OrientNormals(P.points, oopt), fq = OrientNormals(Q.points, oopt);
      log.Log<Utils::Verbose>("Oriented normals: k ", opt.orient_k, opt.orient_viewpoint_set ? ", towards the viewpoint: " : ", outward: ", fp,
                              " of input1 flipped, ", fq, " of input2");
    }
    std::vector<Point3D> Q0;                                // the second input in its own frame: the matcher moves Q.points
    if (opt.icp_iterations > 0 && !opt.icp_scales.empty()) Q0 = Q.points;
    std::vector<Point3D> Qown;                              // --icp-information: the same, kept as it is
    if (!opt.icp_information.empty()) Qown = Q.points;
    const double icp_distance = opt.icp_distance > 0 ? opt.icp_distance : 4.0 * opt.delta;
    MatchSuper4PCS matcher(mopt, log);
    log.Log<Utils::Verbose>("Use Super4PCS");
    std::vector<Match4PCSBase::MatrixType> starts;           // --icp-starts: relative to Q as the matcher leaves it
    if (opt.icp_starts > 0) {
      const TopPoses top(opt.icp_starts, 10.0, 2.0 * icp_distance, TopPoses::Centroid(Q.points));
      score = matcher.ComputeTransformation(P.points, &Q.points, mat, Sampling::UniformDistSampler(), ProgressAndPoses{&top});
      starts = top.StartsAfter(mat);
      log.Log<Utils::Verbose>("ICP starts: ", starts.size(), " of ", top.arrivals(), " candidates (the matcher's own first)");
    } else {
      score = matcher.ComputeTransformation(P.points, &Q.points, mat, Sampling::UniformDistSampler(), Progress());
    }
    const std::vector<Point3D>* sampled[2] = {&matcher.getFirstSampled(), &matcher.getSecondSampled()};
    for (int k = 0; k < 2; ++k) {
      if (opt.sampled[k].empty()) continue;
      log.Log<Utils::Verbose>("Exporting Sampled cloud ", k + 1, " to ", opt.sampled[k].c_str(), " ...");
      save_points(io, opt.sampled[k], *sampled[k]);
    }
    if (opt.icp_iterations > 0) {
      ICPOptions icp;
      icp.max_iterations = opt.icp_iterations;
      icp.max_distance = icp_distance;
      icp.metric = opt.icp_gicp ? ICPMetric::Generalized : (opt.icp_plane ? ICPMetric::PointToPlane : ICPMetric::PointToPoint);
      if (opt.icp_symm) icp.metric = ICPMetric::Symmetric;
      if (opt.icp_color) icp.metric = ICPMetric::Colored;
      icp.color_lambda = opt.icp_color_lambda;
      icp.gicp_epsilon = opt.icp_gicp_epsilon;
      icp.normal_radius = opt.icp_normal_radius;
      icp.loss = opt.icp_loss == 1 ? ICPLoss::Trimmed : (opt.icp_loss == 2 ? ICPLoss::Huber : (opt.icp_loss == 3 ? ICPLoss::Tukey : ICPLoss::None));
      icp.trim_fraction = opt.icp_trim > 0 ? opt.icp_trim : opt.overlap;
      icp.loss_scale = opt.icp_loss_scale;
      icp.reciprocal = opt.icp_reciprocal;
      icp.normal_angle_deg = opt.icp_normal_angle;
      icp.normals_oriented = opt.orient_k > 0;
      if (!opt.icp_scales.empty()) {
        std::vector<ICPLevel> levels;
        for (double v : opt.icp_scales) {
          ICPLevel level;
          level.voxel_size = v;
          level.max_distance = icp.max_distance > 3.0 * v ? icp.max_distance : 3.0 * v;
          level.max_iterations = opt.icp_iterations;
          levels.push_back(level);
        }
        std::vector<ICPResult> res;
        if (!starts.empty()) {
          // the coarsest level as a batch on its clouds (RefineICPMultiScale's order: downsample, move by mat, refine),
          // then the remaining levels from the pose it picked
          std::vector<Point3D> Pl = P.points, Ql = Q0;
          if (levels[0].voxel_size > 0) {
            VoxelGridOptions vopt;
            vopt.voxel_size = levels[0].voxel_size;
            VoxelDownsample(Pl, vopt);
            VoxelDownsample(Ql, vopt);
          }
          detail::icp_move_points(Ql, mat);
          ICPOptions lopt = icp;
          lopt.max_distance = levels[0].max_distance;
          lopt.max_iterations = levels[0].max_iterations;
          std::vector<ICPResult> bres;
          const auto best = RefineICPBatch(Pl, &Ql, starts, lopt, &bres);
          mat = Compose(best.first, mat);
          log.Log<Utils::Verbose>("ICP best pose: start ", best.second, " of ", starts.size(), ", correspondences ",
                                  bres[size_t(best.second)].n_corr, " (start 0: ", bres[0].n_corr, ")");
          const ICPLevel first = levels[0];
          levels.erase(levels.begin());
          std::vector<ICPResult> rest;
          if (!levels.empty()) RefineICPMultiScale(P.points, &Q0, mat, icp, levels, &rest);
          else detail::icp_move_points(Q0, mat);
          levels.insert(levels.begin(), first);
          res.push_back(bres[size_t(best.second)]);
          res.insert(res.end(), rest.begin(), rest.end());
        } else {
          RefineICPMultiScale(P.points, &Q0, mat, icp, levels, &res);
        }
        for (size_t i = 0; i < Q0.size(); ++i) Q.points[i].pos() = Q0[i].pos();
        for (size_t l = 0; l < res.size(); ++l)
          log.Log<Utils::Verbose>("ICP level ", l, " (voxel ", levels[l].voxel_size, ", distance ", levels[l].max_distance, "): ",
                                  res[l].iterations, " iterations, rmse ", res[l].rmse, ", fitness ", res[l].fitness);
      } else if (!starts.empty()) {
        std::vector<ICPResult> bres;
        const auto best = RefineICPBatch(P.points, &Q.points, starts, icp, &bres);
        mat = Compose(best.first, mat);
        const ICPResult& res = bres[size_t(best.second)];
        log.Log<Utils::Verbose>("ICP best pose: start ", best.second, " of ", starts.size(), ", correspondences ", res.n_corr,
                                " (start 0: ", bres[0].n_corr, ")");
        log.Log<Utils::Verbose>("ICP: ", res.iterations, " iterations, rmse ", res.rmse, ", fitness ", res.fitness);
      } else {
        ICPResult res;
        RefineICP(P.points, &Q.points, mat, icp, &res);
        log.Log<Utils::Verbose>("ICP: ", res.iterations, " iterations, rmse ", res.rmse, ", fitness ", res.fitness);
      }
      if (!opt.icp_information.empty()) {
        double T16[16], info[36], rmse = 0.0;
        int64_t n = 0;
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) T16[4 * r + c] = double(mat(r, c));
        ICPInformation(P.points, Qown, T16, icp, info, &n, &rmse);
        log.Log<Utils::Verbose>("Exporting Information matrix to ", opt.icp_information.c_str(), " (", n, " matched points) ...");
        FILE* f = std::fopen(opt.icp_information.c_str(), "w");
        if (!f) throw std::runtime_error("--icp-information: cannot write " + opt.icp_information);
        std::fprintf(f, "VERSION\t=\t1\nPOSE\t=\n");
        for (int r = 0; r < 4; ++r) std::fprintf(f, "%.17g %.17g %.17g %.17g\n", T16[4 * r], T16[4 * r + 1], T16[4 * r + 2], T16[4 * r + 3]);
        std::fprintf(f, "INFORMATION\t=\n");
        for (int r = 0; r < 6; ++r)
          std::fprintf(f, "%.17g %.17g %.17g %.17g %.17g %.17g\n", info[6 * r], info[6 * r + 1], info[6 * r + 2], info[6 * r + 3], info[6 * r + 4],
                       info[6 * r + 5]);
        std::fprintf(f, "CORRESPONDENCES\t=\t%lld\nRMSE\t=\t%.17g\n", (long long)n, rmse);
        std::fclose(f);
      }
    }
  } catch (const std::exception& e) {
    log.Log<Utils::ErrorReport>("[Error]: ", e.what());
    log.Log<Utils::ErrorReport>("Aborting with code -2 ...");
    return -2;
  } catch (...) {
    log.Log<Utils::ErrorReport>("[Unknown Error]: Aborting with code -3 ...");
    return -3;
  }

  log.Log<Utils::Verbose>("Score: ", score);
  log.Log<Utils::Verbose>("(Homogeneous) Transformation from ", opt.second.c_str(), " to ", opt.first.c_str(), ":");
  for (int r = 0; r < 4; ++r) std::printf("%12.6g %12.6g %12.6g %12.6g\n", mat(r, 0), mat(r, 1), mat(r, 2), mat(r, 3));

  if (!opt.matrix.empty()) {
    log.Log<Utils::Verbose>("Exporting Matrix to ", opt.matrix.c_str(), "...");
#ifdef S4P_HAVE_EIGEN
    io.WriteMatrix(opt.matrix, mat.cast<double>(), IOManager::POLYWORKS);
#else
    io.WriteMatrix(opt.matrix, compat::cast_double(mat), IOManager::POLYWORKS);
#endif
  }
  if (!opt.registered.empty()) {
    log.Log<Utils::Verbose>("Exporting Registered geometry to ", opt.registered.c_str(), "...");
    Q.save(io, opt.registered);
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  s4p_cli::Options opt;
  if (argc < 4) {
    s4p_cli::usage(opt, argv[0], false);
    return -2;
  }
  if (s4p_cli::parse(opt, argc, argv) != s4p_cli::Parse::Run) {
    s4p_cli::usage(opt, argv[0], true);
    return 1;            // the reference leaves with 1 for -h and for an unknown flag alike (super4pcs_test.cc:71-76)
  }
  return run(opt, GlobalRegistration::Utils::Logger(GlobalRegistration::Utils::Verbose));
}
