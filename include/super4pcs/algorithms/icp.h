// RefineICP: point-to-point, point-to-plane, generalized, symmetric or coloured ICP on the full-resolution clouds, on the MI355X, after a registration.  The reference's
// documentation recommends refining a coarse Super4PCS pose "using a local algorithm, like the ICP" (doc/Usage.md) instead
// of sampling more; this header does that step through the C ABI of libsuper4pcs_icp.so (include/s4p_icp.h,
// include/s4p_icp_plane.h, include/s4p_icp_gicp.h, include/s4p_icp_symm.h, include/s4p_icp_color.h), and its robust losses (include/s4p_icp_robust.h: trimmed ICP, Huber, Tukey).
// Pair rejection (include/s4p_icp_reject.h: reciprocal pairs, normal angle) applies to every metric and loss.
// Link with -lsuper4pcs_icp.  Builds with and without Eigen, like the rest of the facade.
//
// ICPMetric::Generalized and ICPMetric::Symmetric need normals of both clouds.  Q's own are used when every point of Q has a nonzero one.
// ComputeTransformation moves Q's positions only and leaves its normals in the frame of the file, so RefineICP rotates them
// by the linear part of `transformation` (in double, row by row as (m0 * x + m1 * y) + m2 * z) before the upload.  Otherwise
// the normals are estimated on the moved Q as EstimateNormals does with k = 16 (algorithms/normals.h).  That one step binds
// libsuper4pcs_normals.so at run time (the process's own copy when it is linked, else the library next to
// libsuper4pcs_icp.so), so that programs which link -lsuper4pcs_icp alone keep building.
//
// ICPMetric::Colored adds a photometric term (include/s4p_icp_color.h) and needs the colour of both clouds: every point's
// rgb() (0..255, as io.h reads it) becomes the intensity float(((double r + double g) + double b) / 765).  A point whose
// rgb()[0] < 0 has no colour (the convention of the reference's pair filter), and RefineICP then throws.
//
//   MatchSuper4PCS matcher(options, logger);
//   matcher.ComputeTransformation(P, &Q, mat);           // Q is moved by mat
//   ICPOptions icp; icp.max_distance = 4 * options.delta;
//   RefineICP(P, &Q, mat, icp);                           // Q moved by the refinement too; mat <- dT * mat
#ifndef S4P_FACADE_ICP_H_
#define S4P_FACADE_ICP_H_

#include <dlfcn.h>

#include <cmath>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "s4p_icp.h"
#include "s4p_icp_plane.h"
#include "s4p_icp_robust.h"
#include "s4p_icp_gicp.h"
#include "s4p_icp_symm.h"
#include "s4p_icp_color.h"
#include "s4p_icp_reject.h"
#include "s4p_normals.h"
#include "super4pcs/algorithms/match4pcsBase.h"

namespace GlobalRegistration {

enum class ICPMetric { PointToPoint, PointToPlane, Generalized, Colored, Symmetric };
enum class ICPLoss { None, Trimmed, Huber, Tukey };

struct ICPOptions {
  int max_iterations = 30;
  double max_distance = -1.0;       // required (> 0); 4 * delta is the usual choice after a registration at delta
  double rel_tol = 1e-6;
  int min_correspondences = 3;
  int device = 0;
  ICPMetric metric = ICPMetric::PointToPoint;
  // PointToPlane: P's normals when every point of P has a nonzero one, else normals estimated on the device from the
  // neighbours within normal_radius (<= 0: max_distance; at most max_distance) with at least 6 of them
  double normal_radius = -1.0;
  // Generalized: target normals as for PointToPlane; source normals as described at the top of this header; the covariance
  // parameter epsilon of include/s4p_icp_gicp.h, in [1e-6, 1].  Takes no loss.
  double gicp_epsilon = S4P_ICP_GICP_EPSILON;
  // Symmetric (include/s4p_icp_symm.h): point-to-plane along the sum of both normals; the normals of both clouds as for
  // Generalized, no parameter.  Takes no loss.
  // Colored: target normals as for PointToPlane; intensities from rgb() of both clouds; intensity gradients of P estimated
  // on the device within normal_radius (<= 0: max_distance) with at least 6 neighbours; the weight color_lambda of the
  // geometric term (include/s4p_icp_color.h), in [0, 1].  Takes no loss.
  double color_lambda = S4P_ICP_COLOR_LAMBDA;
  // None: least squares over every pair within max_distance.  Trimmed keeps the pairs whose residual is at most the
  // ceil(trim_fraction |Q|)-th smallest; Huber / Tukey reweight with the scale loss_scale (<= 0: estimated on the device)
  ICPLoss loss = ICPLoss::None;
  double trim_fraction = 1.0;       // Trimmed: in (0, 1], e.g. the registration's overlap
  double loss_scale = -1.0;         // Huber / Tukey
  // Pair rejection (include/s4p_icp_reject.h), for every metric and loss.  reciprocal: a pair is kept only when the source
  // point is the nearest one of its target point too.  normal_angle_deg >= 0: a pair is kept only when the target normal and
  // the (rotated) source normal are at most that far apart, up to sign unless normals_oriented ([0, 90] degrees, oriented
  // [0, 180]); the normals of both clouds are obtained as ICPMetric::Generalized obtains them.  < 0: off.
  bool reciprocal = false;
  double normal_angle_deg = -1;
  bool normals_oriented = false;
};

struct ICPResult {
  int iterations = 0;
  int status = 0;                   // S4P_ICP_MAX_ITERATIONS / _CONVERGED / _TOO_FEW / _DEGENERATE (point-to-plane, generalized, symmetric, coloured)
  int64_t n_corr = 0;
  double rmse = 0.0;
  double fitness = 0.0;             // n_corr / |Q|
  std::vector<double> rmse_history;
};

namespace detail {

// EstimateNormals' computation (k nearest neighbours, no radius) on SoA positions, with libsuper4pcs_normals.so bound at run
// time: out = n x 3 floats.
inline void icp_knn_normals(const std::vector<float> (&c)[3], int k, int device, std::vector<float>* out) {
  void* lib = nullptr;
  auto sym = [&lib](const char* name) -> void* {
    void* f = dlsym(RTLD_DEFAULT, name);
    if (!f) {
      if (!lib) lib = dlopen("libsuper4pcs_normals.so", RTLD_NOW | RTLD_GLOBAL);
      if (lib) f = dlsym(lib, name);
    }
    if (!f) throw std::runtime_error(std::string("RefineICP: libsuper4pcs_normals.so is needed to estimate Q's normals (") + name + ")");
    return f;
  };
  const auto create = reinterpret_cast<decltype(&s4p_normals_create)>(sym("s4p_normals_create"));
  const auto destroy = reinterpret_cast<decltype(&s4p_normals_destroy)>(sym("s4p_normals_destroy"));
  const auto last_error = reinterpret_cast<decltype(&s4p_normals_last_error)>(sym("s4p_normals_last_error"));
  const auto set_cloud = reinterpret_cast<decltype(&s4p_normals_set_cloud)>(sym("s4p_normals_set_cloud"));
  const auto estimate = reinterpret_cast<decltype(&s4p_normals_estimate)>(sym("s4p_normals_estimate"));
  s4p_normals_ctx* h = nullptr;
  if (create(device, &h) != S4P_NORMALS_OK) throw std::runtime_error(std::string("RefineICP (MI355X): ") + last_error(nullptr));
  const int64_t n = int64_t(c[0].size());
  out->resize(3 * size_t(n));
  int32_t rc = set_cloud(h, c[0].data(), c[1].data(), c[2].data(), n);
  if (rc == S4P_NORMALS_OK) rc = estimate(h, k, -1.f, out->data());
  const std::string err = rc == S4P_NORMALS_OK ? std::string() : std::string(last_error(h));
  destroy(h);
  if (rc != S4P_NORMALS_OK) throw std::runtime_error("RefineICP (MI355X): " + err);
}

}  // namespace detail

// Q as it stands after ComputeTransformation (already moved).  Finds dT, moves Q in place (in k_apply's rounding order)
// and sets transformation <- dT * transformation.  Returns the fitness of the refined pose.  Throws std::runtime_error
// when there is no device (no CPU fallback) or an argument is invalid, std::invalid_argument for an empty cloud, a loss with
// the generalized, symmetric or coloured metric, or the coloured metric on a cloud with a point that has no colour.
inline float RefineICP(const std::vector<Point3D>& P, std::vector<Point3D>* Q, Match4PCSBase::MatrixRef transformation,
                       const ICPOptions& options, ICPResult* result = nullptr) {
  if (Q == nullptr || P.empty() || Q->empty()) throw std::invalid_argument("RefineICP: empty cloud");
  const bool gicp = options.metric == ICPMetric::Generalized;
  if (gicp && options.loss != ICPLoss::None) throw std::invalid_argument("RefineICP: the generalized metric takes no loss");
  const bool symm = options.metric == ICPMetric::Symmetric;
  if (symm && options.loss != ICPLoss::None) throw std::invalid_argument("RefineICP: the symmetric metric takes no loss");
  const bool colored = options.metric == ICPMetric::Colored;
  if (colored && options.loss != ICPLoss::None) throw std::invalid_argument("RefineICP: the coloured metric takes no loss");
  std::vector<float> ip, iq;
  if (colored) {
    auto intensity = [](const std::vector<Point3D>& pts, std::vector<float>* out) {
      out->resize(pts.size());
      for (size_t i = 0; i < pts.size(); ++i) {
        const auto& c = pts[i].rgb();
        if (c(0) < 0) throw std::invalid_argument("RefineICP: the coloured metric needs a colour at every point of P and Q");
        (*out)[i] = float(((double(c(0)) + double(c(1))) + double(c(2))) / 765.0);
      }
    };
    intensity(P, &ip);
    intensity(*Q, &iq);
  }
  struct Handle {
    s4p_icp_ctx* h = nullptr;
    ~Handle() { s4p_icp_destroy(h); }
    void check(int32_t rc) const {
      if (rc != S4P_ICP_OK) throw std::runtime_error(std::string("RefineICP (MI355X): ") + s4p_icp_last_error(h));
    }
  } H;
  if (s4p_icp_create(options.device, &H.h) != S4P_ICP_OK)
    throw std::runtime_error(std::string("RefineICP (MI355X): ") + s4p_icp_last_error(nullptr));
  auto soa = [](const std::vector<Point3D>& pts, std::vector<float> (&c)[3]) {
    for (int k = 0; k < 3; ++k) c[k].resize(pts.size());
    for (size_t i = 0; i < pts.size(); ++i) { c[0][i] = pts[i].x(); c[1][i] = pts[i].y(); c[2][i] = pts[i].z(); }
  };
  std::vector<float> p[3], q[3];
  soa(P, p);
  soa(*Q, q);
  H.check(s4p_icp_set_target(H.h, p[0].data(), p[1].data(), p[2].data(), int64_t(P.size()), float(options.max_distance)));
  H.check(s4p_icp_set_source(H.h, q[0].data(), q[1].data(), q[2].data(), int64_t(Q->size())));
  const bool plane = options.metric == ICPMetric::PointToPlane;
  const bool by_normals = options.normal_angle_deg >= 0;
  if (by_normals && !(options.normal_angle_deg <= (options.normals_oriented ? 180.0 : 90.0)))
    throw std::invalid_argument("RefineICP: normal_angle_deg must be at most 90 (oriented normals: 180)");
  if (plane || gicp || symm || colored || by_normals) {
    bool all = true;
    for (const Point3D& pt : P) {
      const auto& nv = pt.normal();
      if (!(nv(0) != 0 || nv(1) != 0 || nv(2) != 0)) { all = false; break; }
    }
    if (all) {
      std::vector<float> n[3];
      for (int k = 0; k < 3; ++k) n[k].resize(P.size());
      for (size_t i = 0; i < P.size(); ++i) for (int k = 0; k < 3; ++k) n[k][i] = float(P[i].normal()(k));
      H.check(s4p_icp_set_target_normals(H.h, n[0].data(), n[1].data(), n[2].data(), int64_t(P.size())));
    } else {
      const double r = options.normal_radius > 0 ? options.normal_radius : options.max_distance;
      H.check(s4p_icp_estimate_normals(H.h, float(r), 6));
    }
  }
  if (gicp || symm || by_normals) {
    bool all = true;
    for (const Point3D& pt : *Q) {
      const auto& nv = pt.normal();
      if (!(nv(0) != 0 || nv(1) != 0 || nv(2) != 0)) { all = false; break; }
    }
    std::vector<float> n[3];
    for (int k = 0; k < 3; ++k) n[k].resize(Q->size());
    if (all) {                                     // Q's own, rotated into the frame Q was moved to
      double m[3][3];
      for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) m[a][b] = double(transformation(a, b));
      for (size_t i = 0; i < Q->size(); ++i) {
        const auto& nv = (*Q)[i].normal();
        const double x = double(nv(0)), y = double(nv(1)), z = double(nv(2));
        for (int a = 0; a < 3; ++a) n[a][i] = float((m[a][0] * x + m[a][1] * y) + m[a][2] * z);
      }
    } else {
      std::vector<float> est;
      detail::icp_knn_normals(q, 16, options.device, &est);
      for (size_t i = 0; i < Q->size(); ++i) for (int k = 0; k < 3; ++k) n[k][i] = est[3 * i + k];
    }
    H.check(s4p_icp_set_source_normals(H.h, n[0].data(), n[1].data(), n[2].data(), int64_t(Q->size())));
  }
  if (colored) {
    H.check(s4p_icp_set_target_intensity(H.h, ip.data(), int64_t(P.size())));
    H.check(s4p_icp_set_source_intensity(H.h, iq.data(), int64_t(Q->size())));
    const double r = options.normal_radius > 0 ? options.normal_radius : options.max_distance;
    H.check(s4p_icp_estimate_color_gradients(H.h, float(r), 6));
  }
  if (options.reciprocal || by_normals) {
    s4p_icp_reject rej;
    s4p_icp_reject_defaults(&rej);
    rej.reciprocal = options.reciprocal ? 1 : 0;
    if (by_normals) {
      rej.normal_mode = options.normals_oriented ? S4P_ICP_REJECT_NORMALS_ORIENTED : S4P_ICP_REJECT_NORMALS_UNORIENTED;
      const double c = std::cos(options.normal_angle_deg * (3.14159265358979323846 / 180.0));
      const double lo = options.normals_oriented ? -1.0 : 0.0;
      rej.normal_cos = c < lo ? lo : (c > 1.0 ? 1.0 : c);
    }
    H.check(s4p_icp_set_rejection(H.h, &rej));
  }
  s4p_icp_params prm;
  s4p_icp_default_params(&prm);
  prm.max_iterations = options.max_iterations;
  prm.min_correspondences = options.min_correspondences;
  prm.rel_tol = options.rel_tol;
  double dT[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  s4p_icp_result r;
  if (options.loss == ICPLoss::None) {
    if (gicp) H.check(s4p_icp_refine_gicp(H.h, &prm, options.gicp_epsilon, dT, &r));
    else if (symm) H.check(s4p_icp_refine_symm(H.h, &prm, dT, &r));
    else if (colored) H.check(s4p_icp_refine_color(H.h, &prm, options.color_lambda, dT, &r));
    else H.check(plane ? s4p_icp_refine_plane(H.h, &prm, dT, &r) : s4p_icp_refine(H.h, &prm, dT, &r));
  } else {
    const int32_t loss = options.loss == ICPLoss::Trimmed ? S4P_ICP_LOSS_TRIMMED
                         : (options.loss == ICPLoss::Huber ? S4P_ICP_LOSS_HUBER : S4P_ICP_LOSS_TUKEY);
    s4p_icp_robust rob;
    s4p_icp_robust_defaults(&rob, loss);
    rob.trim_fraction = options.trim_fraction;
    rob.scale = options.loss_scale;
    H.check(s4p_icp_refine_robust(H.h, &prm, plane ? S4P_ICP_METRIC_PLANE : S4P_ICP_METRIC_POINT, &rob, dT, &r, nullptr));
  }
  H.check(s4p_icp_apply(H.h, dT, q[0].data(), q[1].data(), q[2].data(), int64_t(Q->size())));
  for (size_t i = 0; i < Q->size(); ++i) { (*Q)[i].x() = q[0][i]; (*Q)[i].y() = q[1][i]; (*Q)[i].z() = q[2][i]; }
  double M[16];
  for (int a = 0; a < 4; ++a)
    for (int b = 0; b < 4; ++b) {
      double v = 0.0;
      for (int k = 0; k < 4; ++k) v += dT[4 * a + k] * double(transformation(k, b));
      M[4 * a + b] = v;
    }
  using Scalar = Match4PCSBase::Scalar;
  for (int a = 0; a < 4; ++a)
    for (int b = 0; b < 4; ++b) transformation(a, b) = Scalar(M[4 * a + b]);
  if (result) {
    result->iterations = r.iterations; result->status = r.status; result->n_corr = r.n_corr;
    result->rmse = r.rmse; result->fitness = r.fitness;
    result->rmse_history.assign(r.history_rmse, r.history_rmse + r.history_len);
  }
  return float(r.fitness);
}

}  // namespace GlobalRegistration
#endif
