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
#include "super4pcs/algorithms/match4pcsBase.h"
#include "super4pcs/algorithms/normals_handle.h"

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

// One s4p_icp context; every message starts with "<who> (MI355X): ".
struct IcpHandle {
  s4p_icp_ctx* h = nullptr;
  const char* who;
  explicit IcpHandle(const char* w, int device) : who(w) {
    if (s4p_icp_create(device, &h) != S4P_ICP_OK) throw std::runtime_error(std::string(who) + " (MI355X): " + s4p_icp_last_error(nullptr));
  }
  IcpHandle(const IcpHandle&) = delete;
  IcpHandle& operator=(const IcpHandle&) = delete;
  ~IcpHandle() { s4p_icp_destroy(h); }
  void check(int32_t rc) const {
    if (rc != S4P_ICP_OK) throw std::runtime_error(std::string(who) + " (MI355X): " + s4p_icp_last_error(h));
  }
};

inline void icp_set_target(const IcpHandle& H, const std::vector<float> (&p)[3], double max_distance) {
  H.check(s4p_icp_set_target(H.h, p[0].data(), p[1].data(), p[2].data(), int64_t(p[0].size()), float(max_distance)));
}

inline void icp_set_source(const IcpHandle& H, const std::vector<float> (&q)[3]) {
  H.check(s4p_icp_set_source(H.h, q[0].data(), q[1].data(), q[2].data(), int64_t(q[0].size())));
}

// the cloud's own normals as SoA when every point has a nonzero one
inline bool icp_own_normals(const std::vector<Point3D>& pts, std::vector<float> (&n)[3]) {
  for (const Point3D& pt : pts) {
    const auto& nv = pt.normal();
    if (!(nv(0) != 0 || nv(1) != 0 || nv(2) != 0)) return false;
  }
  for (int k = 0; k < 3; ++k) n[k].resize(pts.size());
  for (size_t i = 0; i < pts.size(); ++i) for (int k = 0; k < 3; ++k) n[k][i] = float(pts[i].normal()(k));
  return true;
}

// EstimateNormals' computation (k nearest neighbours, no radius) on SoA positions, with libsuper4pcs_normals.so bound at run
// time: out = n x 3 floats.  Its messages say RefineICP whoever calls.
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

// the radius of the target's estimated normals and colour gradients
inline double icp_normal_radius(const ICPOptions& o) { return o.normal_radius > 0 ? o.normal_radius : o.max_distance; }

// Target normals: P's own, else estimated on the device with at least 6 neighbours.  RegisterMultiway does not come here: it
// never reads a scan's own normals and always estimates.
inline void icp_target_normals(const IcpHandle& H, const std::vector<Point3D>& P, const ICPOptions& o) {
  std::vector<float> n[3];
  if (icp_own_normals(P, n)) H.check(s4p_icp_set_target_normals(H.h, n[0].data(), n[1].data(), n[2].data(), int64_t(P.size())));
  else H.check(s4p_icp_estimate_normals(H.h, float(icp_normal_radius(o)), 6));
}

// icp_knn_normals' n x 3 floats as the source normals
inline void icp_set_knn_normals(const IcpHandle& H, const std::vector<float>& est) {
  const size_t nq = est.size() / 3;
  std::vector<float> n[3];
  for (int k = 0; k < 3; ++k) n[k].resize(nq);
  for (size_t i = 0; i < nq; ++i) for (int k = 0; k < 3; ++k) n[k][i] = est[3 * i + size_t(k)];
  H.check(s4p_icp_set_source_normals(H.h, n[0].data(), n[1].data(), n[2].data(), int64_t(nq)));
}

// Source normals: Q's own, else the 16-nearest-neighbour ones of the positions q.  rot (row-major 3x3, or null) rotates the
// own ones, in double as (m0 * x + m1 * y) + m2 * z and then rounded to float: RefineICP passes the linear part of the
// pose Q was moved by, ICPInformation passes null because the library rotates them with its T.
inline void icp_source_normals(const IcpHandle& H, const std::vector<Point3D>& Q, const std::vector<float> (&q)[3], int device,
                               const double* rot) {
  std::vector<float> n[3];
  if (!icp_own_normals(Q, n)) {
    std::vector<float> est;
    icp_knn_normals(q, 16, device, &est);
    icp_set_knn_normals(H, est);
    return;
  }
  for (size_t i = 0; rot && i < Q.size(); ++i) {
    const double x = double(n[0][i]), y = double(n[1][i]), z = double(n[2][i]);
    for (int a = 0; a < 3; ++a) n[a][i] = float((rot[3 * a] * x + rot[3 * a + 1] * y) + rot[3 * a + 2] * z);
  }
  H.check(s4p_icp_set_source_normals(H.h, n[0].data(), n[1].data(), n[2].data(), int64_t(Q.size())));
}

// The rejection flags as the library takes them; true when one is set.  Throws for an angle out of range, so where it is
// called decides which error a caller without a device sees: RefineICP calls it after its uploads (the device's),
// ICPInformation and RegisterMultiway before they ask for a device (the angle's).
inline bool icp_rejection(const ICPOptions& o, s4p_icp_reject* rej, const char* who) {
  const bool by_normals = o.normal_angle_deg >= 0;
  if (by_normals && !(o.normal_angle_deg <= (o.normals_oriented ? 180.0 : 90.0)))
    throw std::invalid_argument(std::string(who) + ": normal_angle_deg must be at most 90 (oriented normals: 180)");
  s4p_icp_reject_defaults(rej);
  rej->reciprocal = o.reciprocal ? 1 : 0;
  if (by_normals) {
    rej->normal_mode = o.normals_oriented ? S4P_ICP_REJECT_NORMALS_ORIENTED : S4P_ICP_REJECT_NORMALS_UNORIENTED;
    const double c = std::cos(o.normal_angle_deg * (3.14159265358979323846 / 180.0));
    const double lo = o.normals_oriented ? -1.0 : 0.0;
    rej->normal_cos = c < lo ? lo : (c > 1.0 ? 1.0 : c);
  }
  return o.reciprocal || by_normals;
}

// rgb() as the coloured metric's intensity
inline void icp_intensity(const std::vector<Point3D>& pts, std::vector<float>* out) {
  out->resize(pts.size());
  for (size_t i = 0; i < pts.size(); ++i) {
    const auto& c = pts[i].rgb();
    if (c(0) < 0) throw std::invalid_argument("RefineICP: the coloured metric needs a colour at every point of P and Q");
    (*out)[i] = float(((double(c(0)) + double(c(1))) + double(c(2))) / 765.0);
  }
}

inline s4p_icp_params icp_params(const ICPOptions& o) {
  s4p_icp_params prm;
  s4p_icp_default_params(&prm);
  prm.max_iterations = o.max_iterations;
  prm.min_correspondences = o.min_correspondences;
  prm.rel_tol = o.rel_tol;
  return prm;
}

inline ICPResult icp_result(const s4p_icp_result& r) {
  ICPResult o;
  o.iterations = r.iterations; o.status = r.status; o.n_corr = r.n_corr; o.rmse = r.rmse; o.fitness = r.fitness;
  o.rmse_history.assign(r.history_rmse, r.history_rmse + r.history_len);
  return o;
}

// The refine of o.metric and o.loss from the pose T16 (row-major, refined in place).
inline s4p_icp_result icp_refine(const IcpHandle& H, const ICPOptions& o, double* T16) {
  const s4p_icp_params prm = icp_params(o);
  const bool plane = o.metric == ICPMetric::PointToPlane;
  s4p_icp_result r;
  if (o.loss != ICPLoss::None) {
    const int32_t loss = o.loss == ICPLoss::Trimmed ? S4P_ICP_LOSS_TRIMMED : (o.loss == ICPLoss::Huber ? S4P_ICP_LOSS_HUBER : S4P_ICP_LOSS_TUKEY);
    s4p_icp_robust rob;
    s4p_icp_robust_defaults(&rob, loss);
    rob.trim_fraction = o.trim_fraction;
    rob.scale = o.loss_scale;
    H.check(s4p_icp_refine_robust(H.h, &prm, plane ? S4P_ICP_METRIC_PLANE : S4P_ICP_METRIC_POINT, &rob, T16, &r, nullptr));
  } else if (o.metric == ICPMetric::Generalized) H.check(s4p_icp_refine_gicp(H.h, &prm, o.gicp_epsilon, T16, &r));
  else if (o.metric == ICPMetric::Symmetric) H.check(s4p_icp_refine_symm(H.h, &prm, T16, &r));
  else if (o.metric == ICPMetric::Colored) H.check(s4p_icp_refine_color(H.h, &prm, o.color_lambda, T16, &r));
  else H.check(plane ? s4p_icp_refine_plane(H.h, &prm, T16, &r) : s4p_icp_refine(H.h, &prm, T16, &r));
  return r;
}

// Moves the SoA positions q by T16 on the device (k_apply's rounding order) and writes them into Q.
inline void icp_apply(const IcpHandle& H, const double* T16, std::vector<float> (&q)[3], std::vector<Point3D>* Q) {
  H.check(s4p_icp_apply(H.h, T16, q[0].data(), q[1].data(), q[2].data(), int64_t(Q->size())));
  for (size_t i = 0; i < Q->size(); ++i) { (*Q)[i].x() = q[0][i]; (*Q)[i].y() = q[1][i]; (*Q)[i].z() = q[2][i]; }
}

// C = A B for row-major 4x4 doubles, every entry summed over k = 0..3 from the left.  The one product of the facade: the
// poses that RefineICP, Compose, TopPoses::StartsAfter and RegisterMultiway compose have the same bits.  C is neither A nor B.
inline void icp_product16(const double* A, const double* B, double* C) {
  for (int a = 0; a < 4; ++a)
    for (int b = 0; b < 4; ++b) {
      double v = 0.0;
      for (int k = 0; k < 4; ++k) v += A[4 * a + k] * B[4 * k + b];
      C[4 * a + b] = v;
    }
}

template <typename Matrix>
inline void icp_to16(const Matrix& M, double* out) {
  for (int a = 0; a < 4; ++a) for (int b = 0; b < 4; ++b) out[4 * a + b] = double(M(a, b));
}

template <typename Matrix>
inline void icp_from16(const double* v, Matrix& M) {
  for (int a = 0; a < 4; ++a) for (int b = 0; b < 4; ++b) M(a, b) = Match4PCSBase::Scalar(v[4 * a + b]);
}

}  // namespace detail

// Q as it stands after ComputeTransformation (already moved).  Finds dT, moves Q in place (in k_apply's rounding order)
// and sets transformation <- dT * transformation.  Returns the fitness of the refined pose.  Throws std::runtime_error
// when there is no device (no CPU fallback) or an argument is invalid, std::invalid_argument for an empty cloud, a loss with
// the generalized, symmetric or coloured metric, or the coloured metric on a cloud with a point that has no colour.
inline float RefineICP(const std::vector<Point3D>& P, std::vector<Point3D>* Q, Match4PCSBase::MatrixRef transformation,
                       const ICPOptions& options, ICPResult* result = nullptr) {
  // What is refused before a device is asked for, in this order: the empty cloud, the three "takes no loss", the colours.
  if (Q == nullptr || P.empty() || Q->empty()) throw std::invalid_argument("RefineICP: empty cloud");
  const bool gicp = options.metric == ICPMetric::Generalized;
  if (gicp && options.loss != ICPLoss::None) throw std::invalid_argument("RefineICP: the generalized metric takes no loss");
  const bool symm = options.metric == ICPMetric::Symmetric;
  if (symm && options.loss != ICPLoss::None) throw std::invalid_argument("RefineICP: the symmetric metric takes no loss");
  const bool colored = options.metric == ICPMetric::Colored;
  if (colored && options.loss != ICPLoss::None) throw std::invalid_argument("RefineICP: the coloured metric takes no loss");
  std::vector<float> ip, iq;
  if (colored) {
    detail::icp_intensity(P, &ip);
    detail::icp_intensity(*Q, &iq);
  }
  const detail::IcpHandle H("RefineICP", options.device);
  std::vector<float> p[3], q[3];
  detail::cloud_soa(P, p);
  detail::cloud_soa(*Q, q);
  detail::icp_set_target(H, p, options.max_distance);
  detail::icp_set_source(H, q);
  // The angle's range is checked here, after the device and the uploads (ICPInformation and RegisterMultiway check it first):
  // without a device RefineICP reports the device, not the angle.
  s4p_icp_reject rej;
  const bool reject = detail::icp_rejection(options, &rej, "RefineICP");
  const bool by_normals = options.normal_angle_deg >= 0;
  double T[16];
  detail::icp_to16(transformation, T);
  if (options.metric != ICPMetric::PointToPoint || by_normals) detail::icp_target_normals(H, P, options);
  if (gicp || symm || by_normals) {                // Q's own normals are in the file's frame: rotated into the one Q was moved to
    const double rot[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
    detail::icp_source_normals(H, *Q, q, options.device, rot);
  }
  if (colored) {
    H.check(s4p_icp_set_target_intensity(H.h, ip.data(), int64_t(P.size())));
    H.check(s4p_icp_set_source_intensity(H.h, iq.data(), int64_t(Q->size())));
    H.check(s4p_icp_estimate_color_gradients(H.h, float(detail::icp_normal_radius(options)), 6));
  }
  if (reject) H.check(s4p_icp_set_rejection(H.h, &rej));
  double dT[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, M[16];
  const s4p_icp_result r = detail::icp_refine(H, options, dT);
  detail::icp_apply(H, dT, q, Q);
  detail::icp_product16(dT, T, M);
  detail::icp_from16(M, transformation);
  if (result) *result = detail::icp_result(r);
  return float(r.fitness);
}

}  // namespace GlobalRegistration
#endif
