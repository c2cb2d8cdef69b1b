// TopPoses and RefineICPBatch: refine several candidate poses of one registration side by side on the MI355X and keep the
// one the full-resolution clouds prefer (include/s4p_icp_batch.h, DESIGN.md section "Batched multi-start ICP").
//
// The matcher returns the candidate with the greatest LCP on its samples; on the full clouds another of its good candidates
// is sometimes the right one.  TopPoses listens to ComputeTransformation and keeps the K best distinct candidate poses;
// RefineICPBatch refines them all in one batch and picks by correspondences, then rmse.
//
//   std::vector<Point3D> Q0 = Q;                                   // TopPoses' poses map Q as it was read
//   TopPoses top(4, 10.0, 2 * icp.max_distance, TopPoses::Centroid(Q));
//   matcher.ComputeTransformation(P, &Q, mat, Sampling::UniformDistSampler(), top);     // Q is moved by mat
//   auto starts = top.StartsAfter(mat);                            // relative to the moved Q; the first is the identity
//   auto best = RefineICPBatch(P, &Q, starts, icp);                // Q moved by best.first
//   mat = Compose(best.first, mat);
//
// Listening has a price: a visitor makes the matcher count every candidate in full instead of stopping a count that cannot
// win, and needsGlobalTransformation() == true makes it compose the caller-frame matrix per candidate.
// Link with -lsuper4pcs_icp.  TopPoses itself is host code and needs no library.
#ifndef S4P_FACADE_ICP_BATCH_H_
#define S4P_FACADE_ICP_BATCH_H_

#include <cmath>
#include <cstddef>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "s4p_icp_batch.h"
#include "super4pcs/algorithms/icp.h"

namespace GlobalRegistration {

// A visitor for ComputeTransformation that keeps the K candidate poses of greatest LCP, one per cluster of poses.
//  - Two poses are the same when the rotation between them is at most angle_tol_deg AND the images of Q's centroid lie
//    within dist_tol of each other.
//  - A candidate in the cluster of an entry (the first such entry in the order below) replaces it only with a strictly
//    greater LCP; otherwise it is inserted, and once K entries are held it evicts the smallest LCP only with a strictly
//    greater one (ties keep the earlier arrival).
//  - Entries stay sorted by LCP descending, stable by arrival.
// Only the per-candidate calls (fraction < 0) are candidates; the per-trial progress calls are ignored.
class TopPoses {
 public:
  struct Entry {
    double lcp;
    double M[16];             // row-major, maps Q (as given to the matcher) onto P
    size_t arrival;
  };

  TopPoses(int K, double angle_tol_deg, double dist_tol, const double centroid[3])
      : K_(K), cos_tol_(std::cos(angle_tol_deg * (3.14159265358979323846 / 180.0))), dist_tol_(dist_tol) {
    if (K < 1) throw std::invalid_argument("TopPoses: K must be at least 1");
    if (!(angle_tol_deg >= 0) || !(angle_tol_deg <= 180) || !(dist_tol >= 0)) throw std::invalid_argument("TopPoses: tolerances must be >= 0");
    for (int a = 0; a < 3; ++a) c_[a] = centroid[a];
  }
  TopPoses(int K, double angle_tol_deg, double dist_tol, const std::vector<double>& centroid)
      : TopPoses(K, angle_tol_deg, dist_tol, checked(centroid)) {}

  // the mean position of Q, summed in double in the order of the points
  static std::vector<double> Centroid(const std::vector<Point3D>& Q) {
    std::vector<double> c(3, 0.0);
    for (const Point3D& p : Q) { c[0] += double(p.x()); c[1] += double(p.y()); c[2] += double(p.z()); }
    if (!Q.empty()) for (int a = 0; a < 3; ++a) c[a] /= double(Q.size());
    return c;
  }

  constexpr bool needsGlobalTransformation() const { return true; }

  template <typename Matrix>
  inline void operator()(float fraction, float lcp, Matrix&& T) const {
    if (fraction >= 0) return;
    double M[16];
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) M[4 * r + c] = double(T(r, c));
    Add(double(lcp), M);
  }

  // one candidate; const like operator(): the matcher holds its visitor by const reference
  void Add(double lcp, const double M[16]) const {
    Entry e;
    e.lcp = lcp;
    for (int k = 0; k < 16; ++k) e.M[k] = M[k];
    e.arrival = arrivals_++;
    size_t hit = entries_.size();
    for (size_t i = 0; i < entries_.size() && hit == entries_.size(); ++i)
      if (Same(entries_[i].M, M)) hit = i;
    if (hit < entries_.size()) {
      if (!(lcp > entries_[hit].lcp)) return;
      entries_.erase(entries_.begin() + std::ptrdiff_t(hit));
    } else if (entries_.size() >= size_t(K_)) {
      if (!(lcp > entries_.back().lcp)) return;
      entries_.pop_back();
    }
    size_t at = 0;
    while (at < entries_.size() && entries_[at].lcp >= lcp) ++at;
    entries_.insert(entries_.begin() + std::ptrdiff_t(at), e);
  }

  // rotation between A and B at most the angle tolerance, and the images of the centroid within the distance tolerance
  bool Same(const double A[16], const double B[16]) const {
    double tr = 0.0;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) tr += A[4 * r + c] * B[4 * r + c];      // trace(A B^T)
    if (!(0.5 * (tr - 1.0) >= cos_tol_)) return false;
    double d2 = 0.0;
    for (int r = 0; r < 3; ++r) {
      const double a = ((A[4 * r] * c_[0] + A[4 * r + 1] * c_[1]) + A[4 * r + 2] * c_[2]) + A[4 * r + 3];
      const double b = ((B[4 * r] * c_[0] + B[4 * r + 1] * c_[1]) + B[4 * r + 2] * c_[2]) + B[4 * r + 3];
      d2 += (a - b) * (a - b);
    }
    return d2 <= dist_tol_ * dist_tol_;
  }

  const std::vector<Entry>& entries() const { return entries_; }
  size_t arrivals() const { return arrivals_; }

  // The start poses for RefineICPBatch after ComputeTransformation returned `result` and moved Q by it: the identity first
  // (the matcher's own pose: the batch can never do worse than refining that alone), then every entry M that is not in
  // result's cluster as M * result^-1 (result taken as rigid: [R | t]^-1 = [R^T | -R^T t]), at most K in all.
  template <typename Matrix>
  std::vector<Match4PCSBase::MatrixType> StartsAfter(const Matrix& result) const {
    double R[16], Ri[16];
    detail::icp_to16(result, R);
    for (int k = 0; k < 16; ++k) Ri[k] = k == 15 ? 1.0 : 0.0;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) Ri[4 * r + c] = R[4 * c + r];
      Ri[4 * r + 3] = -((R[r] * R[3] + R[4 + r] * R[7]) + R[8 + r] * R[11]);
    }
    std::vector<Match4PCSBase::MatrixType> out;
    Match4PCSBase::MatrixType I;
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) I(r, c) = Match4PCSBase::Scalar(r == c ? 1 : 0);
    out.push_back(I);
    for (const Entry& e : entries_) {
      if (out.size() >= size_t(K_)) break;
      if (Same(e.M, R)) continue;
      double S16[16];
      detail::icp_product16(e.M, Ri, S16);
      Match4PCSBase::MatrixType S;
      detail::icp_from16(S16, S);
      out.push_back(S);
    }
    return out;
  }

 private:
  static const double* checked(const std::vector<double>& c) {
    if (c.size() != 3) throw std::invalid_argument("TopPoses: the centroid has three coordinates");
    return c.data();
  }
  int K_;
  double cos_tol_, dist_tol_, c_[3];
  mutable std::vector<Entry> entries_;
  mutable size_t arrivals_ = 0;
};

// A * B for two facade matrices, in RefineICP's order (double, sum over k left to right)
inline Match4PCSBase::MatrixType Compose(const Match4PCSBase::MatrixType& A, const Match4PCSBase::MatrixType& B) {
  double a[16], b[16], c[16];
  detail::icp_to16(A, a);
  detail::icp_to16(B, b);
  detail::icp_product16(a, b, c);
  Match4PCSBase::MatrixType C;
  detail::icp_from16(c, C);
  return C;
}

// Q as it stands; every start maps it onto P (after ComputeTransformation: TopPoses::StartsAfter).  Refines all starts in
// one batch (s4p_icp_refine_batch, the source ordered by its image under starts[0]), moves Q in place by the pose of rank 0
// (n_corr descending, then rmse ascending, then the index) and returns that pose and its index in starts.  results, when
// given, gets one ICPResult per start.  Point-to-point and point-to-plane without a loss and without pair rejection only:
// anything else throws std::invalid_argument, as do an empty cloud and a start count outside 1..S4P_ICP_BATCH_MAX;
// std::runtime_error without a device or when the library refuses.
inline std::pair<Match4PCSBase::MatrixType, int> RefineICPBatch(const std::vector<Point3D>& P, std::vector<Point3D>* Q,
                                                                const std::vector<Match4PCSBase::MatrixType>& starts,
                                                                const ICPOptions& options, std::vector<ICPResult>* results = nullptr) {
  if (Q == nullptr || P.empty() || Q->empty()) throw std::invalid_argument("RefineICPBatch: empty cloud");
  if (starts.empty() || starts.size() > size_t(S4P_ICP_BATCH_MAX)) throw std::invalid_argument("RefineICPBatch: 1..64 starts");
  const bool plane = options.metric == ICPMetric::PointToPlane;
  if (!plane && options.metric != ICPMetric::PointToPoint)
    throw std::invalid_argument("RefineICPBatch: point-to-point and point-to-plane only (the generalized, symmetric and coloured metrics have no batch form)");
  if (options.loss != ICPLoss::None) throw std::invalid_argument("RefineICPBatch: robust losses have no batch form");
  if (options.reciprocal || options.normal_angle_deg >= 0) throw std::invalid_argument("RefineICPBatch: pair rejection has no batch form");
  // all of the above is refused before a device is asked for
  const detail::IcpHandle H("RefineICPBatch", options.device);
  std::vector<float> p[3], q[3];
  detail::cloud_soa(P, p);
  detail::cloud_soa(*Q, q);
  detail::icp_set_target(H, p, options.max_distance);
  detail::icp_set_source(H, q);
  if (plane) detail::icp_target_normals(H, P, options);
  s4p_icp_batch_params prm;
  prm.icp = detail::icp_params(options);
  prm.metric = plane ? S4P_ICP_METRIC_PLANE : S4P_ICP_METRIC_POINT;
  prm.reserved = 0;                                // s4p_icp_default_params does not reach the batch's own fields
  const int B = int(starts.size());
  const size_t nB = starts.size();
  std::vector<double> T(nB * 16);
  for (size_t b = 0; b < nB; ++b) detail::icp_to16(starts[b], &T[b * 16]);
  std::vector<s4p_icp_result> res(nB);
  std::vector<int32_t> order(nB);
  H.check(s4p_icp_refine_batch(H.h, &prm, B, T.data(), res.data(), order.data()));
  const int best = order[0];
  detail::icp_apply(H, &T[size_t(best) * 16], q, Q);
  if (results) {
    results->clear();
    for (const s4p_icp_result& r : res) results->push_back(detail::icp_result(r));
  }
  Match4PCSBase::MatrixType M;
  detail::icp_from16(&T[size_t(best) * 16], M);
  return std::make_pair(M, best);
}

}  // namespace GlobalRegistration
#endif
