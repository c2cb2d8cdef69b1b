// Test-side restatement of the plane segmentation contract (include/s4p_plane.h) on the CPU, term by term: the alive list,
// the centred frame, splitmix64 and the 128-bit product for the sample positions, the candidate plane in double, the
// residual as three std::fmaf, the winner as the first largest count, the refit sums in the header's two-level order, the
// covariance, the cyclic Jacobi and the sign rule.  Candidates are counted by 16 threads; nothing else is parallel, and
// nothing here follows the device path: no ballot, no records, no keys.
// Build: g++ -O2 -ffp-contract=off -fopenmp -fPIC -shared (tests/plane_helpers.py).
#include <omp.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

constexpr int64_t kSumBlock = 128;          // S4P_PLANE_SUM_BLOCK

uint64_t splitmix64(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

void jacobi3(double A[3][3], double V[3][3]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 64; ++sweep) {
    const double diag = (A[0][0] * A[0][0] + A[1][1] * A[1][1]) + A[2][2] * A[2][2];
    const double off = (A[0][1] * A[0][1] + A[0][2] * A[0][2]) + A[1][2] * A[1][2];
    if (off == 0.0 || off <= 1e-36 * diag) break;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        if (A[p][q] == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 3; ++k) {
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 3; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < 3; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq;
        }
      }
  }
}

void sign_rule(double v[3]) {
  int lead = 0;
  for (int a = 1; a < 3; ++a) if (std::fabs(v[a]) > std::fabs(v[lead])) lead = a;
  if (v[lead] < 0.0) for (int a = 0; a < 3; ++a) v[a] = -v[a];
}

struct Plane {
  float n[3], d;
};

bool inlier(const Plane& P, const float x[3], float distance) {
  const float r = std::fmaf(P.n[0], x[0], std::fmaf(P.n[1], x[1], std::fmaf(P.n[2], x[2], P.d)));
  return std::fabs(r) <= distance;
}

}  // namespace

extern "C" {

// plane[8]: normal, d, centre, d_centred; ints[4]: inliers, alive, trial, valid_trials; counts[trials] (may be null): the
// inlier count of every candidate, 0 for an invalid one; valid[trials] (may be null); mask[n].
void plane_cpu_segment(const float* x, const float* y, const float* z, int64_t n, float distance, int32_t trials, uint64_t seed, int32_t refine,
                       const uint8_t* exclude, float* plane, int64_t* ints, uint8_t* mask, int32_t* counts, uint8_t* valid, int32_t threads) {
  float lo[3] = {x[0], y[0], z[0]}, hi[3] = {x[0], y[0], z[0]};
  for (int64_t i = 0; i < n; ++i) {
    const float p[3] = {x[i], y[i], z[i]};
    for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], p[a]); hi[a] = std::max(hi[a], p[a]); }
  }
  float c[3];
  for (int a = 0; a < 3; ++a) c[a] = 0.5f * lo[a] + 0.5f * hi[a];
  std::vector<int64_t> alive;
  for (int64_t i = 0; i < n; ++i) if (!exclude || exclude[i] == 0) alive.push_back(i);
  const uint64_t m = alive.size();
  std::vector<float> X(3 * size_t(m));                     // the alive points, centred
  for (uint64_t p = 0; p < m; ++p) {
    X[3 * p] = x[alive[p]] - c[0]; X[3 * p + 1] = y[alive[p]] - c[1]; X[3 * p + 2] = z[alive[p]] - c[2];
  }
  std::vector<Plane> cand(trials);
  std::vector<uint8_t> ok(trials, 0);
  std::vector<int64_t> cnt(trials, 0);
  for (int32_t t = 0; t < trials; ++t) {
    uint64_t s = seed + 3ull * uint64_t(t) * 0x9E3779B97F4A7C15ull;
    uint64_t p[3];
    for (int a = 0; a < 3; ++a) p[a] = uint64_t((unsigned __int128)splitmix64(s) * m >> 64);
    if (m < 3 || p[0] == p[1] || p[0] == p[2] || p[1] == p[2]) continue;
    double q[3][3];
    bool finite = true;
    for (int a = 0; a < 3; ++a)
      for (int k = 0; k < 3; ++k) {
        finite = finite && std::isfinite(X[3 * p[a] + k]);
        q[a][k] = double(X[3 * p[a] + k]);
      }
    if (!finite) continue;
    const double e1[3] = {q[1][0] - q[0][0], q[1][1] - q[0][1], q[1][2] - q[0][2]};
    const double e2[3] = {q[2][0] - q[0][0], q[2][1] - q[0][1], q[2][2] - q[0][2]};
    const double w[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double l2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    if (!(l2 > 0.0) || !std::isfinite(l2)) continue;
    const double sl = std::sqrt(l2);
    double v[3] = {w[0] / sl, w[1] / sl, w[2] / sl};
    sign_rule(v);
    for (int a = 0; a < 3; ++a) cand[t].n[a] = float(v[a]);
    cand[t].d = float(-((v[0] * q[0][0] + v[1] * q[0][1]) + v[2] * q[0][2]));
    ok[t] = 1;
  }
  if (threads > 0) omp_set_num_threads(threads);
#pragma omp parallel for schedule(dynamic, 8)
  for (int32_t t = 0; t < trials; ++t) {
    if (!ok[t]) continue;
    int64_t k = 0;
    for (uint64_t p = 0; p < m; ++p) k += inlier(cand[t], &X[3 * p], distance) ? 1 : 0;
    cnt[t] = k;
  }
  int32_t win = -1, nvalid = 0;
  for (int32_t t = 0; t < trials; ++t) {
    if (!ok[t]) continue;
    ++nvalid;
    if (win < 0 || cnt[t] > cnt[win]) win = t;
  }
  if (counts) for (int32_t t = 0; t < trials; ++t) counts[t] = int32_t(cnt[t]);
  if (valid) std::memcpy(valid, ok.data(), size_t(trials));
  std::memset(mask, 0, size_t(n));
  for (int a = 0; a < 8; ++a) plane[a] = 0.f;
  for (int a = 0; a < 3; ++a) plane[4 + a] = c[a];
  ints[0] = 0; ints[1] = int64_t(m); ints[2] = win; ints[3] = nvalid;
  if (win < 0) return;
  Plane P = cand[win];
  std::vector<uint64_t> in;                                 // positions of the alive list, ascending
  auto recount = [&]() {
    in.clear();
    for (uint64_t p = 0; p < m; ++p) if (inlier(P, &X[3 * p], distance)) in.push_back(p);
  };
  recount();
  for (int32_t r = 0; r < refine; ++r) {
    const int64_t k = int64_t(in.size());
    if (k < 3) break;
    double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t b0 = 0; b0 < k; b0 += kSumBlock) {
      double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      for (int64_t j = b0; j < std::min(k, b0 + kSumBlock); ++j) {
        const double e[3] = {double(X[3 * in[j]]), double(X[3 * in[j] + 1]), double(X[3 * in[j] + 2])};
        s[0] += e[0]; s[1] += e[1]; s[2] += e[2];
        s[3] += e[0] * e[0]; s[4] += e[0] * e[1]; s[5] += e[0] * e[2]; s[6] += e[1] * e[1]; s[7] += e[1] * e[2]; s[8] += e[2] * e[2];
      }
      for (int a = 0; a < 9; ++a) S[a] += s[a];
    }
    const double kk = double(k);
    const double mean[3] = {S[0] / kk, S[1] / kk, S[2] / kk};
    double C[3][3], V[3][3];
    C[0][0] = S[3] / kk - mean[0] * mean[0]; C[0][1] = S[4] / kk - mean[0] * mean[1]; C[0][2] = S[5] / kk - mean[0] * mean[2];
    C[1][1] = S[6] / kk - mean[1] * mean[1]; C[1][2] = S[7] / kk - mean[1] * mean[2]; C[2][2] = S[8] / kk - mean[2] * mean[2];
    C[1][0] = C[0][1]; C[2][0] = C[0][2]; C[2][1] = C[1][2];
    const double tr = (C[0][0] + C[1][1]) + C[2][2];
    if (!(tr > 0.0)) break;
    jacobi3(C, V);
    int best = 0;
    for (int a = 1; a < 3; ++a) if (C[a][a] < C[best][best]) best = a;
    double v[3] = {V[0][best], V[1][best], V[2][best]};
    const double len = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    for (double& e : v) e /= len;
    sign_rule(v);
    for (int a = 0; a < 3; ++a) P.n[a] = float(v[a]);
    P.d = float(-((v[0] * mean[0] + v[1] * mean[1]) + v[2] * mean[2]));
    recount();
  }
  for (uint64_t p : in) mask[alive[p]] = 1;
  for (int a = 0; a < 3; ++a) plane[a] = P.n[a];
  plane[3] = float(double(P.d) - ((double(P.n[0]) * double(c[0]) + double(P.n[1]) * double(c[1])) + double(P.n[2]) * double(c[2])));
  plane[7] = P.d;
  ints[0] = int64_t(in.size());
}

}  // extern "C"
