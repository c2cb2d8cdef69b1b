// CPU restatement of the normal-estimation contract of libsuper4pcs_normals.so (include/s4p_normals.h), written
// independently of the device code: brute-force kNN (every point of the cloud for every query) with the same float d2,
// neighbours ordered by (d2, index), the covariance in double in that order, and the same cyclic 3x3 Jacobi.
// Compiled with g++ -O2 -ffp-contract=off -fopenmp (tests/normals_helpers.py).
#include <omp.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

namespace {

using Hit = std::pair<float, int64_t>;      // (d2, index): std::pair's order is the contract's lexicographic order

// N(q) in ascending (d2, index) order
void knn(const float* p[3], int64_t n, const float q[3], int k, float r2lim, std::vector<Hit>& out) {
  out.clear();
  for (int64_t j = 0; j < n; ++j) {
    const float dx = p[0][j] - q[0], dy = p[1][j] - q[1], dz = p[2][j] - q[2];
    const float d2 = dx * dx + (dy * dy + dz * dz);
    if (!(d2 <= r2lim)) continue;
    const Hit h(d2, j);
    if (int(out.size()) < k) {
      out.push_back(h);
      std::push_heap(out.begin(), out.end());
    } else if (h < out.front()) {
      std::pop_heap(out.begin(), out.end());
      out.back() = h;
      std::push_heap(out.begin(), out.end());
    }
  }
  std::sort(out.begin(), out.end());
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

void normal_of(const float* p[3], const float q[3], const std::vector<Hit>& nb, float* out) {
  out[0] = out[1] = out[2] = 0.f;
  if (nb.size() < 3) return;
  double se[3] = {0, 0, 0}, see[6] = {0, 0, 0, 0, 0, 0};
  for (const Hit& h : nb) {
    const double e[3] = {double(p[0][h.second]) - double(q[0]), double(p[1][h.second]) - double(q[1]), double(p[2][h.second]) - double(q[2])};
    for (int a = 0; a < 3; ++a) se[a] += e[a];
    see[0] += e[0] * e[0]; see[1] += e[0] * e[1]; see[2] += e[0] * e[2]; see[3] += e[1] * e[1]; see[4] += e[1] * e[2]; see[5] += e[2] * e[2];
  }
  const double k = double(nb.size());
  const double m[3] = {se[0] / k, se[1] / k, se[2] / k};
  double C[3][3], V[3][3];
  C[0][0] = see[0] / k - m[0] * m[0]; C[0][1] = see[1] / k - m[0] * m[1]; C[0][2] = see[2] / k - m[0] * m[2];
  C[1][1] = see[3] / k - m[1] * m[1]; C[1][2] = see[4] / k - m[1] * m[2]; C[2][2] = see[5] / k - m[2] * m[2];
  C[1][0] = C[0][1]; C[2][0] = C[0][2]; C[2][1] = C[1][2];
  if (!((C[0][0] + C[1][1]) + C[2][2] > 0.0)) return;
  jacobi3(C, V);
  int best = 0;
  for (int a = 1; a < 3; ++a) if (C[a][a] < C[best][best]) best = a;
  double v[3] = {V[0][best], V[1][best], V[2][best]};
  const double len = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  for (double& x : v) x /= len;
  int lead = 0;
  for (int a = 1; a < 3; ++a) if (std::fabs(v[a]) > std::fabs(v[lead])) lead = a;
  const double sg = v[lead] < 0.0 ? -1.0 : 1.0;
  for (int a = 0; a < 3; ++a) out[a] = float(sg * v[a]);
}

float r2_of(float r) { return r > 0.f ? r * r : INFINITY; }

}  // namespace

extern "C" {

// idx[m * k] (-1 padded), cnt[m]: N(q) of every query in ascending (d2, index) order
void normals_cpu_knn(const float* px, const float* py, const float* pz, int64_t n, const float* qx, const float* qy, const float* qz,
                     int64_t m, int32_t k, float r, int32_t* idx, int32_t* cnt, int32_t threads) {
  const float* p[3] = {px, py, pz};
  if (threads > 0) omp_set_num_threads(threads);
#pragma omp parallel
  {
    std::vector<Hit> nb;
#pragma omp for schedule(dynamic, 64)
    for (int64_t i = 0; i < m; ++i) {
      const float q[3] = {qx[i], qy[i], qz[i]};
      knn(p, n, q, k, r2_of(r), nb);
      cnt[i] = int32_t(nb.size());
      for (int t = 0; t < k; ++t) idx[i * k + t] = t < int(nb.size()) ? int32_t(nb[t].second) : -1;
    }
  }
}

// out[3 m]: the normal of every query
void normals_cpu_normals(const float* px, const float* py, const float* pz, int64_t n, const float* qx, const float* qy, const float* qz,
                         int64_t m, int32_t k, float r, float* out, int32_t threads) {
  const float* p[3] = {px, py, pz};
  if (threads > 0) omp_set_num_threads(threads);
#pragma omp parallel
  {
    std::vector<Hit> nb;
#pragma omp for schedule(dynamic, 64)
    for (int64_t i = 0; i < m; ++i) {
      const float q[3] = {qx[i], qy[i], qz[i]};
      if (!std::isfinite(q[0]) || !std::isfinite(q[1]) || !std::isfinite(q[2])) { out[3 * i] = out[3 * i + 1] = out[3 * i + 2] = 0.f; continue; }
      knn(p, n, q, k, r2_of(r), nb);
      normal_of(p, q, nb, out + 3 * i);
    }
  }
}

// out[3 m]: the normal of every query from the lists it is given (idx[m * k], -1 padded), taken in list order: what the
// contract makes of exactly those neighbours, whoever found them
void normals_cpu_normals_of_lists(const float* px, const float* py, const float* pz, const float* qx, const float* qy, const float* qz,
                                  int64_t m, int32_t k, const int32_t* idx, float* out) {
  const float* p[3] = {px, py, pz};
  std::vector<Hit> nb;
  for (int64_t i = 0; i < m; ++i) {
    const float q[3] = {qx[i], qy[i], qz[i]};
    nb.clear();
    for (int t = 0; t < k; ++t)
      if (idx[i * k + t] >= 0) nb.push_back(Hit(0.f, idx[i * k + t]));
    normal_of(p, q, nb, out + 3 * i);
  }
}

}  // extern "C"
