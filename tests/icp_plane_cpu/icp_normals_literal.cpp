// Literal CPU restatement of k_normals of libsuper4pcs_icp.so (super4pcs_amd/icp_src/s4p_icp_k_build.hip.hpp), for bit-for-bit
// comparison of the estimated target normals: set_target's grid plan in the same double arithmetic, the target in cell
// order (cells ascending, original index ascending inside a cell: the device's radix sort is stable), the 27 cells around a
// point visited in k_normals' order with the neighbours of a cell in cell order, so that every double sum adds the same
// terms in the same order; then the same covariance, the same cyclic Jacobi and the same choice and sign of the
// eigenvector.  Box pruning is not restated: a pruned cell holds no point within r, so it contributes no term.
// Compiled with g++ -O2 -ffp-contract=off -fopenmp, as the device code is with -ffp-contract=off.
#include <omp.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace {

constexpr int kJacobiSweeps = 64;

inline double cell_coord(float x, double o, double inv_h) { return std::floor((double(x) - o) * inv_h); }

void jacobi3(double (&A)[3][3], double (&V)[3][3]) {
  constexpr int N = 3;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < N; ++i) {
      diag += A[i][i] * A[i][i];
      for (int j = i + 1; j < N; ++j) off += A[i][j] * A[i][j];
    }
    if (off == 0.0 || off <= 1e-36 * diag) break;
    for (int p = 0; p < N - 1; ++p)
      for (int q = p + 1; q < N; ++q) {
        if (A[p][q] == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < N; ++k) {
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < N; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < N; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq;
        }
      }
  }
}

}  // namespace

// x, y, z: the centred target P' = fl(P - c), n points.  d: set_target's max_distance.  radius, min_nb: estimate_normals'.
// which[m]: the target indices wanted.  out[3 m]: their normals.  dims_out[3], h_out: the plan (for the caller's asserts).
// Returns 0, or -1 if no grid fits.
extern "C" int32_t icp_normals_literal(const float* x, const float* y, const float* z, int64_t n, float d, float radius, int32_t min_nb,
                                       const int64_t* which, int64_t m, float* out, int32_t* dims_out, double* h_out, int32_t threads) {
  const float* p[3] = {x, y, z};
  float plo[3], phi[3];
  for (int a = 0; a < 3; ++a) {
    plo[a] = *std::min_element(p[a], p[a] + n);
    phi[a] = *std::max_element(p[a], p[a] + n);
  }
  const uint64_t cap = std::min<uint64_t>(1ull << 28, std::max<uint64_t>(1ull << 20, 2 * uint64_t(n)));
  double hh = double(d) * double(1.02f), inv = 0.0;
  int dims[3];
  uint64_t ncell = 0;
  for (int guard = 0;; ++guard) {
    inv = 1.0 / hh;
    bool ok = true;
    uint64_t nc = 1;
    for (int a = 0; a < 3; ++a) {
      const double cc = cell_coord(phi[a], double(plo[a]), inv);
      if (!(cc < 1.0e9)) { ok = false; break; }
      dims[a] = int(cc) + 1;
      nc *= uint64_t(dims[a]);
      if (nc > cap) { ok = false; break; }
    }
    if (ok) { ncell = nc; break; }
    if (guard > 400) return -1;
    hh *= 1.25;
  }
  const double o[3] = {double(plo[0]), double(plo[1]), double(plo[2])};
  for (int a = 0; a < 3; ++a) dims_out[a] = dims[a];
  *h_out = hh;
  // cell order: a stable counting sort by cell key
  std::vector<uint32_t> key(n), start(ncell + 1, 0), order(n);
  for (int64_t i = 0; i < n; ++i) {
    const int ix = int(cell_coord(x[i], o[0], inv)), iy = int(cell_coord(y[i], o[1], inv)), iz = int(cell_coord(z[i], o[2], inv));
    key[i] = (uint32_t(iz) * uint32_t(dims[1]) + uint32_t(iy)) * uint32_t(dims[0]) + uint32_t(ix);
    ++start[key[i] + 1];
  }
  for (uint64_t c = 0; c < ncell; ++c) start[c + 1] += start[c];
  {
    std::vector<uint32_t> fill(start.begin(), start.end() - 1);
    for (int64_t i = 0; i < n; ++i) order[fill[key[i]]++] = uint32_t(i);
  }
  const float r2 = radius * radius;
  if (threads > 0) omp_set_num_threads(threads);
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t w = 0; w < m; ++w) {
    const int64_t i = which[w];
    const float px = x[i], py = y[i], pz = z[i];
    const int cx = int(cell_coord(px, o[0], inv)), cy = int(cell_coord(py, o[1], inv)), cz = int(cell_coord(pz, o[2], inv));
    const double qx = double(px), qy = double(py), qz = double(pz);
    double se[3] = {0.0, 0.0, 0.0}, see[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int32_t cnt = 0;
    for (int t = 0; t < 27; ++t) {
      const int ix = cx + t % 3 - 1, iy = cy + (t / 3) % 3 - 1, iz = cz + t / 9 - 1;
      if (ix < 0 || ix >= dims[0] || iy < 0 || iy >= dims[1] || iz < 0 || iz >= dims[2]) continue;
      const uint32_t c = (uint32_t(iz) * uint32_t(dims[1]) + uint32_t(iy)) * uint32_t(dims[0]) + uint32_t(ix);
      for (uint32_t s = start[c]; s < start[c + 1]; ++s) {
        const uint32_t j = order[s];
        const float dx = px - x[j], dy = py - y[j], dz = pz - z[j];
        if (dx * dx + (dy * dy + dz * dz) > r2) continue;
        const double e0 = double(x[j]) - qx, e1 = double(y[j]) - qy, e2 = double(z[j]) - qz;
        ++cnt;
        se[0] += e0; se[1] += e1; se[2] += e2;
        see[0] += e0 * e0; see[1] += e0 * e1; see[2] += e0 * e2; see[3] += e1 * e1; see[4] += e1 * e2; see[5] += e2 * e2;
      }
    }
    float v[3] = {0.f, 0.f, 0.f};
    if (cnt >= min_nb) {
      const double kk = double(cnt);
      const double m0 = se[0] / kk, m1 = se[1] / kk, m2 = se[2] / kk;
      double C[3][3], V[3][3];
      C[0][0] = see[0] / kk - m0 * m0; C[0][1] = see[1] / kk - m0 * m1; C[0][2] = see[2] / kk - m0 * m2;
      C[1][1] = see[3] / kk - m1 * m1; C[1][2] = see[4] / kk - m1 * m2; C[2][2] = see[5] / kk - m2 * m2;
      C[1][0] = C[0][1]; C[2][0] = C[0][2]; C[2][1] = C[1][2];
      jacobi3(C, V);
      int best = 0;
      if (C[1][1] < C[best][best]) best = 1;
      if (C[2][2] < (best == 0 ? C[0][0] : C[1][1])) best = 2;
      double v0 = V[0][best], v1 = V[1][best], v2 = V[2][best];
      const double nv = std::sqrt(v0 * v0 + v1 * v1 + v2 * v2);
      v0 /= nv; v1 /= nv; v2 /= nv;
      const double a0 = std::fabs(v0), a1 = std::fabs(v1), a2 = std::fabs(v2);
      const double lead = (a0 >= a1 && a0 >= a2) ? v0 : (a1 >= a2 ? v1 : v2);
      if (lead < 0.0) { v0 = -v0; v1 = -v1; v2 = -v2; }
      v[0] = float(v0); v[1] = float(v1); v[2] = float(v2);
    }
    out[3 * w] = v[0]; out[3 * w + 1] = v[1]; out[3 * w + 2] = v[2];
  }
  return 0;
}
