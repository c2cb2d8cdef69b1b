// CPU restatement of the target-normal neighbourhoods of libsuper4pcs_icp.so (include/s4p_icp_plane.h), written
// independently of the device code: a dense grid of edge >= r whose search range per axis is [p - r', p + r'],
// r' = r (1 + 1e-5), checks EVERY point in that range (no box pruning).
// Per target point: k = |N(i)| and the covariance C = sum e e^T / k - m m^T (xx xy xz yy yz zz) in double; the eigenvector
// is taken in numpy (tests/icp_plane_helpers.py).  Compiled with g++ -O2 -ffp-contract=off -fopenmp.
#include <omp.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace {

inline bool within(const float* p[3], int64_t i, int64_t j, float r2) {
  const float dx = p[0][i] - p[0][j], dy = p[1][i] - p[1][j], dz = p[2][i] - p[2][j];
  return dx * dx + (dy * dy + dz * dz) <= r2;
}

// neighbours of i, in any order: k and C
void covariance(const float* p[3], int64_t i, const std::vector<int64_t>& nb, int32_t* k, double* c6) {
  double se[3] = {0, 0, 0}, see[6] = {0, 0, 0, 0, 0, 0};
  for (int64_t j : nb) {
    const double e0 = double(p[0][j]) - double(p[0][i]), e1 = double(p[1][j]) - double(p[1][i]), e2 = double(p[2][j]) - double(p[2][i]);
    se[0] += e0; se[1] += e1; se[2] += e2;
    see[0] += e0 * e0; see[1] += e0 * e1; see[2] += e0 * e2; see[3] += e1 * e1; see[4] += e1 * e2; see[5] += e2 * e2;
  }
  const double n = double(nb.size());
  *k = int32_t(nb.size());
  if (nb.empty()) { for (int a = 0; a < 6; ++a) c6[a] = 0.0; return; }
  const double m[3] = {se[0] / n, se[1] / n, se[2] / n};
  c6[0] = see[0] / n - m[0] * m[0]; c6[1] = see[1] / n - m[0] * m[1]; c6[2] = see[2] / n - m[0] * m[2];
  c6[3] = see[3] / n - m[1] * m[1]; c6[4] = see[4] / n - m[1] * m[2]; c6[5] = see[5] / n - m[2] * m[2];
}

}  // namespace

extern "C" {

// px.. = P' (centred target), n points; k[n], c6[6 n]
void icp_plane_cpu_cov(const float* px, const float* py, const float* pz, int64_t n, float r, int32_t* k, double* c6, int32_t threads) {
  const float* p[3] = {px, py, pz};
  double lo[3], hi[3];
  for (int a = 0; a < 3; ++a) {
    lo[a] = hi[a] = p[a][0];
    for (int64_t i = 1; i < n; ++i) { lo[a] = std::min(lo[a], double(p[a][i])); hi[a] = std::max(hi[a], double(p[a][i])); }
  }
  double h = double(r);
  int64_t dim[3];
  while (true) {
    double nc = 1;
    for (int a = 0; a < 3; ++a) { dim[a] = int64_t(std::floor((hi[a] - lo[a]) / h)) + 1; nc *= double(dim[a]); }
    if (nc <= 4.0 * double(n) + 64) break;
    h *= 1.5;
  }
  auto cell = [&](int a, double x) { return int64_t(std::floor((x - lo[a]) / h)); };
  const int64_t ncell = dim[0] * dim[1] * dim[2];
  std::vector<int64_t> key(n), start(ncell + 1, 0), items(n);
  for (int64_t i = 0; i < n; ++i) {
    key[i] = (cell(2, p[2][i]) * dim[1] + cell(1, p[1][i])) * dim[0] + cell(0, p[0][i]);
    ++start[key[i] + 1];
  }
  for (int64_t c = 0; c < ncell; ++c) start[c + 1] += start[c];
  std::vector<int64_t> fill(start.begin(), start.end() - 1);
  for (int64_t i = 0; i < n; ++i) items[fill[key[i]]++] = i;
  const float r2 = r * r;
  const double rr = double(r) * (1.0 + 1e-5) + 1e-9 * h;
  if (threads > 0) omp_set_num_threads(threads);
#pragma omp parallel
  {
    std::vector<int64_t> nb;
#pragma omp for schedule(dynamic, 256)
    for (int64_t i = 0; i < n; ++i) {
      int64_t l[3], u[3];
      for (int a = 0; a < 3; ++a) {
        l[a] = std::max<int64_t>(0, cell(a, double(p[a][i]) - rr));
        u[a] = std::min<int64_t>(dim[a] - 1, cell(a, double(p[a][i]) + rr));
      }
      nb.clear();
      for (int64_t cz = l[2]; cz <= u[2]; ++cz)
        for (int64_t cy = l[1]; cy <= u[1]; ++cy)
          for (int64_t cx = l[0]; cx <= u[0]; ++cx) {
            const int64_t c = (cz * dim[1] + cy) * dim[0] + cx;
            for (int64_t t = start[c]; t < start[c + 1]; ++t)
              if (within(p, i, items[t], r2)) nb.push_back(items[t]);
          }
      covariance(p, i, nb, &k[i], &c6[6 * i]);
    }
  }
}

}  // extern "C"
