// CPU restatement of the correspondence contract and the per-iteration sums of libsuper4pcs_icp.so (include/s4p_icp.h),
// written independently of the device code: a dense grid of edge >= d whose search range per axis is
// [q - r, q + r], r = d (1 + 1e-5), checks EVERY point in that range (no box pruning), and a brute force over all of P.
// Compiled by tests/icp_helpers.py with g++ -O2 -ffp-contract=off -fopenmp.
#include <omp.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace {

struct Grid {
  double o[3], h;
  int64_t n[3];
  std::vector<int64_t> start;
  std::vector<int32_t> items;
  int64_t cell(int a, double x) const { return int64_t(std::floor((x - o[a]) / h)); }
};

void build_grid(Grid& g, const float* p[3], int64_t np, float d) {
  double lo[3], hi[3];
  for (int a = 0; a < 3; ++a) {
    lo[a] = hi[a] = p[a][0];
    for (int64_t i = 1; i < np; ++i) { lo[a] = std::min(lo[a], double(p[a][i])); hi[a] = std::max(hi[a], double(p[a][i])); }
  }
  g.h = double(d);
  while (true) {
    double nc = 1;
    for (int a = 0; a < 3; ++a) { g.o[a] = lo[a]; g.n[a] = int64_t(std::floor((hi[a] - lo[a]) / g.h)) + 1; nc *= double(g.n[a]); }
    if (nc <= 4.0 * double(np) + 64) break;
    g.h *= 1.5;
  }
  const int64_t ncell = g.n[0] * g.n[1] * g.n[2];
  std::vector<int64_t> key(np);
  g.start.assign(ncell + 1, 0);
  for (int64_t i = 0; i < np; ++i) {
    key[i] = (g.cell(2, p[2][i]) * g.n[1] + g.cell(1, p[1][i])) * g.n[0] + g.cell(0, p[0][i]);
    ++g.start[key[i] + 1];
  }
  for (int64_t c = 0; c < ncell; ++c) g.start[c + 1] += g.start[c];
  std::vector<int64_t> fill(g.start.begin(), g.start.end() - 1);
  g.items.resize(np);
  for (int64_t i = 0; i < np; ++i) g.items[fill[key[i]]++] = int32_t(i);
}

inline void apply(const float* T, float x, float y, float z, float& ox, float& oy, float& oz) {
  ox = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
  oy = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
  oz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
}

inline void consider(const float* p[3], int32_t i, float x, float y, float z, float& best, int32_t& bi) {
  const float dx = x - p[0][i], dy = y - p[1][i], dz = z - p[2][i];
  const float d2 = dx * dx + (dy * dy + dz * dz);
  if (d2 < best || (d2 == best && (bi < 0 || i < bi))) { best = d2; bi = i; }
}

void nearest(const Grid& g, const float* p[3], float x, float y, float z, float d, float d2max, float& best, int32_t& bi) {
  best = d2max;
  bi = -1;
  const double r = double(d) * (1.0 + 1e-5) + 1e-9 * g.h;
  const double q[3] = {x, y, z};
  int64_t lo[3], hi[3];
  for (int a = 0; a < 3; ++a) {
    if (!std::isfinite(q[a])) return;
    lo[a] = std::max<int64_t>(0, g.cell(a, q[a] - r));
    hi[a] = std::min<int64_t>(g.n[a] - 1, g.cell(a, q[a] + r));
    if (lo[a] > hi[a]) return;
  }
  for (int64_t cz = lo[2]; cz <= hi[2]; ++cz)
    for (int64_t cy = lo[1]; cy <= hi[1]; ++cy)
      for (int64_t cx = lo[0]; cx <= hi[0]; ++cx) {
        const int64_t c = (cz * g.n[1] + cy) * g.n[0] + cx;
        for (int64_t k = g.start[c]; k < g.start[c + 1]; ++k) consider(p, g.items[k], x, y, z, best, bi);
      }
  if (bi < 0) best = 0.f;
}

}  // namespace

extern "C" {

// px.. = P' (centred target), qx.. = Q' (centred source); T12 = rows 0..2 of the float 4x4 (centred frame)
// idx / d2 may be null; sums17 may be null.  Returns the number of matched source points.
int64_t icp_cpu_pass(const float* px, const float* py, const float* pz, int64_t np, const float* qx, const float* qy,
                     const float* qz, int64_t nq, const float* T12, float d, int32_t* idx, float* d2out, double* sums17,
                     int32_t threads) {
  const float* p[3] = {px, py, pz};
  Grid g;
  build_grid(g, p, np, d);
  const float d2max = d * d;
  if (threads > 0) omp_set_num_threads(threads);
  const int nt = omp_get_max_threads();
  std::vector<double> part(size_t(nt) * 17, 0.0);
#pragma omp parallel
  {
    double* s = &part[size_t(omp_get_thread_num()) * 17];
#pragma omp for schedule(static)
    for (int64_t j = 0; j < nq; ++j) {
      float x, y, z, best;
      int32_t bi;
      apply(T12, qx[j], qy[j], qz[j], x, y, z);
      nearest(g, p, x, y, z, d, d2max, best, bi);
      if (idx) idx[j] = bi;
      if (d2out) d2out[j] = bi < 0 ? 0.f : best;
      if (bi >= 0) {
        const double qd[3] = {x, y, z}, pd[3] = {p[0][bi], p[1][bi], p[2][bi]};
        s[0] += 1.0;
        for (int a = 0; a < 3; ++a) { s[1 + a] += qd[a]; s[4 + a] += pd[a]; }
        for (int a = 0; a < 3; ++a)
          for (int b = 0; b < 3; ++b) s[7 + 3 * a + b] += qd[a] * pd[b];
        s[16] += double(best);
      }
    }
  }
  double tot[17] = {0};
  for (int t = 0; t < nt; ++t)
    for (int k = 0; k < 17; ++k) tot[k] += part[size_t(t) * 17 + k];
  if (sums17)
    for (int k = 0; k < 17; ++k) sums17[k] = tot[k];
  return int64_t(tot[0]);
}

// the same contract by brute force over all of P (small clouds)
void icp_cpu_brute(const float* px, const float* py, const float* pz, int64_t np, const float* qx, const float* qy, const float* qz,
                   int64_t nq, const float* T12, float d, int32_t* idx, float* d2out) {
  const float* p[3] = {px, py, pz};
  const float d2max = d * d;
#pragma omp parallel for schedule(static)
  for (int64_t j = 0; j < nq; ++j) {
    float x, y, z, best = d2max;
    int32_t bi = -1;
    apply(T12, qx[j], qy[j], qz[j], x, y, z);
    for (int64_t i = 0; i < np; ++i) consider(p, int32_t(i), x, y, z, best, bi);
    idx[j] = bi;
    d2out[j] = bi < 0 ? 0.f : best;
  }
}

}  // extern "C"
