// CPU restatement of the descriptor contract of libsuper4pcs_normals.so (include/s4p_feature.h), written independently of the
// device code, term by term: the valid points; the pairs with 0 < d2 <= fl(r*r); the Darboux frame of a pair with the source
// chosen by the larger |n . d|; the two linear bins and the angle bin against the header's ten boundary directions; the
// 32-bit counters and the SPFH rows S = H 2^15 / c; the weights 64 r^2 / d2 saturated at 2^16; the 64-bit sums A; the three
// normalisations to 4096.  Neighbours come from a plain grid of edge 1.001 r over sorted cell codes (binary search per row
// of cells), or, when asked or when the grid would not fit its codes, from brute force; both visit the points in another
// order than the device does, which integer sums do not see.  The matcher is brute force over every pair of rows.
// Compiled with g++ -O2 -ffp-contract=off -fopenmp (tests/feature_helpers.py).
#include <omp.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <vector>

#include "../../include/s4p_feature.h"

namespace {

const float kBounds[10][2] = S4P_FEATURE_THETA_BOUNDS;

float dot3(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

int bin11(float f) {
  const float t = 11.f * ((f + 1.f) * 0.5f);
  if (!(t >= 1.f)) return 0;
  if (t >= 10.f) return 10;
  return int(std::floor(t));
}

int bin_theta(float x, float y) {
  int bin = 0;
  for (int k = 1; k <= 10; ++k) {
    const float c = kBounds[k - 1][0] * y - kBounds[k - 1][1] * x;
    if (k <= 5) bin += (y >= 0.f || c >= 0.f) ? 1 : 0;
    else bin += (y >= 0.f && c >= 0.f) ? 1 : 0;
  }
  return bin;
}

// the bins (alpha, phi, theta) of the pair i -> j; false when it is skipped
bool pair_bins(const float ni[3], const float nj[3], const float d[3], float d2, int bins[3]) {
  const float len = std::sqrt(d2);
  const float ai = dot3(ni, d), aj = dot3(nj, d);
  const float *ns = ni, *nt = nj;
  float e[3] = {d[0], d[1], d[2]};
  if (!(std::fabs(ai) >= std::fabs(aj))) {
    ns = nj; nt = ni;
    for (float& c : e) c = -c;
  }
  const float phi = dot3(ns, e) / len;
  float v[3] = {e[1] * ns[2] - e[2] * ns[1], e[2] * ns[0] - e[0] * ns[2], e[0] * ns[1] - e[1] * ns[0]};
  const float vn = std::sqrt(dot3(v, v));
  if (!(vn > 0.f)) return false;
  for (float& c : v) c = c / vn;
  const float w[3] = {ns[1] * v[2] - ns[2] * v[1], ns[2] * v[0] - ns[0] * v[2], ns[0] * v[1] - ns[1] * v[0]};
  bins[0] = bin11(dot3(v, nt));
  bins[1] = bin11(phi);
  bins[2] = bin_theta(dot3(ns, nt), dot3(w, nt));
  return true;
}

struct Cloud {
  const float *x, *y, *z, *nrm;
  int64_t n;
  std::vector<uint8_t> valid;
  void p(int64_t i, float out[3]) const { out[0] = x[i]; out[1] = y[i]; out[2] = z[i]; }
  const float* normal(int64_t i) const { return nrm + 3 * i; }
};

// A plain grid of edge h over the bounds of the finite points: the points sorted by cell code (iz ny + iy) nx + ix.
struct Grid {
  bool ok = false;
  double lo[3] = {0, 0, 0}, h = 1.0;
  int64_t dim[3] = {1, 1, 1};
  std::vector<uint64_t> code;
  std::vector<int64_t> who;

  void build(const Cloud& C, double edge) {
    h = edge;
    const float* p[3] = {C.x, C.y, C.z};
    std::vector<int64_t> fin;
    for (int64_t i = 0; i < C.n; ++i)
      if (std::isfinite(C.x[i]) && std::isfinite(C.y[i]) && std::isfinite(C.z[i])) fin.push_back(i);
    if (fin.empty()) return;
    for (int a = 0; a < 3; ++a) {
      double mn = p[a][fin[0]], mx = mn;
      for (int64_t i : fin) { mn = std::min<double>(mn, p[a][i]); mx = std::max<double>(mx, p[a][i]); }
      lo[a] = mn;
      const double cells = std::floor((mx - mn) / h) + 1.0;
      if (!(cells <= double(1 << 20))) return;            // the codes would not fit: brute force instead
      dim[a] = int64_t(cells);
    }
    std::vector<uint64_t> c(fin.size());
    for (size_t t = 0; t < fin.size(); ++t) {
      int64_t k[3];
      for (int a = 0; a < 3; ++a) k[a] = std::min(std::max<int64_t>(int64_t(std::floor((double(p[a][fin[t]]) - lo[a]) / h)), 0), dim[a] - 1);
      c[t] = uint64_t((k[2] * dim[1] + k[1]) * dim[0] + k[0]);
    }
    std::vector<size_t> order(fin.size());
    std::iota(order.begin(), order.end(), size_t(0));
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return c[a] < c[b] || (c[a] == c[b] && a < b); });
    code.resize(fin.size()); who.resize(fin.size());
    for (size_t t = 0; t < fin.size(); ++t) { code[t] = c[order[t]]; who[t] = fin[order[t]]; }
    ok = true;
  }

  template <class F> void around(const float q[3], F&& f) const {
    int64_t c[3];
    for (int a = 0; a < 3; ++a) c[a] = std::min(std::max<int64_t>(int64_t(std::floor((double(q[a]) - lo[a]) / h)), 0), dim[a] - 1);
    const int64_t x0 = std::max<int64_t>(c[0] - 1, 0), x1 = std::min(c[0] + 1, dim[0] - 1);
    for (int64_t iz = std::max<int64_t>(c[2] - 1, 0); iz <= std::min(c[2] + 1, dim[2] - 1); ++iz)
      for (int64_t iy = std::max<int64_t>(c[1] - 1, 0); iy <= std::min(c[1] + 1, dim[1] - 1); ++iy) {
        const uint64_t base = uint64_t((iz * dim[1] + iy) * dim[0]);
        const auto b = std::lower_bound(code.begin(), code.end(), base + uint64_t(x0));
        const auto e = std::upper_bound(b, code.end(), base + uint64_t(x1));
        for (int64_t t = b - code.begin(); t < e - code.begin(); ++t) f(who[t]);
      }
  }
};

// f(j, d, d2) for every pair of the valid point i
template <class F> void pairs_of(const Cloud& C, const Grid& G, int64_t i, float r2, F&& f) {
  float pi[3];
  C.p(i, pi);
  auto test = [&](int64_t j) {
    if (!C.valid[j]) return;
    float pj[3];
    C.p(j, pj);
    const float d[3] = {pj[0] - pi[0], pj[1] - pi[1], pj[2] - pi[2]};
    const float d2 = d[0] * d[0] + (d[1] * d[1] + d[2] * d[2]);
    if (!(d2 > 0.f && d2 <= r2)) return;
    f(j, d, d2);
  };
  if (G.ok) G.around(pi, test);
  else for (int64_t j = 0; j < C.n; ++j) test(j);
}

}  // namespace

extern "C" {

// fpfh[33 n]; count[n] and spfh[33 n] (the S rows, for the numpy statement) may be null.  brute != 0: every point for every
// point.
void feature_cpu_fpfh(const float* px, const float* py, const float* pz, int64_t n, const float* normals, float r, uint16_t* fpfh,
                      int32_t* count, uint16_t* spfh, int32_t threads, int32_t brute) {
  Cloud C{px, py, pz, normals, n, {}};
  C.valid.resize(size_t(n));
  for (int64_t i = 0; i < n; ++i) {
    const float* m = C.normal(i);
    C.valid[i] = std::isfinite(px[i]) && std::isfinite(py[i]) && std::isfinite(pz[i]) && std::isfinite(m[0]) && std::isfinite(m[1]) &&
                 std::isfinite(m[2]) && (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2] > 0.f;
  }
  const float r2 = r * r;
  Grid G;
  if (!brute && n > 0) G.build(C, 1.001 * double(r));
  std::vector<uint16_t> S(size_t(33) * size_t(n), uint16_t(0));
  const int nt = threads > 0 ? threads : 16;
#pragma omp parallel for schedule(dynamic, 64) num_threads(nt)
  for (int64_t i = 0; i < n; ++i) {
    uint32_t H[33] = {0};
    uint32_t c = 0;
    if (C.valid[i])
      pairs_of(C, G, i, r2, [&](int64_t j, const float d[3], float d2) {
        int b[3];
        if (!pair_bins(C.normal(i), C.normal(j), d, d2, b)) return;
        ++c;
        ++H[b[0]]; ++H[11 + b[1]]; ++H[22 + b[2]];
      });
    if (c)
      for (int b = 0; b < 33; ++b) S[33 * i + b] = uint16_t((uint64_t(H[b]) << 15) / c);
    if (count) count[i] = int32_t(c);
  }
#pragma omp parallel for schedule(dynamic, 64) num_threads(nt)
  for (int64_t i = 0; i < n; ++i) {
    uint64_t A[33] = {0};
    if (C.valid[i])
      pairs_of(C, G, i, r2, [&](int64_t j, const float*, float d2) {
        const uint64_t q = uint64_t(int64_t(std::fmin(64.f * (r2 / d2), 65536.f)));
        for (int b = 0; b < 33; ++b) A[b] += q * S[33 * j + b];
      });
    for (int g = 0; g < 3; ++g) {
      uint64_t T = 0;
      for (int b = 0; b < 11; ++b) T += A[11 * g + b];
      for (int b = 0; b < 11; ++b) fpfh[33 * i + 11 * g + b] = T ? uint16_t(std::floor((double(A[11 * g + b]) / double(T)) * 4096.0)) : uint16_t(0);
    }
  }
  if (spfh) std::copy(S.begin(), S.end(), spfh);
}

// idx[m], dist[m] (may be null).  Returns -1 when a value exceeds S4P_FEATURE_MAX (nothing written), else 0.
int32_t feature_cpu_match(const uint16_t* fa, int64_t m, const uint16_t* fb, int64_t n, int32_t mutual, int32_t* idx, int32_t* dist,
                          int32_t threads) {
  for (int64_t t = 0; t < 33 * m; ++t) if (fa[t] > S4P_FEATURE_MAX) return -1;
  for (int64_t t = 0; t < 33 * n; ++t) if (fb[t] > S4P_FEATURE_MAX) return -1;
  auto usable = [](const uint16_t* row) { for (int k = 0; k < 33; ++k) if (row[k]) return true; return false; };
  auto D = [](const uint16_t* a, const uint16_t* b) {
    int32_t s = 0;
    for (int k = 0; k < 33; ++k) { const int32_t d = int32_t(a[k]) - int32_t(b[k]); s += d * d; }
    return s;
  };
  // best[r] over the usable rows of `cols`: the smallest (D, index)
  auto best = [&](const uint16_t* rows, int64_t nr, const uint16_t* cols, int64_t nc, std::vector<int64_t>& bi, std::vector<int32_t>& bd) {
    bi.assign(size_t(nr), -1); bd.assign(size_t(nr), -1);
    std::vector<uint8_t> ok(static_cast<size_t>(nc), uint8_t(0));
    for (int64_t c = 0; c < nc; ++c) ok[c] = usable(cols + 33 * c);
#pragma omp parallel for schedule(static) num_threads(threads > 0 ? threads : 16)
    for (int64_t r = 0; r < nr; ++r) {
      if (!usable(rows + 33 * r)) continue;
      for (int64_t c = 0; c < nc; ++c) {
        if (!ok[c]) continue;
        const int32_t d = D(rows + 33 * r, cols + 33 * c);
        if (bi[r] < 0 || d < bd[r]) { bi[r] = c; bd[r] = d; }
      }
    }
  };
  std::vector<int64_t> ia, ib;
  std::vector<int32_t> da, db;
  best(fa, m, fb, n, ia, da);
  if (mutual) best(fb, n, fa, m, ib, db);
  for (int64_t a = 0; a < m; ++a) {
    int64_t b = ia[a];
    if (b >= 0 && mutual && ib[b] != a) b = -1;
    idx[a] = int32_t(b);
    if (dist) dist[a] = b >= 0 ? da[a] : -1;
  }
  return 0;
}

}  // extern "C"
