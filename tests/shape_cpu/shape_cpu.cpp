// CPU restatement of the radius-normals contract of libsuper4pcs_normals.so (include/s4p_shape.h), written independently of
// the device code, term by term: the float d2 and the bound fl(r*r); the offsets of the accepted neighbours quantised to
// r 2^-18 by rint in double; the nine moments as 64-bit integer sums; the covariance in double; the cyclic 3x3 Jacobi; the
// normal with its sign rule; the eigenvalues unclamped, sorted, scaled by ldexp.  Neighbours come from a plain grid of edge
// 1.001 r over sorted cell codes (binary search per row of cells), or, when asked or when the grid would not fit its codes,
// from brute force; both visit the points in another order than the device does, which integer sums do not see.  The largest
// |u| met is returned, so that the tests can assert the contract's bound 2^19 + 1.
// Compiled with g++ -O2 -ffp-contract=off -fopenmp (tests/shape_helpers.py).
#include <omp.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <vector>

namespace {

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

struct Moments {
  int32_t count = 0;
  int64_t S[3] = {0, 0, 0};
  int64_t Q[6] = {0, 0, 0, 0, 0, 0};      // xx, xy, xz, yy, yz, zz
  int64_t umax = 0;
  // the point p against the query q
  void test(const float p[3], const float q[3], float r2, double scale) {
    const float dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
    const float d2 = dx * dx + (dy * dy + dz * dz);
    if (!(d2 <= r2)) return;
    const float e[3] = {dx, dy, dz};
    int64_t u[3];
    for (int a = 0; a < 3; ++a) {
      u[a] = int64_t(std::rint(double(e[a]) * scale));
      umax = std::max<int64_t>(umax, u[a] < 0 ? -u[a] : u[a]);
    }
    ++count;
    for (int a = 0; a < 3; ++a) S[a] += u[a];
    Q[0] += u[0] * u[0]; Q[1] += u[0] * u[1]; Q[2] += u[0] * u[2]; Q[3] += u[1] * u[1]; Q[4] += u[1] * u[2]; Q[5] += u[2] * u[2];
  }
};

// normal[3], eig[3] of one row from its moments
void solve(const Moments& M, int32_t need, int s, float* normal, float* eig) {
  for (int a = 0; a < 3; ++a) normal[a] = eig[a] = 0.f;
  if (M.count < need) return;
  const double k = double(M.count);
  const double m[3] = {double(M.S[0]) / k, double(M.S[1]) / k, double(M.S[2]) / k};
  double C[3][3], V[3][3];
  C[0][0] = double(M.Q[0]) / k - m[0] * m[0]; C[0][1] = double(M.Q[1]) / k - m[0] * m[1]; C[0][2] = double(M.Q[2]) / k - m[0] * m[2];
  C[1][1] = double(M.Q[3]) / k - m[1] * m[1]; C[1][2] = double(M.Q[4]) / k - m[1] * m[2]; C[2][2] = double(M.Q[5]) / k - m[2] * m[2];
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
  const bool flip = v[lead] < 0.0;
  for (int a = 0; a < 3; ++a) normal[a] = float(flip ? -v[a] : v[a]);
  double l[3] = {C[0][0], C[1][1], C[2][2]};
  std::sort(l, l + 3, [](double a, double b) { return a > b; });
  for (int a = 0; a < 3; ++a) eig[a] = float(std::ldexp(l[a], -2 * s));
}

// A plain grid of edge h over the cloud's bounds: the points sorted by cell code (iz ny + iy) nx + ix.
struct Grid {
  bool ok = false;
  double lo[3] = {0, 0, 0}, h = 1.0;
  int64_t dim[3] = {1, 1, 1};
  std::vector<uint64_t> code;         // ascending
  std::vector<float> x, y, z;         // in that order

  int64_t cell(double v, int a) const { return int64_t(std::floor((v - lo[a]) / h)); }

  void build(const float* p[3], int64_t n, double edge) {
    h = edge;
    double hi[3];
    for (int a = 0; a < 3; ++a) {
      lo[a] = *std::min_element(p[a], p[a] + n);
      hi[a] = *std::max_element(p[a], p[a] + n);
      const double cells = std::floor((hi[a] - lo[a]) / h) + 1.0;
      if (!(cells <= double(1 << 20))) return;          // the codes would not fit: brute force instead
      dim[a] = int64_t(cells);
    }
    std::vector<uint64_t> c(n);
    for (int64_t i = 0; i < n; ++i) {
      int64_t k[3];
      for (int a = 0; a < 3; ++a) k[a] = std::min(std::max<int64_t>(cell(p[a][i], a), 0), dim[a] - 1);
      c[i] = uint64_t((k[2] * dim[1] + k[1]) * dim[0] + k[0]);
    }
    std::vector<int64_t> order(n);
    std::iota(order.begin(), order.end(), int64_t(0));
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return c[a] < c[b] || (c[a] == c[b] && a < b); });
    code.resize(n); x.resize(n); y.resize(n); z.resize(n);
    for (int64_t i = 0; i < n; ++i) { code[i] = c[order[i]]; x[i] = p[0][order[i]]; y[i] = p[1][order[i]]; z[i] = p[2][order[i]]; }
    ok = true;
  }

  // every point in the 3 x 3 x 3 cells around q's cell (not clamped: a position outside the bounds has fewer cells)
  void walk(const float q[3], float r2, double scale, Moments& M) const {
    int64_t c[3];
    for (int a = 0; a < 3; ++a) {
      const double t = std::floor((double(q[a]) - lo[a]) / h);
      c[a] = int64_t(std::min(std::max(t, -3.0), double(dim[a]) + 2.0));
    }
    const int64_t x0 = std::max<int64_t>(c[0] - 1, 0), x1 = std::min(c[0] + 1, dim[0] - 1);
    if (x0 > x1) return;
    for (int64_t iz = std::max<int64_t>(c[2] - 1, 0); iz <= std::min(c[2] + 1, dim[2] - 1); ++iz)
      for (int64_t iy = std::max<int64_t>(c[1] - 1, 0); iy <= std::min(c[1] + 1, dim[1] - 1); ++iy) {
        const uint64_t base = uint64_t((iz * dim[1] + iy) * dim[0]);
        const auto b = std::lower_bound(code.begin(), code.end(), base + uint64_t(x0));
        const auto e = std::upper_bound(b, code.end(), base + uint64_t(x1));
        for (int64_t t = b - code.begin(); t < e - code.begin(); ++t) {
          const float p[3] = {x[t], y[t], z[t]};
          M.test(p, q, r2, scale);
        }
      }
  }
};

}  // namespace

extern "C" {

// normal[3 m], eig[3 m], count[m] (eig, count and moments may be null); moments[10 m]: count, S0..S2, Q0..Q5 of every row;
// *umax: the largest |u| of any accepted neighbour.  brute != 0: every point for every query.
void shape_cpu_estimate(const float* px, const float* py, const float* pz, int64_t n, const float* qx, const float* qy, const float* qz,
                        int64_t m, float r, int32_t min_neighbours, float* normal, float* eig, int32_t* count, int64_t* moments,
                        int64_t* umax, int32_t threads, int32_t brute) {
  const float* p[3] = {px, py, pz};
  const float r2 = r * r;
  const int s = 18 - std::ilogb(r);
  const double scale = std::ldexp(1.0, s);
  const int32_t need = std::max(3, min_neighbours);
  Grid G;
  if (!brute && n > 0) G.build(p, n, 1.001 * double(r));
  int64_t top = 0;
#pragma omp parallel for schedule(dynamic, 64) num_threads(threads > 0 ? threads : 16) reduction(max : top)
  for (int64_t i = 0; i < m; ++i) {
    const float q[3] = {qx[i], qy[i], qz[i]};
    Moments M;
    if (std::isfinite(q[0]) && std::isfinite(q[1]) && std::isfinite(q[2])) {
      if (G.ok) {
        G.walk(q, r2, scale, M);
      } else {
        for (int64_t j = 0; j < n; ++j) {
          const float pj[3] = {px[j], py[j], pz[j]};
          M.test(pj, q, r2, scale);
        }
      }
    }
    float e[3];
    solve(M, need, s, normal + 3 * i, e);
    if (eig) for (int a = 0; a < 3; ++a) eig[3 * i + a] = e[a];
    if (count) count[i] = M.count;
    if (moments) {
      moments[10 * i] = M.count;
      for (int a = 0; a < 3; ++a) moments[10 * i + 1 + a] = M.S[a];
      for (int a = 0; a < 6; ++a) moments[10 * i + 4 + a] = M.Q[a];
    }
    top = std::max(top, M.umax);
  }
  if (umax) *umax = top;
}

}  // extern "C"
