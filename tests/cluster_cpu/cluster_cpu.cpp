// Test-side restatement of the clustering contract (include/s4p_cluster.h) on the CPU: a cell grid of its own (sorted 63-bit
// cell codes, edge 1.001 eps, binary search), exact neighbour counts, a plain union-find over the core points (one per
// thread over the thread's share of the edges, merged in sequence), the border rule as the minimum of (d2 bits, index) and
// labels ranked by the smallest core index.  Nothing here follows the device path: no atomics, no hooks onto roots, no scan.
// Build: g++ -O2 -ffp-contract=off -fopenmp -fPIC -shared (tests/cluster_helpers.py).
#include <omp.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>

namespace {

struct Grid {
  double o[3], inv;
  std::vector<uint64_t> code;      // sorted, unique
  std::vector<uint32_t> begin;     // code.size() + 1
  std::vector<uint32_t> order;     // point indices by cell
  int64_t c[3];
  static uint64_t pack(int64_t x, int64_t y, int64_t z) { return (uint64_t(z) << 42) | (uint64_t(y) << 21) | uint64_t(x); }
  void coords(const float* x, const float* y, const float* z, int64_t i, int64_t out[3]) const {
    out[0] = int64_t(std::floor((double(x[i]) - o[0]) * inv));
    out[1] = int64_t(std::floor((double(y[i]) - o[1]) * inv));
    out[2] = int64_t(std::floor((double(z[i]) - o[2]) * inv));
  }
};

Grid make_grid(const float* x, const float* y, const float* z, int64_t n, float eps) {
  Grid g;
  double lo[3] = {x[0], y[0], z[0]}, hi[3] = {x[0], y[0], z[0]};
  for (int64_t i = 0; i < n; ++i) {
    const double p[3] = {x[i], y[i], z[i]};
    for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], p[a]); hi[a] = std::max(hi[a], p[a]); }
  }
  double edge = double(eps) * 1.001;
  for (;;) {                                             // at most 2^21 - 2 cells per axis
    bool ok = true;
    for (int a = 0; a < 3; ++a) ok = ok && (hi[a] - lo[a]) / edge < 2.0e6;
    if (ok) break;
    edge *= 2.0;
  }
  for (int a = 0; a < 3; ++a) g.o[a] = lo[a] - edge;    // so that every coordinate is >= 1
  g.inv = 1.0 / edge;
  std::vector<uint64_t> all(n);
  for (int64_t i = 0; i < n; ++i) {
    int64_t c[3];
    g.coords(x, y, z, i, c);
    all[i] = Grid::pack(c[0], c[1], c[2]);
  }
  g.order.resize(n);
  std::iota(g.order.begin(), g.order.end(), 0u);
  std::stable_sort(g.order.begin(), g.order.end(), [&](uint32_t a, uint32_t b) { return all[a] < all[b]; });
  for (int64_t k = 0; k < n; ++k) {
    const uint64_t c = all[g.order[k]];
    if (g.code.empty() || g.code.back() != c) { g.code.push_back(c); g.begin.push_back(uint32_t(k)); }
  }
  g.begin.push_back(uint32_t(n));
  return g;
}

// calls f(j, d2) for every neighbour j of i (d2 <= r2), i itself included
template <class F>
void neighbours(const Grid& g, const float* x, const float* y, const float* z, int64_t i, float r2, F&& f) {
  int64_t c[3];
  g.coords(x, y, z, i, c);
  for (int64_t dz = -1; dz <= 1; ++dz)
    for (int64_t dy = -1; dy <= 1; ++dy)
      for (int64_t dx = -1; dx <= 1; ++dx) {
        const uint64_t code = Grid::pack(c[0] + dx, c[1] + dy, c[2] + dz);
        const auto it = std::lower_bound(g.code.begin(), g.code.end(), code);
        if (it == g.code.end() || *it != code) continue;
        const size_t cell = size_t(it - g.code.begin());
        for (uint32_t k = g.begin[cell]; k < g.begin[cell + 1]; ++k) {
          const uint32_t j = g.order[k];
          const float ex = x[j] - x[i], ey = y[j] - y[i], ez = z[j] - z[i];
          const float d2 = ex * ex + (ey * ey + ez * ez);
          if (d2 <= r2) f(j, d2);
        }
      }
}

uint32_t find(std::vector<uint32_t>& p, uint32_t a) {
  while (p[a] != a) { p[a] = p[p[a]]; a = p[a]; }
  return a;
}

}  // namespace

extern "C" {

// count int32[n] (may be null): the exact neighbour counts
void cluster_cpu_density(const float* x, const float* y, const float* z, int64_t n, float radius, int32_t* count, int32_t threads) {
  if (n < 1) return;
  const Grid g = make_grid(x, y, z, n, radius);
  const float r2 = radius * radius;
  if (threads > 0) omp_set_num_threads(threads);
#pragma omp parallel for schedule(dynamic, 1024)
  for (int64_t i = 0; i < n; ++i) {
    int32_t c = 0;
    neighbours(g, x, y, z, i, r2, [&](uint32_t, float) { ++c; });
    count[i] = c;
  }
}

// label int32[n], kind uint8[n], stats int64[4] = core, border, noise, clusters
void cluster_cpu_dbscan(const float* x, const float* y, const float* z, int64_t n, float eps, int32_t min_points, int32_t* label,
                        uint8_t* kind, int64_t* stats, int32_t threads) {
  stats[0] = stats[1] = stats[2] = stats[3] = 0;
  if (n < 1) return;
  const Grid g = make_grid(x, y, z, n, eps);
  const float r2 = eps * eps;
  if (threads > 0) omp_set_num_threads(threads);
  std::vector<uint8_t> core(n);
#pragma omp parallel for schedule(dynamic, 1024)
  for (int64_t i = 0; i < n; ++i) {
    int32_t c = 0;
    neighbours(g, x, y, z, i, r2, [&](uint32_t, float) { ++c; });
    core[i] = c >= min_points;
  }
  // edges between core points into one union-find per thread; the nearest core neighbour of the others
  const int nt = omp_get_max_threads();
  std::vector<std::vector<uint32_t>> parents(nt);
  std::vector<int64_t> nearest(n, -1);
#pragma omp parallel
  {
    std::vector<uint32_t>& p = parents[omp_get_thread_num()];
    p.resize(n);
    std::iota(p.begin(), p.end(), 0u);
#pragma omp for schedule(dynamic, 1024)
    for (int64_t i = 0; i < n; ++i) {
      if (core[i]) {
        neighbours(g, x, y, z, i, r2, [&](uint32_t j, float) {
          if (!core[j] || j == uint32_t(i)) return;
          const uint32_t a = find(p, uint32_t(i)), b = find(p, j);
          if (a != b) p[a] = b;
        });
      } else {
        uint64_t best = ~0ull;
        neighbours(g, x, y, z, i, r2, [&](uint32_t j, float d2) {
          if (!core[j]) return;
          uint32_t bits;
          std::memcpy(&bits, &d2, 4);
          best = std::min(best, uint64_t(bits) << 32 | j);
        });
        if (best != ~0ull) nearest[i] = int64_t(uint32_t(best));
      }
    }
  }
  std::vector<uint32_t> all(n);
  std::iota(all.begin(), all.end(), 0u);
  for (int t = 0; t < nt; ++t) {
    if (parents[t].empty()) continue;
    for (int64_t v = 0; v < n; ++v) {
      const uint32_t r = find(parents[t], uint32_t(v));
      if (r == uint32_t(v)) continue;
      const uint32_t a = find(all, uint32_t(v)), b = find(all, r);
      if (a != b) all[a] = b;
    }
  }
  // clusters in ascending order of their smallest core index: the first core point met of every tree names it
  std::vector<int32_t> of_root(n, -1);
  int32_t next = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (!core[i]) continue;
    const uint32_t r = find(all, uint32_t(i));
    if (of_root[r] < 0) of_root[r] = next++;
    label[i] = of_root[r];
    kind[i] = 2;
    ++stats[0];
  }
  for (int64_t i = 0; i < n; ++i) {
    if (core[i]) continue;
    if (nearest[i] >= 0) { label[i] = label[nearest[i]]; kind[i] = 1; ++stats[1]; }
    else { label[i] = -1; kind[i] = 0; ++stats[2]; }
  }
  stats[3] = next;
}

}  // extern "C"
