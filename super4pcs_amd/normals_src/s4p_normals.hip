// s4p_normals.hip -- libsuper4pcs_normals.so: k-nearest-neighbour normal estimation of whole clouds (include/s4p_normals.h,
// DESIGN.md section "Normal estimation").  One translation unit: device kernels (namespace s4p_nrm) and the C ABI.
//
// Device path:
//   set_cloud   k_pack (SoA -> caller-order float4 x, y, z, index bits) -> k_bounds (per-block float minima / maxima) ->
//               k_gather_samples + k_spacing_hist (a histogram of d2 around 64 seeded sample points: the cell edge is their
//               median 16th-neighbour distance) -> k_cell_keys -> radix sort of (cell, index) -> k_cell_ranges + k_gather:
//               the cloud as cell-ordered float4 and the [begin, end) of every cell.
//   lists and outlier removal (include/s4p_knn.h): s4p_knn.inc, on the same cloud and grid.
//   voxel-grid downsampling (include/s4p_voxel.h): s4p_voxel.inc, of a cloud passed per call, on the context's stream.
//   normal orientation (include/s4p_normals_orient.h): s4p_orient.inc, a minimum spanning forest over the lists' graph.
//   density clustering (include/s4p_cluster.h): s4p_cluster.inc, a fixed-radius walk on a grid of edge eps and a union-find.
//   plane segmentation (include/s4p_plane.h): s4p_plane.inc, RANSAC as a dense candidates x points count, no grid.
//   radius normals (include/s4p_shape.h): s4p_shape.inc, a fixed-radius walk on a grid of edge r that sums integer moments.
//   descriptors (include/s4p_feature.h): s4p_feature.inc, FPFH as two walks of that grid over integer histograms, and a dense
//               rows x columns matcher over integer distances.
//   estimate    queries in cell order (the cloud itself, or QueryStage: k_cell_keys + sort + k_gather of the caller's
//               queries) -> k_knn_normals<K>: one lane per query, knn_walk (ring search with conservative box pruning, the
//               k best (d2, index) sorted in registers), covariance in double, 3x3 Jacobi, the normal scattered to the
//               caller's order.
// Shared by the files included below, and defined here: knn_walk<K>, the one neighbour walk (k_knn_normals and
// s4p_knn.inc's k_knn_search call it); QueryStage, the one staging of caller queries (estimate_at and knn_search_at);
// bounds_rows<SKIP> + cloud_bounds (set_cloud's k_bounds and voxel_downsample's k_voxel_bounds); Arena, arena_reserve and arena_layout, through which
// every per-call entry point states its work memory once.  set_cloud and grid keep per-call allocations (Scratch): their
// memory is proportional to the cloud and is freed on return.
// No float or double atomics: every sum has a fixed order, so two calls return identical bits.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "s4p_knn.h"
#include "s4p_normals.h"

namespace s4p_nrm {

constexpr int kBlock = 256;
constexpr int kMaxBlocks = 2048;
constexpr uint64_t kMaxCells = 1ull << 28;
constexpr int kPlanK = 16;                  // the cell edge follows the distance to the 16th neighbour
constexpr int kSamples = 64;                // seeded sample points of the spacing estimate
constexpr int kBinLo = 252;                 // spacing histogram: 4 bins per octave of d2 / L^2 in [2^-64, 2^-10)
constexpr int kBins = 216;                  //   (bin = (float bits >> 21) - kBinLo; below 2^-64, 0 included, -> bin 0)
constexpr int kJacobiSweeps = 64;
// The smallest cell edge set_cloud accepts.  The walk's (1 - 1e-5) comparison presumes a relative error of a float d2; in
// the subnormal range the error is absolute, up to 1.5 * 2^-149, and the comparison still holds for a skipped point whose
// true d2 exceeds 2^-131.8.  A skipped point lies farther from the query than 1e-6 h less the rounding of its cell
// location, at least 5e-7 h, so h >= 2^-44.9 suffices: 2^-43 leaves a factor of 4 in h (DESIGN.md section "Grid regimes").
constexpr double kMinCellEdge = 0x1p-43;

struct GridDev {
  double ox, oy, oz, h, inv_h;
  int32_t nx, ny, nz;
  const float4* pts;          // cell-ordered cloud: x, y, z, original index (bits)
  const uint2* range;         // [begin, end) of every cell (0, 0 when empty)
};

__host__ __device__ inline double cell_coord(float x, double o, double inv_h) { return floor((double(x) - o) * inv_h); }

inline int blocks_for(int64_t n) { return int(std::max<int64_t>(1, std::min<int64_t>((n + kBlock - 1) / kBlock, kMaxBlocks))); }

// caller SoA -> float4 (x, y, z, index bits)
__global__ __launch_bounds__(kBlock) void k_pack(const float* x, const float* y, const float* z, uint64_t n, float4* out) {
  for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock)
    out[i] = make_float4(x[i], y[i], z[i], __uint_as_float(uint32_t(i)));
}

// per-block float minima and maxima (rows of 6).  A point with a non-finite coordinate is skipped (SKIP: a block that saw
// no finite point leaves +inf / -inf), or poisons the block's row: its first entry is NaN, which the tree and the host
// fold pass on
template <bool SKIP>
__device__ __forceinline__ void bounds_rows(const float4* p, uint64_t n, float* rows) {
  float v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  bool bad = false;
  for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    const float4 q = p[i];
    const bool fin = isfinite(q.x) && isfinite(q.y) && isfinite(q.z);
    if (SKIP && !fin) continue;
    bad |= !fin;
    v[0] = fminf(v[0], q.x); v[1] = fminf(v[1], q.y); v[2] = fminf(v[2], q.z);
    v[3] = fmaxf(v[3], q.x); v[4] = fmaxf(v[4], q.y); v[5] = fmaxf(v[5], q.z);
  }
  if (!SKIP && bad) v[0] = NAN;
  __shared__ float sh[kBlock];
  for (int k = 0; k < 6; ++k) {
    sh[threadIdx.x] = v[k];
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
      if (threadIdx.x < unsigned(w)) {
        const float a = sh[threadIdx.x], b = sh[threadIdx.x + w];
        sh[threadIdx.x] = (!SKIP && (a != a || b != b)) ? NAN : (k < 3 ? fminf(a, b) : fmaxf(a, b));
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) rows[blockIdx.x * 6 + k] = sh[0];
    __syncthreads();
  }
}
__global__ __launch_bounds__(kBlock) void k_bounds(const float4* p, uint64_t n, float* rows) { bounds_rows<false>(p, n, rows); }
__global__ __launch_bounds__(kBlock) void k_voxel_bounds(const float4* p, uint64_t n, float* rows) { bounds_rows<true>(p, n, rows); }

__global__ __launch_bounds__(64) void k_gather_samples(const float4* p, const uint32_t* idx, int s, float4* out) {
  if (int(threadIdx.x) < s) out[threadIdx.x] = p[idx[threadIdx.x]];
}

// hist[s][bin]: points of the cloud whose d2 to sample s, scaled by 1 / L^2, falls in the bin (integer counts: any order of
// the additions gives the same histogram)
__global__ __launch_bounds__(kBlock) void k_spacing_hist(const float4* p, uint64_t n, const float4* samples, float inv_l2, uint32_t* hist) {
  __shared__ uint32_t sh[kSamples * kBins];
  __shared__ float4 sq[kSamples];
  for (int t = threadIdx.x; t < kSamples * kBins; t += kBlock) sh[t] = 0u;
  if (threadIdx.x < kSamples) sq[threadIdx.x] = samples[threadIdx.x];
  __syncthreads();
  for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    const float4 q = p[i];
    for (int s = 0; s < kSamples; ++s) {
      const float dx = q.x - sq[s].x, dy = q.y - sq[s].y, dz = q.z - sq[s].z;
      const float d2n = (dx * dx + (dy * dy + dz * dz)) * inv_l2;
      const int b = int(__float_as_uint(d2n) >> 21) - kBinLo;
      if (b < kBins) atomicAdd(&sh[s * kBins + max(b, 0)], 1u);
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < kSamples * kBins; t += kBlock)
    if (sh[t]) atomicAdd(&hist[t], sh[t]);
}

// cell key of every point (clamped to the grid; a non-finite point -> ncell, sorted last); value = its position
__global__ __launch_bounds__(kBlock) void k_cell_keys(const float4* p, uint64_t n, GridDev g, uint32_t* keys, uint32_t* vals) {
  const uint32_t ncell = uint32_t(g.nx) * uint32_t(g.ny) * uint32_t(g.nz);
  for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    const float4 q = p[i];
    uint32_t key = ncell;
    if (isfinite(q.x) && isfinite(q.y) && isfinite(q.z)) {
      const int ix = int(fmin(fmax(cell_coord(q.x, g.ox, g.inv_h), 0.0), double(g.nx - 1)));
      const int iy = int(fmin(fmax(cell_coord(q.y, g.oy, g.inv_h), 0.0), double(g.ny - 1)));
      const int iz = int(fmin(fmax(cell_coord(q.z, g.oz, g.inv_h), 0.0), double(g.nz - 1)));
      key = (uint32_t(iz) * uint32_t(g.ny) + uint32_t(iy)) * uint32_t(g.nx) + uint32_t(ix);
    }
    keys[i] = key;
    vals[i] = uint32_t(i);
  }
}

// [begin, end) of every non-empty cell from the sorted keys (the range array is zeroed first)
__global__ __launch_bounds__(kBlock) void k_cell_ranges(const uint32_t* keys, uint64_t n, uint2* range) {
  for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    const uint32_t c = keys[i];
    if (i == 0 || keys[i - 1] != c) range[c].x = uint32_t(i);
    if (i + 1 == n || keys[i + 1] != c) range[c].y = uint32_t(i + 1);
  }
}

__global__ __launch_bounds__(kBlock) void k_gather(const float4* p, const uint32_t* order, uint64_t n, float4* out) {
  for (uint64_t k = blockIdx.x * (uint64_t)kBlock + threadIdx.x; k < n; k += (uint64_t)gridDim.x * kBlock) out[k] = p[order[k]];
}

// points per non-empty cell, histogram capped at kOccBins - 1 (profiles only)
constexpr int kOccBins = 4096;
__global__ __launch_bounds__(kBlock) void k_occupancy(const uint2* range, uint64_t ncell, uint32_t* hist) {
  for (uint64_t c = blockIdx.x * (uint64_t)kBlock + threadIdx.x; c < ncell; c += (uint64_t)gridDim.x * kBlock) {
    const uint2 r = range[c];
    if (r.y > r.x) atomicAdd(&hist[min(r.y - r.x, uint32_t(kOccBins - 1))], 1u);
  }
}

// Cyclic Jacobi on a symmetric 3x3: A <- V^T A V (eigenvalues on the diagonal), V orthonormal.  Stop rule and rotation as
// the ICP library's k_normals; fully unrolled, so A and V stay in registers.
__device__ inline void jacobi3(double (&A)[3][3], double (&V)[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
    const double diag = (A[0][0] * A[0][0] + A[1][1] * A[1][1]) + A[2][2] * A[2][2];
    const double off = (A[0][1] * A[0][1] + A[0][2] * A[0][2]) + A[1][2] * A[1][2];
    if (off == 0.0 || off <= 1e-36 * diag) break;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = p + 1; q < 3; ++q) {
        if (A[p][q] == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq;
        }
      }
  }
}

struct KnnArgs {
  GridDev g;
  const float4* qs;           // queries in cell order, w = output slot (bits)
  uint64_t m;
  const float4* pos;          // the cloud in the caller's order (covariance reads)
  int32_t k;
  float r2lim;                // fl(r*r), or +inf (unbounded)
  float* out;                 // 3 floats per query, caller order
};

// (d2, index) as one 64-bit key whose unsigned order is the lexicographic order: d2 >= +0, so its float bits are monotone;
// they are offset by one so that key 0 sorts before every candidate.
__device__ inline uint64_t knn_key(float d2, uint32_t i) { return (uint64_t(__float_as_uint(d2)) + 1u) << 32 | i; }
__device__ inline float key_d2(uint64_t key) { return key == ~0ull ? INFINITY : __uint_as_float(uint32_t(key >> 32) - 1u); }

// The neighbour walk of every list in this library (k_knn_normals here, k_knn_search in s4p_knn.inc), for the query q into
// the list L.  The list holds K keys in ascending order: K - k sentinels 0 in front that no candidate passes, then the k
// best so far, padded with ~0.  Its last entry is the k-th best, the pruning bound.
// Rings of cells around the query's (clamped) cell are visited in order R = 0, 1, ...; before ring R the search stops
// when every cell outside the (2R - 1)^3 block already visited is farther than the bound, and inside a ring a cell is
// skipped when its box is.  Box distances are in double, widened by 1e-6 h for the rounding of the cell location and
// compared with a (1 - 1e-5) factor that exceeds the rounding of any normal float d2 (as the ICP library's nearest()): a
// skipped point can neither enter the list nor tie with its last entry.  A skipped point is farther than 1e-6 h from the
// query, and set_cloud's kMinCellEdge keeps the d2 of such a point a normal float.
// The walk is one text, S4P_KNN_WALK, expanded twice.  In k_knn_normals it stands in the kernel, because a walk that the
// kernel calls is compiled on its own first, with the list in memory behind a reference, and the kernel then carries the
// list twice (156 / 252 VGPRs against 131 / 193, estimate at k = 16 one percent slower).  knn_walk<K>
// is the same text as a function, as k_knn_search has always called it.  PASS is the test for a candidate p that is
// passed over: the own index in knn_walk (no candidate has index 0xFFFFFFFF: n <= 2^31 - 2), nothing in k_knn_normals.
// QX, QY, QZ are the query in double and EPS is 1e-6 h, both computed where the text stands; of the text's own names PASS
// may use only p, the candidate (index in p.w).
// Inside: the nearest face of the visited block beyond which cells remain bounds ring R; the insertion is one min / max
// pass, after which the list is still sorted and its largest key has dropped out.
#define S4P_KNN_WALK(K, G, Q, QX, QY, QZ, EPS, R2LIM, PASS, L)                                                              \
  {                                                                                                                         \
    const int cx = int(fmin(fmax(cell_coord((Q).x, (G).ox, (G).inv_h), 0.0), double((G).nx - 1)));                          \
    const int cy = int(fmin(fmax(cell_coord((Q).y, (G).oy, (G).inv_h), 0.0), double((G).ny - 1)));                          \
    const int cz = int(fmin(fmax(cell_coord((Q).z, (G).oz, (G).inv_h), 0.0), double((G).nz - 1)));                          \
    for (int R = 0;; ++R) {                                                                                                 \
      if (R > 0) {                                                                                                          \
        double lb = INFINITY;                                                                                               \
        bool more = false;                                                                                                  \
        const int c3[3] = {cx, cy, cz}, d3[3] = {(G).nx, (G).ny, (G).nz};                                                   \
        const double o3[3] = {(G).ox, (G).oy, (G).oz}, q3[3] = {(QX), (QY), (QZ)};                                          \
        _Pragma("unroll")                                                                                                   \
        for (int a = 0; a < 3; ++a) {                                                                                       \
          const int lo = c3[a] - R + 1, hi = c3[a] + R;                                                                     \
          if (lo > 0) { more = true; lb = fmin(lb, q3[a] - (o3[a] + lo * (G).h)); }                                         \
          if (hi < d3[a]) { more = true; lb = fmin(lb, (o3[a] + hi * (G).h) - q3[a]); }                                     \
        }                                                                                                                   \
        if (!more) break;                                                                                                   \
        lb -= (EPS);                                                                                                        \
        if (lb > 0.0 && lb * lb * (1.0 - 1e-5) > double(fminf((R2LIM), key_d2(L[K - 1])))) break;                           \
      }                                                                                                                     \
      const int z0 = max(cz - R, 0), z1 = min(cz + R, (G).nz - 1), y0 = max(cy - R, 0), y1 = min(cy + R, (G).ny - 1);       \
      const int x0 = max(cx - R, 0), x1 = min(cx + R, (G).nx - 1);                                                          \
      for (int iz = z0; iz <= z1; ++iz)                                                                                     \
        for (int iy = y0; iy <= y1; ++iy) {                                                                                 \
          const bool face = iz == cz - R || iz == cz + R || iy == cy - R || iy == cy + R;                                   \
          const int step = face ? 1 : 2 * R;                                                                                \
          for (int ix = face ? x0 : cx - R; ix <= x1; ix += step) {                                                         \
            if (ix < 0) continue;                                                                                           \
            const double bx0 = (G).ox + ix * (G).h, by0 = (G).oy + iy * (G).h, bz0 = (G).oz + iz * (G).h;                   \
            const double ex = fmax(0.0, fmax(bx0 - (QX), (QX) - (bx0 + (G).h)) - (EPS));                                    \
            const double ey = fmax(0.0, fmax(by0 - (QY), (QY) - (by0 + (G).h)) - (EPS));                                    \
            const double ez = fmax(0.0, fmax(bz0 - (QZ), (QZ) - (bz0 + (G).h)) - (EPS));                                    \
            if ((ex * ex + ey * ey + ez * ez) * (1.0 - 1e-5) > double(fminf((R2LIM), key_d2(L[K - 1])))) continue;          \
            const uint2 rg = (G).range[(uint32_t(iz) * uint32_t((G).ny) + uint32_t(iy)) * uint32_t((G).nx) + uint32_t(ix)]; \
            for (uint32_t s = rg.x; s < rg.y; ++s) {                                                                        \
              const float4 p = (G).pts[s];                                                                                  \
              const float dx = p.x - (Q).x, dy = p.y - (Q).y, dz = p.z - (Q).z;                                             \
              const float d2 = dx * dx + (dy * dy + dz * dz);                                                               \
              uint64_t c = knn_key(d2, __float_as_uint(p.w));                                                               \
              if (!(d2 <= (R2LIM)) || !(c < L[K - 1]) || (PASS)) continue;                                                  \
              _Pragma("unroll")                                                                                             \
              for (int t = 0; t < K; ++t) {                                                                                 \
                const uint64_t lo = c < L[t] ? c : L[t], hi = c < L[t] ? L[t] : c;                                          \
                L[t] = lo;                                                                                                  \
                c = hi;                                                                                                     \
              }                                                                                                             \
            }                                                                                                               \
          }                                                                                                                 \
        }                                                                                                                   \
    }                                                                                                                       \
  }

template <int K>
__device__ __forceinline__ void knn_walk(const GridDev& g, const float4 q, const float r2lim, const uint32_t skip, uint64_t (&L)[K]) {
  const double eps = 1e-6 * g.h;
  const double qx = double(q.x), qy = double(q.y), qz = double(q.z);
  S4P_KNN_WALK(K, g, q, qx, qy, qz, eps, r2lim, __float_as_uint(p.w) == skip, L)
}

// One lane per query: the walk (no candidate is passed over), then the normal of the list.
template <int K>
__global__ __launch_bounds__(kBlock) void k_knn_normals(KnnArgs A) {
  const GridDev& g = A.g;
  const double eps = 1e-6 * g.h;
  for (uint64_t j = blockIdx.x * (uint64_t)kBlock + threadIdx.x; j < A.m; j += (uint64_t)gridDim.x * kBlock) {
    const float4 q = A.qs[j];
    uint64_t L[K];
#pragma unroll
    for (int t = 0; t < K; ++t) L[t] = t < K - A.k ? 0ull : ~0ull;
    // tested before the conversion, not in the if: the other order compiles to another kernel, 1 % slower
    const bool finite = isfinite(q.x) && isfinite(q.y) && isfinite(q.z);
    const double qx = double(q.x), qy = double(q.y), qz = double(q.z);
    if (finite) S4P_KNN_WALK(K, g, q, qx, qy, qz, eps, A.r2lim, false, L)
    // covariance in double, neighbours in ascending (d2, index) order
    double se[3] = {0.0, 0.0, 0.0}, see[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int32_t cnt = 0;
#pragma unroll
    for (int t = 0; t < K; ++t) {
      if (L[t] == 0ull || L[t] == ~0ull) continue;
      const float4 p = A.pos[uint32_t(L[t])];
      const double e0 = double(p.x) - qx, e1 = double(p.y) - qy, e2 = double(p.z) - qz;
      ++cnt;
      se[0] += e0; se[1] += e1; se[2] += e2;
      see[0] += e0 * e0; see[1] += e0 * e1; see[2] += e0 * e2; see[3] += e1 * e1; see[4] += e1 * e2; see[5] += e2 * e2;
    }
    float n0 = 0.f, n1 = 0.f, n2 = 0.f;
    if (cnt >= 3) {
      const double kk = double(cnt);
      const double m0 = se[0] / kk, m1 = se[1] / kk, m2 = se[2] / kk;
      double C[3][3], V[3][3];
      C[0][0] = see[0] / kk - m0 * m0; C[0][1] = see[1] / kk - m0 * m1; C[0][2] = see[2] / kk - m0 * m2;
      C[1][1] = see[3] / kk - m1 * m1; C[1][2] = see[4] / kk - m1 * m2; C[2][2] = see[5] / kk - m2 * m2;
      C[1][0] = C[0][1]; C[2][0] = C[0][2]; C[2][1] = C[1][2];
      const double tr = (C[0][0] + C[1][1]) + C[2][2];
      if (tr > 0.0) {
        jacobi3(C, V);
        int best = 0;
        if (C[1][1] < C[0][0]) best = 1;
        if (C[2][2] < (best == 0 ? C[0][0] : C[1][1])) best = 2;
        double v0 = best == 0 ? V[0][0] : (best == 1 ? V[0][1] : V[0][2]);
        double v1 = best == 0 ? V[1][0] : (best == 1 ? V[1][1] : V[1][2]);
        double v2 = best == 0 ? V[2][0] : (best == 1 ? V[2][1] : V[2][2]);
        const double nv = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
        v0 /= nv; v1 /= nv; v2 /= nv;
        const double a0 = fabs(v0), a1 = fabs(v1), a2 = fabs(v2);
        const double lead = (a0 >= a1 && a0 >= a2) ? v0 : (a1 >= a2 ? v1 : v2);
        if (lead < 0.0) { v0 = -v0; v1 = -v1; v2 = -v2; }
        n0 = float(v0); n1 = float(v1); n2 = float(v2);
      }
    }
    const uint64_t o = 3ull * __float_as_uint(q.w);
    A.out[o] = n0; A.out[o + 1] = n1; A.out[o + 2] = n2;
  }
}

__host__ __device__ inline uint64_t splitmix64(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

}  // namespace s4p_nrm

using namespace s4p_nrm;

struct s4p_normals_ctx {
  int device = 0;
  hipStream_t st = nullptr;
  std::string err;
  bool has_cloud = false;
  int64_t n = 0;
  GridDev g{};
  uint64_t ncell = 0;
  double spacing = 0.0;
  float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};      // the cloud's bounds (s4p_orient.inc: the outward centre)
  float4* pos = nullptr;             // caller order
  float4* pts = nullptr;             // cell order
  uint2* range = nullptr;
  void* arena = nullptr;             // work memory of the per-call entry points (Arena below): grows, never shrinks
  size_t arena_bytes = 0;
};

namespace {

std::string g_create_error;

int32_t fail(s4p_normals_ctx* h, int32_t code, const std::string& msg) {
  h->err = msg;
  return code;
}

#define NRM_HIP(expr)                                                                                                     \
  do {                                                                                                                    \
    const hipError_t e_ = (expr);                                                                                         \
    if (e_ != hipSuccess) return fail(h, e_ == hipErrorOutOfMemory ? S4P_NORMALS_ERR_OOM : S4P_NORMALS_ERR_HIP,          \
                                      std::string(#expr) + ": " + hipGetErrorString(e_));                                \
  } while (0)

void dfree(void* p) { if (p) (void)hipFree(p); }

struct Scratch {
  std::vector<void*> ptrs;
  ~Scratch() { for (void* p : ptrs) dfree(p); }
  hipError_t alloc(void** p, size_t bytes) {
    const hipError_t e = hipMalloc(p, bytes ? bytes : 16);
    if (e == hipSuccess) ptrs.push_back(*p); else *p = nullptr;
    return e;
  }
};

// The context's arena is the work memory of every per-call entry point; it only grows: a call allocates when it needs more
// than any call before.  An Arena hands out its pieces in order.  Without a base it only measures: take() returns null and
// off ends as the byte count of the pieces.  On a base, a piece that would end past cap is refused (null, over set).
constexpr size_t kArenaAlign = 256;
inline size_t arena_round(size_t b) { return (std::max<size_t>(b, 1) + kArenaAlign - 1) / kArenaAlign * kArenaAlign; }

struct Arena {
  char* base = nullptr;
  size_t cap = 0, off = 0;
  bool over = false;
  template <class T> T* take(size_t count) {
    const size_t at = off;
    off += arena_round(count * sizeof(T));
    if (base && off > cap) over = true;
    return base && !over ? reinterpret_cast<T*>(base + at) : nullptr;
  }
};

int32_t arena_reserve(s4p_normals_ctx* h, size_t bytes, Arena* a) {
  if (h->arena_bytes < bytes) {
    NRM_HIP(hipStreamSynchronize(h->st));
    dfree(h->arena);
    h->arena = nullptr; h->arena_bytes = 0;
    NRM_HIP(hipMalloc(&h->arena, bytes));
    h->arena_bytes = bytes;
  }
  *a = Arena{static_cast<char*>(h->arena), h->arena_bytes};
  return S4P_NORMALS_OK;
}

// The code of a failure that no argument explains; S4P_ORIENT_ERR_INTERNAL and S4P_CLUSTER_ERR_INTERNAL are this value.
// s4p_normals.h, s4p_knn.h and s4p_voxel.h name no internal code and do not document -8; their entry points return it only
// from arena_layout's check, which a single statement of the layout cannot reach.
constexpr int32_t kErrInternal = -8;

// An entry point states its arena pieces once, as a function of an Arena that takes them in order: it is run without a
// base to measure them, the arena is made that large, and it is run again on the arena.  The second run cannot pass the
// first one's end; if a mistake ever lets it, the call fails here, before anything is launched on a piece.
template <class Pieces>
int32_t arena_layout(s4p_normals_ctx* h, const char* what, Pieces&& pieces) {
  Arena ar;
  pieces(ar);
  if (int32_t rc = arena_reserve(h, ar.off, &ar)) return rc;
  pieces(ar);
  if (ar.over) return fail(h, kErrInternal, std::string(what) + ": the arena pieces exceed the bytes measured for them");
  return S4P_NORMALS_OK;
}

int end_bit(uint64_t max_key) {
  int b = 1;
  while (b < 32 && (max_key >> b) != 0) ++b;
  return b;
}

int32_t sort_pairs_bytes(s4p_normals_ctx* h, uint64_t n, uint64_t max_key, size_t* bytes) {
  uint32_t* none = nullptr;
  *bytes = 0;
  NRM_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, *bytes, (const uint32_t*)none, none, (const uint32_t*)none, none, int(n), 0,
                                             end_bit(max_key), h->st));
  return S4P_NORMALS_OK;
}

// The dense grid over [lo, hi] with the cell edge hh, enlarged x 1.25 until it fits the cell cap: origin, edge, dims.
int32_t fit_grid(s4p_normals_ctx* h, const char* what, const float lo[3], const float hi[3], double hh, uint64_t un, GridDev* g,
                 uint64_t* ncell) {
  const uint64_t cap = std::min<uint64_t>(kMaxCells, std::max<uint64_t>(1ull << 20, 4 * un));
  int dims[3];
  for (int guard = 0;; ++guard) {
    const double inv = 1.0 / hh;
    bool ok = true;
    uint64_t nc = 1;
    for (int a = 0; a < 3; ++a) {
      const double cc = cell_coord(hi[a], double(lo[a]), inv);
      if (!(cc < 1.0e9)) { ok = false; break; }
      dims[a] = int(cc) + 1;
      nc *= uint64_t(dims[a]);
      if (nc > cap) { ok = false; break; }
    }
    if (ok) { g->h = hh; g->inv_h = inv; *ncell = nc; break; }
    if (guard > 400) return fail(h, S4P_NORMALS_ERR_BAD_ARG, std::string(what) + ": no grid fits the cloud's extent");
    hh *= 1.25;
  }
  g->ox = lo[0]; g->oy = lo[1]; g->oz = lo[2];
  g->nx = dims[0]; g->ny = dims[1]; g->nz = dims[2];
  return S4P_NORMALS_OK;
}

// The cloud pos on the grid g: cell keys, the radix sort of (cell, index), then the [begin, end) of every cell into range
// (ncell entries) and the cloud in cell order into pts.  keys .. vals2 hold un words each, tmp the sort's work memory.
int32_t fill_grid(s4p_normals_ctx* h, const float4* pos, uint64_t un, const GridDev& g, uint64_t ncell, uint32_t* keys, uint32_t* vals,
                  uint32_t* keys2, uint32_t* vals2, void* tmp, size_t tmp_bytes, uint2* range, float4* pts) {
  const int nb = blocks_for(int64_t(un));
  hipLaunchKernelGGL(k_cell_keys, dim3(nb), dim3(kBlock), 0, h->st, pos, un, g, keys, vals);
  NRM_HIP(hipGetLastError());
  NRM_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, (const uint32_t*)keys, keys2, (const uint32_t*)vals, vals2, int(un), 0,
                                             end_bit(ncell - 1), h->st));
  NRM_HIP(hipMemsetAsync(range, 0, ncell * sizeof(uint2), h->st));
  hipLaunchKernelGGL(k_cell_ranges, dim3(nb), dim3(kBlock), 0, h->st, (const uint32_t*)keys2, un, range);
  NRM_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_gather, dim3(nb), dim3(kBlock), 0, h->st, pos, (const uint32_t*)vals2, un, pts);
  NRM_HIP(hipGetLastError());
  return S4P_NORMALS_OK;
}

constexpr int64_t kMaxPoints = int64_t(0x7FFFFFFE);

// The bounds of pos: k_voxel_bounds (skip) or k_bounds into rows (6 floats per workgroup of blocks_for(n)), brought to the host and folded.
// SKIP: over the finite points, lo > hi when there is none; otherwise lo[a] is NaN when any coordinate is not finite.
// Waits for the stream.
int32_t cloud_bounds(s4p_normals_ctx* h, bool skip, const float4* pos, uint64_t un, float* rows, float lo[3], float hi[3]) {
  const int nb = blocks_for(int64_t(un));
  if (skip) hipLaunchKernelGGL(k_voxel_bounds, dim3(nb), dim3(kBlock), 0, h->st, pos, un, rows);
  else hipLaunchKernelGGL(k_bounds, dim3(nb), dim3(kBlock), 0, h->st, pos, un, rows);
  NRM_HIP(hipGetLastError());
  std::vector<float> hr(size_t(nb) * 6);
  NRM_HIP(hipMemcpyAsync(hr.data(), rows, hr.size() * sizeof(float), hipMemcpyDeviceToHost, h->st));
  NRM_HIP(hipStreamSynchronize(h->st));
  for (int a = 0; a < 3; ++a) { lo[a] = INFINITY; hi[a] = -INFINITY; }
  for (int b = 0; b < nb; ++b)
    for (int a = 0; a < 3; ++a) {
      const float l = hr[size_t(b) * 6 + a], u = hr[size_t(b) * 6 + 3 + a];
      lo[a] = (l != l || lo[a] != lo[a]) ? NAN : std::min(lo[a], l);
      hi[a] = std::max(hi[a], u);
    }
  return S4P_NORMALS_OK;
}

// The cell edge: the median over kSamples seeded sample points of their distance to the kPlanK-th neighbour (the upper
// edge of the histogram bin where the count, the point itself included, reaches kPlanK; at most L / 32).
int32_t plan_spacing(s4p_normals_ctx* h, Scratch& S, const float4* pos, uint64_t n, const float lo[3], const float hi[3], double* spacing) {
  double l2 = 0.0;
  for (int a = 0; a < 3; ++a) l2 += (double(hi[a]) - double(lo[a])) * (double(hi[a]) - double(lo[a]));
  const double L = std::sqrt(l2);
  if (!(L > 0.0)) { *spacing = 0.0; return S4P_NORMALS_OK; }
  uint32_t idx[kSamples];
  uint64_t seed = 0x5334504E524D4C31ull;        // fixed: the plan, and so the grid, depend on the cloud alone
  for (int s = 0; s < kSamples; ++s) idx[s] = uint32_t(splitmix64(seed) % n);
  uint32_t *didx, *dhist;
  float4* samp;
  NRM_HIP(S.alloc((void**)&didx, sizeof(idx)));
  NRM_HIP(S.alloc((void**)&samp, kSamples * sizeof(float4)));
  NRM_HIP(S.alloc((void**)&dhist, kSamples * kBins * sizeof(uint32_t)));
  NRM_HIP(hipMemcpyAsync(didx, idx, sizeof(idx), hipMemcpyHostToDevice, h->st));
  NRM_HIP(hipMemsetAsync(dhist, 0, kSamples * kBins * sizeof(uint32_t), h->st));
  hipLaunchKernelGGL(k_gather_samples, dim3(1), dim3(64), 0, h->st, pos, (const uint32_t*)didx, kSamples, samp);
  NRM_HIP(hipGetLastError());
  const float inv_l2 = float(1.0 / l2);
  hipLaunchKernelGGL(k_spacing_hist, dim3(std::min(blocks_for(int64_t(n)), 512)), dim3(kBlock), 0, h->st, pos, n, (const float4*)samp,
                     inv_l2, dhist);
  NRM_HIP(hipGetLastError());
  std::vector<uint32_t> hist(size_t(kSamples) * kBins);
  NRM_HIP(hipMemcpyAsync(hist.data(), dhist, hist.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, h->st));
  NRM_HIP(hipStreamSynchronize(h->st));
  std::vector<double> r(kSamples);
  for (int s = 0; s < kSamples; ++s) {
    uint64_t cum = 0;
    r[s] = L / 32.0;
    for (int b = 0; b < kBins; ++b) {
      cum += hist[size_t(s) * kBins + b];
      if (cum >= uint64_t(kPlanK)) {
        uint32_t bits = uint32_t(b + kBinLo + 1) << 21;
        float edge;
        std::memcpy(&edge, &bits, 4);
        r[s] = std::min(L / 32.0, std::sqrt(double(edge) / double(inv_l2)));
        break;
      }
    }
  }
  std::sort(r.begin(), r.end());
  *spacing = r[kSamples / 2];
  return S4P_NORMALS_OK;
}

int32_t set_cloud_impl(s4p_normals_ctx* h, const float* x, const float* y, const float* z, int64_t n, hipMemcpyKind kind) {
  if (!h) return S4P_NORMALS_ERR_BAD_ARG;
  if (!x || !y || !z || n < 1) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "set_cloud: empty or null cloud");
  if (n > kMaxPoints) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "set_cloud: more than 2^31 - 2 points");
  NRM_HIP(hipSetDevice(h->device));
  h->has_cloud = false;
  dfree(h->pos); dfree(h->pts); dfree(h->range);
  h->pos = h->pts = nullptr; h->range = nullptr;
  Scratch S;
  const uint64_t un = uint64_t(n);
  float* p[3];
  const float* in[3] = {x, y, z};
  for (int a = 0; a < 3; ++a) {
    NRM_HIP(S.alloc((void**)&p[a], un * sizeof(float)));
    NRM_HIP(hipMemcpyAsync(p[a], in[a], un * sizeof(float), kind, h->st));
  }
  NRM_HIP(hipMalloc((void**)&h->pos, un * sizeof(float4)));
  const int nb = blocks_for(n);
  hipLaunchKernelGGL(k_pack, dim3(nb), dim3(kBlock), 0, h->st, p[0], p[1], p[2], un, h->pos);
  NRM_HIP(hipGetLastError());
  float* rows;
  NRM_HIP(S.alloc((void**)&rows, size_t(nb) * 6 * sizeof(float)));
  float lo[3], hi[3];
  if (int32_t rc = cloud_bounds(h, false, h->pos, un, rows, lo, hi)) return rc;
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(lo[a]) || !std::isfinite(hi[a])) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "set_cloud: non-finite coordinates");
  double spacing = 0.0;
  if (int32_t rc = plan_spacing(h, S, h->pos, un, lo, hi, &spacing)) return rc;
  // grid: edge = the spacing (at least 2^-20 of the extent), enlarged x 1.25 until the dense grid fits the cell cap
  double ext = 0.0;
  for (int a = 0; a < 3; ++a) ext = std::max(ext, double(hi[a]) - double(lo[a]));
  double hh = ext > 0.0 ? std::max(spacing, ext * 0x1p-20) : 1.0;
  if (int32_t rc = fit_grid(h, "set_cloud", lo, hi, hh, un, &h->g, &h->ncell)) return rc;
  if (h->g.h < kMinCellEdge)
    return fail(h, S4P_NORMALS_ERR_BAD_ARG, "set_cloud: the cloud's spacing is too small for float distances (the planned cell edge is below "
                                            "2^-43, where squared distances become subnormal): rescale the cloud");
  h->spacing = spacing;
  for (int a = 0; a < 3; ++a) { h->lo[a] = lo[a]; h->hi[a] = hi[a]; }
  uint32_t *keys, *vals, *keys2, *vals2;
  NRM_HIP(S.alloc((void**)&keys, un * 4)); NRM_HIP(S.alloc((void**)&vals, un * 4));
  NRM_HIP(S.alloc((void**)&keys2, un * 4)); NRM_HIP(S.alloc((void**)&vals2, un * 4));
  size_t sort_bytes = 0;
  if (int32_t rc = sort_pairs_bytes(h, un, h->ncell - 1, &sort_bytes)) return rc;
  void* tmp = nullptr;
  NRM_HIP(S.alloc(&tmp, sort_bytes));
  NRM_HIP(hipMalloc((void**)&h->range, h->ncell * sizeof(uint2)));
  NRM_HIP(hipMalloc((void**)&h->pts, un * sizeof(float4)));
  if (int32_t rc = fill_grid(h, h->pos, un, h->g, h->ncell, keys, vals, keys2, vals2, tmp, sort_bytes, h->range, h->pts)) return rc;
  NRM_HIP(hipStreamSynchronize(h->st));          // the scratch is freed on return
  h->g.pts = h->pts;
  h->g.range = h->range;
  h->n = n;
  h->has_cloud = true;
  return S4P_NORMALS_OK;
}

int32_t check_args(s4p_normals_ctx* h, int32_t k, float radius) {
  if (!h->has_cloud) return fail(h, S4P_NORMALS_ERR_STATE, "estimate: set_cloud first");
  if (k < S4P_NORMALS_MIN_K || k > S4P_NORMALS_MAX_K) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "estimate: k must be in [3, 32]");
  if (!std::isfinite(radius)) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "estimate: radius must be finite (<= 0: unbounded)");
  return S4P_NORMALS_OK;
}

// queries (cell order, w = output slot) -> out (device, 3 floats per query)
int32_t run_knn(s4p_normals_ctx* h, const float4* qs, uint64_t m, int32_t k, float radius, float* out) {
  if (m == 0) return S4P_NORMALS_OK;
  KnnArgs A;
  A.g = h->g; A.qs = qs; A.m = m; A.pos = h->pos; A.k = k; A.out = out;
  A.r2lim = radius > 0.f ? radius * radius : INFINITY;
  const int nb = blocks_for(int64_t(m));
  if (k <= 8) hipLaunchKernelGGL(k_knn_normals<8>, dim3(nb), dim3(kBlock), 0, h->st, A);
  else if (k <= 16) hipLaunchKernelGGL(k_knn_normals<16>, dim3(nb), dim3(kBlock), 0, h->st, A);
  else hipLaunchKernelGGL(k_knn_normals<32>, dim3(nb), dim3(kBlock), 0, h->st, A);
  NRM_HIP(hipGetLastError());
  return S4P_NORMALS_OK;
}

int32_t estimate_impl(s4p_normals_ctx* h, int32_t k, float radius, float* out, bool device_out) {
  if (!h) return S4P_NORMALS_ERR_BAD_ARG;
  if (int32_t rc = check_args(h, k, radius)) return rc;
  if (!out) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "estimate: null output");
  NRM_HIP(hipSetDevice(h->device));
  const uint64_t un = uint64_t(h->n);
  float* dout = out;
  if (int32_t rc = arena_layout(h, "estimate", [&](Arena& ar) { if (!device_out) dout = ar.take<float>(3 * un); })) return rc;
  if (int32_t rc = run_knn(h, h->pts, un, k, radius, dout)) return rc;
  if (!device_out) NRM_HIP(hipMemcpyAsync(out, dout, 3 * un * sizeof(float), hipMemcpyDeviceToHost, h->st));
  NRM_HIP(hipStreamSynchronize(h->st));
  return S4P_NORMALS_OK;
}

// Caller queries -> cell-ordered float4 with the output slot in w (what k_knn_normals and k_knn_search read): the SoA
// copy, k_pack, k_cell_keys on the context's grid, the radix sort of (cell, slot), k_gather.  plan() before the layout,
// take() in it, run() after it; nothing waits.
struct QueryStage {
  uint64_t m = 0;
  size_t sort_bytes = 0;
  float* p[3] = {nullptr, nullptr, nullptr};
  float4 *qp = nullptr, *qs = nullptr;      // caller order, cell order
  uint32_t *keys = nullptr, *vals = nullptr, *keys2 = nullptr, *vals2 = nullptr;
  void* tmp = nullptr;

  int32_t plan(s4p_normals_ctx* h, uint64_t um) {
    m = um;
    return sort_pairs_bytes(h, m, h->ncell, &sort_bytes);      // keys reach ncell: a non-finite query sorts last
  }
  void take(Arena& ar) {
    for (int a = 0; a < 3; ++a) p[a] = ar.take<float>(m);
    qp = ar.take<float4>(m); qs = ar.take<float4>(m);
    keys = ar.take<uint32_t>(m); vals = ar.take<uint32_t>(m); keys2 = ar.take<uint32_t>(m); vals2 = ar.take<uint32_t>(m);
    tmp = ar.take<char>(sort_bytes);
  }
  int32_t run(s4p_normals_ctx* h, const float* qx, const float* qy, const float* qz, hipMemcpyKind kind) const {
    const float* in[3] = {qx, qy, qz};
    for (int a = 0; a < 3; ++a) NRM_HIP(hipMemcpyAsync(p[a], in[a], m * sizeof(float), kind, h->st));
    const int nb = blocks_for(int64_t(m));
    hipLaunchKernelGGL(k_pack, dim3(nb), dim3(kBlock), 0, h->st, p[0], p[1], p[2], m, qp);
    NRM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_cell_keys, dim3(nb), dim3(kBlock), 0, h->st, (const float4*)qp, m, h->g, keys, vals);
    NRM_HIP(hipGetLastError());
    size_t bytes = sort_bytes;
    NRM_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, bytes, (const uint32_t*)keys, keys2, (const uint32_t*)vals, vals2, int(m), 0,
                                               end_bit(h->ncell), h->st));
    hipLaunchKernelGGL(k_gather, dim3(nb), dim3(kBlock), 0, h->st, (const float4*)qp, (const uint32_t*)vals2, m, qs);
    NRM_HIP(hipGetLastError());
    return S4P_NORMALS_OK;
  }
};

int32_t estimate_at_impl(s4p_normals_ctx* h, const float* qx, const float* qy, const float* qz, int64_t m, int32_t k, float radius,
                         float* out, bool device) {
  if (!h) return S4P_NORMALS_ERR_BAD_ARG;
  if (int32_t rc = check_args(h, k, radius)) return rc;
  if (m < 0 || m > kMaxPoints) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "estimate_at: m must be in [0, 2^31 - 2]");
  if (m == 0) return S4P_NORMALS_OK;
  if (!qx || !qy || !qz || !out) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "estimate_at: null argument");
  NRM_HIP(hipSetDevice(h->device));
  const uint64_t um = uint64_t(m);
  QueryStage Q;
  if (int32_t rc = Q.plan(h, um)) return rc;
  float* dout = out;
  if (int32_t rc = arena_layout(h, "estimate_at", [&](Arena& ar) {
        Q.take(ar);
        if (!device) dout = ar.take<float>(3 * um);
      })) return rc;
  if (int32_t rc = Q.run(h, qx, qy, qz, device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice)) return rc;
  if (int32_t rc = run_knn(h, Q.qs, um, k, radius, dout)) return rc;
  if (!device) NRM_HIP(hipMemcpyAsync(out, dout, 3 * um * sizeof(float), hipMemcpyDeviceToHost, h->st));
  NRM_HIP(hipStreamSynchronize(h->st));
  return S4P_NORMALS_OK;
}

}  // namespace

#include "s4p_knn.inc"                   // include/s4p_knn.h: neighbour lists and outlier removal on the same context
#include "s4p_voxel.inc"                 // include/s4p_voxel.h: voxel-grid downsampling on the context's stream and arena
#include "s4p_orient.inc"                // include/s4p_normals_orient.h: consistent normal orientation on the lists of s4p_knn.inc
#include "s4p_cluster.inc"               // include/s4p_cluster.h: density clustering on a grid of its own, on the same stream and arena
#include "s4p_plane.inc"                 // include/s4p_plane.h: RANSAC plane segmentation on the cloud in the caller's order, same stream and arena
#include "s4p_shape.inc"                 // include/s4p_shape.h: radius-neighbourhood normals and eigenvalues on a grid of edge r, same stream and arena
#include "s4p_feature.inc"               // include/s4p_feature.h: FPFH descriptors on the grid of s4p_shape.inc and the feature-space matcher

extern "C" {

const char* s4p_normals_last_error(const s4p_normals_ctx* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int32_t s4p_normals_create(int32_t device, s4p_normals_ctx** out) {
  if (!out) { g_create_error = "null argument"; return S4P_NORMALS_ERR_BAD_ARG; }
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    g_create_error = "no HIP device visible: the MI355X path has no CPU fallback";
    return S4P_NORMALS_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= ndev) { g_create_error = "bad device index"; return S4P_NORMALS_ERR_BAD_ARG; }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) { g_create_error = "hipGetDeviceProperties failed"; return S4P_NORMALS_ERR_HIP; }
  if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos) {
    g_create_error = std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only";
    return S4P_NORMALS_ERR_NO_DEVICE;
  }
  s4p_normals_ctx* h = new s4p_normals_ctx();
  h->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking) != hipSuccess) {
    g_create_error = "HIP stream creation failed";
    s4p_normals_destroy(h);
    return S4P_NORMALS_ERR_HIP;
  }
  *out = h;
  return S4P_NORMALS_OK;
}

void s4p_normals_destroy(s4p_normals_ctx* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->st) (void)hipStreamSynchronize(h->st);
  dfree(h->pos); dfree(h->pts); dfree(h->range); dfree(h->arena);
  if (h->st) (void)hipStreamDestroy(h->st);
  delete h;
}

int32_t s4p_normals_set_cloud(s4p_normals_ctx* h, const float* x, const float* y, const float* z, int64_t n) {
  return set_cloud_impl(h, x, y, z, n, hipMemcpyHostToDevice);
}
int32_t s4p_normals_set_cloud_device(s4p_normals_ctx* h, const float* x, const float* y, const float* z, int64_t n) {
  return set_cloud_impl(h, x, y, z, n, hipMemcpyDeviceToDevice);
}

int32_t s4p_normals_estimate(s4p_normals_ctx* h, int32_t k, float radius, float* out) { return estimate_impl(h, k, radius, out, false); }
int32_t s4p_normals_estimate_device(s4p_normals_ctx* h, int32_t k, float radius, float* out) {
  return estimate_impl(h, k, radius, out, true);
}

int32_t s4p_normals_estimate_at(s4p_normals_ctx* h, const float* qx, const float* qy, const float* qz, int64_t m, int32_t k,
                                float radius, float* out) {
  return estimate_at_impl(h, qx, qy, qz, m, k, radius, out, false);
}
int32_t s4p_normals_estimate_at_device(s4p_normals_ctx* h, const float* qx, const float* qy, const float* qz, int64_t m, int32_t k,
                                       float radius, float* out) {
  return estimate_at_impl(h, qx, qy, qz, m, k, radius, out, true);
}

int32_t s4p_normals_grid(s4p_normals_ctx* h, s4p_normals_grid_info* info) {
  if (!h) return S4P_NORMALS_ERR_BAD_ARG;
  if (!info) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "grid: null argument");
  if (!h->has_cloud) return fail(h, S4P_NORMALS_ERR_STATE, "grid: set_cloud first");
  NRM_HIP(hipSetDevice(h->device));
  Scratch S;
  uint32_t* dh;
  NRM_HIP(S.alloc((void**)&dh, kOccBins * sizeof(uint32_t)));
  NRM_HIP(hipMemsetAsync(dh, 0, kOccBins * sizeof(uint32_t), h->st));
  hipLaunchKernelGGL(k_occupancy, dim3(blocks_for(int64_t(h->ncell))), dim3(kBlock), 0, h->st, (const uint2*)h->range, h->ncell, dh);
  NRM_HIP(hipGetLastError());
  std::vector<uint32_t> hist(kOccBins);
  NRM_HIP(hipMemcpyAsync(hist.data(), dh, kOccBins * sizeof(uint32_t), hipMemcpyDeviceToHost, h->st));
  NRM_HIP(hipStreamSynchronize(h->st));
  std::memset(info, 0, sizeof(*info));
  info->cell = h->g.h;
  info->spacing = h->spacing;
  info->dims[0] = h->g.nx; info->dims[1] = h->g.ny; info->dims[2] = h->g.nz;
  info->cells = int64_t(h->ncell);
  int64_t ne = 0;
  for (int b = 1; b < kOccBins; ++b) ne += hist[b];
  info->nonempty = ne;
  info->mean_per_cell = ne > 0 ? double(h->n) / double(ne) : 0.0;
  int64_t cum = 0;
  const int64_t want = (99 * ne + 99) / 100;
  for (int b = 1; b < kOccBins; ++b) {
    if (hist[b] == 0) continue;
    info->max_per_cell = b;
    if (cum < want && cum + int64_t(hist[b]) >= want) info->p99_per_cell = b;
    cum += hist[b];
  }
  return S4P_NORMALS_OK;
}

}  // extern "C"
