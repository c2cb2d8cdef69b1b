// s4p_icp.hip -- libsuper4pcs_icp.so: point-to-point and point-to-plane ICP on the full-resolution clouds, with robust
// losses, generalized and coloured ICP (include/s4p_icp.h, include/s4p_icp_plane.h, include/s4p_icp_robust.h, include/s4p_icp_gicp.h,
// include/s4p_icp_color.h, DESIGN.md sections "ICP refinement", "Point-to-plane ICP", "Robust ICP", "Generalized ICP" and "Coloured ICP").  One translation unit: device kernels (namespace s4p_icp), the host solve and the C ABI.
//
// Device path:
//   set_target   k_stats (per-block double sums and float bounds of P) -> host frame c and grid plan ->
//                k_cell_keys (cell of fl(P - c)) -> radix sort of (cell, index) -> k_cell_starts + k_gather_target:
//                the target as cell-ordered float4 (x', y', z', index bits) and the start of every cell.
//   refine       once: k_source_keys (cell of the T0-image) -> radix sort -> k_gather_source (the source in that order);
//                per iteration: k_match (correspondence + 17 double sums per lane -> wave -> workgroup -> one slab row),
//                k_final (fixed-order sum of the slab), one pinned read-back, host solve.
//   plane        (include/s4p_icp_plane.h) target normals, cell-ordered next to tgt: k_normals (estimated) or
//                k_gather_normals (the caller's); per iteration k_match_plane (31 double sums) + k_final_plane, host solve.
//   robust       (include/s4p_icp_robust.h) per iteration k_search (winner slot + residual key per lane), the radix select of
//                the keys (k_key_hist + k_key_digit x 4, on the device), k_wsum + k_wfinal (weighted sums), host solve.
//   generalized  (include/s4p_icp_gicp.h) source normals in the order of the source (k_gather_source_normals); per iteration
//                k_search (winner slot per lane), k_gicp_sum (31 double sums streamed from the slots) + k_final_plane, host solve.
//   coloured     (include/s4p_icp_color.h) target intensities in cell order (k_gather_target_intensity), their tangent-plane
//                gradients (k_color_gradient, k_normals' walk), source intensities in the order of the source
//                (k_gather_source_intensity); per iteration k_search, k_color_sum (31 joint sums) + k_final_plane, host solve.
//   rejection    (include/s4p_icp_reject.h) a state of the context: a second grid over the source (set_target's plan and
//                build), and k_reject between k_search and the sum kernel of every split pass: it clears the slot and key of
//                a pair that fails the normal test or the reverse search.  Off: nothing of it is launched.
// No float or double atomics anywhere (the selection's histograms use integer atomics): every sum has a fixed order, so two calls return identical bits.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "s4p_icp.h"
#include "s4p_icp_plane.h"
#include "s4p_icp_robust.h"
#include "s4p_icp_gicp.h"
#include "s4p_icp_color.h"
#include "s4p_icp_reject.h"

namespace s4p_icp {

constexpr int kBlock = 256;
constexpr int kMaxBlocks = 2048;            // grid-stride beyond this: the slab and its final sum stay small
constexpr int kPitch = 18;                  // doubles per slab row (17 used)
constexpr int kStatsPitch = 9;              // k_stats row: 3 double sums, 3 float minima, 3 float maxima (as doubles)
constexpr float kCellFactor = 1.02f;        // cell edge >= 1.02 d: a match is always in the 27 cells around the query's
constexpr uint64_t kMaxCells = 1ull << 28;

// The dense target grid.  Cells are located in double: cell(x) = floor((x - o) * inv_h), monotone in x.
struct GridDev {
  double ox, oy, oz, h, inv_h;
  int32_t nx, ny, nz;
  const float4* tgt;          // cell-ordered target: x', y', z', original index (bits)
  const uint32_t* start;      // ncell + 1 entries
};

__host__ __device__ inline double cell_coord(float x, double o, double inv_h) { return floor((double(x) - o) * inv_h); }

inline int blocks_for(int64_t n) { return int(std::max<int64_t>(1, std::min<int64_t>((n + kBlock - 1) / kBlock, kMaxBlocks))); }

// ---------------------------------------------------------------------------------------------------------------------
// frame and bounds of P: per-block partials in a fixed order (summed on the host in row order)
__global__ __launch_bounds__(kBlock) void k_stats(const float* x, const float* y, const float* z, uint64_t n, double* rows) {
  double s[3] = {0.0, 0.0, 0.0};
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    const float v[3] = {x[i], y[i], z[i]};
    for (int a = 0; a < 3; ++a) { s[a] += double(v[a]); lo[a] = fminf(lo[a], v[a]); hi[a] = fmaxf(hi[a], v[a]); }
  }
  __shared__ double sh[kBlock];
  for (int k = 0; k < kStatsPitch; ++k) {
    const double mine = k < 3 ? s[k] : (k < 6 ? double(lo[k - 3]) : double(hi[k - 6]));
    sh[threadIdx.x] = mine;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
      if (threadIdx.x < unsigned(w)) {
        const double a = sh[threadIdx.x], b = sh[threadIdx.x + w];
        sh[threadIdx.x] = k < 3 ? a + b : (k < 6 ? fmin(a, b) : fmax(a, b));
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) rows[blockIdx.x * kStatsPitch + k] = sh[0];
    __syncthreads();
  }
}

// cell key of every target point fl(P - c); value = its index
__global__ __launch_bounds__(kBlock) void k_cell_keys(const float* x, const float* y, const float* z, uint64_t n, float cx, float cy,
                                                      float cz, GridDev g, uint32_t* keys, uint32_t* vals) {
  for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    const float px = x[i] - cx, py = y[i] - cy, pz = z[i] - cz;
    const int ix = int(cell_coord(px, g.ox, g.inv_h)), iy = int(cell_coord(py, g.oy, g.inv_h)), iz = int(cell_coord(pz, g.oz, g.inv_h));
    keys[i] = (uint32_t(iz) * uint32_t(g.ny) + uint32_t(iy)) * uint32_t(g.nx) + uint32_t(ix);
    vals[i] = uint32_t(i);
  }
}

// start[c] = first sorted position with key >= c (lower bound), for every c in [0, ncell]
__global__ __launch_bounds__(kBlock) void k_cell_starts(const uint32_t* keys, uint64_t n, uint64_t ncell, uint32_t* start) {
  for (uint64_t c = blockIdx.x * (uint64_t)kBlock + threadIdx.x; c <= ncell; c += (uint64_t)gridDim.x * kBlock) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
      const uint64_t mid = (lo + hi) >> 1;
      if (uint64_t(keys[mid]) < c) lo = mid + 1; else hi = mid;
    }
    start[c] = uint32_t(lo);
  }
}

__global__ __launch_bounds__(kBlock) void k_gather_target(const float* x, const float* y, const float* z, uint64_t n, float cx, float cy,
                                                          float cz, const uint32_t* order, float4* tgt) {
  for (uint64_t k = blockIdx.x * (uint64_t)kBlock + threadIdx.x; k < n; k += (uint64_t)gridDim.x * kBlock) {
    const uint32_t i = order[k];
    tgt[k] = make_float4(x[i] - cx, y[i] - cy, z[i] - cz, __uint_as_float(i));
  }
}

// Q' = fl(Q - c), w = original index (bits)
__global__ __launch_bounds__(kBlock) void k_center_source(const float* x, const float* y, const float* z, uint64_t n, float cx, float cy,
                                                          float cz, float4* src) {
  for (uint64_t j = blockIdx.x * (uint64_t)kBlock + threadIdx.x; j < n; j += (uint64_t)gridDim.x * kBlock)
    src[j] = make_float4(x[j] - cx, y[j] - cy, z[j] - cz, __uint_as_float(uint32_t(j)));
}

struct Tf { float m[12]; };

__device__ inline void apply_t(const Tf& T, float x, float y, float z, float& ox, float& oy, float& oz) {
  ox = ((T.m[0] * x + T.m[1] * y) + T.m[2] * z) + T.m[3];
  oy = ((T.m[4] * x + T.m[5] * y) + T.m[6] * z) + T.m[7];
  oz = ((T.m[8] * x + T.m[9] * y) + T.m[10] * z) + T.m[11];
}

// source order for a refine call: cell of the T0-image (ncell for a query outside the grid: sorted last)
__global__ __launch_bounds__(kBlock) void k_source_keys(const float4* src, uint64_t n, Tf T, GridDev g, uint32_t* keys, uint32_t* vals) {
  const uint32_t ncell = uint32_t(g.nx) * uint32_t(g.ny) * uint32_t(g.nz);
  for (uint64_t j = blockIdx.x * (uint64_t)kBlock + threadIdx.x; j < n; j += (uint64_t)gridDim.x * kBlock) {
    const float4 q = src[j];
    float x, y, z;
    apply_t(T, q.x, q.y, q.z, x, y, z);
    const double fx = cell_coord(x, g.ox, g.inv_h), fy = cell_coord(y, g.oy, g.inv_h), fz = cell_coord(z, g.oz, g.inv_h);
    const bool in = fx >= 0.0 && fx < double(g.nx) && fy >= 0.0 && fy < double(g.ny) && fz >= 0.0 && fz < double(g.nz);
    keys[j] = in ? (uint32_t(fz) * uint32_t(g.ny) + uint32_t(fy)) * uint32_t(g.nx) + uint32_t(fx) : ncell;
    vals[j] = uint32_t(j);
  }
}

__global__ __launch_bounds__(kBlock) void k_gather_source(const float4* src, const uint32_t* order, uint64_t n, float4* out) {
  for (uint64_t k = blockIdx.x * (uint64_t)kBlock + threadIdx.x; k < n; k += (uint64_t)gridDim.x * kBlock) out[k] = src[order[k]];
}

// Nearest target within d of q^ (ties to the smallest index).  The 27 cells around q^'s cell hold every candidate: a
// point with fl(d2) <= fl(d*d) is within d (1 + 2^-21) of q^ along each axis, less than the cell edge (>= 1.02 d).  A cell
// is skipped when its box (in double, widened by 1e-6 h for the rounding of the cell location) is farther than the running
// best by a margin (factor 1 - 1e-5) that exceeds the rounding of any float d2 of a point inside it: such a point can
// neither win nor tie.
// SLOT: also report the winner's cell-order position (the slot of its normal); the winner itself is the same.
template <bool SLOT>
__device__ inline void nearest_t(const GridDev& g, float x, float y, float z, float d2max, float& best, uint32_t& bi, float4& bp,
                                 uint32_t& slot) {
  best = d2max;
  bi = 0xFFFFFFFFu;
  bp = make_float4(0.f, 0.f, 0.f, 0.f);
  if (SLOT) slot = 0;
  const double fx = cell_coord(x, g.ox, g.inv_h), fy = cell_coord(y, g.oy, g.inv_h), fz = cell_coord(z, g.oz, g.inv_h);
  // NaN fails every comparison; a query more than one cell outside the grid has no neighbour cell inside it
  if (!(fx >= -1.0 && fx <= double(g.nx) && fy >= -1.0 && fy <= double(g.ny) && fz >= -1.0 && fz <= double(g.nz))) return;
  const int cx = int(fx), cy = int(fy), cz = int(fz);
  const double eps = 1e-6 * g.h;
  const double qx = double(x), qy = double(y), qz = double(z);
  // centre cell first (it usually sets a tight bound), then the other 26 in a fixed order
  for (int s = 0; s < 27; ++s) {
    const int t = s == 0 ? 13 : (s <= 13 ? s - 1 : s);
    const int ix = cx + t % 3 - 1, iy = cy + (t / 3) % 3 - 1, iz = cz + t / 9 - 1;
    if (ix < 0 || ix >= g.nx || iy < 0 || iy >= g.ny || iz < 0 || iz >= g.nz) continue;
    const double bx0 = g.ox + ix * g.h, by0 = g.oy + iy * g.h, bz0 = g.oz + iz * g.h;
    const double ex = fmax(0.0, fmax(bx0 - qx, qx - (bx0 + g.h)) - eps);
    const double ey = fmax(0.0, fmax(by0 - qy, qy - (by0 + g.h)) - eps);
    const double ez = fmax(0.0, fmax(bz0 - qz, qz - (bz0 + g.h)) - eps);
    if ((ex * ex + ey * ey + ez * ez) * (1.0 - 1e-5) > double(best)) continue;
    const uint32_t c = (uint32_t(iz) * uint32_t(g.ny) + uint32_t(iy)) * uint32_t(g.nx) + uint32_t(ix);
    const uint32_t b = g.start[c], e = g.start[c + 1];
    for (uint32_t k = b; k < e; ++k) {
      const float4 p = g.tgt[k];
      const float dx = x - p.x, dy = y - p.y, dz = z - p.z;
      const float d2 = dx * dx + (dy * dy + dz * dz);
      const uint32_t i = __float_as_uint(p.w);
      if (d2 < best || (d2 == best && i < bi)) {
        best = d2; bi = i; bp = p;
        if (SLOT) slot = k;
      }
    }
  }
}

__device__ inline void nearest(const GridDev& g, float x, float y, float z, float d2max, float& best, uint32_t& bi, float4& bp) {
  uint32_t unused;
  nearest_t<false>(g, x, y, z, d2max, best, bi, bp, unused);
}


struct MatchArgs {
  Tf T;
  GridDev g;
  const float4* src;        // w = original source index (bits)
  uint64_t n;
  float d2max;
  int32_t* idx;             // WRITE only: per source point, in the uploaded order
  float* d2;
  double* slab;             // one kPitch row per workgroup
};

// The hot path.  One lane per source point: apply T, nearest target, 17 double sums in registers; then the wave (xor
// butterfly), the workgroup (LDS, waves in order) and one slab row.  No transformed cloud is written.
template <bool WRITE>
__global__ __launch_bounds__(kBlock) void k_match(MatchArgs A) {
  double s[S4P_ICP_NSUMS];
#pragma unroll
  for (int k = 0; k < S4P_ICP_NSUMS; ++k) s[k] = 0.0;
  for (uint64_t j = blockIdx.x * (uint64_t)kBlock + threadIdx.x; j < A.n; j += (uint64_t)gridDim.x * kBlock) {
    const float4 q = A.src[j];
    float x, y, z;
    apply_t(A.T, q.x, q.y, q.z, x, y, z);
    float best;
    uint32_t bi;
    float4 p;
    nearest(A.g, x, y, z, A.d2max, best, bi, p);
    const bool hit = bi != 0xFFFFFFFFu;
    if (WRITE) {
      const uint32_t o = __float_as_uint(q.w);
      A.idx[o] = hit ? int32_t(bi) : -1;
      A.d2[o] = hit ? best : 0.f;
    }
    if (hit) {
      const double qd[3] = {double(x), double(y), double(z)}, pd[3] = {double(p.x), double(p.y), double(p.z)};
      s[0] += 1.0;
#pragma unroll
      for (int a = 0; a < 3; ++a) { s[1 + a] += qd[a]; s[4 + a] += pd[a]; }
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) s[7 + 3 * a + b] += qd[a] * pd[b];      // exact products (24 + 24 bits)
      s[16] += double(best);
    }
  }
  __shared__ double red[kBlock / 64][S4P_ICP_NSUMS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < S4P_ICP_NSUMS; ++k) {
    double v = s[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < S4P_ICP_NSUMS) {
    double v = red[0][threadIdx.x];
    for (int w = 1; w < kBlock / 64; ++w) v += red[w][threadIdx.x];
    A.slab[uint64_t(blockIdx.x) * kPitch + threadIdx.x] = v;
  }
}

// the slab's nb rows -> 17 sums, in a fixed order: 15 parts per column (rows part, part + 15, ...), then the parts in order
__global__ __launch_bounds__(kBlock) void k_final(const double* slab, int nb, double* out) {
  constexpr int kParts = kBlock / S4P_ICP_NSUMS;       // 15
  __shared__ double part[kParts][S4P_ICP_NSUMS];
  const int col = threadIdx.x % S4P_ICP_NSUMS, prt = threadIdx.x / S4P_ICP_NSUMS;
  if (prt < kParts) {
    double v = 0.0;
    for (int r = prt; r < nb; r += kParts) v += slab[uint64_t(r) * kPitch + col];
    part[prt][col] = v;
  }
  __syncthreads();
  if (threadIdx.x < S4P_ICP_NSUMS) {
    double v = part[0][threadIdx.x];
    for (int p = 1; p < kParts; ++p) v += part[p][threadIdx.x];
    out[threadIdx.x] = v;
  }
}

// the returned transform on the caller's cloud, in k_apply's rounding order
__global__ __launch_bounds__(kBlock) void k_apply_icp(Tf T, float* x, float* y, float* z, uint64_t n) {
  for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    float ox, oy, oz;
    apply_t(T, x[i], y[i], z[i], ox, oy, oz);
    x[i] = ox; y[i] = oy; z[i] = oz;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// robust ICP (include/s4p_icp_robust.h).  Per iteration: k_search (the one correspondence search: winner slot and residual
// key per visited lane), the radix select of the keys (k_key_hist + k_key_digit per 8-bit digit, integer atomics only, the
// digit decisions on the device), k_wsum (weighted sums streamed from the slots, k_match / k_match_plane's lane order and
// reduction) and k_wfinal (k_final / k_final_plane's fixed order, plus the count with w > 0 and the info).

constexpr uint32_t kNoKey = 0xFFFFFFFFu;    // a miss, or (plane) a zero normal: above every key (keys are non-negative floats)
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
constexpr int kDigits = 4, kBins = 256;     // 4 digits of 8 bits, most significant first
enum SelMode { kSelNone = 0, kSelTrim = 1, kSelMedian = 2 };

struct SelState {          // zeroed before each pass; written by k_key_digit only
  uint32_t M, k, rank, prefix;
  double s, cs, cs2;
};

// histogram of digit `pass` over the keys whose higher digits equal the selected prefix (LDS, then one add per bin)
__global__ __launch_bounds__(kBlock) void k_key_hist(const uint32_t* key, uint64_t n, int pass, const SelState* st, uint32_t* hist) {
  if (pass > 0 && st->k == 0) return;                     // nothing to select (uniform)
  __shared__ uint32_t h[kBins];
  h[threadIdx.x] = 0u;
  __syncthreads();
  const int shift = 24 - 8 * pass;
  const uint32_t hi = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
  const uint32_t want = st->prefix & hi;
  for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    const uint32_t u = key[i];
    if (u != kNoKey && (u & hi) == want) atomicAdd(&h[(u >> shift) & (kBins - 1)], 1u);
  }
  __syncthreads();
  const uint32_t c = h[threadIdx.x];
  if (c) atomicAdd(&hist[threadIdx.x], c);
}

// One block: the digit of the rank-k key at `pass` (pass 0 first counts M and sets k); the last pass sets the scale.
__global__ __launch_bounds__(kBlock) void k_key_digit(const uint32_t* hist, int pass, bool last, int mode, uint64_t kq, double scale,
                                                      double c, double smin, SelState* st) {
  __shared__ uint32_t h[kBins];
  h[threadIdx.x] = hist[threadIdx.x];
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (pass == 0) {
    uint32_t M = 0;
    for (int b = 0; b < kBins; ++b) M += h[b];
    const uint32_t k = mode == kSelTrim ? uint32_t(min<uint64_t>(uint64_t(M), max<uint64_t>(1, kq)))
                                        : (mode == kSelMedian ? (M + 1) / 2 : 0u);
    st->M = M; st->k = k; st->rank = k; st->prefix = 0u;
  }
  if (st->k > 0) {
    uint32_t r = st->rank;
    int b = 0;
    while (b < kBins - 1 && r > h[b]) { r -= h[b]; ++b; }
    st->prefix |= uint32_t(b) << (24 - 8 * pass);
    st->rank = r;
  }
  if (last) {
    double s = 0.0;
    if (mode == kSelMedian) s = fmax(1.4826 * sqrt(double(__uint_as_float(st->prefix))), smin);   // M == 0: prefix 0, s_min
    else if (scale > 0.0) s = scale;
    const double cs = c * s;
    st->s = s; st->cs = cs; st->cs2 = cs * cs;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// point-to-plane (include/s4p_icp_plane.h): target normals as a cell-ordered float4 array next to tgt (w unused)

constexpr int kPlanePitch = 32;             // doubles per plane slab row (31 used)
constexpr int kJacobiSweeps = 64;           // as jacobi4

// Cyclic Jacobi on a symmetric N x N matrix: A <- V^T A V (eigenvalues on the diagonal), V orthonormal.  Fully unrolled
// inner loops, so that on the device every index is a constant and A, V stay in registers.
template <int N>
__host__ __device__ inline void jacobi_sym(double (&A)[N][N], double (&V)[N][N]) {
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
    double off = 0.0, diag = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      diag += A[i][i] * A[i][i];
#pragma unroll
      for (int j = i + 1; j < N; ++j) off += A[i][j] * A[i][j];
    }
    if (off == 0.0 || off <= 1e-36 * diag) break;
#pragma unroll
    for (int p = 0; p < N - 1; ++p)
#pragma unroll
      for (int q = p + 1; q < N; ++q) {
        if (A[p][q] == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq;
        }
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk;
        }
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq;
        }
      }
  }
}

// Normal of every target point, one lane per point in cell order: the neighbours within r (float d2 <= r2, the point
// itself included) in the 27 cells around it (r <= d < cell edge), cells pruned by box distance with nearest()'s margin.
// Covariance in double, eigenvector of the smallest eigenvalue (first on ties), largest component positive.
__global__ __launch_bounds__(kBlock) void k_normals(GridDev g, uint64_t n, float r2, int32_t min_nb, float4* nrm) {
  const double eps = 1e-6 * g.h;
  for (uint64_t k = blockIdx.x * (uint64_t)kBlock + threadIdx.x; k < n; k += (uint64_t)gridDim.x * kBlock) {
    const float4 p = g.tgt[k];
    const int cx = int(cell_coord(p.x, g.ox, g.inv_h)), cy = int(cell_coord(p.y, g.oy, g.inv_h)), cz = int(cell_coord(p.z, g.oz, g.inv_h));
    const double qx = double(p.x), qy = double(p.y), qz = double(p.z);
    double se[3] = {0.0, 0.0, 0.0}, see[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};    // sum e; sum e e^T (xx xy xz yy yz zz)
    int32_t cnt = 0;
    for (int t = 0; t < 27; ++t) {
      const int ix = cx + t % 3 - 1, iy = cy + (t / 3) % 3 - 1, iz = cz + t / 9 - 1;
      if (ix < 0 || ix >= g.nx || iy < 0 || iy >= g.ny || iz < 0 || iz >= g.nz) continue;
      const double bx0 = g.ox + ix * g.h, by0 = g.oy + iy * g.h, bz0 = g.oz + iz * g.h;
      const double ex = fmax(0.0, fmax(bx0 - qx, qx - (bx0 + g.h)) - eps);
      const double ey = fmax(0.0, fmax(by0 - qy, qy - (by0 + g.h)) - eps);
      const double ez = fmax(0.0, fmax(bz0 - qz, qz - (bz0 + g.h)) - eps);
      if ((ex * ex + ey * ey + ez * ez) * (1.0 - 1e-5) > double(r2)) continue;
      const uint32_t c = (uint32_t(iz) * uint32_t(g.ny) + uint32_t(iy)) * uint32_t(g.nx) + uint32_t(ix);
      const uint32_t b = g.start[c], e = g.start[c + 1];
      for (uint32_t j = b; j < e; ++j) {
        const float4 o = g.tgt[j];
        const float dx = p.x - o.x, dy = p.y - o.y, dz = p.z - o.z;
        if (dx * dx + (dy * dy + dz * dz) > r2) continue;
        const double e0 = double(o.x) - qx, e1 = double(o.y) - qy, e2 = double(o.z) - qz;
        ++cnt;
        se[0] += e0; se[1] += e1; se[2] += e2;
        see[0] += e0 * e0; see[1] += e0 * e1; see[2] += e0 * e2; see[3] += e1 * e1; see[4] += e1 * e2; see[5] += e2 * e2;
      }
    }
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    if (cnt >= min_nb) {
      const double kk = double(cnt);
      const double m0 = se[0] / kk, m1 = se[1] / kk, m2 = se[2] / kk;
      double C[3][3], V[3][3];
      C[0][0] = see[0] / kk - m0 * m0; C[0][1] = see[1] / kk - m0 * m1; C[0][2] = see[2] / kk - m0 * m2;
      C[1][1] = see[3] / kk - m1 * m1; C[1][2] = see[4] / kk - m1 * m2; C[2][2] = see[5] / kk - m2 * m2;
      C[1][0] = C[0][1]; C[2][0] = C[0][2]; C[2][1] = C[1][2];
      jacobi_sym<3>(C, V);
      int best = 0;
      if (C[1][1] < C[best][best]) best = 1;
      if (C[2][2] < (best == 0 ? C[0][0] : C[1][1])) best = 2;
      double v0 = best == 0 ? V[0][0] : (best == 1 ? V[0][1] : V[0][2]);
      double v1 = best == 0 ? V[1][0] : (best == 1 ? V[1][1] : V[1][2]);
      double v2 = best == 0 ? V[2][0] : (best == 1 ? V[2][1] : V[2][2]);
      const double nv = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
      v0 /= nv; v1 /= nv; v2 /= nv;
      const double a0 = fabs(v0), a1 = fabs(v1), a2 = fabs(v2);
      const double lead = (a0 >= a1 && a0 >= a2) ? v0 : (a1 >= a2 ? v1 : v2);
      if (lead < 0.0) { v0 = -v0; v1 = -v1; v2 = -v2; }
      out = make_float4(float(v0), float(v1), float(v2), 0.f);
    }
    nrm[k] = out;
  }
}

// caller normals (uploaded order, already normalised) -> cell order, and back
__global__ __launch_bounds__(kBlock) void k_gather_normals(const float* x, const float* y, const float* z, const float4* tgt, uint64_t n,
                                                           float4* nrm) {
  for (uint64_t k = blockIdx.x * (uint64_t)kBlock + threadIdx.x; k < n; k += (uint64_t)gridDim.x * kBlock) {
    const uint32_t i = __float_as_uint(tgt[k].w);
    nrm[k] = make_float4(x[i], y[i], z[i], 0.f);
  }
}

__global__ __launch_bounds__(kBlock) void k_scatter_normals(const float4* nrm, const float4* tgt, uint64_t n, float* x, float* y, float* z) {
  for (uint64_t k = blockIdx.x * (uint64_t)kBlock + threadIdx.x; k < n; k += (uint64_t)gridDim.x * kBlock) {
    const uint32_t i = __float_as_uint(tgt[k].w);
    const float4 v = nrm[k];
    x[i] = v.x; y[i] = v.y; z[i] = v.z;
  }
}

struct PlaneArgs {
  Tf T;
  GridDev g;
  const float4* src;
  const float4* nrm;        // cell order, as g.tgt
  uint64_t n;
  float d2max;
  double* slab;             // one kPlanePitch row per workgroup
};

// The point-to-plane hot path: k_match's correspondence (nearest_t reports the winner's slot, where its normal lies), then
// 31 double sums in registers -> wave butterfly -> LDS over the waves -> one slab row.
__global__ __launch_bounds__(kBlock) void k_match_plane(PlaneArgs A) {
  double s[S4P_ICP_PLANE_NSUMS];
#pragma unroll
  for (int k = 0; k < S4P_ICP_PLANE_NSUMS; ++k) s[k] = 0.0;
  for (uint64_t j = blockIdx.x * (uint64_t)kBlock + threadIdx.x; j < A.n; j += (uint64_t)gridDim.x * kBlock) {
    const float4 q = A.src[j];
    float x, y, z;
    apply_t(A.T, q.x, q.y, q.z, x, y, z);
    float best;
    uint32_t bi, slot;
    float4 p;
    nearest_t<true>(A.g, x, y, z, A.d2max, best, bi, p, slot);
    if (bi == 0xFFFFFFFFu) continue;
    s[0] += 1.0;
    s[1] += double(best);
    const float4 nf = A.nrm[slot];
    if (nf.x == 0.f && nf.y == 0.f && nf.z == 0.f) continue;
    const double qd[3] = {double(x), double(y), double(z)}, nd[3] = {double(nf.x), double(nf.y), double(nf.z)};
    const double a[6] = {qd[1] * nd[2] - qd[2] * nd[1], qd[2] * nd[0] - qd[0] * nd[2], qd[0] * nd[1] - qd[1] * nd[0], nd[0], nd[1], nd[2]};
    const double r = ((double(p.x) - qd[0]) * nd[0] + (double(p.y) - qd[1]) * nd[1]) + (double(p.z) - qd[2]) * nd[2];
    s[2] += 1.0;
    s[3] += r * r;
    int o = 4;
#pragma unroll
    for (int u = 0; u < 6; ++u)
#pragma unroll
      for (int v = u; v < 6; ++v) s[o++] += a[u] * a[v];
#pragma unroll
    for (int u = 0; u < 6; ++u) s[25 + u] += a[u] * r;
  }
  __shared__ double red[kBlock / 64][S4P_ICP_PLANE_NSUMS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < S4P_ICP_PLANE_NSUMS; ++k) {
    double v = s[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < S4P_ICP_PLANE_NSUMS) {
    double v = red[0][threadIdx.x];
    for (int w = 1; w < kBlock / 64; ++w) v += red[w][threadIdx.x];
    A.slab[uint64_t(blockIdx.x) * kPlanePitch + threadIdx.x] = v;
  }
}

// generalized ICP (include/s4p_icp_gicp.h).  Per iteration: k_search<false> (the one correspondence search: the winner's
// slot per visited lane), k_gicp_sum (the 31 generalized sums streamed from the slots, k_match_plane's reduction) and
// k_final_plane (the same slab pitch and fixed order).  Defined before k_final_plane, which stays the last non-template
// kernel of the translation unit (cf. the robust kernels above).

// source normals (uploaded order, already normalised) -> the order of `src` (w = original source index), next to it.
// The uploaded-order copy stays on the device, so the read-back needs no scatter.
__global__ __launch_bounds__(kBlock) void k_gather_source_normals(const float* x, const float* y, const float* z, const float4* src,
                                                                  uint64_t n, float4* snrm) {
  for (uint64_t k = blockIdx.x * (uint64_t)kBlock + threadIdx.x; k < n; k += (uint64_t)gridDim.x * kBlock) {
    const uint32_t j = __float_as_uint(src[k].w);
    snrm[k] = make_float4(x[j], y[j], z[j], 0.f);
  }
}

struct GicpArgs {
  Tf T;
  GridDev g;
  const float4* src;
  const float4* snrm;       // the order of src
  const float4* nrm;        // cell order, as g.tgt
  uint64_t n;
  const uint32_t* slot;     // k_search's
  double k;                 // 1 - epsilon
  double* slab;             // one kPlanePitch row per workgroup
};

// The generalized sums, term by term as include/s4p_icp_gicp.h states them.  No search: the winner comes from k_search's slot.
__global__ __launch_bounds__(kBlock) void k_gicp_sum(GicpArgs A) {
  constexpr int NS = S4P_ICP_PLANE_NSUMS;
  double s[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) s[k] = 0.0;
  for (uint64_t j = blockIdx.x * (uint64_t)kBlock + threadIdx.x; j < A.n; j += (uint64_t)gridDim.x * kBlock) {
    const uint32_t sl = A.slot[j];
    if (sl == kNoSlot) continue;
    const float4 q = A.src[j];
    float x, y, z;
    apply_t(A.T, q.x, q.y, q.z, x, y, z);
    const float4 p = A.g.tgt[sl];
    const float dx = x - p.x, dy = y - p.y, dz = z - p.z;
    const float d2 = dx * dx + (dy * dy + dz * dz);           // nearest_t's float d2 of the winner
    const float4 nf = A.nrm[sl], mf = A.snrm[j];
    const double qd[3] = {double(x), double(y), double(z)}, np[3] = {double(nf.x), double(nf.y), double(nf.z)};
    const double mq[3] = {double(mf.x), double(mf.y), double(mf.z)};
    double nh[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) nh[a] = (double(A.T.m[4 * a]) * mq[0] + double(A.T.m[4 * a + 1]) * mq[1]) + double(A.T.m[4 * a + 2]) * mq[2];
    const double S00 = (2.0 - A.k * (np[0] * np[0])) - A.k * (nh[0] * nh[0]);
    const double S01 = (0.0 - A.k * (np[0] * np[1])) - A.k * (nh[0] * nh[1]);
    const double S02 = (0.0 - A.k * (np[0] * np[2])) - A.k * (nh[0] * nh[2]);
    const double S11 = (2.0 - A.k * (np[1] * np[1])) - A.k * (nh[1] * nh[1]);
    const double S12 = (0.0 - A.k * (np[1] * np[2])) - A.k * (nh[1] * nh[2]);
    const double S22 = (2.0 - A.k * (np[2] * np[2])) - A.k * (nh[2] * nh[2]);
    const double c00 = S11 * S22 - S12 * S12, c01 = S02 * S12 - S01 * S22, c02 = S01 * S12 - S02 * S11;
    const double c11 = S00 * S22 - S02 * S02, c12 = S01 * S02 - S00 * S12, c22 = S00 * S11 - S01 * S01;
    const double det = (S00 * c00 + S01 * c01) + S02 * c02;
    double M[3][3];
    M[0][0] = c00 / det; M[0][1] = c01 / det; M[0][2] = c02 / det; M[1][1] = c11 / det; M[1][2] = c12 / det; M[2][2] = c22 / det;
    M[1][0] = M[0][1]; M[2][0] = M[0][2]; M[2][1] = M[1][2];
    const double r[3] = {double(p.x) - qd[0], double(p.y) - qd[1], double(p.z) - qd[2]};
    double g[3], B[3][3], W[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) g[a] = (M[a][0] * r[0] + M[a][1] * r[1]) + M[a][2] * r[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      B[0][c] = qd[1] * M[2][c] - qd[2] * M[1][c];
      B[1][c] = qd[2] * M[0][c] - qd[0] * M[2][c];
      B[2][c] = qd[0] * M[1][c] - qd[1] * M[0][c];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      W[a][0] = qd[1] * B[a][2] - qd[2] * B[a][1];
      W[a][1] = qd[2] * B[a][0] - qd[0] * B[a][2];
      W[a][2] = qd[0] * B[a][1] - qd[1] * B[a][0];
    }
    s[0] += 1.0;
    s[1] += double(d2);
    s[2] += 1.0;
    s[3] += (r[0] * g[0] + r[1] * g[1]) + r[2] * g[2];
    s[4] += W[0][0]; s[5] += W[0][1]; s[6] += W[0][2]; s[7] += B[0][0]; s[8] += B[0][1]; s[9] += B[0][2];
    s[10] += W[1][1]; s[11] += W[1][2]; s[12] += B[1][0]; s[13] += B[1][1]; s[14] += B[1][2];
    s[15] += W[2][2]; s[16] += B[2][0]; s[17] += B[2][1]; s[18] += B[2][2];
    s[19] += M[0][0]; s[20] += M[0][1]; s[21] += M[0][2]; s[22] += M[1][1]; s[23] += M[1][2]; s[24] += M[2][2];
    s[25] += qd[1] * g[2] - qd[2] * g[1];
    s[26] += qd[2] * g[0] - qd[0] * g[2];
    s[27] += qd[0] * g[1] - qd[1] * g[0];
    s[28] += g[0]; s[29] += g[1]; s[30] += g[2];
  }
  __shared__ double red[kBlock / 64][NS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    double v = s[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < NS) {
    double v = red[0][threadIdx.x];
    for (int w = 1; w < kBlock / 64; ++w) v += red[w][threadIdx.x];
    A.slab[uint64_t(blockIdx.x) * kPlanePitch + threadIdx.x] = v;
  }
}

// correspondence rejection (include/s4p_icp_reject.h): the per-point answers of s4p_icp_rejection, from the lanes of a
// k_search<false> + k_reject pass (the key of a surviving lane is its forward float d2) to the uploaded source order
__global__ __launch_bounds__(kBlock) void k_reject_out(const float4* src, const float4* tgt, const uint32_t* slot, const uint32_t* key,
                                                       const uint8_t* code, uint64_t n, int32_t* idx, float* d2, int32_t* why) {
  for (uint64_t j = blockIdx.x * (uint64_t)kBlock + threadIdx.x; j < n; j += (uint64_t)gridDim.x * kBlock) {
    const uint32_t o = __float_as_uint(src[j].w), sl = slot[j];
    const bool hit = sl != kNoSlot;
    idx[o] = hit ? int32_t(__float_as_uint(tgt[sl].w)) : -1;
    d2[o] = hit ? __uint_as_float(key[j]) : 0.f;
    why[o] = int32_t(code[j]);
  }
}

// coloured ICP (include/s4p_icp_color.h).  Once per target: the intensities in cell order (k_gather_target_intensity) and
// the intensity gradient of every target point in its tangent plane (k_color_gradient).  Per iteration: k_search<false>,
// k_color_sum (the 31 joint sums streamed from the slots, k_match_plane's reduction) and k_final_plane.  Defined before
// k_final_plane, as the generalized kernels above.

// target intensities (uploaded order) -> cell order, through the index bits of tgt[k].w
__global__ __launch_bounds__(kBlock) void k_gather_target_intensity(const float* in, const float4* tgt, uint64_t n, float* out) {
  for (uint64_t k = blockIdx.x * (uint64_t)kBlock + threadIdx.x; k < n; k += (uint64_t)gridDim.x * kBlock)
    out[k] = in[__float_as_uint(tgt[k].w)];
}

// Intensity gradient of every target point, one lane per point in cell order: k_normals' walk (the same neighbourhood, the
// same conservative cell skip), 9 double sums of the neighbours' tangent-plane offsets u and intensity differences,
// A = S + tr(S) n n^T, the Jacobi gate on A's spectrum and a cofactor solve, term by term as include/s4p_icp_color.h
// states them.  Writes (g, I_p): the sum pass reads gradient and intensity of a winner in one 16-byte load.
__global__ __launch_bounds__(kBlock) void k_color_gradient(GridDev g, const float4* nrm, const float* tint, uint64_t n, float r2,
                                                           int32_t min_nb, float4* grad) {
  const double eps = 1e-6 * g.h;
  for (uint64_t k = blockIdx.x * (uint64_t)kBlock + threadIdx.x; k < n; k += (uint64_t)gridDim.x * kBlock) {
    const float4 p = g.tgt[k];
    const float4 nf = nrm[k];
    const float ip = tint[k];
    float4 out = make_float4(0.f, 0.f, 0.f, ip);
    if (nf.x == 0.f && nf.y == 0.f && nf.z == 0.f) { grad[k] = out; continue; }
    const int cx = int(cell_coord(p.x, g.ox, g.inv_h)), cy = int(cell_coord(p.y, g.oy, g.inv_h)), cz = int(cell_coord(p.z, g.oz, g.inv_h));
    const double qx = double(p.x), qy = double(p.y), qz = double(p.z), qi = double(ip);
    const double n0 = double(nf.x), n1 = double(nf.y), n2 = double(nf.z);
    double S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};    // sum u u^T (xx xy xz yy yz zz); sum u dI
    int32_t cnt = 0;
    for (int t = 0; t < 27; ++t) {
      const int ix = cx + t % 3 - 1, iy = cy + (t / 3) % 3 - 1, iz = cz + t / 9 - 1;
      if (ix < 0 || ix >= g.nx || iy < 0 || iy >= g.ny || iz < 0 || iz >= g.nz) continue;
      const double bx0 = g.ox + ix * g.h, by0 = g.oy + iy * g.h, bz0 = g.oz + iz * g.h;
      const double ex = fmax(0.0, fmax(bx0 - qx, qx - (bx0 + g.h)) - eps);
      const double ey = fmax(0.0, fmax(by0 - qy, qy - (by0 + g.h)) - eps);
      const double ez = fmax(0.0, fmax(bz0 - qz, qz - (bz0 + g.h)) - eps);
      if ((ex * ex + ey * ey + ez * ez) * (1.0 - 1e-5) > double(r2)) continue;
      const uint32_t c = (uint32_t(iz) * uint32_t(g.ny) + uint32_t(iy)) * uint32_t(g.nx) + uint32_t(ix);
      const uint32_t cb = g.start[c], ce = g.start[c + 1];
      for (uint32_t j = cb; j < ce; ++j) {
        const float4 o = g.tgt[j];
        const float dx = p.x - o.x, dy = p.y - o.y, dz = p.z - o.z;
        if (dx * dx + (dy * dy + dz * dz) > r2) continue;
        const double e0 = double(o.x) - qx, e1 = double(o.y) - qy, e2 = double(o.z) - qz;
        const double en = (e0 * n0 + e1 * n1) + e2 * n2;
        const double u0 = e0 - en * n0, u1 = e1 - en * n1, u2 = e2 - en * n2;
        const double dI = double(tint[j]) - qi;
        ++cnt;
        S[0] += u0 * u0; S[1] += u0 * u1; S[2] += u0 * u2; S[3] += u1 * u1; S[4] += u1 * u2; S[5] += u2 * u2;
        b[0] += u0 * dI; b[1] += u1 * dI; b[2] += u2 * dI;
      }
    }
    if (cnt >= min_nb) {
      const double tr = (S[0] + S[3]) + S[5];
      const double A00 = S[0] + tr * (n0 * n0), A01 = S[1] + tr * (n0 * n1), A02 = S[2] + tr * (n0 * n2);
      const double A11 = S[3] + tr * (n1 * n1), A12 = S[4] + tr * (n1 * n2), A22 = S[5] + tr * (n2 * n2);
      double C[3][3], V[3][3];
      C[0][0] = A00; C[0][1] = A01; C[0][2] = A02; C[1][1] = A11; C[1][2] = A12; C[2][2] = A22;
      C[1][0] = A01; C[2][0] = A02; C[2][1] = A12;
      jacobi_sym<3>(C, V);
      const double lmin = fmin(fmin(C[0][0], C[1][1]), C[2][2]), lmax = fmax(fmax(C[0][0], C[1][1]), C[2][2]);
      if (lmin > S4P_ICP_COLOR_GATE * lmax) {
        const double c00 = A11 * A22 - A12 * A12, c01 = A02 * A12 - A01 * A22, c02 = A01 * A12 - A02 * A11;
        const double c11 = A00 * A22 - A02 * A02, c12 = A01 * A02 - A00 * A12, c22 = A00 * A11 - A01 * A01;
        const double det = (A00 * c00 + A01 * c01) + A02 * c02;
        out.x = float(((c00 * b[0] + c01 * b[1]) + c02 * b[2]) / det);
        out.y = float(((c01 * b[0] + c11 * b[1]) + c12 * b[2]) / det);
        out.z = float(((c02 * b[0] + c12 * b[1]) + c22 * b[2]) / det);
      }
    }
    grad[k] = out;
  }
}

// source intensities (uploaded order) -> the order of `src` (w = original source index), next to it
__global__ __launch_bounds__(kBlock) void k_gather_source_intensity(const float* in, const float4* src, uint64_t n, float* out) {
  for (uint64_t k = blockIdx.x * (uint64_t)kBlock + threadIdx.x; k < n; k += (uint64_t)gridDim.x * kBlock)
    out[k] = in[__float_as_uint(src[k].w)];
}

struct ColorArgs {
  Tf T;
  GridDev g;
  const float4* src;
  const float* sint;        // source intensities, the order of src
  const float4* nrm;        // cell order, as g.tgt
  const float4* grad;       // cell order: gradient, target intensity
  uint64_t n;
  const uint32_t* slot;     // k_search's
  double wg, wc;            // lambda, 1 - lambda
  double* slab;             // one kPlanePitch row per workgroup
};

// The joint sums, term by term as include/s4p_icp_color.h states them.  No search: the winner comes from k_search's slot.
__global__ __launch_bounds__(kBlock) void k_color_sum(ColorArgs A) {
  constexpr int NS = S4P_ICP_PLANE_NSUMS;
  double s[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) s[k] = 0.0;
  for (uint64_t j = blockIdx.x * (uint64_t)kBlock + threadIdx.x; j < A.n; j += (uint64_t)gridDim.x * kBlock) {
    const uint32_t sl = A.slot[j];
    if (sl == kNoSlot) continue;
    const float4 q = A.src[j];
    float x, y, z;
    apply_t(A.T, q.x, q.y, q.z, x, y, z);
    const float4 p = A.g.tgt[sl];
    const float dx = x - p.x, dy = y - p.y, dz = z - p.z;
    const float d2 = dx * dx + (dy * dy + dz * dz);           // nearest_t's float d2 of the winner
    s[0] += 1.0;
    s[1] += double(d2);
    const float4 nf = A.nrm[sl];
    if (nf.x == 0.f && nf.y == 0.f && nf.z == 0.f) continue;
    const float4 gf = A.grad[sl];
    const double qd[3] = {double(x), double(y), double(z)}, nd[3] = {double(nf.x), double(nf.y), double(nf.z)};
    const double gd[3] = {double(gf.x), double(gf.y), double(gf.z)};
    const double r[3] = {double(p.x) - qd[0], double(p.y) - qd[1], double(p.z) - qd[2]};
    const double sg = (r[0] * nd[0] + r[1] * nd[1]) + r[2] * nd[2];
    const double gn = (gd[0] * nd[0] + gd[1] * nd[1]) + gd[2] * nd[2];
    const double gp[3] = {gd[0] - gn * nd[0], gd[1] - gn * nd[1], gd[2] - gn * nd[2]};
    const double rc = ((double(A.sint[j]) - double(gf.w)) + ((gd[0] * r[0] + gd[1] * r[1]) + gd[2] * r[2])) - sg * gn;
    const double aG[6] = {qd[1] * nd[2] - qd[2] * nd[1], qd[2] * nd[0] - qd[0] * nd[2], qd[0] * nd[1] - qd[1] * nd[0], nd[0], nd[1], nd[2]};
    const double aC[6] = {qd[1] * gp[2] - qd[2] * gp[1], qd[2] * gp[0] - qd[0] * gp[2], qd[0] * gp[1] - qd[1] * gp[0], gp[0], gp[1], gp[2]};
    s[2] += 1.0;
    s[3] += A.wg * (sg * sg) + A.wc * (rc * rc);
    int o = 4;
#pragma unroll
    for (int u = 0; u < 6; ++u)
#pragma unroll
      for (int v = u; v < 6; ++v) s[o++] += A.wg * (aG[u] * aG[v]) + A.wc * (aC[u] * aC[v]);
#pragma unroll
    for (int u = 0; u < 6; ++u) s[25 + u] += A.wg * (aG[u] * sg) + A.wc * (aC[u] * rc);
  }
  __shared__ double red[kBlock / 64][NS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    double v = s[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < NS) {
    double v = red[0][threadIdx.x];
    for (int w = 1; w < kBlock / 64; ++w) v += red[w][threadIdx.x];
    A.slab[uint64_t(blockIdx.x) * kPlanePitch + threadIdx.x] = v;
  }
}

// the plane slab's nb rows -> 31 sums, in a fixed order: 8 parts per column (rows part, part + 8, ...), then the parts in order
__global__ __launch_bounds__(kBlock) void k_final_plane(const double* slab, int nb, double* out) {
  constexpr int kParts = kBlock / S4P_ICP_PLANE_NSUMS;     // 8
  __shared__ double part[kParts][S4P_ICP_PLANE_NSUMS];
  const int col = threadIdx.x % S4P_ICP_PLANE_NSUMS, prt = threadIdx.x / S4P_ICP_PLANE_NSUMS;
  if (prt < kParts) {
    double v = 0.0;
    for (int r = prt; r < nb; r += kParts) v += slab[uint64_t(r) * kPlanePitch + col];
    part[prt][col] = v;
  }
  __syncthreads();
  if (threadIdx.x < S4P_ICP_PLANE_NSUMS) {
    double v = part[0][threadIdx.x];
    for (int p = 1; p < kParts; ++p) v += part[p][threadIdx.x];
    out[threadIdx.x] = v;
  }
}

// robust ICP, continued: the correspondence search and the weighted sums (templates on the metric)

struct SearchArgs {
  Tf T;
  GridDev g;
  const float4* src;
  const float4* nrm;        // plane: cell order, as g.tgt
  uint64_t n;
  float d2max;
  uint32_t* slot;           // per visited lane: the winner's cell-order position, or kNoSlot
  uint32_t* key;            // per visited lane: the bits of u, or kNoKey
};

template <bool PLANE>
__global__ __launch_bounds__(kBlock) void k_search(SearchArgs A) {
  for (uint64_t j = blockIdx.x * (uint64_t)kBlock + threadIdx.x; j < A.n; j += (uint64_t)gridDim.x * kBlock) {
    const float4 q = A.src[j];
    float x, y, z;
    apply_t(A.T, q.x, q.y, q.z, x, y, z);
    float best;
    uint32_t bi, slot;
    float4 p;
    nearest_t<true>(A.g, x, y, z, A.d2max, best, bi, p, slot);
    uint32_t sl = kNoSlot, ky = kNoKey;
    if (bi != 0xFFFFFFFFu) {
      sl = slot;
      if (PLANE) {
        const float4 nf = A.nrm[slot];
        if (!(nf.x == 0.f && nf.y == 0.f && nf.z == 0.f)) {
          const double qd[3] = {double(x), double(y), double(z)}, nd[3] = {double(nf.x), double(nf.y), double(nf.z)};
          const double r = ((double(p.x) - qd[0]) * nd[0] + (double(p.y) - qd[1]) * nd[1]) + (double(p.z) - qd[2]) * nd[2];
          ky = __float_as_uint(float(r * r));
        }
      } else {
        ky = __float_as_uint(best);
      }
    }
    A.slot[j] = sl;
    A.key[j] = ky;
  }
}

// correspondence rejection (include/s4p_icp_reject.h), between k_search and the sum kernel of a split pass
struct RejectArgs {
  Tf T;                     // the pass's T: its linear part rotates the source normals
  Tf Ti;                    // the reverse map T- (host)
  GridDev g;                // the target grid
  GridDev gs;               // the source grid: tgt = Q' in cell order, w = the uploaded source index
  const float4* src;
  const float4* snrm;       // source normals, the order of src
  const float4* nrm;        // target normals, cell order, as g.tgt
  uint64_t n;
  float d2max;
  int32_t oriented;         // normal test: c >= ncos (else |c| >= ncos)
  double ncos;
  uint32_t* slot;           // k_search's; a rejected lane gets kNoSlot / kNoKey
  uint32_t* key;
  uint8_t* code;            // optional: S4P_ICP_WHY_* per visited lane
  unsigned long long* counts;   // matched, by normals, by reciprocity, kept
};

// One lane per visited source lane, in src's order (the order of the T0-image cells: neighbouring lanes search
// neighbouring source cells backwards).  The normal test first; a pair that fails it is not searched backwards.  Every
// lane of a wave runs the same number of rounds, so each ballot sees the whole wave: the four counters are wave-uniform
// integers, added once per wave at the end (integer atomics only).
template <bool RECIP, bool NORMAL>
__global__ __launch_bounds__(kBlock) void k_reject(RejectArgs A) {
  uint32_t c_matched = 0, c_normal = 0, c_recip = 0, c_kept = 0;
  for (uint64_t base = blockIdx.x * (uint64_t)kBlock; base < A.n; base += (uint64_t)gridDim.x * kBlock) {
    const uint64_t j = base + threadIdx.x;
    const bool in = j < A.n;
    const uint32_t sl = in ? A.slot[j] : kNoSlot;
    const bool matched = sl != kNoSlot;
    bool by_normal = false, by_recip = false;
    if (NORMAL && matched) {
      const float4 nf = A.nrm[sl], mf = A.snrm[j];
      const bool info = !(nf.x == 0.f && nf.y == 0.f && nf.z == 0.f) && !(mf.x == 0.f && mf.y == 0.f && mf.z == 0.f);
      if (info) {
        const double mq[3] = {double(mf.x), double(mf.y), double(mf.z)};
        double nh[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) nh[a] = (double(A.T.m[4 * a]) * mq[0] + double(A.T.m[4 * a + 1]) * mq[1]) + double(A.T.m[4 * a + 2]) * mq[2];
        const double c = (double(nf.x) * nh[0] + double(nf.y) * nh[1]) + double(nf.z) * nh[2];
        by_normal = !((A.oriented ? c : fabs(c)) >= A.ncos);
      }
    }
    if (RECIP && matched && !by_normal) {
      const float4 p = A.g.tgt[sl];
      float x, y, z;
      apply_t(A.Ti, p.x, p.y, p.z, x, y, z);
      float best;
      uint32_t bi;
      float4 bq;
      nearest(A.gs, x, y, z, A.d2max, best, bi, bq);
      by_recip = bi != __float_as_uint(A.src[j].w);
    }
    const bool rejected = by_normal || by_recip;
    if (rejected) { A.slot[j] = kNoSlot; A.key[j] = kNoKey; }
    if (A.code && in)
      A.code[j] = uint8_t(!matched ? S4P_ICP_WHY_UNMATCHED
                                   : (by_normal ? S4P_ICP_WHY_NORMALS : (by_recip ? S4P_ICP_WHY_RECIPROCITY : S4P_ICP_WHY_KEPT)));
    c_matched += uint32_t(__popcll(__ballot(matched)));
    c_normal += uint32_t(__popcll(__ballot(by_normal)));
    c_recip += uint32_t(__popcll(__ballot(by_recip)));
    c_kept += uint32_t(__popcll(__ballot(matched && !rejected)));
  }
  if ((threadIdx.x & 63) == 0) {
    if (c_matched) atomicAdd(&A.counts[0], (unsigned long long)c_matched);
    if (c_normal) atomicAdd(&A.counts[1], (unsigned long long)c_normal);
    if (c_recip) atomicAdd(&A.counts[2], (unsigned long long)c_recip);
    if (c_kept) atomicAdd(&A.counts[3], (unsigned long long)c_kept);
  }
}

constexpr int32_t kLossOnes = 0;            // every weight 1: the plain point / plane sums under rejection

__device__ inline double robust_weight(int loss, float u, uint32_t thr, double cs, double cs2) {
  if (loss == kLossOnes) return 1.0;
  if (loss == S4P_ICP_LOSS_TRIMMED) return __float_as_uint(u) <= thr ? 1.0 : 0.0;
  const double ud = double(u);
  if (loss == S4P_ICP_LOSS_HUBER) return ud <= cs2 ? 1.0 : cs / sqrt(ud);
  if (ud < cs2) {
    const double t = 1.0 - ud / cs2;
    return t * t;
  }
  return 0.0;
}

struct WsumArgs {
  Tf T;
  GridDev g;
  const float4* src;
  const float4* nrm;
  uint64_t n;
  const uint32_t* slot;     // k_search's
  const SelState* st;
  int32_t loss;
  double* slab;             // one kPitch (point) / kPlanePitch (plane) row per workgroup
};

// The weighted sums: k_match / k_match_plane's lanes, terms and reduction with every keyed pair's terms times w (so w == 1
// gives their bits), plus one column: the count with w > 0.  No search: the winner comes from k_search's slot.
template <bool PLANE>
__global__ __launch_bounds__(kBlock) void k_wsum(WsumArgs A) {
  constexpr int NS = PLANE ? S4P_ICP_PLANE_NSUMS : S4P_ICP_NSUMS;
  constexpr int NC = NS + 1;
  constexpr int kRowPitch = PLANE ? kPlanePitch : kPitch;
  static_assert(NC <= kRowPitch, "slab row");
  double s[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) s[k] = 0.0;
  const uint32_t thr = A.st->prefix;
  const double cs = A.st->cs, cs2 = A.st->cs2;
  for (uint64_t j = blockIdx.x * (uint64_t)kBlock + threadIdx.x; j < A.n; j += (uint64_t)gridDim.x * kBlock) {
    const uint32_t sl = A.slot[j];
    if (sl == kNoSlot) continue;
    const float4 q = A.src[j];
    float x, y, z;
    apply_t(A.T, q.x, q.y, q.z, x, y, z);
    const float4 p = A.g.tgt[sl];
    const float dx = x - p.x, dy = y - p.y, dz = z - p.z;
    const float d2 = dx * dx + (dy * dy + dz * dz);           // nearest_t's float d2 of the winner
    const double qd[3] = {double(x), double(y), double(z)};
    if (PLANE) {
      const float4 nf = A.nrm[sl];
      if (nf.x == 0.f && nf.y == 0.f && nf.z == 0.f) {        // no key: counted as in k_match_plane
        s[0] += 1.0;
        s[1] += double(d2);
        s[NS] += 1.0;
        continue;
      }
      const double nd[3] = {double(nf.x), double(nf.y), double(nf.z)};
      const double a[6] = {qd[1] * nd[2] - qd[2] * nd[1], qd[2] * nd[0] - qd[0] * nd[2], qd[0] * nd[1] - qd[1] * nd[0], nd[0], nd[1], nd[2]};
      const double r = ((double(p.x) - qd[0]) * nd[0] + (double(p.y) - qd[1]) * nd[1]) + (double(p.z) - qd[2]) * nd[2];
      const double w = robust_weight(A.loss, float(r * r), thr, cs, cs2);
      if (!(w > 0.0)) continue;
      s[0] += w;
      s[1] += double(d2) * w;
      s[2] += 1.0;
      s[3] += (r * r) * w;
      int o = 4;
#pragma unroll
      for (int u = 0; u < 6; ++u)
#pragma unroll
        for (int v = u; v < 6; ++v) s[o++] += (a[u] * a[v]) * w;
#pragma unroll
      for (int u = 0; u < 6; ++u) s[25 + u] += (a[u] * r) * w;
    } else {
      const double w = robust_weight(A.loss, d2, thr, cs, cs2);
      if (!(w > 0.0)) continue;
      const double pd[3] = {double(p.x), double(p.y), double(p.z)};
      s[0] += w;
#pragma unroll
      for (int a = 0; a < 3; ++a) { s[1 + a] += qd[a] * w; s[4 + a] += pd[a] * w; }
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) s[7 + 3 * a + b] += (qd[a] * pd[b]) * w;
      s[16] += double(d2) * w;
    }
    s[NS] += 1.0;
  }
  __shared__ double red[kBlock / 64][NC];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    double v = s[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < NC) {
    double v = red[0][threadIdx.x];
    for (int w = 1; w < kBlock / 64; ++w) v += red[w][threadIdx.x];
    A.slab[uint64_t(blockIdx.x) * kRowPitch + threadIdx.x] = v;
  }
}

// k_final / k_final_plane's order for the NS sums.  The count column (whole numbers: exact in any order) is summed by all
// threads; the last thread (idle in k_final / k_final_plane's scheme) adds their parts and writes the info.
template <bool PLANE>
__global__ __launch_bounds__(kBlock) void k_wfinal(const double* slab, int nb, const SelState* st, double* out) {
  constexpr int NS = PLANE ? S4P_ICP_PLANE_NSUMS : S4P_ICP_NSUMS;
  constexpr int kRowPitch = PLANE ? kPlanePitch : kPitch;
  constexpr int kParts = kBlock / NS;
  static_assert(kParts * NS < kBlock, "a spare thread");
  __shared__ double part[kParts][NS];
  __shared__ double cpart[kBlock];
  const int col = threadIdx.x % NS, prt = threadIdx.x / NS;
  if (prt < kParts) {
    double v = 0.0;
    for (int r = prt; r < nb; r += kParts) v += slab[uint64_t(r) * kRowPitch + col];
    part[prt][col] = v;
  }
  double c = 0.0;
  for (int r = threadIdx.x; r < nb; r += kBlock) c += slab[uint64_t(r) * kRowPitch + NS];
  cpart[threadIdx.x] = c;
  __syncthreads();
  if (threadIdx.x < NS) {
    double v = part[0][threadIdx.x];
    for (int p = 1; p < kParts; ++p) v += part[p][threadIdx.x];
    out[threadIdx.x] = v;
  }
  if (threadIdx.x == kBlock - 1) {
    double cnt = 0.0;
    for (int t = 0; t < kBlock; ++t) cnt += cpart[t];
    double* info = out + NS;
    info[0] = double(st->M);
    info[1] = double(st->k);
    info[2] = st->k ? double(st->prefix) : 0.0;
    info[3] = st->s;
    info[4] = cnt;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host: Horn's closed form.  N (4x4 symmetric) from the centred cross-covariance; its eigenvector of the largest
// eigenvalue (cyclic Jacobi) is the unit quaternion of the rotation.
void jacobi4(double A[4][4], double V[4][4]) {
  for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 64; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < 4; ++i) { diag += A[i][i] * A[i][i]; for (int j = i + 1; j < 4; ++j) off += A[i][j] * A[i][j]; }
    if (off == 0.0 || off <= 1e-36 * diag) break;
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 4; ++q) {
        if (A[p][q] == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 4; ++k) {            // A <- J^T A J, columns then rows
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 4; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < 4; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq;
        }
      }
  }
}

void mat_mul4(const double* A, const double* B, double* C) {    // C = A B (row-major 4x4); C may not alias
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      double v = 0.0;
      for (int k = 0; k < 4; ++k) v += A[4 * r + k] * B[4 * k + c];
      C[4 * r + c] = v;
    }
}

// caller frame <-> centred frame (p' = p - c, q' = q - c): T' = [R | R c + t - c], T = [R | t' - R c + c]
void to_centred(const double* T, const float* c, double* Tc) {
  std::memcpy(Tc, T, 16 * sizeof(double));
  for (int r = 0; r < 3; ++r) Tc[4 * r + 3] = T[4 * r + 3] + (T[4 * r] * c[0] + T[4 * r + 1] * c[1] + T[4 * r + 2] * c[2]) - double(c[r]);
}
void from_centred(const double* Tc, const float* c, double* T) {
  std::memcpy(T, Tc, 16 * sizeof(double));
  for (int r = 0; r < 3; ++r) T[4 * r + 3] = Tc[4 * r + 3] - (Tc[4 * r] * c[0] + Tc[4 * r + 1] * c[1] + Tc[4 * r + 2] * c[2]) + double(c[r]);
}
Tf to_float(const double* T) {
  Tf f;
  for (int k = 0; k < 12; ++k) f.m[k] = float(T[k]);
  return f;
}

}  // namespace s4p_icp

using namespace s4p_icp;

struct s4p_icp_ctx {
  int device = 0;
  hipStream_t st = nullptr;
  hipEvent_t ev = nullptr;
  std::string err;
  bool has_target = false, has_source = false, src_dirty = true;
  float c[3] = {0.f, 0.f, 0.f};
  float d = 0.f, d2max = 0.f;
  GridDev g{};
  uint64_t ncell = 0;
  int64_t n_p = 0, n_q = 0;
  float4* tgt = nullptr;
  uint32_t* start = nullptr;
  float* qraw[3] = {nullptr, nullptr, nullptr};
  float4* src = nullptr;
  float4* src_ord = nullptr;
  double* slab = nullptr;
  double* dsum = nullptr;
  double* hsum = nullptr;            // pinned
  float4* nrm = nullptr;             // target normals, cell order (point-to-plane)
  bool has_normals = false;
  double* pslab = nullptr;           // plane slab: kMaxBlocks rows of kPlanePitch
  // robust ICP (include/s4p_icp_robust.h), allocated on first use
  int64_t r_n = 0;                   // entries of rslot / rkey
  uint32_t* rslot = nullptr;
  uint32_t* rkey = nullptr;
  uint32_t* rhist = nullptr;         // kDigits x kBins
  SelState* rst = nullptr;
  double* rsum = nullptr;            // sums + info
  double* rhsum = nullptr;           // pinned
  // generalized ICP (include/s4p_icp_gicp.h)
  int64_t sn_n = 0;                  // entries of sn / snrm
  float* sn[3] = {nullptr, nullptr, nullptr};   // source normals as stored, uploaded order
  float4* snrm = nullptr;            // the same in the order of the pass's source
  bool has_src_normals = false;
  // coloured ICP (include/s4p_icp_color.h)
  float* tint = nullptr;             // target intensities, cell order
  float4* grad = nullptr;            // target gradients and intensities, cell order
  bool has_tint = false, has_grad = false;
  int64_t si_n = 0;                  // entries of si / sint
  float* si = nullptr;               // source intensities, uploaded order
  float* sint = nullptr;             // the same in the order of the pass's source
  bool has_sint = false;
  // correspondence rejection (include/s4p_icp_reject.h)
  s4p_icp_reject rej{};              // validated; everything off by default
  bool rej_on = false;
  GridDev gs{};                      // the source grid (reverse search), built when a pass first needs it
  float4* sgrid = nullptr;           // Q' in its cell order, w = the uploaded source index
  uint32_t* sstart = nullptr;
  bool sgrid_valid = false;
  unsigned long long* rcnt = nullptr;    // the four counters of a pass
  unsigned long long* rhcnt = nullptr;   // pinned
  int64_t rej_counts[4] = {0, 0, 0, 0};
};

namespace {

std::string g_create_error;
constexpr int kSumsCap = S4P_ICP_PLANE_NSUMS;       // dsum / hsum hold the 17 point or the 31 plane sums
static_assert(S4P_ICP_PLANE_NSUMS >= S4P_ICP_NSUMS, "sum buffers");

int32_t fail(s4p_icp_ctx* h, int32_t code, const std::string& msg) {
  h->err = msg;
  return code;
}

#define ICP_HIP(expr)                                                                                             \
  do {                                                                                                            \
    const hipError_t e_ = (expr);                                                                                 \
    if (e_ != hipSuccess) return fail(h, e_ == hipErrorOutOfMemory ? S4P_ICP_ERR_OOM : S4P_ICP_ERR_HIP,          \
                                      std::string(#expr) + ": " + hipGetErrorString(e_));                        \
  } while (0)

void dfree(void* p) { if (p) (void)hipFree(p); }

// device temporaries of one call, released on every exit
struct Scratch {
  std::vector<void*> ptrs;
  ~Scratch() { for (void* p : ptrs) dfree(p); }
  hipError_t alloc(void** p, size_t bytes) {
    const hipError_t e = hipMalloc(p, bytes ? bytes : 16);
    if (e == hipSuccess) ptrs.push_back(*p); else *p = nullptr;
    return e;
  }
};

int end_bit(uint64_t max_key) {
  int b = 1;
  while (b < 32 && (max_key >> b) != 0) ++b;
  return b;
}

// (keys, vals) sorted by key into (keys_out, vals_out): radix sort (stable, deterministic)
int32_t sort_pairs(s4p_icp_ctx* h, Scratch& S, const uint32_t* keys, uint32_t* keys_out, const uint32_t* vals, uint32_t* vals_out,
                   uint64_t n, uint64_t max_key) {
  size_t bytes = 0;
  ICP_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, keys, keys_out, vals, vals_out, int(n), 0, end_bit(max_key), h->st));
  void* tmp = nullptr;
  ICP_HIP(S.alloc(&tmp, bytes));
  ICP_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, bytes, keys, keys_out, vals, vals_out, int(n), 0, end_bit(max_key), h->st));
  return S4P_ICP_OK;
}

// coordinate sums and float bounds of a cloud on the device: k_stats' per-block partials, combined on the host in row order
int32_t cloud_stats(s4p_icp_ctx* h, Scratch& S, float* const p[3], int64_t n, double sum[3], float lo[3], float hi[3]) {
  const int nb = blocks_for(n);
  double* rows = nullptr;
  ICP_HIP(S.alloc((void**)&rows, size_t(nb) * kStatsPitch * sizeof(double)));
  hipLaunchKernelGGL(k_stats, dim3(nb), dim3(kBlock), 0, h->st, p[0], p[1], p[2], uint64_t(n), rows);
  ICP_HIP(hipGetLastError());
  std::vector<double> hr(size_t(nb) * kStatsPitch);
  ICP_HIP(hipMemcpyAsync(hr.data(), rows, hr.size() * sizeof(double), hipMemcpyDeviceToHost, h->st));
  ICP_HIP(hipStreamSynchronize(h->st));
  for (int a = 0; a < 3; ++a) { sum[a] = 0.0; lo[a] = float(hr[3 + a]); hi[a] = float(hr[6 + a]); }
  for (int b = 0; b < nb; ++b)
    for (int a = 0; a < 3; ++a) {
      sum[a] += hr[size_t(b) * kStatsPitch + a];
      lo[a] = std::min(lo[a], float(hr[size_t(b) * kStatsPitch + 3 + a]));
      hi[a] = std::max(hi[a], float(hr[size_t(b) * kStatsPitch + 6 + a]));
    }
  return S4P_ICP_OK;
}

// grid plan over the centred bounds [plo, phi] of n points: cell edge 1.02 d, enlarged x 1.25 until the dense grid fits the
// cell cap (cf. LcpGridHost::plan)
int32_t plan_grid(s4p_icp_ctx* h, const float plo[3], const float phi[3], uint64_t un, float d, GridDev* g, uint64_t* ncell,
                  const char* who) {
  const uint64_t cap = std::min<uint64_t>(kMaxCells, std::max<uint64_t>(1ull << 20, 2 * un));
  double hh = double(d) * double(kCellFactor);
  int dims[3];
  for (int guard = 0;; ++guard) {
    const double inv = 1.0 / hh;
    bool ok = true;
    uint64_t nc = 1;
    for (int a = 0; a < 3; ++a) {
      const double cc = cell_coord(phi[a], double(plo[a]), inv);
      if (!(cc < 1.0e9)) { ok = false; break; }
      dims[a] = int(cc) + 1;
      nc *= uint64_t(dims[a]);
      if (nc > cap) { ok = false; break; }
    }
    if (ok) { g->h = hh; g->inv_h = inv; *ncell = nc; break; }
    if (guard > 400) return fail(h, S4P_ICP_ERR_BAD_ARG, std::string(who) + ": no grid fits the cloud's extent");
    hh *= 1.25;
  }
  g->ox = plo[0]; g->oy = plo[1]; g->oz = plo[2];
  g->nx = dims[0]; g->ny = dims[1]; g->nz = dims[2];
  return S4P_ICP_OK;
}

// the cell-ordered cloud fl(p - c) (w = the index) and the start of every cell of the planned grid g; *pts and *start are
// allocated here and entered into g
int32_t build_grid(s4p_icp_ctx* h, Scratch& S, float* const p[3], uint64_t un, const float c[3], GridDev* g, uint64_t ncell, float4** pts,
                   uint32_t** start) {
  const int nb = blocks_for(int64_t(un));
  uint32_t *keys, *vals, *keys2, *vals2;
  ICP_HIP(S.alloc((void**)&keys, un * 4)); ICP_HIP(S.alloc((void**)&vals, un * 4));
  ICP_HIP(S.alloc((void**)&keys2, un * 4)); ICP_HIP(S.alloc((void**)&vals2, un * 4));
  hipLaunchKernelGGL(k_cell_keys, dim3(nb), dim3(kBlock), 0, h->st, p[0], p[1], p[2], un, c[0], c[1], c[2], *g, keys, vals);
  ICP_HIP(hipGetLastError());
  if (int32_t rc = sort_pairs(h, S, keys, keys2, vals, vals2, un, ncell - 1)) return rc;
  ICP_HIP(hipMalloc((void**)start, (ncell + 1) * sizeof(uint32_t)));
  ICP_HIP(hipMalloc((void**)pts, un * sizeof(float4)));
  hipLaunchKernelGGL(k_cell_starts, dim3(blocks_for(int64_t(ncell) + 1)), dim3(kBlock), 0, h->st, keys2, un, ncell, *start);
  ICP_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_gather_target, dim3(nb), dim3(kBlock), 0, h->st, p[0], p[1], p[2], un, c[0], c[1], c[2], vals2, *pts);
  ICP_HIP(hipGetLastError());
  ICP_HIP(hipStreamSynchronize(h->st));          // the scratch is freed on return
  g->tgt = *pts;
  g->start = *start;
  return S4P_ICP_OK;
}

void drop_source_grid(s4p_icp_ctx* h) {
  h->sgrid_valid = false;
  dfree(h->sgrid); dfree(h->sstart);
  h->sgrid = nullptr; h->sstart = nullptr;
}

int32_t set_target_impl(s4p_icp_ctx* h, const float* x, const float* y, const float* z, int64_t n, float d, hipMemcpyKind kind) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!x || !y || !z || n < 1) return fail(h, S4P_ICP_ERR_BAD_ARG, "set_target: empty or null cloud");
  if (n >= int64_t(0x7FFFFFFF)) return fail(h, S4P_ICP_ERR_BAD_ARG, "set_target: more than 2^31 - 1 points");
  if (!(d > 0.f) || !std::isfinite(d)) return fail(h, S4P_ICP_ERR_BAD_ARG, "set_target: max_distance must be finite and > 0");
  ICP_HIP(hipSetDevice(h->device));
  h->has_target = false;
  h->has_normals = false;
  dfree(h->nrm); h->nrm = nullptr;
  h->has_tint = h->has_grad = false;
  dfree(h->tint); dfree(h->grad); h->tint = nullptr; h->grad = nullptr;
  dfree(h->tgt); h->tgt = nullptr;
  dfree(h->start); h->start = nullptr;
  drop_source_grid(h);                            // the frame and d are the target's
  Scratch S;
  const uint64_t un = uint64_t(n);
  float* p[3];
  const float* in[3] = {x, y, z};
  for (int a = 0; a < 3; ++a) {
    ICP_HIP(S.alloc((void**)&p[a], un * sizeof(float)));
    ICP_HIP(hipMemcpyAsync(p[a], in[a], un * sizeof(float), kind, h->st));
  }
  // frame and bounds
  double sum[3];
  float lo[3], hi[3];
  if (int32_t rc = cloud_stats(h, S, p, n, sum, lo, hi)) return rc;
  for (int a = 0; a < 3; ++a) {
    if (!std::isfinite(lo[a]) || !std::isfinite(hi[a])) return fail(h, S4P_ICP_ERR_BAD_ARG, "set_target: non-finite coordinates");
    h->c[a] = float(sum[a] / double(n));
  }
  // bounds of P' = fl(P - c): rounding is monotone, so they are fl(lo - c), fl(hi - c)
  float plo[3], phi[3];
  for (int a = 0; a < 3; ++a) { plo[a] = lo[a] - h->c[a]; phi[a] = hi[a] - h->c[a]; }
  if (int32_t rc = plan_grid(h, plo, phi, un, d, &h->g, &h->ncell, "set_target")) return rc;
  h->d = d;
  h->d2max = d * d;
  if (int32_t rc = build_grid(h, S, p, un, h->c, &h->g, h->ncell, &h->tgt, &h->start)) return rc;
  h->n_p = n;
  h->has_target = true;
  h->src_dirty = true;                          // Q' depends on c
  return S4P_ICP_OK;
}

// The source grid of the reverse search (include/s4p_icp_reject.h): set_target's plan and build over Q' = fl(Q - c) in the
// uploaded order, from the coordinates as uploaded.  Built once; set_source and set_target drop it.
int32_t source_grid_ready(s4p_icp_ctx* h) {
  if (h->sgrid_valid) return S4P_ICP_OK;
  drop_source_grid(h);
  Scratch S;
  double sum[3];
  float lo[3], hi[3];
  if (int32_t rc = cloud_stats(h, S, h->qraw, h->n_q, sum, lo, hi)) return rc;
  float plo[3], phi[3];
  for (int a = 0; a < 3; ++a) {
    plo[a] = lo[a] - h->c[a]; phi[a] = hi[a] - h->c[a];
    if (!std::isfinite(plo[a]) || !std::isfinite(phi[a])) return fail(h, S4P_ICP_ERR_BAD_ARG, "rejection: non-finite source coordinates");
  }
  uint64_t ncell = 0;
  if (int32_t rc = plan_grid(h, plo, phi, uint64_t(h->n_q), h->d, &h->gs, &ncell, "rejection")) return rc;
  if (int32_t rc = build_grid(h, S, h->qraw, uint64_t(h->n_q), h->c, &h->gs, ncell, &h->sgrid, &h->sstart)) return rc;
  h->sgrid_valid = true;
  return S4P_ICP_OK;
}

int32_t set_source_impl(s4p_icp_ctx* h, const float* x, const float* y, const float* z, int64_t n, hipMemcpyKind kind) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!x || !y || !z || n < 1) return fail(h, S4P_ICP_ERR_BAD_ARG, "set_source: empty or null cloud");
  if (n >= int64_t(0x7FFFFFFF)) return fail(h, S4P_ICP_ERR_BAD_ARG, "set_source: more than 2^31 - 1 points");
  ICP_HIP(hipSetDevice(h->device));
  h->has_source = false;
  h->has_src_normals = false;
  h->has_sint = false;
  drop_source_grid(h);
  if (n != h->n_q) {
    for (int a = 0; a < 3; ++a) { dfree(h->qraw[a]); h->qraw[a] = nullptr; }
    dfree(h->src); dfree(h->src_ord); h->src = h->src_ord = nullptr;
    dfree(h->slab); h->slab = nullptr;
    h->n_q = 0;
    for (int a = 0; a < 3; ++a) ICP_HIP(hipMalloc((void**)&h->qraw[a], size_t(n) * sizeof(float)));
    ICP_HIP(hipMalloc((void**)&h->src, size_t(n) * sizeof(float4)));
    ICP_HIP(hipMalloc((void**)&h->src_ord, size_t(n) * sizeof(float4)));
    ICP_HIP(hipMalloc((void**)&h->slab, size_t(blocks_for(n)) * kPitch * sizeof(double)));
    h->n_q = n;
  }
  const float* in[3] = {x, y, z};
  for (int a = 0; a < 3; ++a) ICP_HIP(hipMemcpyAsync(h->qraw[a], in[a], size_t(n) * sizeof(float), kind, h->st));
  ICP_HIP(hipStreamSynchronize(h->st));
  h->has_source = true;
  h->src_dirty = true;
  return S4P_ICP_OK;
}

int32_t ready(s4p_icp_ctx* h) {
  if (!h->has_target || !h->has_source) return fail(h, S4P_ICP_ERR_STATE, "set_target and set_source first");
  ICP_HIP(hipSetDevice(h->device));
  if (h->src_dirty) {
    hipLaunchKernelGGL(k_center_source, dim3(blocks_for(h->n_q)), dim3(kBlock), 0, h->st, h->qraw[0], h->qraw[1], h->qraw[2],
                       uint64_t(h->n_q), h->c[0], h->c[1], h->c[2], h->src);
    ICP_HIP(hipGetLastError());
    h->src_dirty = false;
  }
  return S4P_ICP_OK;
}

// a validated s4p_icp_robust: the loss, the selection and its inputs
struct RobustCfg {
  int32_t loss = 0;
  int mode = kSelNone;
  uint64_t kq = 0;          // TRIMMED: ceil(trim_fraction * n_Q)
  double scale = 0.0, c = 0.0, smin = 0.0;
};

int32_t robust_cfg(s4p_icp_ctx* h, int32_t metric, const s4p_icp_robust* R, RobustCfg* out) {
  if (!R) return fail(h, S4P_ICP_ERR_BAD_ARG, "robust: null parameters");
  if (metric != S4P_ICP_METRIC_POINT && metric != S4P_ICP_METRIC_PLANE) return fail(h, S4P_ICP_ERR_BAD_ARG, "robust: unknown metric");
  RobustCfg C;
  C.loss = R->loss;
  C.smin = 1e-6 * double(h->d);
  if (R->loss == S4P_ICP_LOSS_TRIMMED) {
    if (!(R->trim_fraction > 0.0 && R->trim_fraction <= 1.0))
      return fail(h, S4P_ICP_ERR_BAD_ARG, "robust: trim_fraction must be in (0, 1]");
    C.mode = kSelTrim;
    C.kq = uint64_t(std::ceil(R->trim_fraction * double(h->n_q)));
  } else if (R->loss == S4P_ICP_LOSS_HUBER || R->loss == S4P_ICP_LOSS_TUKEY) {
    if (!(R->c > 0.0) || !std::isfinite(R->c)) return fail(h, S4P_ICP_ERR_BAD_ARG, "robust: c must be finite and > 0");
    if (std::isnan(R->scale) || !(R->scale < INFINITY)) return fail(h, S4P_ICP_ERR_BAD_ARG, "robust: scale must be finite");
    C.c = R->c;
    C.scale = R->scale > 0.0 ? R->scale : 0.0;
    C.mode = R->scale > 0.0 ? kSelNone : kSelMedian;
  } else {
    return fail(h, S4P_ICP_ERR_BAD_ARG, "robust: unknown loss");
  }
  *out = C;
  return S4P_ICP_OK;
}

// T- of include/s4p_icp_reject.h: the transposed float entries and t-_a = float(-((m_0a t_0 + m_1a t_1) + m_2a t_2)) in double
Tf reverse_map(const Tf& T) {
  Tf R;
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) R.m[4 * a + b] = T.m[4 * b + a];
    R.m[4 * a + 3] = float(-((double(T.m[a]) * double(T.m[3]) + double(T.m[4 + a]) * double(T.m[7])) + double(T.m[8 + a]) * double(T.m[11])));
  }
  return R;
}

// k_reject on the slots and keys k_search has just written for (T, src), after reject_prepare for this src; the counters
// follow the pass's sums to the host (reject_done after the pass's synchronisation).  code: optional, per visited lane.
int32_t launch_reject(s4p_icp_ctx* h, const Tf& T, const float4* src, uint8_t* code) {
  ICP_HIP(hipMemsetAsync(h->rcnt, 0, 4 * sizeof(unsigned long long), h->st));
  RejectArgs A;
  A.T = T; A.Ti = reverse_map(T); A.g = h->g; A.gs = h->gs; A.src = src; A.snrm = h->snrm; A.nrm = h->nrm; A.n = uint64_t(h->n_q);
  A.d2max = h->d2max; A.oriented = h->rej.normal_mode == S4P_ICP_REJECT_NORMALS_ORIENTED; A.ncos = h->rej.normal_cos;
  A.slot = h->rslot; A.key = h->rkey; A.code = code; A.counts = h->rcnt;
  const int nb = blocks_for(h->n_q);
  const bool rc = h->rej.reciprocal != 0, nm = h->rej.normal_mode != S4P_ICP_REJECT_NORMALS_OFF;
  if (rc && nm) hipLaunchKernelGGL((k_reject<true, true>), dim3(nb), dim3(kBlock), 0, h->st, A);
  else if (rc) hipLaunchKernelGGL((k_reject<true, false>), dim3(nb), dim3(kBlock), 0, h->st, A);
  else if (nm) hipLaunchKernelGGL((k_reject<false, true>), dim3(nb), dim3(kBlock), 0, h->st, A);
  else hipLaunchKernelGGL((k_reject<false, false>), dim3(nb), dim3(kBlock), 0, h->st, A);      // s4p_icp_rejection with everything off
  ICP_HIP(hipGetLastError());
  ICP_HIP(hipMemcpyAsync(h->rhcnt, h->rcnt, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->st));
  return S4P_ICP_OK;
}

void reject_done(s4p_icp_ctx* h) {
  for (int k = 0; k < 4; ++k) h->rej_counts[k] = int64_t(h->rhcnt[k]);
}

// One robust pass over `src` for T: one search, the selection, the weighted sums; sums and info on the host.
int32_t robust_pass(s4p_icp_ctx* h, const Tf& T, const float4* src, bool plane, const RobustCfg& C, double* sums, double* info) {
  const uint64_t un = uint64_t(h->n_q);
  if (h->r_n != h->n_q) {
    dfree(h->rslot); dfree(h->rkey); h->rslot = h->rkey = nullptr;
    h->r_n = 0;
    ICP_HIP(hipMalloc((void**)&h->rslot, un * sizeof(uint32_t)));
    ICP_HIP(hipMalloc((void**)&h->rkey, un * sizeof(uint32_t)));
    h->r_n = h->n_q;
  }
  constexpr int kOut = S4P_ICP_PLANE_NSUMS + S4P_ICP_ROBUST_NINFO;
  if (!h->rhist) ICP_HIP(hipMalloc((void**)&h->rhist, kDigits * kBins * sizeof(uint32_t)));
  if (!h->rst) ICP_HIP(hipMalloc((void**)&h->rst, sizeof(SelState)));
  if (!h->rsum) ICP_HIP(hipMalloc((void**)&h->rsum, kOut * sizeof(double)));
  if (!h->rhsum) ICP_HIP(hipHostMalloc((void**)&h->rhsum, kOut * sizeof(double), hipHostMallocDefault));
  if (plane && !h->pslab) ICP_HIP(hipMalloc((void**)&h->pslab, size_t(kMaxBlocks) * kPlanePitch * sizeof(double)));
  const int nb = blocks_for(h->n_q);
  ICP_HIP(hipMemsetAsync(h->rhist, 0, kDigits * kBins * sizeof(uint32_t), h->st));
  ICP_HIP(hipMemsetAsync(h->rst, 0, sizeof(SelState), h->st));
  SearchArgs S;
  S.T = T; S.g = h->g; S.src = src; S.nrm = h->nrm; S.n = un; S.d2max = h->d2max; S.slot = h->rslot; S.key = h->rkey;
  if (plane) hipLaunchKernelGGL(k_search<true>, dim3(nb), dim3(kBlock), 0, h->st, S);
  else hipLaunchKernelGGL(k_search<false>, dim3(nb), dim3(kBlock), 0, h->st, S);
  ICP_HIP(hipGetLastError());
  if (h->rej_on) if (int32_t rc = launch_reject(h, T, src, nullptr)) return rc;
  const int passes = C.mode == kSelNone ? 1 : kDigits;         // without a selection, pass 0 still counts M
  for (int p = 0; p < passes; ++p) {
    hipLaunchKernelGGL(k_key_hist, dim3(nb), dim3(kBlock), 0, h->st, (const uint32_t*)h->rkey, un, p, (const SelState*)h->rst,
                       h->rhist + p * kBins);
    ICP_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_key_digit, dim3(1), dim3(kBlock), 0, h->st, (const uint32_t*)(h->rhist + p * kBins), p, p == passes - 1, C.mode,
                       C.kq, C.scale, C.c, C.smin, h->rst);
    ICP_HIP(hipGetLastError());
  }
  WsumArgs W;
  W.T = T; W.g = h->g; W.src = src; W.nrm = h->nrm; W.n = un; W.slot = h->rslot; W.st = h->rst; W.loss = C.loss;
  W.slab = plane ? h->pslab : h->slab;
  const int ns = plane ? S4P_ICP_PLANE_NSUMS : S4P_ICP_NSUMS;
  if (plane) {
    hipLaunchKernelGGL(k_wsum<true>, dim3(nb), dim3(kBlock), 0, h->st, W);
    ICP_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_wfinal<true>, dim3(1), dim3(kBlock), 0, h->st, (const double*)h->pslab, nb, (const SelState*)h->rst, h->rsum);
  } else {
    hipLaunchKernelGGL(k_wsum<false>, dim3(nb), dim3(kBlock), 0, h->st, W);
    ICP_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_wfinal<false>, dim3(1), dim3(kBlock), 0, h->st, (const double*)h->slab, nb, (const SelState*)h->rst, h->rsum);
  }
  ICP_HIP(hipGetLastError());
  ICP_HIP(hipMemcpyAsync(h->rhsum, h->rsum, (ns + 5) * sizeof(double), hipMemcpyDeviceToHost, h->st));
  ICP_HIP(hipEventRecord(h->ev, h->st));
  ICP_HIP(hipEventSynchronize(h->ev));
  std::memcpy(sums, h->rhsum, ns * sizeof(double));
  for (int k = 0; k < S4P_ICP_ROBUST_NINFO; ++k) info[k] = k < 5 ? h->rhsum[ns + k] : 0.0;
  info[5] = sums[0];
  if (h->rej_on) reject_done(h);
  return S4P_ICP_OK;
}

// The plain point / plane sums under rejection: search, k_reject, and the weighted sums with every weight 1
// (s4p_icp_sums' / s4p_icp_plane_sums' bits on the surviving pairs, as include/s4p_icp_robust.h states).
int32_t ones_pass(s4p_icp_ctx* h, const Tf& T, const float4* src, bool plane, double* sums) {
  RobustCfg C;
  C.loss = kLossOnes;
  double info[S4P_ICP_ROBUST_NINFO];
  return robust_pass(h, T, src, plane, C, sums, info);
}

// one correspondence pass over `src` for T: the 17 sums (and, if idx, the per-point answers) on the host
int32_t pass(s4p_icp_ctx* h, const Tf& T, const float4* src, int32_t* idx_dev, float* d2_dev, double* out) {
  MatchArgs A;
  A.T = T; A.g = h->g; A.src = src; A.n = uint64_t(h->n_q); A.d2max = h->d2max; A.idx = idx_dev; A.d2 = d2_dev; A.slab = h->slab;
  const int nb = blocks_for(h->n_q);
  if (idx_dev) hipLaunchKernelGGL(k_match<true>, dim3(nb), dim3(kBlock), 0, h->st, A);
  else hipLaunchKernelGGL(k_match<false>, dim3(nb), dim3(kBlock), 0, h->st, A);
  ICP_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_final, dim3(1), dim3(kBlock), 0, h->st, (const double*)h->slab, nb, h->dsum);
  ICP_HIP(hipGetLastError());
  ICP_HIP(hipMemcpyAsync(h->hsum, h->dsum, S4P_ICP_NSUMS * sizeof(double), hipMemcpyDeviceToHost, h->st));
  ICP_HIP(hipEventRecord(h->ev, h->st));
  ICP_HIP(hipEventSynchronize(h->ev));
  std::memcpy(out, h->hsum, S4P_ICP_NSUMS * sizeof(double));
  return S4P_ICP_OK;
}

// one point-to-plane pass over `src` for T: the 31 sums on the host
int32_t plane_pass(s4p_icp_ctx* h, const Tf& T, const float4* src, double* out) {
  if (!h->pslab) ICP_HIP(hipMalloc((void**)&h->pslab, size_t(kMaxBlocks) * kPlanePitch * sizeof(double)));
  PlaneArgs A;
  A.T = T; A.g = h->g; A.src = src; A.nrm = h->nrm; A.n = uint64_t(h->n_q); A.d2max = h->d2max; A.slab = h->pslab;
  const int nb = blocks_for(h->n_q);
  hipLaunchKernelGGL(k_match_plane, dim3(nb), dim3(kBlock), 0, h->st, A);
  ICP_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_final_plane, dim3(1), dim3(kBlock), 0, h->st, (const double*)h->pslab, nb, h->dsum);
  ICP_HIP(hipGetLastError());
  ICP_HIP(hipMemcpyAsync(h->hsum, h->dsum, S4P_ICP_PLANE_NSUMS * sizeof(double), hipMemcpyDeviceToHost, h->st));
  ICP_HIP(hipEventRecord(h->ev, h->st));
  ICP_HIP(hipEventSynchronize(h->ev));
  std::memcpy(out, h->hsum, S4P_ICP_PLANE_NSUMS * sizeof(double));
  return S4P_ICP_OK;
}

int32_t plane_ready(s4p_icp_ctx* h) {
  if (int32_t rc = ready(h)) return rc;
  if (!h->has_normals) return fail(h, S4P_ICP_ERR_STATE, "target normals first (set_target_normals or estimate_normals)");
  return S4P_ICP_OK;
}

int32_t alloc_normals(s4p_icp_ctx* h) {
  h->has_normals = false;
  h->has_grad = false;                           // the gradients lie in the tangent planes of the normals they were made with
  if (!h->nrm) ICP_HIP(hipMalloc((void**)&h->nrm, size_t(h->n_p) * sizeof(float4)));
  return S4P_ICP_OK;
}

// normalised in double, rounded to float; zero or non-finite -> (0, 0, 0)
void normalise_host(const float* nx, const float* ny, const float* nz, size_t n, std::vector<float> (&v)[3]) {
  for (int a = 0; a < 3; ++a) v[a].assign(n, 0.f);
  for (size_t i = 0; i < n; ++i) {
    const double x = nx[i], y = ny[i], z = nz[i];
    const double len = std::sqrt(x * x + y * y + z * z);
    if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z) || !(len > 0.0) || !std::isfinite(len)) continue;
    v[0][i] = float(x / len); v[1][i] = float(y / len); v[2][i] = float(z / len);
  }
}

// caller normals in the uploaded order (host)
int32_t set_normals_host(s4p_icp_ctx* h, const float* nx, const float* ny, const float* nz) {
  const size_t n = size_t(h->n_p);
  std::vector<float> v[3];
  normalise_host(nx, ny, nz, n, v);
  if (int32_t rc = alloc_normals(h)) return rc;
  Scratch S;
  float* d[3];
  for (int a = 0; a < 3; ++a) {
    ICP_HIP(S.alloc((void**)&d[a], n * sizeof(float)));
    ICP_HIP(hipMemcpyAsync(d[a], v[a].data(), n * sizeof(float), hipMemcpyHostToDevice, h->st));
  }
  hipLaunchKernelGGL(k_gather_normals, dim3(blocks_for(h->n_p)), dim3(kBlock), 0, h->st, d[0], d[1], d[2], (const float4*)h->tgt,
                     uint64_t(n), h->nrm);
  ICP_HIP(hipGetLastError());
  ICP_HIP(hipStreamSynchronize(h->st));
  h->has_normals = true;
  return S4P_ICP_OK;
}

// source normals in the uploaded order (host): stored on the device as they are read back
int32_t set_source_normals_host(s4p_icp_ctx* h, const float* nx, const float* ny, const float* nz) {
  const size_t n = size_t(h->n_q);
  std::vector<float> v[3];
  normalise_host(nx, ny, nz, n, v);
  h->has_src_normals = false;
  if (h->sn_n != h->n_q) {
    for (int a = 0; a < 3; ++a) { dfree(h->sn[a]); h->sn[a] = nullptr; }
    dfree(h->snrm); h->snrm = nullptr;
    h->sn_n = 0;
    for (int a = 0; a < 3; ++a) ICP_HIP(hipMalloc((void**)&h->sn[a], n * sizeof(float)));
    ICP_HIP(hipMalloc((void**)&h->snrm, n * sizeof(float4)));
    h->sn_n = h->n_q;
  }
  for (int a = 0; a < 3; ++a) ICP_HIP(hipMemcpyAsync(h->sn[a], v[a].data(), n * sizeof(float), hipMemcpyHostToDevice, h->st));
  ICP_HIP(hipStreamSynchronize(h->st));          // v is released on return
  h->has_src_normals = true;
  return S4P_ICP_OK;
}

int32_t gicp_ready(s4p_icp_ctx* h, double epsilon) {
  if (!(epsilon >= S4P_ICP_GICP_EPSILON_MIN && epsilon <= S4P_ICP_GICP_EPSILON_MAX))
    return fail(h, S4P_ICP_ERR_BAD_ARG, "gicp: epsilon must be in [1e-6, 1]");
  if (int32_t rc = plane_ready(h)) return rc;
  if (!h->has_src_normals) return fail(h, S4P_ICP_ERR_STATE, "source normals first (set_source_normals)");
  return S4P_ICP_OK;
}

// the buffers of a split pass (k_search's slots and keys, the plane slab): none is allocated inside the iteration loop
int32_t split_buffers(s4p_icp_ctx* h) {
  const uint64_t un = uint64_t(h->n_q);
  if (h->r_n != h->n_q) {
    dfree(h->rslot); dfree(h->rkey); h->rslot = h->rkey = nullptr;
    h->r_n = 0;
    ICP_HIP(hipMalloc((void**)&h->rslot, un * sizeof(uint32_t)));
    ICP_HIP(hipMalloc((void**)&h->rkey, un * sizeof(uint32_t)));
    h->r_n = h->n_q;
  }
  if (!h->pslab) ICP_HIP(hipMalloc((void**)&h->pslab, size_t(kMaxBlocks) * kPlanePitch * sizeof(double)));
  return S4P_ICP_OK;
}

// Before the passes of a stage call or a refine over `src` with the rejection on (always: s4p_icp_rejection): the split
// buffers, the counters, the source grid (reciprocity) and the source normals in src's order (normal test, gicp_prepare's
// gather).  Nothing of a rejection is built or allocated inside the iteration loop.
int32_t reject_prepare(s4p_icp_ctx* h, const float4* src, bool always = false) {
  if (!h->rej_on && !always) return S4P_ICP_OK;
  const bool nm = h->rej.normal_mode != S4P_ICP_REJECT_NORMALS_OFF;
  if (nm && !h->has_normals) return fail(h, S4P_ICP_ERR_STATE, "rejection by normals: target normals first (set_target_normals or estimate_normals)");
  if (nm && !h->has_src_normals) return fail(h, S4P_ICP_ERR_STATE, "rejection by normals: source normals first (set_source_normals)");
  if (int32_t rc = split_buffers(h)) return rc;
  if (!h->rcnt) ICP_HIP(hipMalloc((void**)&h->rcnt, 4 * sizeof(unsigned long long)));
  if (!h->rhcnt) ICP_HIP(hipHostMalloc((void**)&h->rhcnt, 4 * sizeof(unsigned long long), hipHostMallocDefault));
  if (h->rej.reciprocal) if (int32_t rc = source_grid_ready(h)) return rc;
  if (nm) {
    hipLaunchKernelGGL(k_gather_source_normals, dim3(blocks_for(h->n_q)), dim3(kBlock), 0, h->st, (const float*)h->sn[0],
                       (const float*)h->sn[1], (const float*)h->sn[2], src, uint64_t(h->n_q), h->snrm);
    ICP_HIP(hipGetLastError());
  }
  return S4P_ICP_OK;
}

// the buffers of a generalized pass and the source normals in src's order
int32_t gicp_prepare(s4p_icp_ctx* h, const float4* src) {
  if (int32_t rc = split_buffers(h)) return rc;
  const uint64_t un = uint64_t(h->n_q);
  hipLaunchKernelGGL(k_gather_source_normals, dim3(blocks_for(h->n_q)), dim3(kBlock), 0, h->st, (const float*)h->sn[0],
                     (const float*)h->sn[1], (const float*)h->sn[2], src, un, h->snrm);
  ICP_HIP(hipGetLastError());
  return S4P_ICP_OK;
}

// one generalized pass over `src` for T (after gicp_prepare for this src): the 31 sums on the host
int32_t gicp_pass(s4p_icp_ctx* h, const Tf& T, const float4* src, double epsilon, double* out) {
  const int nb = blocks_for(h->n_q);
  SearchArgs S;
  S.T = T; S.g = h->g; S.src = src; S.nrm = h->nrm; S.n = uint64_t(h->n_q); S.d2max = h->d2max; S.slot = h->rslot; S.key = h->rkey;
  hipLaunchKernelGGL(k_search<false>, dim3(nb), dim3(kBlock), 0, h->st, S);
  ICP_HIP(hipGetLastError());
  if (h->rej_on) if (int32_t rc = launch_reject(h, T, src, nullptr)) return rc;
  GicpArgs A;
  A.T = T; A.g = h->g; A.src = src; A.snrm = h->snrm; A.nrm = h->nrm; A.n = uint64_t(h->n_q); A.slot = h->rslot;
  A.k = 1.0 - epsilon; A.slab = h->pslab;
  hipLaunchKernelGGL(k_gicp_sum, dim3(nb), dim3(kBlock), 0, h->st, A);
  ICP_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_final_plane, dim3(1), dim3(kBlock), 0, h->st, (const double*)h->pslab, nb, h->dsum);
  ICP_HIP(hipGetLastError());
  ICP_HIP(hipMemcpyAsync(h->hsum, h->dsum, S4P_ICP_GICP_NSUMS * sizeof(double), hipMemcpyDeviceToHost, h->st));
  ICP_HIP(hipEventRecord(h->ev, h->st));
  ICP_HIP(hipEventSynchronize(h->ev));
  std::memcpy(out, h->hsum, S4P_ICP_GICP_NSUMS * sizeof(double));
  if (h->rej_on) reject_done(h);
  return S4P_ICP_OK;
}

// intensities: every value finite
int32_t check_intensity(s4p_icp_ctx* h, const float* v, size_t n, const char* who) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return fail(h, S4P_ICP_ERR_BAD_ARG, std::string(who) + ": non-finite intensity");
  return S4P_ICP_OK;
}

// target intensities in the uploaded order (host) -> cell order
int32_t set_target_intensity_host(s4p_icp_ctx* h, const float* v) {
  const size_t n = size_t(h->n_p);
  if (int32_t rc = check_intensity(h, v, n, "set_target_intensity")) return rc;
  h->has_tint = h->has_grad = false;
  if (!h->tint) ICP_HIP(hipMalloc((void**)&h->tint, n * sizeof(float)));
  Scratch S;
  float* d = nullptr;
  ICP_HIP(S.alloc((void**)&d, n * sizeof(float)));
  ICP_HIP(hipMemcpyAsync(d, v, n * sizeof(float), hipMemcpyHostToDevice, h->st));
  hipLaunchKernelGGL(k_gather_target_intensity, dim3(blocks_for(h->n_p)), dim3(kBlock), 0, h->st, (const float*)d, (const float4*)h->tgt,
                     uint64_t(n), h->tint);
  ICP_HIP(hipGetLastError());
  ICP_HIP(hipStreamSynchronize(h->st));          // v may be released on return; the scratch is
  h->has_tint = true;
  return S4P_ICP_OK;
}

// source intensities in the uploaded order (host): kept on the device in that order
int32_t set_source_intensity_host(s4p_icp_ctx* h, const float* v) {
  const size_t n = size_t(h->n_q);
  if (int32_t rc = check_intensity(h, v, n, "set_source_intensity")) return rc;
  h->has_sint = false;
  if (h->si_n != h->n_q) {
    dfree(h->si); dfree(h->sint); h->si = h->sint = nullptr;
    h->si_n = 0;
    ICP_HIP(hipMalloc((void**)&h->si, n * sizeof(float)));
    ICP_HIP(hipMalloc((void**)&h->sint, n * sizeof(float)));
    h->si_n = h->n_q;
  }
  ICP_HIP(hipMemcpyAsync(h->si, v, n * sizeof(float), hipMemcpyHostToDevice, h->st));
  ICP_HIP(hipStreamSynchronize(h->st));          // v may be released on return
  h->has_sint = true;
  return S4P_ICP_OK;
}

int32_t color_ready(s4p_icp_ctx* h, double lambda) {
  if (!(lambda >= 0.0 && lambda <= 1.0)) return fail(h, S4P_ICP_ERR_BAD_ARG, "color: lambda must be in [0, 1]");
  if (int32_t rc = plane_ready(h)) return rc;
  if (!h->has_tint) return fail(h, S4P_ICP_ERR_STATE, "target intensity first (set_target_intensity)");
  if (!h->has_grad) return fail(h, S4P_ICP_ERR_STATE, "colour gradients first (estimate_color_gradients)");
  if (!h->has_sint) return fail(h, S4P_ICP_ERR_STATE, "source intensity first (set_source_intensity)");
  return S4P_ICP_OK;
}

// the buffers of a colour pass and the source intensities in src's order
int32_t color_prepare(s4p_icp_ctx* h, const float4* src) {
  if (int32_t rc = split_buffers(h)) return rc;
  const uint64_t un = uint64_t(h->n_q);
  hipLaunchKernelGGL(k_gather_source_intensity, dim3(blocks_for(h->n_q)), dim3(kBlock), 0, h->st, (const float*)h->si, src, un, h->sint);
  ICP_HIP(hipGetLastError());
  return S4P_ICP_OK;
}

// one colour pass over `src` for T (after color_prepare for this src): the 31 sums on the host
int32_t color_pass(s4p_icp_ctx* h, const Tf& T, const float4* src, double lambda, double* out) {
  const int nb = blocks_for(h->n_q);
  SearchArgs S;
  S.T = T; S.g = h->g; S.src = src; S.nrm = h->nrm; S.n = uint64_t(h->n_q); S.d2max = h->d2max; S.slot = h->rslot; S.key = h->rkey;
  hipLaunchKernelGGL(k_search<false>, dim3(nb), dim3(kBlock), 0, h->st, S);
  ICP_HIP(hipGetLastError());
  if (h->rej_on) if (int32_t rc = launch_reject(h, T, src, nullptr)) return rc;
  ColorArgs A;
  A.T = T; A.g = h->g; A.src = src; A.sint = h->sint; A.nrm = h->nrm; A.grad = h->grad; A.n = uint64_t(h->n_q); A.slot = h->rslot;
  A.wg = lambda; A.wc = 1.0 - lambda; A.slab = h->pslab;
  hipLaunchKernelGGL(k_color_sum, dim3(nb), dim3(kBlock), 0, h->st, A);
  ICP_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_final_plane, dim3(1), dim3(kBlock), 0, h->st, (const double*)h->pslab, nb, h->dsum);
  ICP_HIP(hipGetLastError());
  ICP_HIP(hipMemcpyAsync(h->hsum, h->dsum, S4P_ICP_COLOR_NSUMS * sizeof(double), hipMemcpyDeviceToHost, h->st));
  ICP_HIP(hipEventRecord(h->ev, h->st));
  ICP_HIP(hipEventSynchronize(h->ev));
  std::memcpy(out, h->hsum, S4P_ICP_COLOR_NSUMS * sizeof(double));
  if (h->rej_on) reject_done(h);
  return S4P_ICP_OK;
}

// refine's source: as uploaded, or (order_source) in the cell order of its T0-image, so that a wave's lanes read
// neighbouring cells
int32_t source_for(s4p_icp_ctx* h, const s4p_icp_params& P, const double* T, const float4** src) {
  *src = h->src;
  if (!P.order_source) return S4P_ICP_OK;
  Scratch S;
  const uint64_t un = uint64_t(h->n_q);
  uint32_t *keys, *vals, *keys2, *vals2;
  ICP_HIP(S.alloc((void**)&keys, un * 4)); ICP_HIP(S.alloc((void**)&vals, un * 4));
  ICP_HIP(S.alloc((void**)&keys2, un * 4)); ICP_HIP(S.alloc((void**)&vals2, un * 4));
  const int nb = blocks_for(h->n_q);
  hipLaunchKernelGGL(k_source_keys, dim3(nb), dim3(kBlock), 0, h->st, (const float4*)h->src, un, to_float(T), h->g, keys, vals);
  ICP_HIP(hipGetLastError());
  if (int32_t rc = sort_pairs(h, S, keys, keys2, vals, vals2, un, h->ncell)) return rc;
  hipLaunchKernelGGL(k_gather_source, dim3(nb), dim3(kBlock), 0, h->st, (const float4*)h->src, (const uint32_t*)vals2, un, h->src_ord);
  ICP_HIP(hipGetLastError());
  ICP_HIP(hipStreamSynchronize(h->st));
  *src = h->src_ord;
  return S4P_ICP_OK;
}

Tf centred_from_float16(const float* T16) {
  Tf f;
  for (int k = 0; k < 12; ++k) f.m[k] = T16[k];
  return f;
}

}  // namespace

namespace {

enum RefineMetric { kRefinePoint = 0, kRefinePlane = 1, kRefineGicp = 2, kRefineColor = 3 };

// The refine loop of the four metrics (epsilon: the generalized metric's, or the coloured metric's lambda).  plane /
// generalized / coloured: the 31 sums (sum d2 at [1]) and s4p_icp_solve_plane, whose
// degenerate system stops the loop with T_k; otherwise the 17 sums (sum d2 at [16]) and Horn's solve.
int32_t refine_impl(s4p_icp_ctx* h, const s4p_icp_params* params, double* T16_inout, s4p_icp_result* result, int metric,
                    double epsilon = 0.0) {
  const bool gicp = metric == kRefineGicp, color = metric == kRefineColor, plane = metric != kRefinePoint;
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!T16_inout) return fail(h, S4P_ICP_ERR_BAD_ARG, "refine: null transform");
  s4p_icp_params P;
  s4p_icp_default_params(&P);
  if (params) P = *params;
  if (P.max_iterations < 0 || P.min_correspondences < 0 || !(P.rel_tol >= 0.0))
    return fail(h, S4P_ICP_ERR_BAD_ARG, "refine: negative max_iterations / min_correspondences / rel_tol");
  if (int32_t rc = gicp ? gicp_ready(h, epsilon) : (color ? color_ready(h, epsilon) : (plane ? plane_ready(h) : ready(h)))) return rc;
  s4p_icp_result R;
  std::memset(&R, 0, sizeof(R));
  double T[16], Tn[16], dT[16], sums[kSumsCap];
  const int i_d2 = plane ? 1 : 16;
  auto run_pass = [&](const float4* src) {
    if (gicp) return gicp_pass(h, to_float(T), src, epsilon, sums);
    if (color) return color_pass(h, to_float(T), src, epsilon, sums);
    if (h->rej_on) return ones_pass(h, to_float(T), src, plane, sums);       // off: the fused k_match / k_match_plane, untouched
    return plane ? plane_pass(h, to_float(T), src, sums) : pass(h, to_float(T), src, nullptr, nullptr, sums);
  };
  to_centred(T16_inout, h->c, T);
  const float4* src = nullptr;
  if (int32_t rc = source_for(h, P, T, &src)) return rc;
  if (gicp) if (int32_t rc = gicp_prepare(h, src)) return rc;      // the normals follow the source's order
  if (color) if (int32_t rc = color_prepare(h, src)) return rc;    // and so do the intensities
  if (int32_t rc = reject_prepare(h, src)) return rc;
  double prev = 0.0;
  R.status = S4P_ICP_MAX_ITERATIONS;
  for (int k = 0; k < P.max_iterations; ++k) {
    if (int32_t rc = run_pass(src)) return rc;
    const double n = sums[0];
    const double rmse = n > 0.0 ? std::sqrt(sums[i_d2] / n) : 0.0;
    if (k < S4P_ICP_HISTORY) { R.history_rmse[k] = rmse; R.history_n[k] = int64_t(n); R.history_len = k + 1; }
    if (n < double(std::max(P.min_correspondences, 1))) { R.status = S4P_ICP_TOO_FEW; break; }
    if (plane) {
      if (s4p_icp_solve_plane(sums, dT) != S4P_ICP_OK) { R.status = S4P_ICP_DEGENERATE; break; }
    } else {
      s4p_icp_solve(sums, dT);
    }
    mat_mul4(dT, T, Tn);
    std::memcpy(T, Tn, sizeof(T));
    R.iterations = k + 1;
    if (k + 1 == P.max_iterations) { R.status = S4P_ICP_MAX_ITERATIONS; break; }
    if (k > 0 && std::fabs(rmse - prev) <= P.rel_tol * prev) { R.status = S4P_ICP_CONVERGED; break; }
    prev = rmse;
  }
  // final pass: the statistics of the returned transform
  if (int32_t rc = run_pass(src)) return rc;
  R.n_corr = int64_t(sums[0]);
  R.rmse = sums[0] > 0.0 ? std::sqrt(sums[i_d2] / sums[0]) : 0.0;
  R.fitness = double(R.n_corr) / double(h->n_q);
  from_centred(T, h->c, T16_inout);
  if (result) *result = R;
  return S4P_ICP_OK;
}

// refine_impl's loop on the weighted sums: rmse = sqrt(sum w d2 / sum w), n = the count with w > 0 (info[4])
int32_t refine_robust_impl(s4p_icp_ctx* h, const s4p_icp_params* params, int32_t metric, const s4p_icp_robust* robust, double* T16_inout,
                           s4p_icp_result* result, double* info_out) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!T16_inout) return fail(h, S4P_ICP_ERR_BAD_ARG, "refine_robust: null transform");
  s4p_icp_params P;
  s4p_icp_default_params(&P);
  if (params) P = *params;
  if (P.max_iterations < 0 || P.min_correspondences < 0 || !(P.rel_tol >= 0.0))
    return fail(h, S4P_ICP_ERR_BAD_ARG, "refine_robust: negative max_iterations / min_correspondences / rel_tol");
  const bool plane = metric == S4P_ICP_METRIC_PLANE;
  if (int32_t rc = plane ? plane_ready(h) : ready(h)) return rc;
  RobustCfg C;
  if (int32_t rc = robust_cfg(h, metric, robust, &C)) return rc;
  s4p_icp_result R;
  std::memset(&R, 0, sizeof(R));
  double T[16], Tn[16], dT[16], sums[kSumsCap], info[S4P_ICP_ROBUST_NINFO];
  const int i_d2 = plane ? 1 : 16;
  to_centred(T16_inout, h->c, T);
  const float4* src = nullptr;
  if (int32_t rc = source_for(h, P, T, &src)) return rc;
  if (int32_t rc = reject_prepare(h, src)) return rc;
  double prev = 0.0;
  R.status = S4P_ICP_MAX_ITERATIONS;
  for (int k = 0; k < P.max_iterations; ++k) {
    if (int32_t rc = robust_pass(h, to_float(T), src, plane, C, sums, info)) return rc;
    const double n = info[4], sw = sums[0];
    const double rmse = sw > 0.0 ? std::sqrt(sums[i_d2] / sw) : 0.0;
    if (k < S4P_ICP_HISTORY) { R.history_rmse[k] = rmse; R.history_n[k] = int64_t(n); R.history_len = k + 1; }
    if (n < double(std::max(P.min_correspondences, 1)) || (!plane && !(sw >= 1.0))) { R.status = S4P_ICP_TOO_FEW; break; }
    if (plane) {
      if (s4p_icp_solve_plane(sums, dT) != S4P_ICP_OK) { R.status = S4P_ICP_DEGENERATE; break; }
    } else {
      s4p_icp_solve(sums, dT);
    }
    mat_mul4(dT, T, Tn);
    std::memcpy(T, Tn, sizeof(T));
    R.iterations = k + 1;
    if (k + 1 == P.max_iterations) { R.status = S4P_ICP_MAX_ITERATIONS; break; }
    if (k > 0 && std::fabs(rmse - prev) <= P.rel_tol * prev) { R.status = S4P_ICP_CONVERGED; break; }
    prev = rmse;
  }
  // final pass: the statistics of the returned transform
  if (int32_t rc = robust_pass(h, to_float(T), src, plane, C, sums, info)) return rc;
  R.n_corr = int64_t(info[4]);
  R.rmse = sums[0] > 0.0 ? std::sqrt(sums[i_d2] / sums[0]) : 0.0;
  R.fitness = double(R.n_corr) / double(h->n_q);
  from_centred(T, h->c, T16_inout);
  if (result) *result = R;
  if (info_out) std::memcpy(info_out, info, sizeof(info));
  return S4P_ICP_OK;
}

}  // namespace

extern "C" {

void s4p_icp_default_params(s4p_icp_params* p) {
  if (!p) return;
  p->max_iterations = 30;
  p->min_correspondences = 3;
  p->rel_tol = 1e-6;
  p->order_source = 1;
  p->reserved = 0;
}

const char* s4p_icp_last_error(const s4p_icp_ctx* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int32_t s4p_icp_create(int32_t device, s4p_icp_ctx** out) {
  if (!out) { g_create_error = "null argument"; return S4P_ICP_ERR_BAD_ARG; }
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    g_create_error = "no HIP device visible: the MI355X path has no CPU fallback";
    return S4P_ICP_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= ndev) { g_create_error = "bad device index"; return S4P_ICP_ERR_BAD_ARG; }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) { g_create_error = "hipGetDeviceProperties failed"; return S4P_ICP_ERR_HIP; }
  if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos) {
    g_create_error = std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only";
    return S4P_ICP_ERR_NO_DEVICE;
  }
  s4p_icp_ctx* h = new s4p_icp_ctx();
  h->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&h->ev, hipEventDisableTiming) != hipSuccess ||
      hipMalloc((void**)&h->dsum, kSumsCap * sizeof(double)) != hipSuccess ||
      hipHostMalloc((void**)&h->hsum, kSumsCap * sizeof(double), hipHostMallocDefault) != hipSuccess) {
    g_create_error = "HIP stream / event / buffer creation failed";
    s4p_icp_destroy(h);
    return S4P_ICP_ERR_HIP;
  }
  *out = h;
  return S4P_ICP_OK;
}

void s4p_icp_destroy(s4p_icp_ctx* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->st) (void)hipStreamSynchronize(h->st);
  dfree(h->tgt); dfree(h->start); dfree(h->src); dfree(h->src_ord); dfree(h->slab); dfree(h->dsum); dfree(h->nrm); dfree(h->pslab);
  for (int a = 0; a < 3; ++a) dfree(h->qraw[a]);
  dfree(h->rslot); dfree(h->rkey); dfree(h->rhist); dfree(h->rst); dfree(h->rsum);
  for (int a = 0; a < 3; ++a) dfree(h->sn[a]);
  dfree(h->snrm);
  dfree(h->tint); dfree(h->grad); dfree(h->si); dfree(h->sint);
  dfree(h->sgrid); dfree(h->sstart); dfree(h->rcnt);
  if (h->rhcnt) (void)hipHostFree(h->rhcnt);
  if (h->rhsum) (void)hipHostFree(h->rhsum);
  if (h->hsum) (void)hipHostFree(h->hsum);
  if (h->ev) (void)hipEventDestroy(h->ev);
  if (h->st) (void)hipStreamDestroy(h->st);
  delete h;
}

int32_t s4p_icp_set_target(s4p_icp_ctx* h, const float* x, const float* y, const float* z, int64_t n, float max_distance) {
  return set_target_impl(h, x, y, z, n, max_distance, hipMemcpyHostToDevice);
}
int32_t s4p_icp_set_target_device(s4p_icp_ctx* h, const float* x, const float* y, const float* z, int64_t n, float max_distance) {
  return set_target_impl(h, x, y, z, n, max_distance, hipMemcpyDeviceToDevice);
}
int32_t s4p_icp_set_source(s4p_icp_ctx* h, const float* x, const float* y, const float* z, int64_t n) {
  return set_source_impl(h, x, y, z, n, hipMemcpyHostToDevice);
}
int32_t s4p_icp_set_source_device(s4p_icp_ctx* h, const float* x, const float* y, const float* z, int64_t n) {
  return set_source_impl(h, x, y, z, n, hipMemcpyDeviceToDevice);
}

int32_t s4p_icp_frame(const s4p_icp_ctx* h, float* c3) {
  if (!h || !c3) return S4P_ICP_ERR_BAD_ARG;
  if (!h->has_target) return S4P_ICP_ERR_STATE;
  for (int a = 0; a < 3; ++a) c3[a] = h->c[a];
  return S4P_ICP_OK;
}

int32_t s4p_icp_correspondences(s4p_icp_ctx* h, const float* T16_centred, int32_t* idx, float* d2) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!T16_centred || !idx || !d2) return fail(h, S4P_ICP_ERR_BAD_ARG, "correspondences: null argument");
  if (int32_t rc = ready(h)) return rc;
  Scratch S;
  int32_t* di;
  float* dd;
  ICP_HIP(S.alloc((void**)&di, size_t(h->n_q) * 4));
  ICP_HIP(S.alloc((void**)&dd, size_t(h->n_q) * 4));
  double sums[S4P_ICP_NSUMS];
  if (int32_t rc = pass(h, centred_from_float16(T16_centred), h->src, di, dd, sums)) return rc;
  ICP_HIP(hipMemcpy(idx, di, size_t(h->n_q) * 4, hipMemcpyDeviceToHost));
  ICP_HIP(hipMemcpy(d2, dd, size_t(h->n_q) * 4, hipMemcpyDeviceToHost));
  return S4P_ICP_OK;
}

int32_t s4p_icp_sums(s4p_icp_ctx* h, const float* T16_centred, double* sums) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!T16_centred || !sums) return fail(h, S4P_ICP_ERR_BAD_ARG, "sums: null argument");
  if (int32_t rc = ready(h)) return rc;
  if (h->rej_on) {
    if (int32_t rc = reject_prepare(h, h->src)) return rc;
    return ones_pass(h, centred_from_float16(T16_centred), h->src, false, sums);
  }
  return pass(h, centred_from_float16(T16_centred), h->src, nullptr, nullptr, sums);
}

int32_t s4p_icp_solve(const double* sums, double* dT16) {
  if (!sums || !dT16) return S4P_ICP_ERR_BAD_ARG;
  const double n = sums[0];
  if (!(n >= 1.0)) return S4P_ICP_ERR_BAD_ARG;
  double mq[3], mp[3], S[3][3];
  for (int a = 0; a < 3; ++a) { mq[a] = sums[1 + a] / n; mp[a] = sums[4 + a] / n; }
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) S[a][b] = sums[7 + 3 * a + b] / n - mq[a] * mp[b];
  const double Sxx = S[0][0], Sxy = S[0][1], Sxz = S[0][2], Syx = S[1][0], Syy = S[1][1], Syz = S[1][2], Szx = S[2][0],
               Szy = S[2][1], Szz = S[2][2];
  double N[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                    {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                    {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                    {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
  double V[4][4];
  jacobi4(N, V);
  int best = 0;
  for (int k = 1; k < 4; ++k) if (N[k][k] > N[best][best]) best = k;
  double w = V[0][best], x = V[1][best], y = V[2][best], z = V[3][best];
  const double nq = std::sqrt(w * w + x * x + y * y + z * z);
  w /= nq; x /= nq; y /= nq; z /= nq;
  const double R[3][3] = {{w * w + x * x - y * y - z * z, 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)},
                          {2.0 * (x * y + w * z), w * w - x * x + y * y - z * z, 2.0 * (y * z - w * x)},
                          {2.0 * (x * z - w * y), 2.0 * (y * z + w * x), w * w - x * x - y * y + z * z}};
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) dT16[4 * r + c] = R[r][c];
    dT16[4 * r + 3] = mp[r] - (R[r][0] * mq[0] + R[r][1] * mq[1] + R[r][2] * mq[2]);
  }
  dT16[12] = dT16[13] = dT16[14] = 0.0;
  dT16[15] = 1.0;
  return S4P_ICP_OK;
}

int32_t s4p_icp_refine(s4p_icp_ctx* h, const s4p_icp_params* params, double* T16_inout, s4p_icp_result* result) {
  return refine_impl(h, params, T16_inout, result, kRefinePoint);
}

int32_t s4p_icp_apply(s4p_icp_ctx* h, const double* T16, float* x, float* y, float* z, int64_t n) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!T16 || !x || !y || !z || n < 0) return fail(h, S4P_ICP_ERR_BAD_ARG, "apply: null argument");
  if (n == 0) return S4P_ICP_OK;
  ICP_HIP(hipSetDevice(h->device));
  Scratch S;
  float* p[3];
  float* io[3] = {x, y, z};
  for (int a = 0; a < 3; ++a) {
    ICP_HIP(S.alloc((void**)&p[a], size_t(n) * sizeof(float)));
    ICP_HIP(hipMemcpyAsync(p[a], io[a], size_t(n) * sizeof(float), hipMemcpyHostToDevice, h->st));
  }
  hipLaunchKernelGGL(k_apply_icp, dim3(blocks_for(n)), dim3(kBlock), 0, h->st, to_float(T16), p[0], p[1], p[2], uint64_t(n));
  ICP_HIP(hipGetLastError());
  for (int a = 0; a < 3; ++a) ICP_HIP(hipMemcpyAsync(io[a], p[a], size_t(n) * sizeof(float), hipMemcpyDeviceToHost, h->st));
  ICP_HIP(hipStreamSynchronize(h->st));
  return S4P_ICP_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// point-to-plane (include/s4p_icp_plane.h)

int32_t s4p_icp_set_target_normals(s4p_icp_ctx* h, const float* nx, const float* ny, const float* nz, int64_t n) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!h->has_target) return fail(h, S4P_ICP_ERR_STATE, "set_target_normals: set_target first");
  if (!nx || !ny || !nz || n != h->n_p) return fail(h, S4P_ICP_ERR_BAD_ARG, "set_target_normals: null or not one per target point");
  ICP_HIP(hipSetDevice(h->device));
  return set_normals_host(h, nx, ny, nz);
}

int32_t s4p_icp_set_target_normals_device(s4p_icp_ctx* h, const float* nx, const float* ny, const float* nz, int64_t n) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!h->has_target) return fail(h, S4P_ICP_ERR_STATE, "set_target_normals: set_target first");
  if (!nx || !ny || !nz || n != h->n_p) return fail(h, S4P_ICP_ERR_BAD_ARG, "set_target_normals: null or not one per target point");
  ICP_HIP(hipSetDevice(h->device));
  // normalised on the host, as for host input: both entry points store the same bits
  std::vector<float> v[3];
  const float* in[3] = {nx, ny, nz};
  for (int a = 0; a < 3; ++a) {
    v[a].resize(size_t(n));
    ICP_HIP(hipMemcpy(v[a].data(), in[a], size_t(n) * sizeof(float), hipMemcpyDeviceToHost));
  }
  return set_normals_host(h, v[0].data(), v[1].data(), v[2].data());
}

int32_t s4p_icp_estimate_normals(s4p_icp_ctx* h, float radius, int32_t min_neighbours) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!h->has_target) return fail(h, S4P_ICP_ERR_STATE, "estimate_normals: set_target first");
  if (!(radius > 0.f) || !(radius <= h->d))
    return fail(h, S4P_ICP_ERR_BAD_ARG, "estimate_normals: radius must be in (0, max_distance]");
  if (min_neighbours < 3) return fail(h, S4P_ICP_ERR_BAD_ARG, "estimate_normals: min_neighbours must be >= 3");
  ICP_HIP(hipSetDevice(h->device));
  if (int32_t rc = alloc_normals(h)) return rc;
  hipLaunchKernelGGL(k_normals, dim3(blocks_for(h->n_p)), dim3(kBlock), 0, h->st, h->g, uint64_t(h->n_p), radius * radius, min_neighbours,
                     h->nrm);
  ICP_HIP(hipGetLastError());
  ICP_HIP(hipStreamSynchronize(h->st));
  h->has_normals = true;
  return S4P_ICP_OK;
}

int32_t s4p_icp_target_normals(s4p_icp_ctx* h, float* nx, float* ny, float* nz) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!nx || !ny || !nz) return fail(h, S4P_ICP_ERR_BAD_ARG, "target_normals: null argument");
  if (!h->has_target || !h->has_normals) return fail(h, S4P_ICP_ERR_STATE, "target_normals: no normals");
  ICP_HIP(hipSetDevice(h->device));
  Scratch S;
  const size_t n = size_t(h->n_p);
  float* d[3];
  for (int a = 0; a < 3; ++a) ICP_HIP(S.alloc((void**)&d[a], n * sizeof(float)));
  hipLaunchKernelGGL(k_scatter_normals, dim3(blocks_for(h->n_p)), dim3(kBlock), 0, h->st, (const float4*)h->nrm, (const float4*)h->tgt,
                     uint64_t(n), d[0], d[1], d[2]);
  ICP_HIP(hipGetLastError());
  float* out[3] = {nx, ny, nz};
  for (int a = 0; a < 3; ++a) ICP_HIP(hipMemcpyAsync(out[a], d[a], n * sizeof(float), hipMemcpyDeviceToHost, h->st));
  ICP_HIP(hipStreamSynchronize(h->st));
  return S4P_ICP_OK;
}

int32_t s4p_icp_plane_sums(s4p_icp_ctx* h, const float* T16_centred, double* sums) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!T16_centred || !sums) return fail(h, S4P_ICP_ERR_BAD_ARG, "plane_sums: null argument");
  if (int32_t rc = plane_ready(h)) return rc;
  if (h->rej_on) {
    if (int32_t rc = reject_prepare(h, h->src)) return rc;
    return ones_pass(h, centred_from_float16(T16_centred), h->src, true, sums);
  }
  return plane_pass(h, centred_from_float16(T16_centred), h->src, sums);
}

int32_t s4p_icp_solve_plane(const double* sums, double* dT16) {
  if (!sums || !dT16) return S4P_ICP_ERR_BAD_ARG;
  if (!(sums[2] >= 6.0)) return S4P_ICP_ERR_DEGENERATE;
  double A[6][6], b[6];
  for (int u = 0, o = 4; u < 6; ++u)
    for (int v = u; v < 6; ++v, ++o) A[u][v] = A[v][u] = sums[o];
  for (int u = 0; u < 6; ++u) b[u] = sums[25 + u];
  // balance the rotation block (length^2) against the translation block (unitless): the test below is unit-free
  const double tw = A[0][0] + A[1][1] + A[2][2], tt = A[3][3] + A[4][4] + A[5][5];
  if (!(tw > 0.0) || !(tt > 0.0) || !std::isfinite(tw) || !std::isfinite(tt)) return S4P_ICP_ERR_DEGENERATE;
  const double sc = std::sqrt(tt / tw);
  const double D[6] = {sc, sc, sc, 1.0, 1.0, 1.0};
  double B[6][6], E[6][6], V[6][6], bb[6];
  for (int u = 0; u < 6; ++u) {
    bb[u] = D[u] * b[u];
    for (int v = 0; v < 6; ++v) B[u][v] = E[u][v] = D[u] * A[u][v] * D[v];
  }
  jacobi_sym<6>(E, V);
  double lmin = E[0][0], lmax = E[0][0];
  for (int u = 1; u < 6; ++u) { lmin = std::min(lmin, E[u][u]); lmax = std::max(lmax, E[u][u]); }
  if (!(lmin > 1e-10 * lmax)) return S4P_ICP_ERR_DEGENERATE;
  // Cholesky B = L L^T, then B y = D b, x = D y
  double L[6][6] = {};
  for (int u = 0; u < 6; ++u)
    for (int v = 0; v <= u; ++v) {
      double acc = B[u][v];
      for (int k = 0; k < v; ++k) acc -= L[u][k] * L[v][k];
      if (u == v) {
        if (!(acc > 0.0)) return S4P_ICP_ERR_DEGENERATE;
        L[u][u] = std::sqrt(acc);
      } else {
        L[u][v] = acc / L[v][v];
      }
    }
  double y[6], x[6];
  for (int u = 0; u < 6; ++u) {
    double acc = bb[u];
    for (int k = 0; k < u; ++k) acc -= L[u][k] * y[k];
    y[u] = acc / L[u][u];
  }
  for (int u = 5; u >= 0; --u) {
    double acc = y[u];
    for (int k = u + 1; k < 6; ++k) acc -= L[k][u] * x[k];
    x[u] = acc / L[u][u];
  }
  for (int u = 0; u < 6; ++u) x[u] *= D[u];
  // exact rotation of omega (Rodrigues): R = I + sin(th)/th K + (1 - cos(th))/th^2 K^2, K = [omega]x, K^2 = w w^T - th^2 I
  const double w[3] = {x[0], x[1], x[2]};
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = std::sqrt(th2);
  const double c1 = th > 0.0 ? std::sin(th) / th : 1.0;
  const double sh = th > 0.0 ? std::sin(0.5 * th) / th : 0.5;
  const double c2 = 2.0 * sh * sh;                                  // (1 - cos th) / th^2 without cancellation
  const double K[3][3] = {{0.0, -w[2], w[1]}, {w[2], 0.0, -w[0]}, {-w[1], w[0], 0.0}};
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) dT16[4 * r + c] = (r == c ? 1.0 : 0.0) + c1 * K[r][c] + c2 * (w[r] * w[c] - (r == c ? th2 : 0.0));
    dT16[4 * r + 3] = x[3 + r];
  }
  dT16[12] = dT16[13] = dT16[14] = 0.0;
  dT16[15] = 1.0;
  return S4P_ICP_OK;
}

int32_t s4p_icp_refine_plane(s4p_icp_ctx* h, const s4p_icp_params* params, double* T16_inout, s4p_icp_result* result) {
  return refine_impl(h, params, T16_inout, result, kRefinePlane);
}

// ---------------------------------------------------------------------------------------------------------------------
// robust ICP (include/s4p_icp_robust.h)

void s4p_icp_robust_defaults(s4p_icp_robust* r, int32_t loss) {
  if (!r) return;
  std::memset(r, 0, sizeof(*r));
  r->loss = loss;
  r->trim_fraction = 1.0;
  r->scale = 0.0;
  r->c = loss == S4P_ICP_LOSS_HUBER ? S4P_ICP_HUBER_C : (loss == S4P_ICP_LOSS_TUKEY ? S4P_ICP_TUKEY_C : 0.0);
}

int32_t s4p_icp_robust_sums(s4p_icp_ctx* h, const float* T16_centred, int32_t metric, const s4p_icp_robust* robust, double* sums,
                            double* info) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!T16_centred || !sums) return fail(h, S4P_ICP_ERR_BAD_ARG, "robust_sums: null argument");
  const bool plane = metric == S4P_ICP_METRIC_PLANE;
  if (int32_t rc = plane ? plane_ready(h) : ready(h)) return rc;
  RobustCfg C;
  if (int32_t rc = robust_cfg(h, metric, robust, &C)) return rc;
  double inf[S4P_ICP_ROBUST_NINFO];
  if (int32_t rc = reject_prepare(h, h->src)) return rc;
  if (int32_t rc = robust_pass(h, centred_from_float16(T16_centred), h->src, plane, C, sums, inf)) return rc;
  if (info) std::memcpy(info, inf, sizeof(inf));
  return S4P_ICP_OK;
}

int32_t s4p_icp_refine_robust(s4p_icp_ctx* h, const s4p_icp_params* params, int32_t metric, const s4p_icp_robust* robust,
                              double* T16_inout, s4p_icp_result* result, double* info_out) {
  return refine_robust_impl(h, params, metric, robust, T16_inout, result, info_out);
}

// ---------------------------------------------------------------------------------------------------------------------
// generalized ICP (include/s4p_icp_gicp.h)

int32_t s4p_icp_set_source_normals(s4p_icp_ctx* h, const float* nx, const float* ny, const float* nz, int64_t n) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!h->has_source) return fail(h, S4P_ICP_ERR_STATE, "set_source_normals: set_source first");
  if (!nx || !ny || !nz || n != h->n_q) return fail(h, S4P_ICP_ERR_BAD_ARG, "set_source_normals: null or not one per source point");
  ICP_HIP(hipSetDevice(h->device));
  return set_source_normals_host(h, nx, ny, nz);
}

int32_t s4p_icp_set_source_normals_device(s4p_icp_ctx* h, const float* nx, const float* ny, const float* nz, int64_t n) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!h->has_source) return fail(h, S4P_ICP_ERR_STATE, "set_source_normals: set_source first");
  if (!nx || !ny || !nz || n != h->n_q) return fail(h, S4P_ICP_ERR_BAD_ARG, "set_source_normals: null or not one per source point");
  ICP_HIP(hipSetDevice(h->device));
  // normalised on the host, as for host input: both entry points store the same bits
  std::vector<float> v[3];
  const float* in[3] = {nx, ny, nz};
  for (int a = 0; a < 3; ++a) {
    v[a].resize(size_t(n));
    ICP_HIP(hipMemcpy(v[a].data(), in[a], size_t(n) * sizeof(float), hipMemcpyDeviceToHost));
  }
  return set_source_normals_host(h, v[0].data(), v[1].data(), v[2].data());
}

int32_t s4p_icp_source_normals(s4p_icp_ctx* h, float* nx, float* ny, float* nz) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!nx || !ny || !nz) return fail(h, S4P_ICP_ERR_BAD_ARG, "source_normals: null argument");
  if (!h->has_source || !h->has_src_normals) return fail(h, S4P_ICP_ERR_STATE, "source_normals: no normals");
  ICP_HIP(hipSetDevice(h->device));
  float* out[3] = {nx, ny, nz};
  for (int a = 0; a < 3; ++a) ICP_HIP(hipMemcpyAsync(out[a], h->sn[a], size_t(h->n_q) * sizeof(float), hipMemcpyDeviceToHost, h->st));
  ICP_HIP(hipStreamSynchronize(h->st));
  return S4P_ICP_OK;
}

int32_t s4p_icp_gicp_sums(s4p_icp_ctx* h, const float* T16_centred, double epsilon, double* sums) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!T16_centred || !sums) return fail(h, S4P_ICP_ERR_BAD_ARG, "gicp_sums: null argument");
  if (int32_t rc = gicp_ready(h, epsilon)) return rc;
  if (int32_t rc = gicp_prepare(h, h->src)) return rc;
  if (int32_t rc = reject_prepare(h, h->src)) return rc;
  return gicp_pass(h, centred_from_float16(T16_centred), h->src, epsilon, sums);
}

int32_t s4p_icp_refine_gicp(s4p_icp_ctx* h, const s4p_icp_params* params, double epsilon, double* T16_inout, s4p_icp_result* result) {
  return refine_impl(h, params, T16_inout, result, kRefineGicp, epsilon);
}

// ---------------------------------------------------------------------------------------------------------------------
// coloured ICP (include/s4p_icp_color.h)

int32_t s4p_icp_set_target_intensity(s4p_icp_ctx* h, const float* intensity, int64_t n) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!h->has_target) return fail(h, S4P_ICP_ERR_STATE, "set_target_intensity: set_target first");
  if (!intensity || n != h->n_p) return fail(h, S4P_ICP_ERR_BAD_ARG, "set_target_intensity: null or not one per target point");
  ICP_HIP(hipSetDevice(h->device));
  return set_target_intensity_host(h, intensity);
}

int32_t s4p_icp_set_target_intensity_device(s4p_icp_ctx* h, const float* intensity, int64_t n) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!h->has_target) return fail(h, S4P_ICP_ERR_STATE, "set_target_intensity: set_target first");
  if (!intensity || n != h->n_p) return fail(h, S4P_ICP_ERR_BAD_ARG, "set_target_intensity: null or not one per target point");
  ICP_HIP(hipSetDevice(h->device));
  // checked on the host, as for host input: both entry points store the same bits
  std::vector<float> v(static_cast<size_t>(n));
  ICP_HIP(hipMemcpy(v.data(), intensity, size_t(n) * sizeof(float), hipMemcpyDeviceToHost));
  return set_target_intensity_host(h, v.data());
}

int32_t s4p_icp_set_source_intensity(s4p_icp_ctx* h, const float* intensity, int64_t n) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!h->has_source) return fail(h, S4P_ICP_ERR_STATE, "set_source_intensity: set_source first");
  if (!intensity || n != h->n_q) return fail(h, S4P_ICP_ERR_BAD_ARG, "set_source_intensity: null or not one per source point");
  ICP_HIP(hipSetDevice(h->device));
  return set_source_intensity_host(h, intensity);
}

int32_t s4p_icp_set_source_intensity_device(s4p_icp_ctx* h, const float* intensity, int64_t n) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!h->has_source) return fail(h, S4P_ICP_ERR_STATE, "set_source_intensity: set_source first");
  if (!intensity || n != h->n_q) return fail(h, S4P_ICP_ERR_BAD_ARG, "set_source_intensity: null or not one per source point");
  ICP_HIP(hipSetDevice(h->device));
  std::vector<float> v(static_cast<size_t>(n));
  ICP_HIP(hipMemcpy(v.data(), intensity, size_t(n) * sizeof(float), hipMemcpyDeviceToHost));
  return set_source_intensity_host(h, v.data());
}

int32_t s4p_icp_estimate_color_gradients(s4p_icp_ctx* h, float radius, int32_t min_neighbours) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!h->has_target) return fail(h, S4P_ICP_ERR_STATE, "estimate_color_gradients: set_target first");
  if (!h->has_normals) return fail(h, S4P_ICP_ERR_STATE, "estimate_color_gradients: target normals first");
  if (!h->has_tint) return fail(h, S4P_ICP_ERR_STATE, "estimate_color_gradients: target intensity first");
  if (!(radius > 0.f) || !(radius <= h->d))
    return fail(h, S4P_ICP_ERR_BAD_ARG, "estimate_color_gradients: radius must be in (0, max_distance]");
  if (min_neighbours < S4P_ICP_COLOR_MIN_NEIGHBOURS)
    return fail(h, S4P_ICP_ERR_BAD_ARG, "estimate_color_gradients: min_neighbours must be >= 4");
  ICP_HIP(hipSetDevice(h->device));
  h->has_grad = false;
  if (!h->grad) ICP_HIP(hipMalloc((void**)&h->grad, size_t(h->n_p) * sizeof(float4)));
  hipLaunchKernelGGL(k_color_gradient, dim3(blocks_for(h->n_p)), dim3(kBlock), 0, h->st, h->g, (const float4*)h->nrm, (const float*)h->tint,
                     uint64_t(h->n_p), radius * radius, min_neighbours, h->grad);
  ICP_HIP(hipGetLastError());
  ICP_HIP(hipStreamSynchronize(h->st));
  h->has_grad = true;
  return S4P_ICP_OK;
}

int32_t s4p_icp_target_color_gradients(s4p_icp_ctx* h, float* gx, float* gy, float* gz) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!gx || !gy || !gz) return fail(h, S4P_ICP_ERR_BAD_ARG, "target_color_gradients: null argument");
  if (!h->has_target || !h->has_grad) return fail(h, S4P_ICP_ERR_STATE, "target_color_gradients: no gradients");
  ICP_HIP(hipSetDevice(h->device));
  Scratch S;
  const size_t n = size_t(h->n_p);
  float* d[3];
  for (int a = 0; a < 3; ++a) ICP_HIP(S.alloc((void**)&d[a], n * sizeof(float)));
  hipLaunchKernelGGL(k_scatter_normals, dim3(blocks_for(h->n_p)), dim3(kBlock), 0, h->st, (const float4*)h->grad, (const float4*)h->tgt,
                     uint64_t(n), d[0], d[1], d[2]);
  ICP_HIP(hipGetLastError());
  float* out[3] = {gx, gy, gz};
  for (int a = 0; a < 3; ++a) ICP_HIP(hipMemcpyAsync(out[a], d[a], n * sizeof(float), hipMemcpyDeviceToHost, h->st));
  ICP_HIP(hipStreamSynchronize(h->st));
  return S4P_ICP_OK;
}

int32_t s4p_icp_color_sums(s4p_icp_ctx* h, const float* T16_centred, double lambda, double* sums) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!T16_centred || !sums) return fail(h, S4P_ICP_ERR_BAD_ARG, "color_sums: null argument");
  if (int32_t rc = color_ready(h, lambda)) return rc;
  if (int32_t rc = color_prepare(h, h->src)) return rc;
  if (int32_t rc = reject_prepare(h, h->src)) return rc;
  return color_pass(h, centred_from_float16(T16_centred), h->src, lambda, sums);
}

int32_t s4p_icp_refine_color(s4p_icp_ctx* h, const s4p_icp_params* params, double lambda, double* T16_inout, s4p_icp_result* result) {
  return refine_impl(h, params, T16_inout, result, kRefineColor, lambda);
}

// ---------------------------------------------------------------------------------------------------------------------
// correspondence rejection (include/s4p_icp_reject.h)

void s4p_icp_reject_defaults(s4p_icp_reject* r) {
  if (r) std::memset(r, 0, sizeof(*r));
}

int32_t s4p_icp_set_rejection(s4p_icp_ctx* h, const s4p_icp_reject* r) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  s4p_icp_reject R;
  s4p_icp_reject_defaults(&R);
  if (r) {
    if (r->reciprocal != 0 && r->reciprocal != 1) return fail(h, S4P_ICP_ERR_BAD_ARG, "set_rejection: reciprocal must be 0 or 1");
    R.reciprocal = r->reciprocal;
    R.normal_mode = r->normal_mode;
    if (r->normal_mode == S4P_ICP_REJECT_NORMALS_UNORIENTED) {
      if (!(r->normal_cos >= 0.0 && r->normal_cos <= 1.0)) return fail(h, S4P_ICP_ERR_BAD_ARG, "set_rejection: normal_cos must be in [0, 1] (unoriented)");
      R.normal_cos = r->normal_cos;
    } else if (r->normal_mode == S4P_ICP_REJECT_NORMALS_ORIENTED) {
      if (!(r->normal_cos >= -1.0 && r->normal_cos <= 1.0)) return fail(h, S4P_ICP_ERR_BAD_ARG, "set_rejection: normal_cos must be in [-1, 1] (oriented)");
      R.normal_cos = r->normal_cos;
    } else if (r->normal_mode != S4P_ICP_REJECT_NORMALS_OFF) {
      return fail(h, S4P_ICP_ERR_BAD_ARG, "set_rejection: unknown normal_mode");
    }
  }
  h->rej = R;
  h->rej_on = R.reciprocal != 0 || R.normal_mode != S4P_ICP_REJECT_NORMALS_OFF;
  return S4P_ICP_OK;
}

int32_t s4p_icp_rejection(s4p_icp_ctx* h, const float* T16_centred, int32_t* idx, float* d2, int32_t* why) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!T16_centred || !idx || !d2 || !why) return fail(h, S4P_ICP_ERR_BAD_ARG, "rejection: null argument");
  if (int32_t rc = ready(h)) return rc;
  if (int32_t rc = reject_prepare(h, h->src, true)) return rc;
  Scratch S;
  const uint64_t un = uint64_t(h->n_q);
  int32_t *di, *dw;
  float* dd;
  uint8_t* code;
  ICP_HIP(S.alloc((void**)&di, un * 4)); ICP_HIP(S.alloc((void**)&dd, un * 4)); ICP_HIP(S.alloc((void**)&dw, un * 4));
  ICP_HIP(S.alloc((void**)&code, un));
  const Tf T = centred_from_float16(T16_centred);
  const int nb = blocks_for(h->n_q);
  SearchArgs A;
  A.T = T; A.g = h->g; A.src = h->src; A.nrm = h->nrm; A.n = un; A.d2max = h->d2max; A.slot = h->rslot; A.key = h->rkey;
  hipLaunchKernelGGL(k_search<false>, dim3(nb), dim3(kBlock), 0, h->st, A);
  ICP_HIP(hipGetLastError());
  if (int32_t rc = launch_reject(h, T, h->src, code)) return rc;
  hipLaunchKernelGGL(k_reject_out, dim3(nb), dim3(kBlock), 0, h->st, (const float4*)h->src, (const float4*)h->tgt, (const uint32_t*)h->rslot,
                     (const uint32_t*)h->rkey, (const uint8_t*)code, un, di, dd, dw);
  ICP_HIP(hipGetLastError());
  ICP_HIP(hipMemcpyAsync(idx, di, un * 4, hipMemcpyDeviceToHost, h->st));
  ICP_HIP(hipMemcpyAsync(d2, dd, un * 4, hipMemcpyDeviceToHost, h->st));
  ICP_HIP(hipMemcpyAsync(why, dw, un * 4, hipMemcpyDeviceToHost, h->st));
  ICP_HIP(hipStreamSynchronize(h->st));
  reject_done(h);
  return S4P_ICP_OK;
}

int32_t s4p_icp_rejection_counts(const s4p_icp_ctx* h, int64_t counts[4]) {
  if (!h || !counts) return S4P_ICP_ERR_BAD_ARG;
  for (int k = 0; k < 4; ++k) counts[k] = h->rej_counts[k];
  return S4P_ICP_OK;
}

}  // extern "C"
