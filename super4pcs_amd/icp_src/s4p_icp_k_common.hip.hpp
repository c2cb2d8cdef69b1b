// s4p_icp_k_common.hip.hpp -- what every kernel of libsuper4pcs_icp.so shares: launch constants, the grid, the float
// transform, the nearest-neighbour walk, the symmetric Jacobi and the small device helpers.
#pragma once

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

struct Tf { float m[12]; };

__device__ inline void apply_t(const Tf& T, float x, float y, float z, float& ox, float& oy, float& oz) {
  ox = ((T.m[0] * x + T.m[1] * y) + T.m[2] * z) + T.m[3];
  oy = ((T.m[4] * x + T.m[5] * y) + T.m[6] * z) + T.m[7];
  oz = ((T.m[8] * x + T.m[9] * y) + T.m[10] * z) + T.m[11];
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

constexpr uint32_t kNoKey = 0xFFFFFFFFu;    // a miss, or (plane) a zero normal: above every key (keys are non-negative floats)
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
constexpr int kDigits = 4, kBins = 256;     // 4 digits of 8 bits, most significant first
enum SelMode { kSelNone = 0, kSelTrim = 1, kSelMedian = 2 };

struct SelState {          // zeroed before each pass; written by k_key_digit only
  uint32_t M, k, rank, prefix;
  double s, cs, cs2;
};

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

// ---------------------------------------------------------------------------------------------------------------------
// Device helpers shared by the kernels.  The float4 arguments go by value: by reference, some callers' instructions change
// ("ICP sources: layout", has the rule: a helper that moves a measured kernel's digest is not used in it).

__device__ inline bool is_zero(float4 v) { return v.x == 0.f && v.y == 0.f && v.z == 0.f; }

// nearest_t's float d2 between (x, y, z) and the winner p, for the kernels that take the winner from k_search's slot
__device__ inline float winner_d2(float x, float y, float z, float4 p) {
  const float dx = x - p.x, dy = y - p.y, dz = z - p.z;
  return dx * dx + (dy * dy + dz * dz);
}

// the point-to-plane residual (p - q) . n in double
__device__ inline double plane_residual(float4 p, const double (&qd)[3], const double (&nd)[3]) {
  return ((double(p.x) - qd[0]) * nd[0] + (double(p.y) - qd[1]) * nd[1]) + (double(p.z) - qd[2]) * nd[2];
}

// The end of every sum kernel: a lane's N sums -> the wave (xor butterfly) -> the workgroup (LDS, waves in order) -> row
// blockIdx.x of the slab.  No atomics: the order is fixed.
template <int N, int PITCH>
__device__ inline void block_row(const double (&s)[N], double* slab) {
  __shared__ double red[kBlock / 64][N];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    double v = s[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    double v = red[0][threadIdx.x];
    for (int w = 1; w < kBlock / 64; ++w) v += red[w][threadIdx.x];
    slab[uint64_t(blockIdx.x) * PITCH + threadIdx.x] = v;
  }
}

// One workgroup: the slab's nb rows -> NS sums, in a fixed order: kBlock / NS parts per column (rows part, part + parts,
// ...), then the parts in order (17 sums: 15 parts; 31 sums: 8 parts)
template <int NS, int PITCH>
__device__ inline void slab_total(const double* slab, int nb, double* out) {
  constexpr int kParts = kBlock / NS;
  __shared__ double part[kParts][NS];
  const int col = threadIdx.x % NS, prt = threadIdx.x / NS;
  if (prt < kParts) {
    double v = 0.0;
    for (int r = prt; r < nb; r += kParts) v += slab[uint64_t(r) * PITCH + col];
    part[prt][col] = v;
  }
  __syncthreads();
  if (threadIdx.x < NS) {
    double v = part[0][threadIdx.x];
    for (int p = 1; p < kParts; ++p) v += part[p][threadIdx.x];
    out[threadIdx.x] = v;
  }
}

}  // namespace s4p_icp
