// s4p_feature.inc -- FPFH descriptors and the feature-space matcher of libsuper4pcs_normals.so (include/s4p_feature.h, DESIGN.md
// section 35).  Included by s4p_normals.hip after s4p_shape.inc.  s4p_feature_fpfh works on an s4p_normals_ctx after set_cloud,
// on its cloud, stream and arena, and leaves the context's own grid alone; s4p_feature_match needs the stream and the arena
// only.
//
// Device path of fpfh:
//   grid      section 34's: shape_grid_plan + cluster_grid_build into the arena, the cloud in cell order, shape_cells and
//             cluster_row for the block of cells around a point.
//   normals   k_feature_normals: the caller's normals into the same cell order as float4, w = 1 for a valid point and 0
//             otherwise (the contract's "valid point").
//   spfh      k_feature_spfh: a lane per point walks its block of cells; every accepted pair adds one to three of the lane's
//             33 counters, which live in LDS as [bin][lane] (a lane cannot index registers dynamically; 64 lanes of a wave
//             touch 64 different banks whatever their bins).  The lane then writes its S row, 33 values of at most 2^15 packed
//             into 17 dwords, in cell order.
//   fpfh      k_feature_fpfh: the walk again; per pair the weight and 33 integer multiply-adds of the neighbour's S row into
//             64-bit accumulators in registers (constant indices: the loops are unrolled), then the three normalisations.
// Device path of match: k_feature_rows packs both tables into rows of 17 dwords (the spare half word says "not all zeros")
// and flags a value above 4096; k_feature_match is dense rows x columns: a lane per row, the columns in LDS tiles of 64 that
// every lane reads at the same address (a broadcast), 16 packed 16-bit subtracts and 16 signed dot2 accumulates per pair and
// one scalar term, the minimum as a packed key D << 32 | index; columns are split across workgroups and joined by a 64-bit
// atomicMin, which has no order.  k_feature_pick writes idx and dist, with the mutual test.
// Integer sums and minima have no order: the bits do not depend on the grid, the walk or the launch.  Every loop is bounded
// at entry.  No float atomics; the only atomics are the matcher's atomicMin and the flag's atomicOr.

#include "s4p_feature.h"

namespace s4p_nrm {

constexpr int kFeatBins = S4P_FEATURE_BINS;
constexpr int kFeatRow = 17;                     // dwords of a packed row: 33 half words and one spare
constexpr int kFeatTile = 64;                    // columns of the matcher's LDS tile
// The SPFH counters of the contract are 32 bits.  -DS4P_FEATURE_COUNT_BITS=16 builds a library for measurement only
// (tools/feature_timing.py --lib): half the LDS and so twice the waves per SIMD, the same bits while no point has 2^16 pairs.
#ifndef S4P_FEATURE_COUNT_BITS
#define S4P_FEATURE_COUNT_BITS 32
#endif
using FeatureCount = std::conditional_t<S4P_FEATURE_COUNT_BITS == 16, uint16_t, uint32_t>;
static_assert(S4P_FEATURE_COUNT_BITS == 16 || (S4P_FEATURE_COUNT_BITS == 32 && sizeof(FeatureCount) == 4),
              "the SPFH counters are 32 bits: a point with 2^32 pairs within r is outside the contract");
static_assert(kFeatBins == 33 && 2 * kFeatRow == kFeatBins + 1, "three groups of eleven, packed in pairs");

struct FeatureArgs {
  GridDev g;                  // the grid of this call (shape_grid_plan)
  int32_t rings;
  uint64_t n;
  float r2;                   // fl(r * r)
  const float4* nrm;          // n, cell order: the normal, w = 1 (valid) or 0
  uint32_t* S;                // 17 n, cell order: the SPFH rows
  uint16_t* fpfh;             // 33 n, the caller's order
  int32_t* count;             // n or null, the caller's order
};

__device__ __forceinline__ float feat_dot(float a0, float a1, float a2, float b0, float b1, float b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

__device__ __forceinline__ int feat_bin11(float f) {
  const float t = 11.f * ((f + 1.f) * 0.5f);
  if (!(t >= 1.f)) return 0;
  if (t >= 10.f) return 10;
  return int(floorf(t));
}

__device__ __forceinline__ int feat_bin_theta(float x, float y) {
  const float B[10][2] = S4P_FEATURE_THETA_BOUNDS;
  const bool up = y >= 0.f;
  int bin = 0;
#pragma unroll
  for (int k = 0; k < 10; ++k) {
    const float c = B[k][0] * y - B[k][1] * x;
    bin += k < 5 ? ((up || c >= 0.f) ? 1 : 0) : ((up && c >= 0.f) ? 1 : 0);
  }
  return bin;
}

// The three bins of the pair (i, j), d = p_j - p_i with d2 = |d|^2 > 0; false when the pair is skipped.
__device__ __forceinline__ bool feat_pair(const float4 ni, const float4 nj, float dx, float dy, float dz, float d2, int* ba, int* bp, int* bt) {
  const float len = sqrtf(d2);
  const float ai = feat_dot(ni.x, ni.y, ni.z, dx, dy, dz), aj = feat_dot(nj.x, nj.y, nj.z, dx, dy, dz);
  const bool swap = !(fabsf(ai) >= fabsf(aj));
  const float s0 = swap ? nj.x : ni.x, s1 = swap ? nj.y : ni.y, s2 = swap ? nj.z : ni.z;
  const float t0 = swap ? ni.x : nj.x, t1 = swap ? ni.y : nj.y, t2 = swap ? ni.z : nj.z;
  const float e0 = swap ? -dx : dx, e1 = swap ? -dy : dy, e2 = swap ? -dz : dz;
  const float as = feat_dot(s0, s1, s2, e0, e1, e2);
  const float phi = as / len;
  float v0 = e1 * s2 - e2 * s1, v1 = e2 * s0 - e0 * s2, v2 = e0 * s1 - e1 * s0;
  const float vn = sqrtf(feat_dot(v0, v1, v2, v0, v1, v2));
  if (!(vn > 0.f)) return false;
  v0 /= vn; v1 /= vn; v2 /= vn;
  const float w0 = s1 * v2 - s2 * v1, w1 = s2 * v0 - s0 * v2, w2 = s0 * v1 - s1 * v0;
  const float alpha = feat_dot(v0, v1, v2, t0, t1, t2);
  const float x = feat_dot(s0, s1, s2, t0, t1, t2), y = feat_dot(w0, w1, w2, t0, t1, t2);
  *ba = feat_bin11(alpha);
  *bp = feat_bin11(phi);
  *bt = feat_bin_theta(x, y);
  return true;
}

// the caller's normals into the grid's cell order; w says whether the point is valid
__global__ __launch_bounds__(kBlock) void k_feature_normals(const float4* pts, uint64_t n, const float* normals, float4* out) {
  for (uint64_t s = blockIdx.x * (uint64_t)kBlock + threadIdx.x; s < n; s += (uint64_t)gridDim.x * kBlock) {
    const float4 p = pts[s];
    const uint64_t i = __float_as_uint(p.w);
    const float n0 = normals[3 * i], n1 = normals[3 * i + 1], n2 = normals[3 * i + 2];
    const bool ok = isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && isfinite(n0) && isfinite(n1) && isfinite(n2) &&
                    (n0 * n0 + n1 * n1) + n2 * n2 > 0.f;
    out[s] = make_float4(n0, n1, n2, ok ? 1.f : 0.f);
  }
}

// The walk of both passes: body(t, dx, dy, dz, d2, nt) for every pair of the lane's point q, t the pair's slot in cell order.
template <class Body>
__device__ __forceinline__ void feature_walk(const FeatureArgs& A, const float4 q, Body&& body) {
  const GridDev& g = A.g;
  int x0, x1, y0, y1, z0, z1;
  shape_cells(q.x, g.ox, g.inv_h, g.nx, A.rings, &x0, &x1);
  shape_cells(q.y, g.oy, g.inv_h, g.ny, A.rings, &y0, &y1);
  shape_cells(q.z, g.oz, g.inv_h, g.nz, A.rings, &z0, &z1);
  if (x0 > x1) return;
  for (int iz = z0; iz <= z1; ++iz)
    for (int iy = y0; iy <= y1; ++iy) {
      const uint2 rg = cluster_row(g, iz, iy, x0, x1);
      for (uint32_t t = rg.x; t < rg.y; ++t) {
        const float4 p = g.pts[t];
        const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
        const float d2 = dx * dx + (dy * dy + dz * dz);
        if (!(d2 > 0.f && d2 <= A.r2)) continue;
        const float4 nt = A.nrm[t];
        if (nt.w == 0.f) continue;
        body(t, dx, dy, dz, d2, nt);
      }
    }
}

__global__ __launch_bounds__(kBlock) void k_feature_spfh(FeatureArgs A) {
  __shared__ FeatureCount hist[kFeatBins * kBlock];          // [bin][lane]
  const GridDev& g = A.g;
  FeatureCount* my = hist + threadIdx.x;
  for (uint64_t j = blockIdx.x * (uint64_t)kBlock + threadIdx.x; j < A.n; j += (uint64_t)gridDim.x * kBlock) {
#pragma unroll
    for (int b = 0; b < kFeatBins; ++b) my[b * kBlock] = 0;
    const float4 q = g.pts[j];
    const float4 nq = A.nrm[j];
    uint32_t c = 0u;
    if (nq.w != 0.f)
      feature_walk(A, q, [&](uint32_t, float dx, float dy, float dz, float d2, const float4 nt) {
        int ba, bp, bt;
        if (feat_pair(nq, nt, dx, dy, dz, d2, &ba, &bp, &bt)) {
          ++c;
          my[ba * kBlock] += 1; my[(11 + bp) * kBlock] += 1; my[(22 + bt) * kBlock] += 1;
        }
      });
    uint32_t* row = A.S + uint64_t(kFeatRow) * j;
#pragma unroll
    for (int k = 0; k < kFeatRow; ++k) {
      const uint32_t lo = c ? uint32_t((uint64_t(my[(2 * k) * kBlock]) << 15) / c) : 0u;
      uint32_t hi = 0u;
      if (2 * k + 1 < kFeatBins && c) hi = uint32_t((uint64_t(my[(2 * k + 1) % kFeatBins * kBlock]) << 15) / c);
      row[k] = lo | hi << 16;
    }
    if (A.count) A.count[__float_as_uint(q.w)] = int32_t(c);
  }
}

__global__ __launch_bounds__(kBlock) void k_feature_fpfh(FeatureArgs A) {
  const GridDev& g = A.g;
  for (uint64_t j = blockIdx.x * (uint64_t)kBlock + threadIdx.x; j < A.n; j += (uint64_t)gridDim.x * kBlock) {
    const float4 q = g.pts[j];
    const float4 nq = A.nrm[j];
    unsigned long long acc[kFeatBins];
#pragma unroll
    for (int b = 0; b < kFeatBins; ++b) acc[b] = 0ull;
    if (nq.w != 0.f)
      feature_walk(A, q, [&](uint32_t t, float, float, float, float d2, const float4) {
        const uint32_t w = uint32_t(fminf(64.f * (A.r2 / d2), 65536.f));
        const uint32_t* row = A.S + uint64_t(kFeatRow) * t;
#pragma unroll
        for (int k = 0; k < kFeatRow - 1; ++k) {
          const uint32_t v = row[k];
          acc[2 * k] += (unsigned long long)w * (v & 0xFFFFu);
          acc[2 * k + 1] += (unsigned long long)w * (v >> 16);
        }
        acc[kFeatBins - 1] += (unsigned long long)w * row[kFeatRow - 1];
      });
    uint16_t* out = A.fpfh + uint64_t(kFeatBins) * __float_as_uint(q.w);
#pragma unroll
    for (int grp = 0; grp < 3; ++grp) {
      unsigned long long T = 0ull;
#pragma unroll
      for (int b = 0; b < 11; ++b) T += acc[11 * grp + b];
      const double dT = double(T);
#pragma unroll
      for (int b = 0; b < 11; ++b) out[11 * grp + b] = T ? uint16_t(floor((double(acc[11 * grp + b]) / dT) * 4096.0)) : uint16_t(0);
    }
  }
}

// One lane per row of a table: the row packed into 17 dwords, the spare half word 1 when the row is not all zeros; *bad is
// set when a value exceeds S4P_FEATURE_MAX.
__global__ __launch_bounds__(kBlock) void k_feature_rows(const uint16_t* f, uint64_t rows, uint32_t* packed, uint32_t* bad) {
  bool over = false;
  for (uint64_t r = blockIdx.x * (uint64_t)kBlock + threadIdx.x; r < rows; r += (uint64_t)gridDim.x * kBlock) {
    const uint16_t* src = f + uint64_t(kFeatBins) * r;
    uint32_t* dst = packed + uint64_t(kFeatRow) * r;
    uint32_t any = 0u;
#pragma unroll
    for (int k = 0; k < kFeatRow - 1; ++k) {
      const uint32_t a = src[2 * k], b = src[2 * k + 1];
      any |= a | b;
      over |= a > uint32_t(S4P_FEATURE_MAX) || b > uint32_t(S4P_FEATURE_MAX);
      dst[k] = a | b << 16;
    }
    const uint32_t a = src[kFeatBins - 1];
    any |= a;
    over |= a > uint32_t(S4P_FEATURE_MAX);
    dst[kFeatRow - 1] = a | (any ? 1u << 16 : 0u);
  }
  if (over) atomicOr(bad, 1u);
}

struct MatchArgs {
  const uint32_t* rows;       // 17 m: the table whose rows look for a partner
  uint64_t m;
  const uint32_t* cols;       // 17 n: the table searched
  uint64_t n;
  uint64_t chunk;             // columns per blockIdx.y, a multiple of kFeatTile
  unsigned long long* key;    // m: min (D << 32 | column) over the usable columns, ~0 before
};

typedef short feat_short2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ feat_short2 feat_halves(uint32_t v) { return __builtin_bit_cast(feat_short2, v); }

__global__ __launch_bounds__(kBlock) void k_feature_match(MatchArgs A) {
  __shared__ uint32_t tile[kFeatTile * kFeatRow];
  const uint64_t a = blockIdx.x * (uint64_t)kBlock + threadIdx.x;
  const bool live = a < A.m;
  uint32_t ra[kFeatRow];
#pragma unroll
  for (int k = 0; k < kFeatRow; ++k) ra[k] = live ? A.rows[uint64_t(kFeatRow) * a + k] : 0u;
  const bool use = live && (ra[kFeatRow - 1] >> 16) != 0u;
  const int32_t a16 = int32_t(ra[kFeatRow - 1] & 0xFFFFu);
  const uint64_t c0 = blockIdx.y * A.chunk, c1 = c0 + A.chunk < A.n ? c0 + A.chunk : A.n;
  uint32_t bestD = 0xFFFFFFFFu, bestB = 0xFFFFFFFFu;
  for (uint64_t base = c0; base < c1; base += kFeatTile) {
    const uint32_t cnt = uint32_t(c1 - base < uint64_t(kFeatTile) ? c1 - base : uint64_t(kFeatTile));
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < cnt * kFeatRow; t += kBlock) tile[t] = A.cols[uint64_t(kFeatRow) * base + t];
    __syncthreads();
    if (use)
      for (uint32_t c = 0; c < cnt; ++c) {
        const uint32_t* rb = tile + kFeatRow * c;
        int32_t acc = 0;
#pragma unroll
        for (int k = 0; k < kFeatRow - 1; ++k) {
          const feat_short2 d = feat_halves(ra[k]) - feat_halves(rb[k]);          // |d| <= 4096: no 16-bit wrap
          acc = __builtin_amdgcn_sdot2(d, d, acc, false);
        }
        const uint32_t last = rb[kFeatRow - 1];
        const int32_t d16 = a16 - int32_t(last & 0xFFFFu);
        acc += d16 * d16;
        // ascending columns and a strict comparison: the smallest column among equal distances
        if ((last >> 16) != 0u && uint32_t(acc) < bestD) { bestD = uint32_t(acc); bestB = uint32_t(base + c); }
      }
  }
  if (use && bestB != 0xFFFFFFFFu) atomicMin(A.key + a, (unsigned long long)bestD << 32 | bestB);
}

// idx and dist from the keys; with keyB (mutual) a row keeps its partner only when it is its partner's best
__global__ __launch_bounds__(kBlock) void k_feature_pick(const unsigned long long* keyA, uint64_t m, const unsigned long long* keyB,
                                                         int32_t* idx, int32_t* dist) {
  for (uint64_t a = blockIdx.x * (uint64_t)kBlock + threadIdx.x; a < m; a += (uint64_t)gridDim.x * kBlock) {
    const unsigned long long key = keyA[a];
    int32_t b = -1, d = -1;
    if (key != ~0ull) {
      b = int32_t(uint32_t(key)); d = int32_t(key >> 32);
      if (keyB && uint32_t(keyB[uint32_t(key)]) != uint32_t(a)) b = d = -1;
    }
    idx[a] = b;
    if (dist) dist[a] = d;
  }
}

}  // namespace s4p_nrm

namespace {

int32_t feature_fpfh_impl(s4p_normals_ctx* h, const float* normals, float radius, uint16_t* fpfh, int32_t* count, bool device) {
  if (!h) return S4P_NORMALS_ERR_BAD_ARG;
  if (int32_t rc = cluster_check(h, "feature_fpfh", "radius", radius)) return rc;
  if (!normals) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "feature_fpfh: null normals");
  if (!fpfh) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "feature_fpfh: null fpfh");
  NRM_HIP(hipSetDevice(h->device));
  const uint64_t un = uint64_t(h->n);
  ClusterGrid G;
  int rings = 1;
  if (int32_t rc = shape_grid_plan(h, "feature_fpfh", radius, &G, &rings)) return rc;
  const float* dn = normals;
  float4* nrm = nullptr;
  uint32_t* S = nullptr;
  uint16_t* dF = fpfh;
  int32_t* dc = count;
  if (int32_t rc = arena_layout(h, "feature_fpfh", [&](Arena& ar) {
        G.take(ar, un);
        nrm = ar.take<float4>(un);
        S = ar.take<uint32_t>(kFeatRow * un);
        if (!device) {
          dn = ar.take<float>(3 * un);
          dF = ar.take<uint16_t>(kFeatBins * un);
          if (count) dc = ar.take<int32_t>(un);
        }
      })) return rc;
  if (int32_t rc = cluster_grid_build(h, &G)) return rc;
  if (!device) NRM_HIP(hipMemcpyAsync(const_cast<float*>(dn), normals, 3 * un * sizeof(float), hipMemcpyHostToDevice, h->st));
  const int nb = blocks_for(h->n);
  hipLaunchKernelGGL(k_feature_normals, dim3(nb), dim3(kBlock), 0, h->st, G.g.pts, un, dn, nrm);
  NRM_HIP(hipGetLastError());
  FeatureArgs A{};
  A.g = G.g; A.rings = rings; A.n = un; A.r2 = radius * radius; A.nrm = nrm; A.S = S; A.fpfh = dF; A.count = dc;
  hipLaunchKernelGGL(k_feature_spfh, dim3(nb), dim3(kBlock), 0, h->st, A);
  NRM_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_feature_fpfh, dim3(nb), dim3(kBlock), 0, h->st, A);
  NRM_HIP(hipGetLastError());
  if (!device) {
    NRM_HIP(hipMemcpyAsync(fpfh, dF, kFeatBins * un * sizeof(uint16_t), hipMemcpyDeviceToHost, h->st));
    if (count) NRM_HIP(hipMemcpyAsync(count, dc, un * sizeof(int32_t), hipMemcpyDeviceToHost, h->st));
  }
  NRM_HIP(hipStreamSynchronize(h->st));
  return S4P_NORMALS_OK;
}

// rows x cols through k_feature_match: the columns are split so that about kMaxBlocks workgroups run
int32_t feature_match_launch(s4p_normals_ctx* h, const uint32_t* rows, uint64_t m, const uint32_t* cols, uint64_t n, unsigned long long* key) {
  NRM_HIP(hipMemsetAsync(key, 0xFF, m * sizeof(unsigned long long), h->st));
  if (n == 0) return S4P_NORMALS_OK;
  const uint64_t row_tiles = (m + kBlock - 1) / kBlock;
  const uint64_t chunks = std::max<uint64_t>(1, std::min<uint64_t>((n + 511) / 512, uint64_t(kMaxBlocks) / std::min<uint64_t>(row_tiles, kMaxBlocks)));
  MatchArgs A{};
  A.rows = rows; A.m = m; A.cols = cols; A.n = n; A.key = key;
  A.chunk = ((n + chunks - 1) / chunks + kFeatTile - 1) / kFeatTile * kFeatTile;
  hipLaunchKernelGGL(k_feature_match, dim3(uint32_t(row_tiles), uint32_t(chunks)), dim3(kBlock), 0, h->st, A);
  NRM_HIP(hipGetLastError());
  return S4P_NORMALS_OK;
}

int32_t feature_match_impl(s4p_normals_ctx* h, const uint16_t* fa, int64_t m, const uint16_t* fb, int64_t n, int32_t mutual, int32_t* idx,
                           int32_t* dist, bool device) {
  if (!h) return S4P_NORMALS_ERR_BAD_ARG;
  if (m < 0 || m > kMaxPoints || n < 0 || n > kMaxPoints) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "feature_match: m and n must be in [0, 2^31 - 2]");
  if (m == 0) return S4P_NORMALS_OK;
  if (!fa || !idx || (n > 0 && !fb)) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "feature_match: null fa, fb or idx");
  NRM_HIP(hipSetDevice(h->device));
  const uint64_t um = uint64_t(m), un = uint64_t(n);
  const uint16_t *da = fa, *db = fb;
  uint32_t *pa = nullptr, *pb = nullptr, *bad = nullptr;
  unsigned long long *keyA = nullptr, *keyB = nullptr;
  int32_t *didx = idx, *ddist = dist;
  if (int32_t rc = arena_layout(h, "feature_match", [&](Arena& ar) {
        pa = ar.take<uint32_t>(kFeatRow * um);
        pb = ar.take<uint32_t>(kFeatRow * un);
        keyA = ar.take<unsigned long long>(um);
        if (mutual) keyB = ar.take<unsigned long long>(un);
        bad = ar.take<uint32_t>(1);
        if (!device) {
          da = ar.take<uint16_t>(kFeatBins * um);
          db = ar.take<uint16_t>(kFeatBins * un);
          didx = ar.take<int32_t>(um);
          if (dist) ddist = ar.take<int32_t>(um);
        }
      })) return rc;
  if (!device) {
    NRM_HIP(hipMemcpyAsync(const_cast<uint16_t*>(da), fa, kFeatBins * um * sizeof(uint16_t), hipMemcpyHostToDevice, h->st));
    if (un) NRM_HIP(hipMemcpyAsync(const_cast<uint16_t*>(db), fb, kFeatBins * un * sizeof(uint16_t), hipMemcpyHostToDevice, h->st));
  }
  NRM_HIP(hipMemsetAsync(bad, 0, sizeof(uint32_t), h->st));
  hipLaunchKernelGGL(k_feature_rows, dim3(blocks_for(m)), dim3(kBlock), 0, h->st, da, um, pa, bad);
  NRM_HIP(hipGetLastError());
  if (un) {
    hipLaunchKernelGGL(k_feature_rows, dim3(blocks_for(n)), dim3(kBlock), 0, h->st, db, un, pb, bad);
    NRM_HIP(hipGetLastError());
  }
  uint32_t hbad = 0u;
  NRM_HIP(hipMemcpyAsync(&hbad, bad, sizeof(uint32_t), hipMemcpyDeviceToHost, h->st));
  NRM_HIP(hipStreamSynchronize(h->st));
  if (hbad) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "feature_match: a descriptor value above 4096 (S4P_FEATURE_MAX)");
  if (int32_t rc = feature_match_launch(h, pa, um, pb, un, keyA)) return rc;
  if (mutual && un)
    if (int32_t rc = feature_match_launch(h, pb, un, pa, um, keyB)) return rc;
  hipLaunchKernelGGL(k_feature_pick, dim3(blocks_for(m)), dim3(kBlock), 0, h->st, (const unsigned long long*)keyA, um,
                     (const unsigned long long*)((mutual && un) ? keyB : nullptr), didx, ddist);
  NRM_HIP(hipGetLastError());
  if (!device) {
    NRM_HIP(hipMemcpyAsync(idx, didx, um * sizeof(int32_t), hipMemcpyDeviceToHost, h->st));
    if (dist) NRM_HIP(hipMemcpyAsync(dist, ddist, um * sizeof(int32_t), hipMemcpyDeviceToHost, h->st));
  }
  NRM_HIP(hipStreamSynchronize(h->st));
  return S4P_NORMALS_OK;
}

}  // namespace

extern "C" {

int32_t s4p_feature_fpfh(s4p_normals_ctx* h, const float* normals, float radius, uint16_t* fpfh, int32_t* count) {
  return feature_fpfh_impl(h, normals, radius, fpfh, count, false);
}
int32_t s4p_feature_fpfh_device(s4p_normals_ctx* h, const float* normals, float radius, uint16_t* fpfh, int32_t* count) {
  return feature_fpfh_impl(h, normals, radius, fpfh, count, true);
}

int32_t s4p_feature_match(s4p_normals_ctx* h, const uint16_t* fa, int64_t m, const uint16_t* fb, int64_t n, int32_t mutual, int32_t* idx,
                          int32_t* dist) {
  return feature_match_impl(h, fa, m, fb, n, mutual, idx, dist, false);
}
int32_t s4p_feature_match_device(s4p_normals_ctx* h, const uint16_t* fa, int64_t m, const uint16_t* fb, int64_t n, int32_t mutual,
                                 int32_t* idx, int32_t* dist) {
  return feature_match_impl(h, fa, m, fb, n, mutual, idx, dist, true);
}

}  // extern "C"
