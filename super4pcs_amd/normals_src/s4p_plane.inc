// s4p_plane.inc -- RANSAC plane segmentation of libsuper4pcs_normals.so (include/s4p_plane.h, DESIGN.md section 32).  Included
// by s4p_normals.hip after s4p_cluster.inc: the functions work on an s4p_normals_ctx after set_cloud, on its cloud in the
// caller's order, its bounds, stream and arena; the context's grid is not used.
//
// Device path (kernel boundaries are the only ordering the phases rely on; nothing visits the host before the end):
//   alive       hipCUB select of the indices whose exclude byte is 0 (only with an exclude mask)
//   candidates  k_plane_candidates: a lane per trial draws three alive positions and writes a 32-byte record
//   count       k_plane_count: candidates x points.  A lane keeps kPlanePts centred points in registers, the workgroup loops
//               over a batch of kPlaneBatch records that arrive by scalar loads; a wave's count is ballot + popcount
//   argmax      k_plane_argmax: one workgroup, the maximum of (count << 32 | ~t) over the valid candidates -> PlaneState
//   mask        k_plane_mask: the inlier bytes of the state's plane and their number
//   refit       hipCUB select of the inlier indices, k_plane_moments (a lane sums a block of S4P_PLANE_SUM_BLOCK list
//               positions in order), k_plane_refit (the block sums in order, then one lane: covariance, jacobi3, the new
//               plane into PlaneState), k_plane_mask again
// No float or double atomics: the counts are integers, the sums have the one order the header states.

#include "s4p_plane.h"

namespace s4p_nrm {

constexpr int kPlanePts = 16;                         // centred points a lane of k_plane_count keeps in registers
constexpr int kPlaneTile = kBlock * kPlanePts;        // points one workgroup pass covers
constexpr int kPlaneBatch = 128;                      // candidate records one workgroup loops over
constexpr int kPlaneMaxTiles = 128;                   // grid.x of k_plane_count: beyond 128 x 4096 points a lane takes more trips
constexpr int kPlaneSumBlock = S4P_PLANE_SUM_BLOCK;

struct PlaneCand {            // 32 bytes: one scalar load of eight words
  float n0, n1, n2, d;
  uint32_t valid;
  uint32_t pad[3];
};
static_assert(sizeof(PlaneCand) == 32, "a candidate record is 32 bytes");

struct PlaneState {
  unsigned long long key;     // (count << 32 | ~t) of the winner, 0: none
  float n0, n1, n2, d;        // the current plane in the centred frame
  uint32_t inliers;           // of the current plane
  int32_t trial;
  uint32_t valid_trials;
  uint32_t stopped;           // a refit found fewer than 3 inliers or no spread: the plane stays, later rounds do nothing
  uint32_t m;                 // alive points (written by the select when there is an exclude mask)
  uint32_t k;                 // entries of the inlier list
};

struct PlaneFrame {
  float cx, cy, cz;
};

// the indices whose byte equals `want`
struct PlaneByteIs {
  const uint8_t* b;
  uint8_t want;
  __host__ __device__ bool operator()(const uint32_t& i) const { return (b[i] != 0) == (want != 0); }
};

// the sign rule of k_knn_normals: the component of largest magnitude is positive
__device__ inline void plane_sign(double& v0, double& v1, double& v2) {
  const double a0 = fabs(v0), a1 = fabs(v1), a2 = fabs(v2);
  const double lead = (a0 >= a1 && a0 >= a2) ? v0 : (a1 >= a2 ? v1 : v2);
  if (lead < 0.0) { v0 = -v0; v1 = -v1; v2 = -v2; }
}

// A lane per trial.  alive: the list of alive indices and *m_dev their number, or null: every point is alive and m = n.
__global__ __launch_bounds__(kBlock) void k_plane_candidates(const float4* __restrict__ pos, uint32_t n, const uint32_t* __restrict__ alive,
                                                             const uint32_t* __restrict__ m_dev, PlaneFrame F, uint64_t seed, uint32_t trials,
                                                             PlaneCand* __restrict__ cand) {
  const uint32_t t = blockIdx.x * uint32_t(kBlock) + threadIdx.x;
  if (t >= trials) return;
  const uint64_t m = alive ? uint64_t(*m_dev) : uint64_t(n);
  PlaneCand c{};
  c.n0 = c.n1 = c.n2 = c.d = NAN;                     // an invalid record counts nothing: its residuals are NaN
  c.valid = 0u;
  if (m >= 3) {
    uint64_t s = seed + 3ull * t * 0x9E3779B97F4A7C15ull;
    uint64_t p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = __umul64hi(splitmix64(s), m);           // < m
    if (p[0] != p[1] && p[0] != p[2] && p[1] != p[2]) {
      double q[3][3];
      bool finite = true;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float4 x = pos[alive ? alive[p[a]] : uint32_t(p[a])];
        const float x0 = x.x - F.cx, x1 = x.y - F.cy, x2 = x.z - F.cz;
        finite = finite && isfinite(x0) && isfinite(x1) && isfinite(x2);
        q[a][0] = double(x0); q[a][1] = double(x1); q[a][2] = double(x2);
      }
      const double e1x = q[1][0] - q[0][0], e1y = q[1][1] - q[0][1], e1z = q[1][2] - q[0][2];
      const double e2x = q[2][0] - q[0][0], e2y = q[2][1] - q[0][1], e2z = q[2][2] - q[0][2];
      const double w0 = e1y * e2z - e1z * e2y, w1 = e1z * e2x - e1x * e2z, w2 = e1x * e2y - e1y * e2x;
      const double l2 = (w0 * w0 + w1 * w1) + w2 * w2;
      if (finite && l2 > 0.0 && isfinite(l2)) {
        const double sl = sqrt(l2);
        double v0 = w0 / sl, v1 = w1 / sl, v2 = w2 / sl;
        plane_sign(v0, v1, v2);
        c.n0 = float(v0); c.n1 = float(v1); c.n2 = float(v2);
        c.d = float(-((v0 * q[0][0] + v1 * q[0][1]) + v2 * q[0][2]));
        c.valid = 1u;
      }
    }
  }
  cand[t] = c;
}

// kPlanePts points of a lane, centred; an excluded point and a slot past the cloud are NaN: no residual of theirs passes
__device__ __forceinline__ void plane_load(const float4* __restrict__ pos, const uint8_t* __restrict__ exclude, uint64_t n, uint64_t first,
                                           const PlaneFrame& F, float (&x)[kPlanePts], float (&y)[kPlanePts], float (&z)[kPlanePts]) {
#pragma unroll
  for (int j = 0; j < kPlanePts; ++j) {
    const uint64_t i = first + uint64_t(j) * kBlock + threadIdx.x;
    x[j] = y[j] = z[j] = NAN;
    if (i < n && !(exclude && exclude[i])) {
      const float4 q = pos[i];
      x[j] = q.x - F.cx; y[j] = q.y - F.cy; z[j] = q.z - F.cz;
    }
  }
}

__device__ __forceinline__ float plane_residual(float n0, float n1, float n2, float d, float x, float y, float z) {
  return fmaf(n0, x, fmaf(n1, y, fmaf(n2, z, d)));
}

// The hot path.  grid = (point tiles, candidate batches).  The record index b0 + b is made of blockIdx and a loop counter, so
// the record is read by scalar loads; per (point, candidate) pair that leaves three FMAs and a compare whose result is the
// ballot.  The wave's count goes to LDS once per candidate and tile, the workgroup's to memory once per candidate.
__global__ __launch_bounds__(kBlock) void k_plane_count(const float4* __restrict__ pos, const uint8_t* __restrict__ exclude, uint64_t n,
                                                        PlaneFrame F, float distance, const PlaneCand* __restrict__ cand, uint32_t trials,
                                                        uint32_t* __restrict__ count) {
  __shared__ uint32_t sh[kPlaneBatch];
  const uint32_t b0 = blockIdx.y * uint32_t(kPlaneBatch);
  const uint32_t nb = min(uint32_t(kPlaneBatch), trials - b0);
  if (threadIdx.x < kPlaneBatch) sh[threadIdx.x] = 0u;
  __syncthreads();
  const uint64_t ntiles = (n + kPlaneTile - 1) / kPlaneTile;
  const bool first_lane = (threadIdx.x & 63u) == 0u;
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    float x[kPlanePts], y[kPlanePts], z[kPlanePts];
    plane_load(pos, exclude, n, tile * kPlaneTile, F, x, y, z);
    for (uint32_t b = 0; b < nb; ++b) {
      const PlaneCand c = cand[b0 + b];
      uint32_t wc = 0u;
#pragma unroll
      for (int j = 0; j < kPlanePts; ++j) {
        const float r = plane_residual(c.n0, c.n1, c.n2, c.d, x[j], y[j], z[j]);
        wc += uint32_t(__popcll(__ballot(fabsf(r) <= distance)));
      }
      if (first_lane && wc) atomicAdd(&sh[b], wc);
    }
  }
  __syncthreads();
  if (threadIdx.x < nb && sh[threadIdx.x]) atomicAdd(&count[b0 + threadIdx.x], sh[threadIdx.x]);      // integer counts: no order matters
}

// One workgroup: the largest (count << 32 | ~t) over the valid candidates and the number of valid candidates -> the state.
__global__ __launch_bounds__(kBlock) void k_plane_argmax(const PlaneCand* __restrict__ cand, const uint32_t* __restrict__ count, uint32_t trials,
                                                         PlaneState* __restrict__ S) {
  unsigned long long best = 0ull;
  uint32_t valid = 0u;
  for (uint32_t t = threadIdx.x; t < trials; t += kBlock) {
    if (!cand[t].valid) continue;
    ++valid;
    const unsigned long long key = (unsigned long long)count[t] << 32 | (unsigned long long)(~t);
    best = key > best ? key : best;
  }
  __shared__ unsigned long long shk[kBlock];
  __shared__ uint32_t shv[kBlock];
  shk[threadIdx.x] = best; shv[threadIdx.x] = valid;
  __syncthreads();
  for (int w = kBlock / 2; w > 0; w >>= 1) {
    if (threadIdx.x < unsigned(w)) {
      const unsigned long long o = shk[threadIdx.x + w];
      if (o > shk[threadIdx.x]) shk[threadIdx.x] = o;
      shv[threadIdx.x] += shv[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const unsigned long long key = shk[0];
    S->key = key;
    S->valid_trials = shv[0];
    S->inliers = 0u;
    S->stopped = 0u;
    S->k = 0u;
    if (key) {
      const uint32_t t = ~uint32_t(key);
      const PlaneCand c = cand[t];
      S->trial = int32_t(t);
      S->n0 = c.n0; S->n1 = c.n1; S->n2 = c.n2; S->d = c.d;
    } else {
      S->trial = -1;
      S->n0 = S->n1 = S->n2 = S->d = 0.f;
    }
  }
}

// The inlier bytes of the state's plane (all zero when there is none) and their number.  After a refit that stopped the
// mask and the number stand as they are.
__global__ __launch_bounds__(kBlock) void k_plane_mask(const float4* __restrict__ pos, const uint8_t* __restrict__ exclude, uint64_t n,
                                                       PlaneFrame F, float distance, PlaneState* S, uint8_t* __restrict__ mask) {
  if (S->stopped) return;
  const bool none = S->trial < 0;
  const float n0 = S->n0, n1 = S->n1, n2 = S->n2, d = S->d;
  uint32_t mine = 0u;
  for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    uint8_t in = 0;
    if (!none && !(exclude && exclude[i])) {
      const float4 q = pos[i];
      const float r = plane_residual(n0, n1, n2, d, q.x - F.cx, q.y - F.cy, q.z - F.cz);
      in = fabsf(r) <= distance ? 1 : 0;
    }
    mask[i] = in;
    mine += in;
  }
  __shared__ uint32_t sh[kBlock];
  sh[threadIdx.x] = mine;
  __syncthreads();
  for (int w = kBlock / 2; w > 0; w >>= 1) {
    if (threadIdx.x < unsigned(w)) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0 && sh[0]) atomicAdd(&S->inliers, sh[0]);
}

// A lane per block of kPlaneSumBlock positions of the inlier list: the nine sums of the block from zero, in list order.
__global__ __launch_bounds__(kBlock) void k_plane_moments(const float4* __restrict__ pos, const uint32_t* __restrict__ list, const PlaneState* S,
                                                          PlaneFrame F, uint64_t max_blocks, double* __restrict__ part) {
  if (S->stopped) return;
  const uint64_t k = S->k;
  const uint64_t nblk = (k + kPlaneSumBlock - 1) / kPlaneSumBlock;
  for (uint64_t b = blockIdx.x * (uint64_t)kBlock + threadIdx.x; b < nblk && b < max_blocks; b += (uint64_t)gridDim.x * kBlock) {
    double s[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < kPlaneSumBlock; ++j) {
      const uint64_t at = b * kPlaneSumBlock + uint64_t(j);
      if (at >= k) break;
      const float4 q = pos[list[at]];
      const double x = double(q.x - F.cx), y = double(q.y - F.cy), z = double(q.z - F.cz);
      s[0] += x; s[1] += y; s[2] += z;
      s[3] += x * x; s[4] += x * y; s[5] += x * z; s[6] += y * y; s[7] += y * z; s[8] += z * z;
    }
#pragma unroll
    for (int a = 0; a < 9; ++a) part[b * 9 + a] = s[a];
  }
}

// The block sums in order, nine lanes with one sum each (lane a adds part[9 b + a] over ascending b from zero, so every sum
// keeps the header's order and the loads of a step are one line); then one lane: the covariance as k_knn_normals computes
// it, jacobi3, the new plane into the state.
__global__ __launch_bounds__(64) void k_plane_refit(const double* __restrict__ part, uint64_t max_blocks, PlaneState* S) {
  __shared__ double s[9];
  if (blockIdx.x != 0 || S->stopped) return;
  const uint64_t k = S->k;
  const bool none = S->trial < 0 || k < 3;
  const uint64_t nblk = min((k + kPlaneSumBlock - 1) / kPlaneSumBlock, max_blocks);
  if (!none && threadIdx.x < 9) {
    double acc = 0.0;
#pragma unroll 8
    for (uint64_t b = 0; b < nblk; ++b) acc += part[b * 9 + threadIdx.x];
    s[threadIdx.x] = acc;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (none) { S->stopped = 1u; return; }
  const double kk = double(k);
  const double m0 = s[0] / kk, m1 = s[1] / kk, m2 = s[2] / kk;
  double C[3][3], V[3][3];
  C[0][0] = s[3] / kk - m0 * m0; C[0][1] = s[4] / kk - m0 * m1; C[0][2] = s[5] / kk - m0 * m2;
  C[1][1] = s[6] / kk - m1 * m1; C[1][2] = s[7] / kk - m1 * m2; C[2][2] = s[8] / kk - m2 * m2;
  C[1][0] = C[0][1]; C[2][0] = C[0][2]; C[2][1] = C[1][2];
  const double tr = (C[0][0] + C[1][1]) + C[2][2];
  if (!(tr > 0.0)) { S->stopped = 1u; return; }
  jacobi3(C, V);
  int best = 0;
  if (C[1][1] < C[0][0]) best = 1;
  if (C[2][2] < (best == 0 ? C[0][0] : C[1][1])) best = 2;
  double v0 = best == 0 ? V[0][0] : (best == 1 ? V[0][1] : V[0][2]);
  double v1 = best == 0 ? V[1][0] : (best == 1 ? V[1][1] : V[1][2]);
  double v2 = best == 0 ? V[2][0] : (best == 1 ? V[2][1] : V[2][2]);
  const double nv = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
  v0 /= nv; v1 /= nv; v2 /= nv;
  plane_sign(v0, v1, v2);
  S->n0 = float(v0); S->n1 = float(v1); S->n2 = float(v2);
  S->d = float(-((v0 * m0 + v1 * m1) + v2 * m2));
  S->inliers = 0u;                                    // k_plane_mask counts them again
}

}  // namespace s4p_nrm

namespace {

using PlaneCounting = hipcub::CountingInputIterator<uint32_t>;

int32_t plane_select(s4p_normals_ctx* h, void* tmp, size_t& bytes, const uint8_t* flag, uint8_t want, uint32_t* list, uint32_t* num, uint64_t un) {
  NRM_HIP(hipcub::DeviceSelect::If(tmp, bytes, PlaneCounting(0u), list, num, int(un), PlaneByteIs{flag, want}, h->st));
  return S4P_NORMALS_OK;
}

int32_t plane_impl(s4p_normals_ctx* h, const s4p_plane_options* o, const uint8_t* exclude, s4p_plane_result* result, uint8_t* inlier,
                   bool device) {
  if (!h) return S4P_NORMALS_ERR_BAD_ARG;
  if (!h->has_cloud) return fail(h, S4P_NORMALS_ERR_STATE, "plane_segment: set_cloud first");
  if (!o || !result || !inlier) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "plane_segment: null options, result or inlier");
  if (!std::isfinite(o->distance) || !(o->distance >= 0.f))
    return fail(h, S4P_NORMALS_ERR_BAD_ARG, "plane_segment: distance must be finite and >= 0");
  if (o->trials < 1 || o->trials > S4P_PLANE_MAX_TRIALS) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "plane_segment: trials must be in [1, 2^20]");
  if (o->refine < 0 || o->refine > S4P_PLANE_MAX_REFINE) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "plane_segment: refine must be in [0, 16]");
  NRM_HIP(hipSetDevice(h->device));
  const uint64_t un = uint64_t(h->n);
  const uint32_t trials = uint32_t(o->trials);
  PlaneFrame F;
  F.cx = 0.5f * h->lo[0] + 0.5f * h->hi[0];
  F.cy = 0.5f * h->lo[1] + 0.5f * h->hi[1];
  F.cz = 0.5f * h->lo[2] + 0.5f * h->hi[2];
  size_t sel_bytes = 0;
  if (int32_t rc = plane_select(h, nullptr, sel_bytes, nullptr, 0, nullptr, nullptr, un)) return rc;
  const uint64_t max_blocks = (un + kPlaneSumBlock - 1) / kPlaneSumBlock;
  PlaneCand* cand = nullptr;
  uint32_t *count = nullptr, *list = nullptr;
  PlaneState* S = nullptr;
  void* sel_tmp = nullptr;
  double* part = nullptr;
  uint8_t* dmask = inlier;
  const uint8_t* dex = exclude;
  uint8_t* dex_own = nullptr;
  if (int32_t rc = arena_layout(h, "plane_segment", [&](Arena& ar) {
        cand = ar.take<PlaneCand>(trials);
        count = ar.take<uint32_t>(trials);
        S = ar.take<PlaneState>(1);
        list = ar.take<uint32_t>(un);
        sel_tmp = ar.take<char>(sel_bytes);
        part = ar.take<double>(o->refine > 0 ? 9 * max_blocks : 1);
        if (!device) {
          dmask = ar.take<uint8_t>(un);
          if (exclude) dex_own = ar.take<uint8_t>(un);
        }
      })) return rc;
  if (!device && exclude) {
    NRM_HIP(hipMemcpyAsync(dex_own, exclude, un, hipMemcpyHostToDevice, h->st));
    dex = dex_own;
  }
  NRM_HIP(hipMemsetAsync(S, 0, sizeof(PlaneState), h->st));
  NRM_HIP(hipMemsetAsync(count, 0, size_t(trials) * 4, h->st));
  if (dex) {
    size_t bytes = sel_bytes;
    if (int32_t rc = plane_select(h, sel_tmp, bytes, dex, 0, list, &S->m, un)) return rc;
  }
  hipLaunchKernelGGL(k_plane_candidates, dim3((trials + kBlock - 1) / kBlock), dim3(kBlock), 0, h->st, (const float4*)h->pos, uint32_t(un),
                     (const uint32_t*)(dex ? list : nullptr), (const uint32_t*)(dex ? &S->m : nullptr), F, uint64_t(o->seed), trials, cand);
  NRM_HIP(hipGetLastError());
  const uint64_t ntiles = (un + kPlaneTile - 1) / kPlaneTile;
  const dim3 cgrid(unsigned(std::min<uint64_t>(ntiles, kPlaneMaxTiles)), (trials + kPlaneBatch - 1) / kPlaneBatch);
  hipLaunchKernelGGL(k_plane_count, cgrid, dim3(kBlock), 0, h->st, (const float4*)h->pos, dex, un, F, o->distance, (const PlaneCand*)cand, trials,
                     count);
  NRM_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_plane_argmax, dim3(1), dim3(kBlock), 0, h->st, (const PlaneCand*)cand, (const uint32_t*)count, trials, S);
  NRM_HIP(hipGetLastError());
  const int nb = blocks_for(h->n);
  hipLaunchKernelGGL(k_plane_mask, dim3(nb), dim3(kBlock), 0, h->st, (const float4*)h->pos, dex, un, F, o->distance, S, dmask);
  NRM_HIP(hipGetLastError());
  for (int32_t r = 0; r < o->refine; ++r) {
    size_t bytes = sel_bytes;
    if (int32_t rc = plane_select(h, sel_tmp, bytes, dmask, 1, list, &S->k, un)) return rc;
    hipLaunchKernelGGL(k_plane_moments, dim3(blocks_for(int64_t(max_blocks))), dim3(kBlock), 0, h->st, (const float4*)h->pos, (const uint32_t*)list,
                       (const PlaneState*)S, F, max_blocks, part);
    NRM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_plane_refit, dim3(1), dim3(64), 0, h->st, (const double*)part, max_blocks, S);
    NRM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_plane_mask, dim3(nb), dim3(kBlock), 0, h->st, (const float4*)h->pos, dex, un, F, o->distance, S, dmask);
    NRM_HIP(hipGetLastError());
  }
  PlaneState hs{};
  NRM_HIP(hipMemcpyAsync(&hs, S, sizeof(hs), hipMemcpyDeviceToHost, h->st));
  if (!device) NRM_HIP(hipMemcpyAsync(inlier, dmask, un, hipMemcpyDeviceToHost, h->st));
  NRM_HIP(hipStreamSynchronize(h->st));
  std::memset(result, 0, sizeof(*result));
  result->centre[0] = F.cx; result->centre[1] = F.cy; result->centre[2] = F.cz;
  result->alive = dex ? int64_t(hs.m) : h->n;
  result->trial = hs.trial;
  result->valid_trials = int32_t(hs.valid_trials);
  if (hs.trial >= 0) {
    result->normal[0] = hs.n0; result->normal[1] = hs.n1; result->normal[2] = hs.n2;
    result->d_centred = hs.d;
    result->d = float(double(hs.d) - ((double(hs.n0) * double(F.cx) + double(hs.n1) * double(F.cy)) + double(hs.n2) * double(F.cz)));
    result->inliers = int64_t(hs.inliers);
  }
  return S4P_NORMALS_OK;
}

}  // namespace

extern "C" {

int32_t s4p_plane_segment(s4p_normals_ctx* h, const s4p_plane_options* options, const uint8_t* exclude, s4p_plane_result* result,
                          uint8_t* inlier) {
  return plane_impl(h, options, exclude, result, inlier, false);
}
int32_t s4p_plane_segment_device(s4p_normals_ctx* h, const s4p_plane_options* options, const uint8_t* exclude, s4p_plane_result* result,
                                 uint8_t* inlier) {
  return plane_impl(h, options, exclude, result, inlier, true);
}

}  // extern "C"
