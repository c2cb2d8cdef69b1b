// s4p_icp_k_batch.hip.hpp -- the kernels of a batched pass (include/s4p_icp_batch.h): k_match_batch and k_final_batch.  The
// poses of a batch share the target grid, the source and the normals; a pose is one row of workgroups (blockIdx.y), not a
// loop inside a lane: nothing but the 16 bytes of the source point would be shared, and the 2-D grid runs side by side what
// such a loop would serialise.  Workgroups are dispatched x-major, so one pose's workgroups walk neighbouring target cells.
//
// Included after the existing parts: the kernels here are instantiated last, so they follow k_match<false> in the code
// object (s4p_icp_k_pass.hip.hpp has the rule; DESIGN.md, "Batched multi-start ICP", has what that moved).
#pragma once

namespace s4p_icp {

// What one upload per iteration carries: the transform of every pose of the call and the poses still iterating.
struct BatchPoses {
  Tf T[S4P_ICP_BATCH_MAX];                // by pose
  int32_t active[S4P_ICP_BATCH_MAX];      // by row of the launch (blockIdx.y): the pose
};

struct MatchBatchArgs {
  const BatchPoses* poses;
  GridDev g;
  const float4* src;        // w = original source index (bits)
  const float4* nrm;        // PLANE: cell order, as g.tgt
  uint64_t n;
  float d2max;
  double* slab;             // [pose][kMaxBlocks] rows of kPitch (point) / kPlanePitch (plane)
};

// k_match<false> (point) or k_match_plane (plane) for the pose of this row of workgroups: the same grid in x, the same lane
// for every source point, the same expressions in the same order, block_row into the pose's part of the slab -- so the
// pose's slab rows hold the bits the single kernel writes.  The pose and its transform are read through blockIdx.y alone:
// uniform over the workgroup, so they sit in scalar registers.
template <bool PLANE>
__global__ __launch_bounds__(kBlock) void k_match_batch(MatchBatchArgs A) {
  constexpr int NS = PLANE ? S4P_ICP_PLANE_NSUMS : S4P_ICP_NSUMS;
  constexpr int kRowPitch = PLANE ? kPlanePitch : kPitch;
  const int pose = A.poses->active[blockIdx.y];
  const Tf T = A.poses->T[pose];
  double s[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) s[k] = 0.0;
  for (uint64_t j = blockIdx.x * (uint64_t)kBlock + threadIdx.x; j < A.n; j += (uint64_t)gridDim.x * kBlock) {
    const float4 q = A.src[j];
    float x, y, z;
    apply_t(T, q.x, q.y, q.z, x, y, z);
    float best;
    uint32_t bi, slot;
    float4 p;
    if (PLANE) {
      nearest_t<true>(A.g, x, y, z, A.d2max, best, bi, p, slot);
      if (bi == 0xFFFFFFFFu) continue;
      s[0] += 1.0;
      s[1] += double(best);
      const float4 nf = A.nrm[slot];
      if (is_zero(nf)) continue;
      const double qd[3] = {double(x), double(y), double(z)}, nd[3] = {double(nf.x), double(nf.y), double(nf.z)};
      const double a[6] = {qd[1] * nd[2] - qd[2] * nd[1], qd[2] * nd[0] - qd[0] * nd[2], qd[0] * nd[1] - qd[1] * nd[0], nd[0], nd[1], nd[2]};
      const double r = plane_residual(p, qd, nd);
      s[2] += 1.0;
      s[3] += r * r;
      int o = 4;
#pragma unroll
      for (int u = 0; u < 6; ++u)
#pragma unroll
        for (int v = u; v < 6; ++v) s[o++] += a[u] * a[v];
#pragma unroll
      for (int u = 0; u < 6; ++u) s[25 + u] += a[u] * r;
    } else {
      nearest(A.g, x, y, z, A.d2max, best, bi, p);
      if (bi != 0xFFFFFFFFu) {
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
  }
  block_row<NS, kRowPitch>(s, A.slab + uint64_t(pose) * kMaxBlocks * kRowPitch);
}

// One workgroup per row of the launch: slab_total (k_final's / k_final_plane's order) over the pose's nb slab rows, into
// row blockIdx.x of the sums, so that the rows of the poses still iterating are contiguous for the one read-back.
template <bool PLANE>
__global__ __launch_bounds__(kBlock) void k_final_batch(const BatchPoses* poses, const double* slab, int nb, double* out) {
  constexpr int NS = PLANE ? S4P_ICP_PLANE_NSUMS : S4P_ICP_NSUMS;
  constexpr int kRowPitch = PLANE ? kPlanePitch : kPitch;
  const int pose = poses->active[blockIdx.x];
  slab_total<NS, kRowPitch>(slab + uint64_t(pose) * kMaxBlocks * kRowPitch, nb, out + uint64_t(blockIdx.x) * NS);
}

}  // namespace s4p_icp
