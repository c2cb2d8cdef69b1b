// s4p_icp_k_pass.hip.hpp -- the kernels of a pass: the fused k_match / k_match_plane, and the split passes' k_search,
// k_reject, the selection (k_key_hist, k_key_digit), the sum kernels (k_wsum, k_gicp_sum, k_symm_sum, k_info_sum, k_color_sum), the final sums and
// k_reject_out.  Every sum kernel ends in block_row and every final sum is slab_total's order (s4p_icp_k_common.hip.hpp).
//
// The measured kernels are pinned instruction for instruction ("ICP sources: layout").  What a change here can
// move without touching a kernel's own code: a kernel's code ends with the padding up to the next one, so the last kernel
// of the code object differs from one that is followed.  Non-template kernels are emitted in the order of their
// definitions and k_final_plane is the last of them; template kernels follow in the order of their first launch in the
// host parts, and k_match<false> is the last of those in these parts (s4p_icp_pass.inc); the kernels of s4p_icp_k_batch.hip.hpp
// are launched from a later part and follow it.
#pragma once

namespace s4p_icp {

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
  block_row<S4P_ICP_NSUMS, kPitch>(s, A.slab);
}

// the slab's nb rows -> 17 sums, in a fixed order: 15 parts per column (rows part, part + 15, ...), then the parts in order
__global__ __launch_bounds__(kBlock) void k_final(const double* slab, int nb, double* out) {
  slab_total<S4P_ICP_NSUMS, kPitch>(slab, nb, out);
}

// ---------------------------------------------------------------------------------------------------------------------
// robust ICP (include/s4p_icp_robust.h).  Per iteration: k_search (the one correspondence search: winner slot and residual
// key per visited lane), the radix select of the keys (k_key_hist + k_key_digit per 8-bit digit, integer atomics only, the
// digit decisions on the device), k_wsum (weighted sums streamed from the slots, k_match / k_match_plane's lane order and
// reduction) and k_wfinal (k_final / k_final_plane's fixed order, plus the count with w > 0 and the info).

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
  }
  block_row<S4P_ICP_PLANE_NSUMS, kPlanePitch>(s, A.slab);
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
    const float d2 = winner_d2(x, y, z, p);
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
  block_row<NS, kPlanePitch>(s, A.slab);
}

struct SymmArgs {
  Tf T;
  GridDev g;
  const float4* src;
  const float4* snrm;       // the order of src
  const float4* nrm;        // cell order, as g.tgt
  uint64_t n;
  const uint32_t* slot;     // k_search's
  double* slab;             // one kPlanePitch row per workgroup
};

// The symmetric sums, term by term as include/s4p_icp_symm.h states them: k_match_plane's shape with n = np +- nh (both
// normals on one side) and a = (q^ + p') x n.  No search: the winner comes from k_search's slot.
__global__ __launch_bounds__(kBlock) void k_symm_sum(SymmArgs A) {
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
    const float d2 = winner_d2(x, y, z, p);
    s[0] += 1.0;
    s[1] += double(d2);
    const float4 nf = A.nrm[sl], mf = A.snrm[j];
    const double np[3] = {double(nf.x), double(nf.y), double(nf.z)}, mq[3] = {double(mf.x), double(mf.y), double(mf.z)};
    double nh[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) nh[a] = (double(A.T.m[4 * a]) * mq[0] + double(A.T.m[4 * a + 1]) * mq[1]) + double(A.T.m[4 * a + 2]) * mq[2];
    const double dot = (np[0] * nh[0] + np[1] * nh[1]) + np[2] * nh[2];
    const bool flip = dot < 0.0;
    const double nd[3] = {flip ? np[0] - nh[0] : np[0] + nh[0], flip ? np[1] - nh[1] : np[1] + nh[1], flip ? np[2] - nh[2] : np[2] + nh[2]};
    if (nd[0] == 0.0 && nd[1] == 0.0 && nd[2] == 0.0) continue;
    const double u[3] = {double(x), double(y), double(z)}, v[3] = {double(p.x), double(p.y), double(p.z)};
    const double e[3] = {v[0] - u[0], v[1] - u[1], v[2] - u[2]}, h[3] = {u[0] + v[0], u[1] + v[1], u[2] + v[2]};
    const double a[6] = {h[1] * nd[2] - h[2] * nd[1], h[2] * nd[0] - h[0] * nd[2], h[0] * nd[1] - h[1] * nd[0], nd[0], nd[1], nd[2]};
    const double r = (e[0] * nd[0] + e[1] * nd[1]) + e[2] * nd[2];
    s[2] += 1.0;
    s[3] += r * r;
    int o = 4;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int k = i; k < 6; ++k) s[o++] += a[i] * a[k];
#pragma unroll
    for (int i = 0; i < 6; ++i) s[25 + i] += a[i] * r;
  }
  block_row<NS, kPlanePitch>(s, A.slab);
}

struct InfoArgs {
  Tf T;
  const float4* src;
  const float4* tgt;        // cell order: the winner of lane j is tgt[slot[j]]
  uint64_t n;
  const uint32_t* slot;     // k_search's
  double* slab;             // one kPlanePitch row per workgroup (11 used)
};

// The information sums, term by term as include/s4p_icp_info.h states them: n, sum d2, sum p', the upper triangle of
// sum p' p'^T over the winners.  No search: the winner comes from k_search's slot; q^ is recomputed for the contract's d2.
__global__ __launch_bounds__(kBlock) void k_info_sum(InfoArgs A) {
  constexpr int NS = S4P_ICP_INFO_NSUMS;
  double s[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) s[k] = 0.0;
  for (uint64_t j = blockIdx.x * (uint64_t)kBlock + threadIdx.x; j < A.n; j += (uint64_t)gridDim.x * kBlock) {
    const uint32_t sl = A.slot[j];
    if (sl == kNoSlot) continue;
    const float4 q = A.src[j];
    float x, y, z;
    apply_t(A.T, q.x, q.y, q.z, x, y, z);
    const float4 p = A.tgt[sl];
    const float d2 = winner_d2(x, y, z, p);
    const double pd[3] = {double(p.x), double(p.y), double(p.z)};
    s[0] += 1.0;
    s[1] += double(d2);
    int o = 5;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      s[2 + a] += pd[a];
#pragma unroll
      for (int b = a; b < 3; ++b) s[o++] += pd[a] * pd[b];                  // exact products (24 + 24 bits)
    }
  }
  block_row<NS, kPlanePitch>(s, A.slab);
}

// the plane slab's nb rows -> 11 information sums, in a fixed order: 23 parts per column (rows part, part + 23, ...), then
// the parts in order
__global__ __launch_bounds__(kBlock) void k_final_info(const double* slab, int nb, double* out) {
  slab_total<S4P_ICP_INFO_NSUMS, kPlanePitch>(slab, nb, out);
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
    const float d2 = winner_d2(x, y, z, p);
    s[0] += 1.0;
    s[1] += double(d2);
    const float4 nf = A.nrm[sl];
    if (is_zero(nf)) continue;
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
  block_row<NS, kPlanePitch>(s, A.slab);
}

// the plane slab's nb rows -> 31 sums, in a fixed order: 8 parts per column (rows part, part + 8, ...), then the parts in order
__global__ __launch_bounds__(kBlock) void k_final_plane(const double* slab, int nb, double* out) {
  slab_total<S4P_ICP_PLANE_NSUMS, kPlanePitch>(slab, nb, out);
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
        if (!is_zero(nf)) {
          const double qd[3] = {double(x), double(y), double(z)}, nd[3] = {double(nf.x), double(nf.y), double(nf.z)};
          const double r = plane_residual(p, qd, nd);
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
      const bool info = !is_zero(nf) && !is_zero(mf);
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
    const float d2 = winner_d2(x, y, z, p);
    const double qd[3] = {double(x), double(y), double(z)};
    if (PLANE) {
      const float4 nf = A.nrm[sl];
      if (is_zero(nf)) {        // no key: counted as in k_match_plane
        s[0] += 1.0;
        s[1] += double(d2);
        s[NS] += 1.0;
        continue;
      }
      const double nd[3] = {double(nf.x), double(nf.y), double(nf.z)};
      const double a[6] = {qd[1] * nd[2] - qd[2] * nd[1], qd[2] * nd[0] - qd[0] * nd[2], qd[0] * nd[1] - qd[1] * nd[0], nd[0], nd[1], nd[2]};
      const double r = plane_residual(p, qd, nd);
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
  block_row<NC, kRowPitch>(s, A.slab);
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

}  // namespace s4p_icp
