// s4p_voxel.inc -- voxel-grid downsampling of libsuper4pcs_normals.so (include/s4p_voxel.h, DESIGN.md section "Voxel-grid
// downsampling and multi-scale ICP").  Included by s4p_normals.hip after s4p_knn.inc: the functions use the context's
// device, stream, arena and error string, and leave its cloud and grid alone.
//
// Device path:
//   k_pack (SoA -> float4) -> k_voxel_bounds (per-block minima / maxima of the finite points; the host turns them into
//   index bounds, floor(x / v) being monotone in x, and checks the extents) -> k_voxel_keys ((iz - iz0) << 42 |
//   (iy - iy0) << 21 | (ix - ix0), all ones for a dropped point) -> radix sort of (key, index) over the bits the extents
//   need (stable: members in ascending index) -> k_voxel_heads + inclusive scan (row numbers, m) -> k_voxel_runs (run
//   begins, voxel_of through the sorted index) -> k_voxel_reduce<NA>: one lane per voxel, runs of at most 64 members summed
//   in place.  Longer runs: k_voxel_segs + exclusive scan (64-member blocks per long run) -> k_voxel_partials<NA>: one lane
//   per block, its sum into the arena -> k_voxel_long: one lane per (long voxel, channel) adds the blocks' sums in order.
//   Both read the number of blocks from the scan's last entry on the device and are launched for its upper bound, so the
//   host waits twice per call (bounds, m) and not a third time; without long runs their lanes leave at once.
// The order of the additions is the header's; there are no atomics at all.
#include <cstdio>

#include "s4p_voxel.h"

namespace s4p_nrm {

constexpr uint32_t kVoxBlock = S4P_VOXEL_BLOCK;
constexpr uint64_t kVoxDropped = ~0ull;

struct VoxGrid {
  double v;                   // the voxel edge
  double i0[3];               // smallest index of the finite points per axis (integer-valued)
};

__host__ __device__ inline double voxel_coord(float x, double v) { return floor(double(x) / v); }

// packed voxel key of every point (offsets from the smallest index, 21 bits per axis); a dropped point gets all ones
__global__ __launch_bounds__(kBlock) void k_voxel_keys(const float4* p, uint64_t n, VoxGrid g, uint64_t* keys, uint32_t* vals) {
  for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    const float4 q = p[i];
    uint64_t key = kVoxDropped;
    if (isfinite(q.x) && isfinite(q.y) && isfinite(q.z)) {
      const uint64_t ox = uint64_t(voxel_coord(q.x, g.v) - g.i0[0]);
      const uint64_t oy = uint64_t(voxel_coord(q.y, g.v) - g.i0[1]);
      const uint64_t oz = uint64_t(voxel_coord(q.z, g.v) - g.i0[2]);
      key = oz << 42 | oy << 21 | ox;
    }
    keys[i] = key;
    vals[i] = uint32_t(i);
  }
}

// 1 where a run of equal keys begins (dropped points begin none)
__global__ __launch_bounds__(kBlock) void k_voxel_heads(const uint64_t* keys, uint64_t n, uint32_t* flags) {
  for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    const uint64_t key = keys[i];
    flags[i] = (key != kVoxDropped && (i == 0 || keys[i - 1] != key)) ? 1u : 0u;
  }
}

// rows1 = the inclusive scan of the flags: position i belongs to row rows1[i] - 1.  begin[r] = the first position of row r,
// begin[m] = the number of kept points; voxel_of through the sorted index.
__global__ __launch_bounds__(kBlock) void k_voxel_runs(const uint64_t* keys, const uint32_t* order, const uint32_t* rows1, uint64_t n,
                                                       uint32_t* begin, int32_t* voxel_of) {
  for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    const uint64_t key = keys[i];
    const bool kept = key != kVoxDropped;
    if (kept) {
      const uint32_t r = rows1[i] - 1u;
      if (i == 0 || keys[i - 1] != key) begin[r] = uint32_t(i);
      if (i + 1 == n || keys[i + 1] == kVoxDropped) begin[r + 1] = uint32_t(i + 1);
      if (voxel_of) voxel_of[order[i]] = int32_t(r);
    } else if (voxel_of) {
      voxel_of[order[i]] = -1;
    }
  }
}

// blocks of kVoxBlock members per long run (0 for a run that one lane sums in place); nseg[m] = 0 closes the scan
__global__ __launch_bounds__(kBlock) void k_voxel_segs(const uint32_t* begin, uint32_t m, uint32_t* nseg) {
  for (uint64_t r = blockIdx.x * (uint64_t)kBlock + threadIdx.x; r <= m; r += (uint64_t)gridDim.x * kBlock) {
    uint32_t s = 0;
    if (r < m) {
      const uint32_t c = begin[r + 1] - begin[r];
      if (c > kVoxBlock) s = (c + kVoxBlock - 1) / kVoxBlock;
    }
    nseg[r] = s;
  }
}

struct VoxReduce {
  const float4* pos;          // the cloud in the caller's order
  const float* attr;          // n * nattr interleaved, or null
  const uint32_t* order;      // the sorted index
  const uint32_t* begin;      // m + 1 run begins
  uint32_t m;
  const uint32_t* segoff;     // m + 1: first block of every long run; segoff[m] = the blocks of all long runs
  uint32_t max_seg;           // what the arena holds: at least n / 64 + n / 65 blocks
  double* partial;            // block sums, 3 + nattr per block
  uint32_t* segrow;           // the run of every block
  int32_t nattr;
  float* out_xyz;
  float* out_attr;
  int32_t* out_count;
};

// the sequential sum of the members at the sorted positions [b, e), b < e, per channel: the first value, then += in order
template <int NA>
__device__ __forceinline__ void voxel_block_sum(const VoxReduce& A, uint32_t b, uint32_t e, double (&acc)[3 + NA]) {
  {
    const uint32_t j = A.order[b];
    const float4 q = A.pos[j];
    acc[0] = double(q.x); acc[1] = double(q.y); acc[2] = double(q.z);
#pragma unroll
    for (int a = 0; a < NA; ++a) acc[3 + a] = double(A.attr[uint64_t(j) * NA + a]);
  }
  for (uint32_t s = b + 1; s < e; ++s) {
    const uint32_t j = A.order[s];
    const float4 q = A.pos[j];
    acc[0] += double(q.x); acc[1] += double(q.y); acc[2] += double(q.z);
#pragma unroll
    for (int a = 0; a < NA; ++a) acc[3 + a] += double(A.attr[uint64_t(j) * NA + a]);
  }
}

// one lane per voxel: the count, and the means of a run of at most kVoxBlock members
template <int NA>
__global__ __launch_bounds__(kBlock) void k_voxel_reduce(VoxReduce A) {
  for (uint64_t r = blockIdx.x * (uint64_t)kBlock + threadIdx.x; r < A.m; r += (uint64_t)gridDim.x * kBlock) {
    const uint32_t b = A.begin[r], e = A.begin[r + 1];
    const uint32_t c = e - b;
    if (A.out_count) A.out_count[r] = int32_t(c);
    if (c > kVoxBlock) continue;
    double acc[3 + NA];
    voxel_block_sum<NA>(A, b, e, acc);
    const double dc = double(c);
    A.out_xyz[3 * r] = float(acc[0] / dc); A.out_xyz[3 * r + 1] = float(acc[1] / dc); A.out_xyz[3 * r + 2] = float(acc[2] / dc);
#pragma unroll
    for (int a = 0; a < NA; ++a) A.out_attr[r * NA + a] = float(acc[3 + a] / dc);
  }
}

// one lane per block of a long run: its sum into partial[block]
template <int NA>
__global__ __launch_bounds__(kBlock) void k_voxel_partials(VoxReduce A) {
  const uint32_t nseg = min(A.segoff[A.m], A.max_seg);
  for (uint64_t s = blockIdx.x * (uint64_t)kBlock + threadIdx.x; s < nseg; s += (uint64_t)gridDim.x * kBlock) {
    // the run of block s: the last r with segoff[r] <= s (runs without blocks repeat their successor's offset)
    uint32_t lo = 0, hi = A.m;                   // segoff[lo] <= s < segoff[hi] (segoff[m] = nseg)
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (A.segoff[mid] <= uint32_t(s)) lo = mid; else hi = mid;
    }
    const uint32_t blk = uint32_t(s) - A.segoff[lo];
    const uint32_t end = A.begin[lo + 1];
    const uint32_t b = A.begin[lo] + blk * kVoxBlock;
    const uint32_t e = end - b > kVoxBlock ? b + kVoxBlock : end;
    double acc[3 + NA];
    voxel_block_sum<NA>(A, b, e, acc);
#pragma unroll
    for (int k = 0; k < 3 + NA; ++k) A.partial[s * (3 + NA) + k] = acc[k];
    A.segrow[s] = lo;
  }
}

// one lane per (block, channel); the lanes of a long run's first block add its block sums in order and write the mean, the
// others leave: only long runs cost anything, however many voxels there are
__global__ __launch_bounds__(kBlock) void k_voxel_long(VoxReduce A) {
  const uint32_t C = 3u + uint32_t(A.nattr);
  const uint64_t total = uint64_t(min(A.segoff[A.m], A.max_seg)) * C;
  for (uint64_t t = blockIdx.x * (uint64_t)kBlock + threadIdx.x; t < total; t += (uint64_t)gridDim.x * kBlock) {
    const uint32_t s0 = uint32_t(t / C);
    const uint32_t k = uint32_t(t - uint64_t(s0) * C);
    const uint64_t r = A.segrow[s0];
    if (A.segoff[r] != s0) continue;
    const uint32_t c = A.begin[r + 1] - A.begin[r];
    const uint32_t s1 = A.segoff[r + 1];
    double S = A.partial[uint64_t(s0) * C + k];
    for (uint32_t s = s0 + 1; s < s1; ++s) S += A.partial[uint64_t(s) * C + k];
    const float mean = float(S / double(c));
    if (k < 3) A.out_xyz[3 * r + k] = mean;
    else A.out_attr[r * uint64_t(A.nattr) + (k - 3)] = mean;
  }
}

}  // namespace s4p_nrm

namespace {

template <int NA>
void voxel_launch(s4p_normals_ctx* h, const VoxReduce& A, bool partials) {
  if (partials) hipLaunchKernelGGL(k_voxel_partials<NA>, dim3(blocks_for(int64_t(A.max_seg))), dim3(kBlock), 0, h->st, A);
  else hipLaunchKernelGGL(k_voxel_reduce<NA>, dim3(blocks_for(int64_t(A.m))), dim3(kBlock), 0, h->st, A);
}

void voxel_dispatch(s4p_normals_ctx* h, const VoxReduce& A, bool partials) {
  switch (A.nattr) {
    case 0: voxel_launch<0>(h, A, partials); break;
    case 1: voxel_launch<1>(h, A, partials); break;
    case 2: voxel_launch<2>(h, A, partials); break;
    case 3: voxel_launch<3>(h, A, partials); break;
    case 4: voxel_launch<4>(h, A, partials); break;
    case 5: voxel_launch<5>(h, A, partials); break;
    case 6: voxel_launch<6>(h, A, partials); break;
    case 7: voxel_launch<7>(h, A, partials); break;
    default: voxel_launch<8>(h, A, partials); break;
  }
}

int32_t voxel_impl(s4p_normals_ctx* h, const float* x, const float* y, const float* z, int64_t n, float voxel, const float* attr,
                   int32_t nattr, float* out_xyz, float* out_attr, int32_t* out_count, int32_t* voxel_of, int64_t* m_out, bool device) {
  if (!h) return S4P_NORMALS_ERR_BAD_ARG;
  if (n < 1 || n > kMaxPoints) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "voxel_downsample: n must be in [1, 2^31 - 2]");
  if (!std::isfinite(voxel) || !(voxel > 0.f)) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "voxel_downsample: voxel must be finite and > 0");
  if (nattr < 0 || nattr > S4P_VOXEL_MAX_ATTR) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "voxel_downsample: nattr must be in [0, 8]");
  if (!x || !y || !z || !out_xyz || !m_out) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "voxel_downsample: null argument");
  if ((nattr == 0) != (attr == nullptr) || (nattr == 0) != (out_attr == nullptr))
    return fail(h, S4P_NORMALS_ERR_BAD_ARG, "voxel_downsample: attr and out_attr must be null exactly when nattr == 0");
  NRM_HIP(hipSetDevice(h->device));
  const uint64_t un = uint64_t(n);
  const size_t na = size_t(nattr), C = 3 + na;
  const int nb = blocks_for(n);
  const size_t max_seg = size_t(un / 32 + 2);               // blocks of all runs longer than 64: at most n / 64 + n / 65

  uint64_t* nokey = nullptr;
  uint32_t* noval = nullptr;
  size_t sort_bytes = 0, scan_bytes = 0, scan2_bytes = 0;
  NRM_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (const uint64_t*)nokey, nokey, (const uint32_t*)noval, noval, int(un), 0, 64,
                                             h->st));
  NRM_HIP(hipcub::DeviceScan::InclusiveSum(nullptr, scan_bytes, (const uint32_t*)noval, noval, int(un), h->st));
  NRM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan2_bytes, (const uint32_t*)noval, noval, int(un + 1), h->st));
  const size_t tmp_bytes = std::max(sort_bytes, std::max(scan_bytes, scan2_bytes));

  float *stage[3] = {nullptr, nullptr, nullptr}, *stage_attr = nullptr;      // host form: device copies of the caller's arrays
  float *d_xyz = out_xyz, *d_attr = out_attr, *rows = nullptr;
  int32_t *d_count = out_count, *d_vof = voxel_of;
  float4* pos = nullptr;
  uint64_t *keys = nullptr, *keys2 = nullptr;
  uint32_t *vals = nullptr, *order = nullptr, *flags = nullptr, *rows1 = nullptr, *begin = nullptr, *nseg = nullptr, *segoff = nullptr, *segrow = nullptr;
  double* partial = nullptr;
  void* tmp = nullptr;
  if (int32_t rc = arena_layout(h, "voxel_downsample", [&](Arena& ar) {
        if (!device) {
          for (int a = 0; a < 3; ++a) stage[a] = ar.take<float>(un);
          if (nattr > 0) stage_attr = ar.take<float>(un * na);
          d_xyz = ar.take<float>(3 * un);
          if (nattr > 0) d_attr = ar.take<float>(un * na);
          if (out_count) d_count = ar.take<int32_t>(un);
          if (voxel_of) d_vof = ar.take<int32_t>(un);
        }
        pos = ar.take<float4>(un);
        rows = ar.take<float>(size_t(nb) * 6);
        keys = ar.take<uint64_t>(un);
        keys2 = ar.take<uint64_t>(un);
        vals = ar.take<uint32_t>(un);
        order = ar.take<uint32_t>(un);
        flags = ar.take<uint32_t>(un);
        rows1 = ar.take<uint32_t>(un);
        begin = ar.take<uint32_t>(un + 1);
        nseg = ar.take<uint32_t>(un + 1);
        segoff = ar.take<uint32_t>(un + 1);
        partial = ar.take<double>(max_seg * C);
        segrow = ar.take<uint32_t>(max_seg);
        tmp = ar.take<char>(tmp_bytes);
      })) return rc;
  const float* in[3] = {x, y, z};
  const float* dattr = attr;
  if (!device) {
    for (int a = 0; a < 3; ++a) {
      NRM_HIP(hipMemcpyAsync(stage[a], in[a], un * sizeof(float), hipMemcpyHostToDevice, h->st));
      in[a] = stage[a];
    }
    if (nattr > 0) {
      NRM_HIP(hipMemcpyAsync(stage_attr, attr, un * na * sizeof(float), hipMemcpyHostToDevice, h->st));
      dattr = stage_attr;
    }
  }

  hipLaunchKernelGGL(k_pack, dim3(nb), dim3(kBlock), 0, h->st, in[0], in[1], in[2], un, pos);
  NRM_HIP(hipGetLastError());
  float lo[3], hi[3];
  if (int32_t rc = cloud_bounds(h, true, pos, un, rows, lo, hi)) return rc;
  *m_out = 0;
  if (!(lo[0] <= hi[0])) {                                    // no finite point: nothing is kept
    if (voxel_of) {
      NRM_HIP(hipMemsetAsync(d_vof, 0xFF, un * sizeof(int32_t), h->st));
      if (!device) NRM_HIP(hipMemcpyAsync(voxel_of, d_vof, un * sizeof(int32_t), hipMemcpyDeviceToHost, h->st));
      NRM_HIP(hipStreamSynchronize(h->st));
    }
    return S4P_NORMALS_OK;
  }
  VoxGrid g;
  g.v = double(voxel);
  uint64_t max_key = 0;
  for (int a = 0; a < 3; ++a) {
    g.i0[a] = voxel_coord(lo[a], g.v);
    const double ext = voxel_coord(hi[a], g.v) - g.i0[a] + 1.0;
    if (!(ext <= double(S4P_VOXEL_MAX_EXTENT))) {
      char msg[160];
      std::snprintf(msg, sizeof(msg), "voxel_downsample: the %c axis spans %.0f voxels, more than 2^21: use a larger voxel", "xyz"[a], ext);
      return fail(h, S4P_NORMALS_ERR_BAD_ARG, msg);
    }
    max_key |= uint64_t(ext - 1.0) << (21 * a);
  }
  int sort_bits = 1;                                          // 2^bits > max_key + 1: the dropped points' ones sort last
  while (sort_bits < 64 && ((max_key + 1) >> sort_bits) != 0) ++sort_bits;

  hipLaunchKernelGGL(k_voxel_keys, dim3(nb), dim3(kBlock), 0, h->st, (const float4*)pos, un, g, keys, vals);
  NRM_HIP(hipGetLastError());
  NRM_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, sort_bytes, (const uint64_t*)keys, keys2, (const uint32_t*)vals, order, int(un), 0, sort_bits,
                                             h->st));
  hipLaunchKernelGGL(k_voxel_heads, dim3(nb), dim3(kBlock), 0, h->st, (const uint64_t*)keys2, un, flags);
  NRM_HIP(hipGetLastError());
  NRM_HIP(hipcub::DeviceScan::InclusiveSum(tmp, scan_bytes, (const uint32_t*)flags, rows1, int(un), h->st));
  hipLaunchKernelGGL(k_voxel_runs, dim3(nb), dim3(kBlock), 0, h->st, (const uint64_t*)keys2, (const uint32_t*)order, (const uint32_t*)rows1, un,
                     begin, d_vof);
  NRM_HIP(hipGetLastError());
  uint32_t m = 0;
  NRM_HIP(hipMemcpyAsync(&m, rows1 + (un - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, h->st));
  NRM_HIP(hipStreamSynchronize(h->st));

  hipLaunchKernelGGL(k_voxel_segs, dim3(blocks_for(int64_t(m) + 1)), dim3(kBlock), 0, h->st, (const uint32_t*)begin, m, nseg);
  NRM_HIP(hipGetLastError());
  NRM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, scan2_bytes, (const uint32_t*)nseg, segoff, int(m + 1), h->st));
  VoxReduce A{};
  A.pos = pos; A.attr = dattr; A.order = order; A.begin = begin; A.m = m; A.segoff = segoff; A.partial = partial; A.nattr = nattr;
  A.max_seg = uint32_t(max_seg); A.segrow = segrow;
  A.out_xyz = d_xyz; A.out_attr = d_attr; A.out_count = d_count;
  voxel_dispatch(h, A, false);
  NRM_HIP(hipGetLastError());
  if (un > kVoxBlock) {                                      // a run longer than a block needs more points than that
    voxel_dispatch(h, A, true);
    NRM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_voxel_long, dim3(blocks_for(int64_t(max_seg) * int64_t(C))), dim3(kBlock), 0, h->st, A);
    NRM_HIP(hipGetLastError());
  }
  if (!device) {
    const size_t um = size_t(m);
    NRM_HIP(hipMemcpyAsync(out_xyz, d_xyz, 3 * um * sizeof(float), hipMemcpyDeviceToHost, h->st));
    if (nattr > 0) NRM_HIP(hipMemcpyAsync(out_attr, d_attr, um * na * sizeof(float), hipMemcpyDeviceToHost, h->st));
    if (out_count) NRM_HIP(hipMemcpyAsync(out_count, d_count, um * sizeof(int32_t), hipMemcpyDeviceToHost, h->st));
    if (voxel_of) NRM_HIP(hipMemcpyAsync(voxel_of, d_vof, un * sizeof(int32_t), hipMemcpyDeviceToHost, h->st));
  }
  NRM_HIP(hipStreamSynchronize(h->st));
  *m_out = int64_t(m);
  return S4P_NORMALS_OK;
}

}  // namespace

extern "C" {

int32_t s4p_voxel_downsample(s4p_normals_ctx* h, const float* x, const float* y, const float* z, int64_t n, float voxel,
                             const float* attr, int32_t nattr, float* out_xyz, float* out_attr, int32_t* out_count, int32_t* voxel_of,
                             int64_t* m_out) {
  return voxel_impl(h, x, y, z, n, voxel, attr, nattr, out_xyz, out_attr, out_count, voxel_of, m_out, false);
}
int32_t s4p_voxel_downsample_device(s4p_normals_ctx* h, const float* x, const float* y, const float* z, int64_t n, float voxel,
                                    const float* attr, int32_t nattr, float* out_xyz, float* out_attr, int32_t* out_count,
                                    int32_t* voxel_of, int64_t* m_out) {
  return voxel_impl(h, x, y, z, n, voxel, attr, nattr, out_xyz, out_attr, out_count, voxel_of, m_out, true);
}

}  // extern "C"
