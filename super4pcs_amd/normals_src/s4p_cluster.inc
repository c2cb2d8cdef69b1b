// s4p_cluster.inc -- density clustering and fixed-radius density of libsuper4pcs_normals.so (include/s4p_cluster.h, DESIGN.md
// section 29).  Included by s4p_normals.hip after s4p_orient.inc: the functions work on an s4p_normals_ctx after set_cloud,
// on its cloud, stream and arena; the context's own grid is left alone.
//
// Device path (every phase is a kernel of its own, so kernel boundaries are the only ordering the phases rely on):
//   grid      a grid of its own over the cloud's bounds with the cell edge eps (1 + 2^-16), enlarged as set_cloud's is: every
//             neighbour of a point lies in the 3 x 3 x 3 cells around the point's cell (DESIGN.md section 29 derives the
//             margin).  fit_grid + fill_grid of s4p_normals.hip, into the arena.
//   walk      k_cluster_walk<kCount>: a lane per point in cell order counts its neighbours exactly (density);
//             k_cluster_walk<kCore>: it stops at min_points, writes the core flag and makes the point a tree of its own.
//   link      k_cluster_link: the walk again.  A core lane unites itself with every core neighbour of smaller index in a
//             lock-free union-find whose root is the smallest index of its tree; a lane that is not core keeps the minimum
//             (d2 bits, index) over its core neighbours in registers and writes it once.
//   flatten   k_cluster_flatten: every core point walks to its root; the roots are flagged.  An exclusive scan of the flags in
//             index order (hipCUB) ranks the roots: clusters are numbered by their smallest core index.
//   label     k_cluster_label: core -> rank[root], border -> rank[root[nearest core]], noise -> -1; the four counts are
//             integer sums, one atomic per workgroup and count.
// No float or double atomics.  Every loop over parent words has a hop bound that its derivation excludes; a lane that
// reaches it raises a flag, which the host turns into S4P_CLUSTER_ERR_INTERNAL.

#include "s4p_cluster.h"

namespace s4p_nrm {

static_assert(S4P_CLUSTER_ERR_INTERNAL == kErrInternal, "arena_layout fails with the family's internal code");
enum ClusterMode { kCount = 0, kCore = 1 };
enum ClusterWord { kClCore = 0, kClBorder = 1, kClNoise = 2, kClClusters = 3, kClOverrun = 4, kClWords = 8 };
constexpr uint32_t kNoCore = 0xFFFFFFFFu;       // nearest-core word of a point without a core neighbour

struct ClusterArgs {
  GridDev g;                  // the clustering grid: cell edge >= eps (1 + 2^-16)
  uint64_t n;
  float r2;                   // fl(eps * eps)
  int32_t min_points;
  int32_t* count;             // kCount: n, the caller's order
  uint8_t* core;              // n, cell order (walk writes, link reads)
  uint32_t* parent;           // n, the caller's order: the union-find
  uint32_t* near;             // n, the caller's order: the nearest core neighbour of a point that is not core, or kNoCore
  uint8_t* kind;              // n, the caller's order
  uint64_t max_hops;
  unsigned long long* words;  // kClWords
};

// the 3 x 3 x 3 block of cells around the cell of q, clamped to the grid
struct CellBlock {
  int x0, x1, y0, y1, z0, z1;
};
__device__ inline CellBlock cluster_block(const GridDev& g, const float4 q) {
  const int cx = int(fmin(fmax(cell_coord(q.x, g.ox, g.inv_h), 0.0), double(g.nx - 1)));
  const int cy = int(fmin(fmax(cell_coord(q.y, g.oy, g.inv_h), 0.0), double(g.ny - 1)));
  const int cz = int(fmin(fmax(cell_coord(q.z, g.oz, g.inv_h), 0.0), double(g.nz - 1)));
  return CellBlock{max(cx - 1, 0), min(cx + 1, g.nx - 1), max(cy - 1, 0), min(cy + 1, g.ny - 1), max(cz - 1, 0), min(cz + 1, g.nz - 1)};
}
__device__ inline uint2 cluster_row(const GridDev& g, int iz, int iy, int x0, int x1) {
  // the cells x0 .. x1 of one row are consecutive keys: their points are one range of the sorted cloud, unless all are empty
  const uint32_t base = (uint32_t(iz) * uint32_t(g.ny) + uint32_t(iy)) * uint32_t(g.nx);
  uint32_t b = 0u, e = 0u;
  for (int ix = x0; ix <= x1; ++ix) {
    const uint2 r = g.range[base + uint32_t(ix)];
    if (r.y > r.x) {
      if (e == 0u) b = r.x;
      e = r.y;
    }
  }
  return make_uint2(b, e);
}

// A lane per point in cell order: the lanes of a wave read the same few rows of cells.
template <int MODE>
__global__ __launch_bounds__(kBlock) void k_cluster_walk(ClusterArgs A) {
  const GridDev& g = A.g;
  for (uint64_t s = blockIdx.x * (uint64_t)kBlock + threadIdx.x; s < A.n; s += (uint64_t)gridDim.x * kBlock) {
    const float4 q = g.pts[s];
    const CellBlock c = cluster_block(g, q);
    const int32_t stop = MODE == kCore ? A.min_points : 0x7FFFFFFF;
    int32_t cnt = 0;
    for (int iz = c.z0; iz <= c.z1 && cnt < stop; ++iz)
      for (int iy = c.y0; iy <= c.y1 && cnt < stop; ++iy) {
        const uint2 rg = cluster_row(g, iz, iy, c.x0, c.x1);
        for (uint32_t t = rg.x; t < rg.y && cnt < stop; ++t) {
          const float4 p = g.pts[t];
          const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
          const float d2 = dx * dx + (dy * dy + dz * dz);
          cnt += d2 <= A.r2 ? 1 : 0;
        }
      }
    const uint32_t i = __float_as_uint(q.w);
    if (MODE == kCount) {
      A.count[i] = cnt;
    } else {
      A.core[s] = cnt >= A.min_points ? 1 : 0;
      A.parent[i] = i;
    }
  }
}

// Parent words are read and written by agent-scope atomics only: a plain load may come from this CU's L1, which no other
// CU's store refreshes.  A word only ever decreases, and always names a member of its point's component.
__device__ inline uint32_t cluster_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of x's tree as far as this lane can tell (it may have been hooked since); the grandparent is written over the
// parent on the way (atomicMin: the word names an ancestor, and the former parent keeps its own link).
__device__ inline uint32_t cluster_find(uint32_t* parent, uint32_t x, uint64_t& hops) {
  for (;;) {
    const uint32_t p = cluster_load(parent + x);
    if (p == x || hops == 0) return x;
    const uint32_t gp = cluster_load(parent + p);
    if (gp != p) atomicMin(parent + x, gp);
    x = gp;
    --hops;
  }
}

// Unites the trees of a and b and returns the root that remains (a hint).  Each hook is an atomicCAS on a word that still
// holds its own index, so it hooks a root, and onto a smaller index; a failed CAS goes on from the value it returned.  Both
// walks only ever move to smaller indices, so a + b + 2 hops suffice; hops counts down from the call's bound.
__device__ inline uint32_t cluster_unite(uint32_t* parent, uint32_t a, uint32_t b, uint64_t& hops) {
  for (;;) {
    a = cluster_find(parent, a, hops);
    b = cluster_find(parent, b, hops);
    if (a == b || hops == 0) return a;
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    const uint32_t was = atomicCAS(parent + hi, hi, lo);
    if (was == hi) return lo;
    a = was; b = lo;
    --hops;
  }
}

__global__ __launch_bounds__(kBlock) void k_cluster_link(ClusterArgs A) {
  const GridDev& g = A.g;
  bool overrun = false;
  for (uint64_t s = blockIdx.x * (uint64_t)kBlock + threadIdx.x; s < A.n; s += (uint64_t)gridDim.x * kBlock) {
    const float4 q = g.pts[s];
    const uint32_t i = __float_as_uint(q.w);
    const bool core = A.core[s] != 0;
    const CellBlock c = cluster_block(g, q);
    uint32_t cur = i;                                   // a member of i's tree, its root when last seen
    uint64_t best = ~0ull;                              // not core: min (d2 bits << 32 | index) over the core neighbours
    for (int iz = c.z0; iz <= c.z1; ++iz)
      for (int iy = c.y0; iy <= c.y1; ++iy) {
        const uint2 rg = cluster_row(g, iz, iy, c.x0, c.x1);
        for (uint32_t t = rg.x; t < rg.y; ++t) {
          if (!A.core[t]) continue;
          const float4 p = g.pts[t];
          const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
          const float d2 = dx * dx + (dy * dy + dz * dz);
          if (!(d2 <= A.r2)) continue;
          const uint32_t j = __float_as_uint(p.w);
          if (core) {
            // a plain load is a hint only, but whatever it returns was stored there once and so names a member of j's
            // component: when that is cur, a member of i's, the two are united already
            if (j < i && A.parent[j] != cur) {
              uint64_t hops = A.max_hops;
              cur = cluster_unite(A.parent, cur, j, hops);
              overrun |= hops == 0;
            }
          } else {
            const uint64_t key = uint64_t(__float_as_uint(d2)) << 32 | j;
            best = key < best ? key : best;
          }
        }
      }
    if (!core) A.near[i] = best == ~0ull ? kNoCore : uint32_t(best);
    A.kind[i] = core ? S4P_CLUSTER_CORE : (best == ~0ull ? S4P_CLUSTER_NOISE : S4P_CLUSTER_BORDER);
  }
  if (overrun) atomicMax(A.words + kClOverrun, 1ull);
}

// After the link kernel has ended, plain loads see every hook.  root[i] of a core point, and the flag of a root.
__global__ __launch_bounds__(kBlock) void k_cluster_flatten(uint64_t n, const uint8_t* kind, const uint32_t* parent, uint32_t* root,
                                                            uint32_t* flag, unsigned long long* words) {
  bool overrun = false;
  for (uint64_t v = blockIdx.x * (uint64_t)kBlock + threadIdx.x; v < n; v += (uint64_t)gridDim.x * kBlock) {
    uint32_t r = uint32_t(v);
    uint32_t f = 0u;
    if (kind[v] == S4P_CLUSTER_CORE) {
      uint64_t hops = n;                                  // every step moves to a smaller index
      for (uint32_t p = parent[r]; p != r && hops > 0; p = parent[r], --hops) r = p;
      overrun |= parent[r] != r;
      f = r == uint32_t(v) ? 1u : 0u;
    }
    root[v] = r;
    flag[v] = f;
  }
  if (overrun) atomicMax(words + kClOverrun, 1ull);
}

__global__ __launch_bounds__(kBlock) void k_cluster_label(uint64_t n, const uint8_t* kind, const uint32_t* root, const uint32_t* near,
                                                          const uint32_t* rank, int32_t* label, unsigned long long* words) {
  uint32_t ncore = 0u, nborder = 0u, nnoise = 0u;          // of this lane (n < 2^31)
  for (uint64_t v = blockIdx.x * (uint64_t)kBlock + threadIdx.x; v < n; v += (uint64_t)gridDim.x * kBlock) {
    const uint8_t k = kind[v];
    int32_t lab = -1;
    if (k == S4P_CLUSTER_CORE) lab = int32_t(rank[root[v]]);
    else if (k == S4P_CLUSTER_BORDER) lab = int32_t(rank[root[near[v]]]);
    label[v] = lab;
    ncore += k == S4P_CLUSTER_CORE; nborder += k == S4P_CLUSTER_BORDER; nnoise += k == S4P_CLUSTER_NOISE;
  }
  __shared__ uint32_t sh[3][kBlock];
  sh[kClCore][threadIdx.x] = ncore; sh[kClBorder][threadIdx.x] = nborder; sh[kClNoise][threadIdx.x] = nnoise;
  __syncthreads();
  for (int w = kBlock / 2; w > 0; w >>= 1) {
    if (threadIdx.x < unsigned(w))
      for (int a = 0; a < 3; ++a) sh[a][threadIdx.x] += sh[a][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x < 3 && sh[threadIdx.x][0]) atomicAdd(words + threadIdx.x, (unsigned long long)sh[threadIdx.x][0]);   // integer counts
}

}  // namespace s4p_nrm

namespace {

// eps (1 + 2^-16): see DESIGN.md section 29 for why no neighbour can lie two cells away
constexpr double kClusterEdgeMargin = 1.0 + 0x1p-16;

int32_t cluster_check(s4p_normals_ctx* h, const char* what, const char* name, float eps) {
  if (!h->has_cloud) return fail(h, S4P_NORMALS_ERR_STATE, std::string(what) + ": set_cloud first");
  const float r2 = eps * eps;
  // a subnormal or zero r2 has no relative precision left: the cell margin of the grid no longer covers d2 <= r2
  if (!std::isfinite(eps) || !(eps > 0.f) || !std::isfinite(r2) || !(r2 >= FLT_MIN))
    return fail(h, S4P_NORMALS_ERR_BAD_ARG, std::string(what) + ": " + name + " must be finite and > 0, with a finite and normal square in float (>= 2^-126)");
  return S4P_NORMALS_OK;
}

struct ClusterGrid {
  GridDev g{};
  uint64_t ncell = 0;
  size_t sort_bytes = 0;
  uint32_t *keys = nullptr, *vals = nullptr, *keys2 = nullptr, *vals2 = nullptr;      // the arena pieces of build
  void* tmp = nullptr;
  uint2* range = nullptr;
  float4* pts = nullptr;
  void take(Arena& ar, uint64_t un) {
    keys = ar.take<uint32_t>(un); vals = ar.take<uint32_t>(un); keys2 = ar.take<uint32_t>(un); vals2 = ar.take<uint32_t>(un);
    tmp = ar.take<char>(sort_bytes);
    range = ar.take<uint2>(ncell);
    pts = ar.take<float4>(un);
  }
};

// rings: how many cells on each side of a point's cell hold its neighbours (s4p_shape.inc asks for 2: half the edge)
int32_t cluster_grid_plan(s4p_normals_ctx* h, const char* what, float eps, ClusterGrid* G, int rings = 1) {
  const uint64_t un = uint64_t(h->n);
  double ext = 0.0;
  for (int a = 0; a < 3; ++a) ext = std::max(ext, double(h->hi[a]) - double(h->lo[a]));
  const double hh = std::max(double(eps) * kClusterEdgeMargin / rings, ext * 0x1p-20);
  if (int32_t rc = fit_grid(h, what, h->lo, h->hi, hh, un, &G->g, &G->ncell)) return rc;
  if (int32_t rc = sort_pairs_bytes(h, un, G->ncell - 1, &G->sort_bytes)) return rc;
  return S4P_NORMALS_OK;
}

int32_t cluster_grid_build(s4p_normals_ctx* h, ClusterGrid* G) {
  if (int32_t rc = fill_grid(h, h->pos, uint64_t(h->n), G->g, G->ncell, G->keys, G->vals, G->keys2, G->vals2, G->tmp, G->sort_bytes,
                             G->range, G->pts)) return rc;
  G->g.pts = G->pts;
  G->g.range = G->range;
  return S4P_NORMALS_OK;
}

int32_t density_impl(s4p_normals_ctx* h, float radius, int32_t* count, bool device) {
  if (!h) return S4P_NORMALS_ERR_BAD_ARG;
  if (int32_t rc = cluster_check(h, "cluster_density", "radius", radius)) return rc;
  if (!count) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "cluster_density: null count");
  NRM_HIP(hipSetDevice(h->device));
  const uint64_t un = uint64_t(h->n);
  ClusterGrid G;
  if (int32_t rc = cluster_grid_plan(h, "cluster_density", radius, &G)) return rc;
  int32_t* dcount = count;
  if (int32_t rc = arena_layout(h, "cluster_density", [&](Arena& ar) {
        G.take(ar, un);
        if (!device) dcount = ar.take<int32_t>(un);
      })) return rc;
  if (int32_t rc = cluster_grid_build(h, &G)) return rc;
  ClusterArgs A{};
  A.g = G.g; A.n = un; A.r2 = radius * radius; A.min_points = 0;
  A.count = dcount;
  hipLaunchKernelGGL(k_cluster_walk<kCount>, dim3(blocks_for(h->n)), dim3(kBlock), 0, h->st, A);
  NRM_HIP(hipGetLastError());
  if (!device) NRM_HIP(hipMemcpyAsync(count, A.count, un * 4, hipMemcpyDeviceToHost, h->st));
  NRM_HIP(hipStreamSynchronize(h->st));
  return S4P_NORMALS_OK;
}

int32_t dbscan_impl(s4p_normals_ctx* h, float eps, int32_t min_points, int32_t* label, uint8_t* kind, s4p_cluster_stats* stats,
                    bool device) {
  if (!h) return S4P_NORMALS_ERR_BAD_ARG;
  if (int32_t rc = cluster_check(h, "cluster_dbscan", "eps", eps)) return rc;
  if (min_points < 1) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "cluster_dbscan: min_points must be at least 1");
  if (!label) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "cluster_dbscan: null label");
  NRM_HIP(hipSetDevice(h->device));
  const uint64_t un = uint64_t(h->n);
  const int nb = blocks_for(h->n);
  ClusterGrid G;
  if (int32_t rc = cluster_grid_plan(h, "cluster_dbscan", eps, &G)) return rc;
  size_t scan_bytes = 0;
  uint32_t* none = nullptr;
  NRM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (const uint32_t*)none, none, int(un), h->st));
  unsigned long long* words = nullptr;
  uint8_t *core = nullptr, *dkind = nullptr;
  uint32_t *parent = nullptr, *near = nullptr, *root = nullptr, *flag = nullptr, *rank = nullptr;
  void* scan_tmp = nullptr;
  int32_t* dlabel = label;
  if (int32_t rc = arena_layout(h, "cluster_dbscan", [&](Arena& ar) {
        G.take(ar, un);
        words = ar.take<unsigned long long>(kClWords);
        core = ar.take<uint8_t>(un);
        dkind = ar.take<uint8_t>(un);
        parent = ar.take<uint32_t>(un);
        near = ar.take<uint32_t>(un);
        root = ar.take<uint32_t>(un);
        flag = ar.take<uint32_t>(un);
        rank = ar.take<uint32_t>(un);
        scan_tmp = ar.take<char>(scan_bytes);
        if (!device) dlabel = ar.take<int32_t>(un);
      })) return rc;
  if (int32_t rc = cluster_grid_build(h, &G)) return rc;
  NRM_HIP(hipMemsetAsync(words, 0, kClWords * 8, h->st));
  ClusterArgs A{};
  A.g = G.g; A.n = un; A.r2 = eps * eps; A.min_points = min_points;
  A.core = core; A.parent = parent; A.near = near; A.kind = dkind; A.words = words;
  A.max_hops = 2 * un + 2;
  hipLaunchKernelGGL(k_cluster_walk<kCore>, dim3(nb), dim3(kBlock), 0, h->st, A);
  NRM_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_cluster_link, dim3(nb), dim3(kBlock), 0, h->st, A);
  NRM_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_cluster_flatten, dim3(nb), dim3(kBlock), 0, h->st, un, (const uint8_t*)dkind, (const uint32_t*)parent, root, flag, words);
  NRM_HIP(hipGetLastError());
  NRM_HIP(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, (const uint32_t*)flag, rank, int(un), h->st));
  hipLaunchKernelGGL(k_cluster_label, dim3(nb), dim3(kBlock), 0, h->st, un, (const uint8_t*)dkind, (const uint32_t*)root, (const uint32_t*)near,
                     (const uint32_t*)rank, dlabel, words);
  NRM_HIP(hipGetLastError());
  unsigned long long hw[kClWords] = {};
  uint32_t last[2] = {0u, 0u};                           // rank and flag of the last point: their sum is the number of clusters
  NRM_HIP(hipMemcpyAsync(hw, words, sizeof(hw), hipMemcpyDeviceToHost, h->st));
  NRM_HIP(hipMemcpyAsync(&last[0], rank + (un - 1), 4, hipMemcpyDeviceToHost, h->st));
  NRM_HIP(hipMemcpyAsync(&last[1], flag + (un - 1), 4, hipMemcpyDeviceToHost, h->st));
  if (!device) NRM_HIP(hipMemcpyAsync(label, dlabel, un * 4, hipMemcpyDeviceToHost, h->st));
  if (kind) NRM_HIP(hipMemcpyAsync(kind, dkind, un, device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->st));
  NRM_HIP(hipStreamSynchronize(h->st));
  if (hw[kClOverrun])
    return fail(h, S4P_CLUSTER_ERR_INTERNAL, "cluster_dbscan: a walk of the union-find did not end within its bound (the parent words must only decrease)");
  if (stats) {
    stats->core = int64_t(hw[kClCore]); stats->border = int64_t(hw[kClBorder]); stats->noise = int64_t(hw[kClNoise]);
    stats->clusters = int64_t(last[0]) + int64_t(last[1]);
  }
  return S4P_NORMALS_OK;
}

}  // namespace

extern "C" {

int32_t s4p_cluster_dbscan(s4p_normals_ctx* h, float eps, int32_t min_points, int32_t* label, uint8_t* kind, s4p_cluster_stats* stats) {
  return dbscan_impl(h, eps, min_points, label, kind, stats, false);
}
int32_t s4p_cluster_dbscan_device(s4p_normals_ctx* h, float eps, int32_t min_points, int32_t* label, uint8_t* kind,
                                  s4p_cluster_stats* stats) {
  return dbscan_impl(h, eps, min_points, label, kind, stats, true);
}

int32_t s4p_cluster_density(s4p_normals_ctx* h, float radius, int32_t* count) { return density_impl(h, radius, count, false); }
int32_t s4p_cluster_density_device(s4p_normals_ctx* h, float radius, int32_t* count) { return density_impl(h, radius, count, true); }

}  // extern "C"
