// s4p_shape.inc -- radius-neighbourhood normals and surface variation of libsuper4pcs_normals.so (include/s4p_shape.h, DESIGN.md
// section 34).  Included by s4p_normals.hip after s4p_plane.inc: the functions work on an s4p_normals_ctx after set_cloud, on
// its cloud, stream and arena; the context's own grid is left alone.
//
// Device path:
//   grid      the clustering grid of s4p_cluster.inc (cluster_grid_plan + cluster_grid_build, into the arena) with the cell edge
//             r (1 + 2^-16) / rings, rings = 2 when that grid fits the cell cap as it is and 1 otherwise: every neighbour of a
//             position lies in the (2 rings + 1)^3 cells around the position's cell (section 29's margin; section 34 extends
//             it to half the edge and to positions outside the cloud's bounds).
//   queries   the cloud in that grid's cell order, or QueryStage's cell order of the caller's positions.
//   walk      k_shape_walk: a lane per query walks the block of cells row by row, and for every point with d2 <= fl(r*r) adds
//             the offsets quantised to r 2^-18 into nine 64-bit integer moments; the lane then solves its 3 x 3 covariance
//             (jacobi3) and writes normal, eigenvalues and count to the query's row in the caller's order.
// Integer sums have no order: the bits do not depend on the grid, the walk or the launch.  Every loop is bounded at entry;
// there are no atomics at all.

#include "s4p_shape.h"

namespace s4p_nrm {

// Rings: the cells on each side of a query's cell that hold its neighbours; the cell edge is r (1 + 2^-16) / rings.  Two rings
// (125 cells of edge r / 2) test 3.7 times the ball's volume, one ring (27 cells of edge r) 6.4 times; the finer grid has eight
// times the cells, so it is taken when it fits the cell cap as it is (shape_grid_plan).  -DS4P_SHAPE_RINGS=1 or 2 builds a
// library with one choice for every call (tools/shape_timing.py --variants measures such builds against each other).
#ifndef S4P_SHAPE_RINGS
#define S4P_SHAPE_RINGS 0
#endif
constexpr int kShapeForceRings = S4P_SHAPE_RINGS;
static_assert(kShapeForceRings >= 0 && kShapeForceRings <= 2, "0: chosen per call; 1: an edge of r; 2: an edge of r / 2");

struct ShapeArgs {
  GridDev g;                  // the grid of this call: cell edge >= r (1 + 2^-16) / rings
  int32_t rings;
  const float4* qs;           // the queries, w = output row (bits)
  uint64_t m;
  float r2;                   // fl(r * r)
  double scale;               // 2^s, s = 18 - ilogb(r)
  int32_t unscale;            // -2 s: the eigenvalues go back to the cloud's squared units
  int32_t need;               // max(3, min_neighbours)
  float* normal;              // 3 m, the caller's order
  float* eig;                 // 3 m or null
  int32_t* count;             // m or null
};

// The cells c - rings .. c + rings around the cell c of x along one axis of n cells, clamped to the grid; empty (lo > hi) when
// x lies more than rings cells outside it.  c is not clamped first, as a cloud point's is: a position outside the bounds has
// neighbours on one side only.  Beyond rings + 2 cells outside nothing is within r, and the clamp of t keeps the conversion
// to int defined.
__device__ inline void shape_cells(float x, double o, double inv_h, int n, int rings, int* lo, int* hi) {
  const double t = fmin(fmax(cell_coord(x, o, inv_h), -double(rings + 2)), double(n + rings + 1));
  const int c = int(t);
  *lo = max(c - rings, 0);
  *hi = min(c + rings, n - 1);
}

// The nine moments of one query.  add() takes the three quantised offsets as the doubles rint left them (integers of at most
// 2^19 + 1 in magnitude): a product of two fits 39 bits, and 2^24 of them 63.
struct ShapeMoments {
  int32_t cnt = 0;
  long long S[3] = {0, 0, 0}, Q[6] = {0, 0, 0, 0, 0, 0};
  __device__ __forceinline__ void add(double d0, double d1, double d2) {
    const int32_t u0 = int32_t(d0), u1 = int32_t(d1), u2 = int32_t(d2);
    ++cnt;
    S[0] += u0; S[1] += u1; S[2] += u2;
    Q[0] += (long long)u0 * u0; Q[1] += (long long)u0 * u1; Q[2] += (long long)u0 * u2;
    Q[3] += (long long)u1 * u1; Q[4] += (long long)u1 * u2; Q[5] += (long long)u2 * u2;
  }
};

// The row of a query from its moments: contract steps "Covariance" to "Eigenvalues" of include/s4p_shape.h.
__device__ inline void shape_solve(int32_t cnt, const long long (&S)[3], const long long (&Q)[6], int32_t need, int32_t unscale,
                                   float (&nrm)[3], float (&ev)[3]) {
  nrm[0] = nrm[1] = nrm[2] = 0.f;
  ev[0] = ev[1] = ev[2] = 0.f;
  if (cnt < need) return;
  const double kk = double(cnt);
  const double m0 = double(S[0]) / kk, m1 = double(S[1]) / kk, m2 = double(S[2]) / kk;
  double C[3][3], V[3][3];
  C[0][0] = double(Q[0]) / kk - m0 * m0; C[0][1] = double(Q[1]) / kk - m0 * m1; C[0][2] = double(Q[2]) / kk - m0 * m2;
  C[1][1] = double(Q[3]) / kk - m1 * m1; C[1][2] = double(Q[4]) / kk - m1 * m2; C[2][2] = double(Q[5]) / kk - m2 * m2;
  C[1][0] = C[0][1]; C[2][0] = C[0][2]; C[2][1] = C[1][2];
  const double tr = (C[0][0] + C[1][1]) + C[2][2];
  if (!(tr > 0.0)) return;
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
  nrm[0] = float(v0); nrm[1] = float(v1); nrm[2] = float(v2);
  // descending, not clamped
  double l0 = C[0][0], l1 = C[1][1], l2 = C[2][2], t;
  if (l0 < l1) { t = l0; l0 = l1; l1 = t; }
  if (l1 < l2) { t = l1; l1 = l2; l2 = t; }
  if (l0 < l1) { t = l0; l0 = l1; l1 = t; }
  ev[0] = float(ldexp(l0, unscale)); ev[1] = float(ldexp(l1, unscale)); ev[2] = float(ldexp(l2, unscale));
}

// A lane per query.  Consecutive queries are neighbours in space (cell order), so the lanes of a wave read the same few
// rows of cells.  The three or five cells of a row along x are one range of the sorted cloud (cluster_row).
__global__ __launch_bounds__(kBlock) void k_shape_walk(ShapeArgs A) {
  const GridDev& g = A.g;
  for (uint64_t j = blockIdx.x * (uint64_t)kBlock + threadIdx.x; j < A.m; j += (uint64_t)gridDim.x * kBlock) {
    const float4 q = A.qs[j];
    ShapeMoments M;
    if (isfinite(q.x) && isfinite(q.y) && isfinite(q.z)) {
      int x0, x1, y0, y1, z0, z1;
      shape_cells(q.x, g.ox, g.inv_h, g.nx, A.rings, &x0, &x1);
      shape_cells(q.y, g.oy, g.inv_h, g.ny, A.rings, &y0, &y1);
      shape_cells(q.z, g.oz, g.inv_h, g.nz, A.rings, &z0, &z1);
      if (x0 <= x1)
        for (int iz = z0; iz <= z1; ++iz)
          for (int iy = y0; iy <= y1; ++iy) {
            const uint2 rg = cluster_row(g, iz, iy, x0, x1);
            for (uint32_t t = rg.x; t < rg.y; ++t) {
              const float4 p = g.pts[t];
              const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
              const float d2 = dx * dx + (dy * dy + dz * dz);
              if (!(d2 <= A.r2)) continue;
              // exact products; rint rounds ties to even
              M.add(rint(double(dx) * A.scale), rint(double(dy) * A.scale), rint(double(dz) * A.scale));
            }
          }
    }
    float nrm[3], ev[3];
    shape_solve(M.cnt, M.S, M.Q, A.need, A.unscale, nrm, ev);
    const uint64_t row = __float_as_uint(q.w);
    A.normal[3 * row] = nrm[0]; A.normal[3 * row + 1] = nrm[1]; A.normal[3 * row + 2] = nrm[2];
    if (A.eig) { A.eig[3 * row] = ev[0]; A.eig[3 * row + 1] = ev[1]; A.eig[3 * row + 2] = ev[2]; }
    if (A.count) A.count[row] = M.cnt;
  }
}

}  // namespace s4p_nrm

namespace {

int32_t shape_check(s4p_normals_ctx* h, const char* what, float radius, int32_t min_neighbours, const float* normal) {
  if (int32_t rc = cluster_check(h, what, "radius", radius)) return rc;
  if (min_neighbours < 1) return fail(h, S4P_NORMALS_ERR_BAD_ARG, std::string(what) + ": min_neighbours must be at least 1");
  if (!normal) return fail(h, S4P_NORMALS_ERR_BAD_ARG, std::string(what) + ": null normal");
  return S4P_NORMALS_OK;
}

// The output rows of a call: the caller's pointers in the device form, arena pieces in the host form (a null eig or count
// stays null either way, and the kernel skips it).
struct ShapeOut {
  float *normal = nullptr, *eig = nullptr;
  int32_t* count = nullptr;
  void take(Arena& ar, uint64_t rows, bool device, float* n, float* e, int32_t* c) {
    normal = device ? n : ar.take<float>(3 * rows);
    eig = !e ? nullptr : (device ? e : ar.take<float>(3 * rows));
    count = !c ? nullptr : (device ? c : ar.take<int32_t>(rows));
  }
};

// The grid of a call: of edge r / 2 when that fits the cell cap as it is, else of edge r, enlarged where it has to be (an
// enlarged finer grid would only widen a block of 125 cells).
int32_t shape_grid_plan(s4p_normals_ctx* h, const char* what, float radius, ClusterGrid* G, int* rings) {
  for (int r = kShapeForceRings ? kShapeForceRings : 2;; --r) {
    if (int32_t rc = cluster_grid_plan(h, what, radius, G, r)) return rc;
    *rings = r;
    if (r == 1 || kShapeForceRings || G->g.h <= double(radius) * kClusterEdgeMargin / r) return S4P_NORMALS_OK;
  }
}

// grid -> walk -> (host form) the rows back; waits for the stream
int32_t shape_run(s4p_normals_ctx* h, ClusterGrid* G, int rings, const float4* qs, uint64_t rows, float radius, int32_t min_neighbours,
                  const ShapeOut& D, bool device, float* normal, float* eig, int32_t* count) {
  const int s = 18 - std::ilogb(radius);
  ShapeArgs A{};
  A.g = G->g; A.rings = rings; A.qs = qs ? qs : G->g.pts; A.m = rows; A.r2 = radius * radius;
  A.scale = std::ldexp(1.0, s); A.unscale = -2 * s; A.need = std::max(3, min_neighbours);
  A.normal = D.normal; A.eig = D.eig; A.count = D.count;
  hipLaunchKernelGGL(k_shape_walk, dim3(blocks_for(int64_t(rows))), dim3(kBlock), 0, h->st, A);
  NRM_HIP(hipGetLastError());
  if (!device) {
    NRM_HIP(hipMemcpyAsync(normal, D.normal, 3 * rows * sizeof(float), hipMemcpyDeviceToHost, h->st));
    if (eig) NRM_HIP(hipMemcpyAsync(eig, D.eig, 3 * rows * sizeof(float), hipMemcpyDeviceToHost, h->st));
    if (count) NRM_HIP(hipMemcpyAsync(count, D.count, rows * sizeof(int32_t), hipMemcpyDeviceToHost, h->st));
  }
  NRM_HIP(hipStreamSynchronize(h->st));
  return S4P_NORMALS_OK;
}

int32_t shape_estimate_impl(s4p_normals_ctx* h, float radius, int32_t min_neighbours, float* normal, float* eig, int32_t* count, bool device) {
  if (!h) return S4P_NORMALS_ERR_BAD_ARG;
  if (int32_t rc = shape_check(h, "shape_estimate", radius, min_neighbours, normal)) return rc;
  NRM_HIP(hipSetDevice(h->device));
  const uint64_t un = uint64_t(h->n);
  ClusterGrid G;
  int rings = 1;
  if (int32_t rc = shape_grid_plan(h, "shape_estimate", radius, &G, &rings)) return rc;
  ShapeOut D;
  if (int32_t rc = arena_layout(h, "shape_estimate", [&](Arena& ar) {
        G.take(ar, un);
        D.take(ar, un, device, normal, eig, count);
      })) return rc;
  if (int32_t rc = cluster_grid_build(h, &G)) return rc;
  return shape_run(h, &G, rings, nullptr, un, radius, min_neighbours, D, device, normal, eig, count);
}

int32_t shape_estimate_at_impl(s4p_normals_ctx* h, const float* qx, const float* qy, const float* qz, int64_t m, float radius,
                               int32_t min_neighbours, float* normal, float* eig, int32_t* count, bool device) {
  if (!h) return S4P_NORMALS_ERR_BAD_ARG;
  if (int32_t rc = shape_check(h, "shape_estimate_at", radius, min_neighbours, normal)) return rc;
  if (m < 0 || m > kMaxPoints) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "shape_estimate_at: m must be in [0, 2^31 - 2]");
  if (m == 0) return S4P_NORMALS_OK;
  if (!qx || !qy || !qz) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "shape_estimate_at: null query pointers");
  NRM_HIP(hipSetDevice(h->device));
  const uint64_t un = uint64_t(h->n), um = uint64_t(m);
  ClusterGrid G;
  int rings = 1;
  if (int32_t rc = shape_grid_plan(h, "shape_estimate_at", radius, &G, &rings)) return rc;
  QueryStage Qs;
  if (int32_t rc = Qs.plan(h, um)) return rc;
  ShapeOut D;
  if (int32_t rc = arena_layout(h, "shape_estimate_at", [&](Arena& ar) {
        G.take(ar, un);
        Qs.take(ar);
        D.take(ar, um, device, normal, eig, count);
      })) return rc;
  if (int32_t rc = cluster_grid_build(h, &G)) return rc;
  if (int32_t rc = Qs.run(h, qx, qy, qz, device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice)) return rc;
  return shape_run(h, &G, rings, Qs.qs, um, radius, min_neighbours, D, device, normal, eig, count);
}

}  // namespace

extern "C" {

int32_t s4p_shape_estimate(s4p_normals_ctx* h, float radius, int32_t min_neighbours, float* normal, float* eig, int32_t* count) {
  return shape_estimate_impl(h, radius, min_neighbours, normal, eig, count, false);
}
int32_t s4p_shape_estimate_device(s4p_normals_ctx* h, float radius, int32_t min_neighbours, float* normal, float* eig, int32_t* count) {
  return shape_estimate_impl(h, radius, min_neighbours, normal, eig, count, true);
}

int32_t s4p_shape_estimate_at(s4p_normals_ctx* h, const float* qx, const float* qy, const float* qz, int64_t m, float radius,
                              int32_t min_neighbours, float* normal, float* eig, int32_t* count) {
  return shape_estimate_at_impl(h, qx, qy, qz, m, radius, min_neighbours, normal, eig, count, false);
}
int32_t s4p_shape_estimate_at_device(s4p_normals_ctx* h, const float* qx, const float* qy, const float* qz, int64_t m, float radius,
                                     int32_t min_neighbours, float* normal, float* eig, int32_t* count) {
  return shape_estimate_at_impl(h, qx, qy, qz, m, radius, min_neighbours, normal, eig, count, true);
}

}  // extern "C"
