// s4p_icp_k_build.hip.hpp -- kernels that run once per cloud or per call, not per iteration: statistics, cell keys and
// starts, gathers and scatters, the source order, the final apply, target normals and colour gradients.
#pragma once

namespace s4p_icp {

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

// the returned transform on the caller's cloud, in k_apply's rounding order
__global__ __launch_bounds__(kBlock) void k_apply_icp(Tf T, float* x, float* y, float* z, uint64_t n) {
  for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    float ox, oy, oz;
    apply_t(T, x[i], y[i], z[i], ox, oy, oz);
    x[i] = ox; y[i] = oy; z[i] = oz;
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


// source normals (uploaded order, already normalised) -> the order of `src` (w = original source index), next to it.
// The uploaded-order copy stays on the device, so the read-back needs no scatter.
__global__ __launch_bounds__(kBlock) void k_gather_source_normals(const float* x, const float* y, const float* z, const float4* src,
                                                                  uint64_t n, float4* snrm) {
  for (uint64_t k = blockIdx.x * (uint64_t)kBlock + threadIdx.x; k < n; k += (uint64_t)gridDim.x * kBlock) {
    const uint32_t j = __float_as_uint(src[k].w);
    snrm[k] = make_float4(x[j], y[j], z[j], 0.f);
  }
}

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
    if (is_zero(nf)) { grad[k] = out; continue; }
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

}  // namespace s4p_icp
