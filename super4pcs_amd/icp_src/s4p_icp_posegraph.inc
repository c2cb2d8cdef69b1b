// s4p_icp_posegraph.inc -- pose-graph optimisation with a line process (include/s4p_icp_posegraph.h): host only, double.
// The residual and its Jacobians, the robust cost, one Levenberg-Marquardt stage on the dense system, the two stages.

namespace {
namespace pg {

using Edge = s4p_icp_posegraph_edge;

constexpr double kLambda0 = 1e-6, kLambdaMin = 1e-15, kLambdaMax = 1e12;     // damping, relative to the diagonal

void rigid_inverse(const double* X, double* Xi) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) Xi[4 * r + c] = X[4 * c + r];
    Xi[4 * r + 3] = -((X[r] * X[3] + X[4 + r] * X[7]) + X[8 + r] * X[11]);
  }
  Xi[12] = Xi[13] = Xi[14] = 0.0;
  Xi[15] = 1.0;
}

// the rotation vector of the rotation block of E (row-major 4x4), through the unit quaternion (stable up to pi)
void rotation_vector(const double* E, double* w) {
  const double m00 = E[0], m01 = E[1], m02 = E[2], m10 = E[4], m11 = E[5], m12 = E[6], m20 = E[8], m21 = E[9], m22 = E[10];
  double q[4];                                       // w, x, y, z
  const double tr = m00 + m11 + m22;
  if (tr > 0.0) {
    const double s = std::sqrt(tr + 1.0) * 2.0;
    q[0] = 0.25 * s; q[1] = (m21 - m12) / s; q[2] = (m02 - m20) / s; q[3] = (m10 - m01) / s;
  } else if (m00 > m11 && m00 > m22) {
    const double s = std::sqrt(1.0 + m00 - m11 - m22) * 2.0;
    q[0] = (m21 - m12) / s; q[1] = 0.25 * s; q[2] = (m01 + m10) / s; q[3] = (m02 + m20) / s;
  } else if (m11 > m22) {
    const double s = std::sqrt(1.0 + m11 - m00 - m22) * 2.0;
    q[0] = (m02 - m20) / s; q[1] = (m01 + m10) / s; q[2] = 0.25 * s; q[3] = (m12 + m21) / s;
  } else {
    const double s = std::sqrt(1.0 + m22 - m00 - m11) * 2.0;
    q[0] = (m10 - m01) / s; q[1] = (m02 + m20) / s; q[2] = (m12 + m21) / s; q[3] = 0.25 * s;
  }
  if (q[0] < 0.0) for (int k = 0; k < 4; ++k) q[k] = -q[k];
  const double vn = std::sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double f = vn > 1e-12 ? 2.0 * std::atan2(vn, q[0]) / vn : 2.0 / q[0];
  for (int a = 0; a < 3; ++a) w[a] = f * q[1 + a];
}

// Rodrigues, as s4p_icp_solve_plane builds it
void rodrigues(const double* w, double R[3][3]) {
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = std::sqrt(th2);
  const double c1 = th > 0.0 ? std::sin(th) / th : 1.0;
  const double sh = th > 0.0 ? std::sin(0.5 * th) / th : 0.5;
  const double c2 = 2.0 * sh * sh;
  const double K[3][3] = {{0.0, -w[2], w[1]}, {w[2], 0.0, -w[0]}, {-w[1], w[0], 0.0}};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) R[r][c] = (r == c ? 1.0 : 0.0) + c1 * K[r][c] + c2 * (w[r] * w[c] - (r == c ? th2 : 0.0));
}

// X <- X [Rodrigues(d[0..2]) | d[3..5]]
void retract(const double* X, const double* d, double* out) {
  double R[3][3], D[16];
  rodrigues(d, R);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) D[4 * r + c] = R[r][c];
    D[4 * r + 3] = d[3 + r];
  }
  D[12] = D[13] = D[14] = 0.0;
  D[15] = 1.0;
  mat_mul4(X, D, out);
  out[12] = X[12]; out[13] = X[13]; out[14] = X[14]; out[15] = X[15];
}

// E_e = X_t^-1 X_s T_e^-1 and r_e
void residual(const double* Xs, const double* Xt, const Edge& e, double* E, double* r) {
  double Xti[16], Ti[16], A[16];
  rigid_inverse(Xt, Xti);
  rigid_inverse(e.T, Ti);
  mat_mul4(Xti, Xs, A);
  mat_mul4(A, Ti, E);
  rotation_vector(E, r);
  r[3] = E[3]; r[4] = E[7]; r[5] = E[11];
}

double quad(const double* L, const double* r) {
  double v = 0.0;
  for (int a = 0; a < 6; ++a) {
    double row = 0.0;
    for (int b = 0; b < 6; ++b) row += L[6 * a + b] * r[b];
    v += r[a] * row;
  }
  return v;
}

double line_value(const Edge& e, double chi2, double mu) {
  if (!e.uncertain) return 1.0;
  const double l = mu / (mu + chi2);
  return l * l;
}

// F over the active edges (active null: all); chi2 / line: optional, per edge (written for active edges only)
double cost(const double* poses, int32_t n_edges, const Edge* edges, const char* active, double mu, double* chi2, double* line) {
  double F = 0.0;
  for (int32_t k = 0; k < n_edges; ++k) {
    if (active && !active[k]) continue;
    const Edge& e = edges[k];
    double E[16], r[6];
    residual(poses + 16 * e.source, poses + 16 * e.target, e, E, r);
    const double c = quad(e.info, r);
    if (chi2) chi2[k] = c;
    if (line) line[k] = line_value(e, c, mu);
    F += e.uncertain ? mu * c / (mu + c) : c;
  }
  return F;
}

// the inverse right Jacobian of SO(3) at the rotation vector w
void right_jacobian_inverse(const double* w, double J[3][3]) {
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = std::sqrt(th2);
  const double c = th < 1e-4 ? 1.0 / 12.0 + th2 / 720.0 : 1.0 / th2 - (1.0 + std::cos(th)) / (2.0 * th * std::sin(th));
  const double K[3][3] = {{0.0, -w[2], w[1]}, {w[2], 0.0, -w[0]}, {-w[1], w[0], 0.0}};
  for (int r = 0; r < 3; ++r)
    for (int s = 0; s < 3; ++s) J[r][s] = (r == s ? 1.0 : 0.0) + 0.5 * K[r][s] + c * (w[r] * w[s] - (r == s ? th2 : 0.0));
}

// d r_e / d delta_s and d r_e / d delta_t (6x6 each; rows (omega, v) of r, columns (omega, v) of the node's step)
void jacobians(const double* E, const double* r, const Edge& e, double Js[6][6], double Jt[6][6]) {
  double Ji[3][3];
  right_jacobian_inverse(r, Ji);
  double RE[3][3], RA[3][3];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) { RE[a][b] = E[4 * a + b]; RA[a][b] = e.T[4 * a + b]; }
  const double tA[3] = {e.T[3], e.T[7], e.T[11]}, tE[3] = {r[3], r[4], r[5]};
  const double XA[3][3] = {{0.0, -tA[2], tA[1]}, {tA[2], 0.0, -tA[0]}, {-tA[1], tA[0], 0.0}};
  const double XE[3][3] = {{0.0, -tE[2], tE[1]}, {tE[2], 0.0, -tE[0]}, {-tE[1], tE[0], 0.0}};
  double XARA[3][3];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) XARA[a][b] = XA[a][0] * RA[0][b] + XA[a][1] * RA[1][b] + XA[a][2] * RA[2][b];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      Js[a][b] = Ji[a][0] * RA[0][b] + Ji[a][1] * RA[1][b] + Ji[a][2] * RA[2][b];
      Js[a][3 + b] = 0.0;
      Js[3 + a][b] = RE[a][0] * XARA[0][b] + RE[a][1] * XARA[1][b] + RE[a][2] * XARA[2][b];
      Js[3 + a][3 + b] = RE[a][0] * RA[0][b] + RE[a][1] * RA[1][b] + RE[a][2] * RA[2][b];
      Jt[a][b] = -(Ji[a][0] * RE[b][0] + Ji[a][1] * RE[b][1] + Ji[a][2] * RE[b][2]);
      Jt[a][3 + b] = 0.0;
      Jt[3 + a][b] = XE[a][b];
      Jt[3 + a][3 + b] = a == b ? -1.0 : 0.0;
    }
}

// every node reaches `ref` over the active edges (active null: all)
bool connected(int32_t n_nodes, int32_t n_edges, const Edge* edges, const char* active, int32_t ref) {
  std::vector<int32_t> root(static_cast<size_t>(n_nodes));
  for (int32_t i = 0; i < n_nodes; ++i) root[size_t(i)] = i;
  auto find = [&](int32_t i) {
    while (root[size_t(i)] != i) { root[size_t(i)] = root[size_t(root[size_t(i)])]; i = root[size_t(i)]; }
    return i;
  };
  for (int32_t k = 0; k < n_edges; ++k)
    if (!active || active[k]) root[size_t(find(edges[k].source))] = find(edges[k].target);
  const int32_t r = find(ref);
  for (int32_t i = 0; i < n_nodes; ++i) if (find(i) != r) return false;
  return true;
}

// A = L L^T in place (lower triangle, row-major n x n); false when A is not positive definite
bool cholesky(std::vector<double>& A, int n) {
  for (int u = 0; u < n; ++u) {
    double* Lu = &A[size_t(u) * n];
    for (int v = 0; v <= u; ++v) {
      const double* Lv = &A[size_t(v) * n];
      double acc = Lu[v];
      for (int k = 0; k < v; ++k) acc -= Lu[k] * Lv[k];
      if (u == v) {
        if (!(acc > 0.0) || !std::isfinite(acc)) return false;
        Lu[u] = std::sqrt(acc);
      } else {
        Lu[v] = acc / Lv[v];
      }
    }
  }
  return true;
}

void cholesky_solve(const std::vector<double>& L, int n, const double* b, double* x) {
  std::vector<double> y(static_cast<size_t>(n));
  for (int u = 0; u < n; ++u) {
    double acc = b[u];
    for (int k = 0; k < u; ++k) acc -= L[size_t(u) * n + k] * y[size_t(k)];
    y[size_t(u)] = acc / L[size_t(u) * n + u];
  }
  for (int u = n - 1; u >= 0; --u) {
    double acc = y[size_t(u)];
    for (int k = u + 1; k < n; ++k) acc -= L[size_t(k) * n + u] * x[k];
    x[u] = acc / L[size_t(u) * n + u];
  }
}

// H (dim x dim, both triangles) and g of the active edges at the poses: the header's matrix and gradient
void build_system(const double* poses, int32_t n_edges, const Edge* edges, const char* active, int32_t ref, double mu, int dim,
                  std::vector<double>& H, std::vector<double>& g) {
  std::fill(H.begin(), H.end(), 0.0);
  std::fill(g.begin(), g.end(), 0.0);
  for (int32_t k = 0; k < n_edges; ++k) {
    if (!active[k]) continue;
    const Edge& e = edges[k];
    double E[16], r[6], J[2][6][6], LJ[2][6][6], u[2][6], Lr[6];
    residual(poses + 16 * e.source, poses + 16 * e.target, e, E, r);
    jacobians(E, r, e, J[0], J[1]);
    const double c = quad(e.info, r), l = line_value(e, c, mu);
    const double d2 = e.uncertain && c < mu / 3.0 ? -4.0 * (mu * mu) / ((mu + c) * (mu + c) * (mu + c)) : 0.0;   // 2 rho''
    for (int a = 0; a < 6; ++a) {
      Lr[a] = 0.0;
      for (int b = 0; b < 6; ++b) Lr[a] += e.info[6 * a + b] * r[b];
    }
    const int32_t node[2] = {e.source, e.target};
    int off[2];
    for (int s = 0; s < 2; ++s) {
      off[s] = node[s] == ref ? -1 : 6 * (node[s] < ref ? node[s] : node[s] - 1);
      for (int a = 0; a < 6; ++a) {
        u[s][a] = 0.0;
        for (int b = 0; b < 6; ++b) {
          u[s][a] += J[s][b][a] * Lr[b];
          double v = 0.0;
          for (int m = 0; m < 6; ++m) v += e.info[6 * a + m] * J[s][m][b];
          LJ[s][a][b] = v;
        }
      }
    }
    for (int s = 0; s < 2; ++s) {
      if (off[s] < 0) continue;
      for (int a = 0; a < 6; ++a) g[size_t(off[s] + a)] += l * u[s][a];
      for (int t = 0; t < 2; ++t) {
        if (off[t] < 0) continue;
        for (int a = 0; a < 6; ++a)
          for (int b = 0; b < 6; ++b) {
            double v = 0.0;
            for (int m = 0; m < 6; ++m) v += J[s][m][a] * LJ[t][m][b];
            H[size_t(off[s] + a) * dim + size_t(off[t] + b)] += l * v + d2 * (u[s][a] * u[t][b]);
          }
      }
    }
  }
}

// One Levenberg-Marquardt stage over the active edges; poses (all n_nodes) in and out, F_end and the iterations out.
int32_t run_stage(int32_t n_nodes, std::vector<double>& poses, int32_t n_edges, const Edge* edges, const char* active, int32_t ref,
                  double mu, const s4p_icp_posegraph_params& P, int32_t* iterations, double* F_end) {
  const int dim = 6 * (n_nodes - 1);
  double F = cost(poses.data(), n_edges, edges, active, mu, nullptr, nullptr);
  *iterations = 0;
  *F_end = F;
  if (dim == 0) return S4P_ICP_POSEGRAPH_CONVERGED;
  const size_t n = static_cast<size_t>(dim);
  std::vector<double> H(n * n), A(n * n), g(n), step(n), trial(poses.size());
  double lambda = kLambda0;
  bool rebuild = true;
  int32_t status = S4P_ICP_POSEGRAPH_MAX_ITERATIONS;
  while (*iterations < P.max_iterations) {
    if (F == 0.0) { status = S4P_ICP_POSEGRAPH_CONVERGED; break; }
    if (rebuild) build_system(poses.data(), n_edges, edges, active, ref, mu, dim, H, g);
    rebuild = false;
    A = H;
    for (int u = 0; u < dim; ++u) A[size_t(u) * dim + u] += lambda * H[size_t(u) * dim + u];
    ++*iterations;
    bool kept = false;
    if (cholesky(A, dim)) {
      cholesky_solve(A, dim, g.data(), step.data());
      trial = poses;
      for (int32_t i = 0; i < n_nodes; ++i) {
        if (i == ref) continue;
        double d[6];
        const int o = 6 * (i < ref ? i : i - 1);
        for (int a = 0; a < 6; ++a) d[a] = -step[size_t(o + a)];
        retract(&poses[size_t(16) * i], d, &trial[size_t(16) * i]);
      }
      const double Fn = cost(trial.data(), n_edges, edges, active, mu, nullptr, nullptr);
      if (Fn < F) {
        const double fall = F - Fn;
        const bool done = fall <= P.rel_tol * F;
        poses.swap(trial);
        F = Fn;
        kept = rebuild = true;
        lambda = std::max(lambda * 0.1, kLambdaMin);
        if (done) { status = S4P_ICP_POSEGRAPH_CONVERGED; break; }
      }
    }
    if (!kept) {
      lambda *= 10.0;
      if (lambda > kLambdaMax) { status = S4P_ICP_POSEGRAPH_STALLED; break; }
    }
  }
  *F_end = F;
  return status;
}

bool finite_all(const double* v, int n) {
  for (int k = 0; k < n; ++k) if (!std::isfinite(v[k])) return false;
  return true;
}

bool edges_in_range(int32_t n_nodes, int32_t n_edges, const Edge* edges) {
  for (int32_t k = 0; k < n_edges; ++k) {
    const Edge& e = edges[k];
    if (e.source < 0 || e.source >= n_nodes || e.target < 0 || e.target >= n_nodes || e.source == e.target) return false;
    if (e.uncertain != 0 && e.uncertain != 1) return false;
  }
  return true;
}

}  // namespace pg
}  // namespace

extern "C" {

void s4p_icp_posegraph_default_params(s4p_icp_posegraph_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->max_iterations = 100;
  p->reference = 0;
  p->line_process_weight = 0.0;
  p->prune_threshold = 0.25;
  p->rel_tol = 1e-12;
}

double s4p_icp_posegraph_cost(int32_t n_nodes, const double* poses, int32_t n_edges, const s4p_icp_posegraph_edge* edges, double mu,
                              double* chi2_out) {
  if (n_nodes < 1 || !poses || n_edges < 0 || (n_edges > 0 && !edges) || !pg::edges_in_range(n_nodes, n_edges, edges)) return NAN;
  for (int32_t k = 0; k < n_edges; ++k) if (edges[k].uncertain && !(mu > 0.0 && std::isfinite(mu))) return NAN;
  return pg::cost(poses, n_edges, edges, nullptr, mu, chi2_out, nullptr);
}

int32_t s4p_icp_posegraph_optimize(int32_t n_nodes, double* poses_inout, int32_t n_edges, const s4p_icp_posegraph_edge* edges,
                                   const s4p_icp_posegraph_params* params, double* line_out, s4p_icp_posegraph_result* result) {
  if (n_nodes < 1 || n_nodes > S4P_ICP_POSEGRAPH_MAX_NODES || !poses_inout || n_edges < 0 || (n_edges > 0 && !edges))
    return S4P_ICP_ERR_BAD_ARG;
  s4p_icp_posegraph_params P;
  s4p_icp_posegraph_default_params(&P);
  if (params) P = *params;
  if (P.max_iterations < 0 || P.reference < 0 || P.reference >= n_nodes || !(P.prune_threshold >= 0.0) || !(P.rel_tol >= 0.0))
    return S4P_ICP_ERR_BAD_ARG;
  if (!pg::edges_in_range(n_nodes, n_edges, edges) || !pg::finite_all(poses_inout, 16 * n_nodes)) return S4P_ICP_ERR_BAD_ARG;
  bool any_uncertain = false;
  for (int32_t k = 0; k < n_edges; ++k) {
    const s4p_icp_posegraph_edge& e = edges[k];
    if (!pg::finite_all(e.T, 16) || !pg::finite_all(e.info, 36)) return S4P_ICP_ERR_BAD_ARG;
    double big = 0.0;
    for (int a = 0; a < 36; ++a) big = std::max(big, std::fabs(e.info[a]));
    for (int a = 0; a < 6; ++a)
      for (int b = a + 1; b < 6; ++b)
        if (std::fabs(e.info[6 * a + b] - e.info[6 * b + a]) > 1e-9 * big) return S4P_ICP_ERR_BAD_ARG;
    any_uncertain = any_uncertain || e.uncertain != 0;
  }
  const double mu = P.line_process_weight;
  if (any_uncertain && !(mu > 0.0 && std::isfinite(mu))) return S4P_ICP_ERR_BAD_ARG;
  if (!pg::connected(n_nodes, n_edges, edges, nullptr, P.reference)) return S4P_ICP_ERR_BAD_ARG;

  s4p_icp_posegraph_result R;
  std::memset(&R, 0, sizeof(R));
  std::vector<double> poses(poses_inout, poses_inout + size_t(16) * n_nodes), chi2(size_t(std::max(n_edges, 1))),
      line(size_t(std::max(n_edges, 1)), 1.0);
  std::vector<char> active(size_t(std::max(n_edges, 1)), 1);
  R.cost_start = pg::cost(poses.data(), n_edges, edges, active.data(), mu, nullptr, nullptr);
  R.status = pg::run_stage(n_nodes, poses, n_edges, edges, active.data(), P.reference, mu, P, &R.iterations[0], &R.cost_end);
  pg::cost(poses.data(), n_edges, edges, active.data(), mu, chi2.data(), line.data());
  for (int32_t k = 0; k < n_edges; ++k)
    if (edges[k].uncertain && line[size_t(k)] < P.prune_threshold) { active[size_t(k)] = 0; ++R.n_pruned; }
  if (R.n_pruned > 0) {
    if (!pg::connected(n_nodes, n_edges, edges, active.data(), P.reference)) {
      R.status = S4P_ICP_POSEGRAPH_STAGE2_SKIPPED;
    } else {
      R.status = pg::run_stage(n_nodes, poses, n_edges, edges, active.data(), P.reference, mu, P, &R.iterations[1], &R.cost_end);
      pg::cost(poses.data(), n_edges, edges, active.data(), mu, chi2.data(), line.data());       // pruned edges keep stage 1's
    }
  }
  for (int32_t i = 0; i < n_nodes; ++i)
    if (i != P.reference) std::memcpy(poses_inout + size_t(16) * i, &poses[size_t(16) * i], 16 * sizeof(double));
  if (line_out) for (int32_t k = 0; k < n_edges; ++k) line_out[k] = line[size_t(k)];
  if (result) *result = R;
  return S4P_ICP_OK;
}

}  // extern "C"
