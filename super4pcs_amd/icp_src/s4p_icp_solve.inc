// s4p_icp_solve.inc -- host only: the closed-form solves of the two kinds of sums and the transform helpers.

namespace s4p_icp {

// ---------------------------------------------------------------------------------------------------------------------
// host: Horn's closed form.  N (4x4 symmetric) from the centred cross-covariance; its eigenvector of the largest
// eigenvalue (cyclic Jacobi) is the unit quaternion of the rotation.
void jacobi4(double A[4][4], double V[4][4]) {
  for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 64; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < 4; ++i) { diag += A[i][i] * A[i][i]; for (int j = i + 1; j < 4; ++j) off += A[i][j] * A[i][j]; }
    if (off == 0.0 || off <= 1e-36 * diag) break;
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 4; ++q) {
        if (A[p][q] == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 4; ++k) {            // A <- J^T A J, columns then rows
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 4; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < 4; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq;
        }
      }
  }
}

void mat_mul4(const double* A, const double* B, double* C) {    // C = A B (row-major 4x4); C may not alias
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      double v = 0.0;
      for (int k = 0; k < 4; ++k) v += A[4 * r + k] * B[4 * k + c];
      C[4 * r + c] = v;
    }
}

// caller frame <-> centred frame (p' = p - c, q' = q - c): T' = [R | R c + t - c], T = [R | t' - R c + c]
void to_centred(const double* T, const float* c, double* Tc) {
  std::memcpy(Tc, T, 16 * sizeof(double));
  for (int r = 0; r < 3; ++r) Tc[4 * r + 3] = T[4 * r + 3] + (T[4 * r] * c[0] + T[4 * r + 1] * c[1] + T[4 * r + 2] * c[2]) - double(c[r]);
}
void from_centred(const double* Tc, const float* c, double* T) {
  std::memcpy(T, Tc, 16 * sizeof(double));
  for (int r = 0; r < 3; ++r) T[4 * r + 3] = Tc[4 * r + 3] - (Tc[4 * r] * c[0] + Tc[4 * r + 1] * c[1] + Tc[4 * r + 2] * c[2]) + double(c[r]);
}
Tf to_float(const double* T) {
  Tf f;
  for (int k = 0; k < 12; ++k) f.m[k] = float(T[k]);
  return f;
}

}  // namespace s4p_icp

using namespace s4p_icp;

namespace {

Tf centred_from_float16(const float* T16) {
  Tf f;
  for (int k = 0; k < 12; ++k) f.m[k] = T16[k];
  return f;
}

// The 6x6 step of the 31 sums (include/s4p_icp_plane.h's layout), shared by s4p_icp_solve_plane and s4p_icp_solve_symmetric:
// x = (rotation part, translation part) of A x = b, or S4P_ICP_ERR_DEGENERATE.
int32_t solve_sums6(const double* sums, double* x) {
  if (!(sums[2] >= 6.0)) return S4P_ICP_ERR_DEGENERATE;
  double A[6][6], b[6];
  for (int u = 0, o = 4; u < 6; ++u)
    for (int v = u; v < 6; ++v, ++o) A[u][v] = A[v][u] = sums[o];
  for (int u = 0; u < 6; ++u) b[u] = sums[25 + u];
  // balance the rotation block (length^2) against the translation block (unitless): the test below is unit-free
  const double tw = A[0][0] + A[1][1] + A[2][2], tt = A[3][3] + A[4][4] + A[5][5];
  if (!(tw > 0.0) || !(tt > 0.0) || !std::isfinite(tw) || !std::isfinite(tt)) return S4P_ICP_ERR_DEGENERATE;
  const double sc = std::sqrt(tt / tw);
  const double D[6] = {sc, sc, sc, 1.0, 1.0, 1.0};
  double B[6][6], E[6][6], V[6][6], bb[6];
  for (int u = 0; u < 6; ++u) {
    bb[u] = D[u] * b[u];
    for (int v = 0; v < 6; ++v) B[u][v] = E[u][v] = D[u] * A[u][v] * D[v];
  }
  jacobi_sym<6>(E, V);
  double lmin = E[0][0], lmax = E[0][0];
  for (int u = 1; u < 6; ++u) { lmin = std::min(lmin, E[u][u]); lmax = std::max(lmax, E[u][u]); }
  if (!(lmin > 1e-10 * lmax)) return S4P_ICP_ERR_DEGENERATE;
  // Cholesky B = L L^T, then B y = D b, x = D y
  double L[6][6] = {};
  for (int u = 0; u < 6; ++u)
    for (int v = 0; v <= u; ++v) {
      double acc = B[u][v];
      for (int k = 0; k < v; ++k) acc -= L[u][k] * L[v][k];
      if (u == v) {
        if (!(acc > 0.0)) return S4P_ICP_ERR_DEGENERATE;
        L[u][u] = std::sqrt(acc);
      } else {
        L[u][v] = acc / L[v][v];
      }
    }
  double y[6];
  for (int u = 0; u < 6; ++u) {
    double acc = bb[u];
    for (int k = 0; k < u; ++k) acc -= L[u][k] * y[k];
    y[u] = acc / L[u][u];
  }
  for (int u = 5; u >= 0; --u) {
    double acc = y[u];
    for (int k = u + 1; k < 6; ++k) acc -= L[k][u] * x[k];
    x[u] = acc / L[u][u];
  }
  for (int u = 0; u < 6; ++u) x[u] *= D[u];
  return S4P_ICP_OK;
}

}  // namespace

extern "C" {

int32_t s4p_icp_solve(const double* sums, double* dT16) {
  if (!sums || !dT16) return S4P_ICP_ERR_BAD_ARG;
  const double n = sums[0];
  if (!(n >= 1.0)) return S4P_ICP_ERR_BAD_ARG;
  double mq[3], mp[3], S[3][3];
  for (int a = 0; a < 3; ++a) { mq[a] = sums[1 + a] / n; mp[a] = sums[4 + a] / n; }
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) S[a][b] = sums[7 + 3 * a + b] / n - mq[a] * mp[b];
  const double Sxx = S[0][0], Sxy = S[0][1], Sxz = S[0][2], Syx = S[1][0], Syy = S[1][1], Syz = S[1][2], Szx = S[2][0],
               Szy = S[2][1], Szz = S[2][2];
  double N[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                    {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                    {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                    {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
  double V[4][4];
  jacobi4(N, V);
  int best = 0;
  for (int k = 1; k < 4; ++k) if (N[k][k] > N[best][best]) best = k;
  double w = V[0][best], x = V[1][best], y = V[2][best], z = V[3][best];
  const double nq = std::sqrt(w * w + x * x + y * y + z * z);
  w /= nq; x /= nq; y /= nq; z /= nq;
  const double R[3][3] = {{w * w + x * x - y * y - z * z, 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)},
                          {2.0 * (x * y + w * z), w * w - x * x + y * y - z * z, 2.0 * (y * z - w * x)},
                          {2.0 * (x * z - w * y), 2.0 * (y * z + w * x), w * w - x * x - y * y + z * z}};
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) dT16[4 * r + c] = R[r][c];
    dT16[4 * r + 3] = mp[r] - (R[r][0] * mq[0] + R[r][1] * mq[1] + R[r][2] * mq[2]);
  }
  dT16[12] = dT16[13] = dT16[14] = 0.0;
  dT16[15] = 1.0;
  return S4P_ICP_OK;
}

int32_t s4p_icp_solve_plane(const double* sums, double* dT16) {
  if (!sums || !dT16) return S4P_ICP_ERR_BAD_ARG;
  double x[6];
  if (int32_t rc = solve_sums6(sums, x)) return rc;
  // exact rotation of omega (Rodrigues): R = I + sin(th)/th K + (1 - cos(th))/th^2 K^2, K = [omega]x, K^2 = w w^T - th^2 I
  const double w[3] = {x[0], x[1], x[2]};
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = std::sqrt(th2);
  const double c1 = th > 0.0 ? std::sin(th) / th : 1.0;
  const double sh = th > 0.0 ? std::sin(0.5 * th) / th : 0.5;
  const double c2 = 2.0 * sh * sh;                                  // (1 - cos th) / th^2 without cancellation
  const double K[3][3] = {{0.0, -w[2], w[1]}, {w[2], 0.0, -w[0]}, {-w[1], w[0], 0.0}};
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) dT16[4 * r + c] = (r == c ? 1.0 : 0.0) + c1 * K[r][c] + c2 * (w[r] * w[c] - (r == c ? th2 : 0.0));
    dT16[4 * r + 3] = x[3 + r];
  }
  dT16[12] = dT16[13] = dT16[14] = 0.0;
  dT16[15] = 1.0;
  return S4P_ICP_OK;
}

int32_t s4p_icp_solve_symmetric(const double* sums, double* dT16) {
  if (!sums || !dT16) return S4P_ICP_ERR_BAD_ARG;
  double x[6];
  if (int32_t rc = solve_sums6(sums, x)) return rc;
  // Rh: the rotation by atan |a~| about a~ (include/s4p_icp_symm.h); dT = [Rh Rh | Rh t'], t' = c t~
  const double w[3] = {x[0], x[1], x[2]};
  const double m2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
  const double c = 1.0 / std::sqrt(1.0 + m2), k = (c * c) / (1.0 + c);
  const double K[3][3] = {{0.0, -w[2], w[1]}, {w[2], 0.0, -w[0]}, {-w[1], w[0], 0.0}};
  double Rh[3][3], t[3];
  for (int r = 0; r < 3; ++r) {
    for (int s = 0; s < 3; ++s) Rh[r][s] = ((r == s ? 1.0 : 0.0) + c * K[r][s]) + k * (w[r] * w[s] - (r == s ? m2 : 0.0));
    t[r] = c * x[3 + r];
  }
  for (int r = 0; r < 3; ++r) {
    for (int s = 0; s < 3; ++s) dT16[4 * r + s] = (Rh[r][0] * Rh[0][s] + Rh[r][1] * Rh[1][s]) + Rh[r][2] * Rh[2][s];
    dT16[4 * r + 3] = (Rh[r][0] * t[0] + Rh[r][1] * t[1]) + Rh[r][2] * t[2];
  }
  dT16[12] = dT16[13] = dT16[14] = 0.0;
  dT16[15] = 1.0;
  return S4P_ICP_OK;
}

}  // extern "C"
