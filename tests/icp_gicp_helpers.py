"""Test-side restatement of the generalized ICP contract (include/s4p_icp_gicp.h) in numpy: the 31 generalized sums, term by
term in the header's operation order, on top of the correspondence restatement (tests/icp_cpu), and the refine loop on top
of them with the library's host solve (s4p_icp_solve_plane)."""
import numpy as np

from tests import icp_helpers as H


def pair_terms(Pc, Qc, T, idx, Np, Nq, eps):
    """Per matched pair, in double and in the header's order: (q^, r, S as a dict of its 6 entries, M (n, 3, 3))."""
    T = np.asarray(T, np.float32).reshape(4, 4)
    x, y, z = Qc[:, 0], Qc[:, 1], Qc[:, 2]
    qh = np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1)      # float32
    hit = idx >= 0
    q = qh[hit].astype(np.float64)
    p = Pc[idx[hit]].astype(np.float64)
    n_p = np.asarray(Np, np.float32)[idx[hit]].astype(np.float64)
    n_q = np.asarray(Nq, np.float32)[hit].astype(np.float64)
    R = T[:3, :3].astype(np.float64)
    nh = np.stack([(R[a, 0] * n_q[:, 0] + R[a, 1] * n_q[:, 1]) + R[a, 2] * n_q[:, 2] for a in range(3)], 1)
    k = 1.0 - float(eps)
    S = {}
    for a in range(3):
        for b in range(a, 3):
            S[a, b] = ((2.0 if a == b else 0.0) - k * (n_p[:, a] * n_p[:, b])) - k * (nh[:, a] * nh[:, b])
    c00 = S[1, 1] * S[2, 2] - S[1, 2] * S[1, 2]
    c01 = S[0, 2] * S[1, 2] - S[0, 1] * S[2, 2]
    c02 = S[0, 1] * S[1, 2] - S[0, 2] * S[1, 1]
    c11 = S[0, 0] * S[2, 2] - S[0, 2] * S[0, 2]
    c12 = S[0, 1] * S[0, 2] - S[0, 0] * S[1, 2]
    c22 = S[0, 0] * S[1, 1] - S[0, 1] * S[0, 1]
    det = (S[0, 0] * c00 + S[0, 1] * c01) + S[0, 2] * c02
    M = np.empty((len(q), 3, 3))
    M[:, 0, 0], M[:, 0, 1], M[:, 0, 2] = c00 / det, c01 / det, c02 / det
    M[:, 1, 1], M[:, 1, 2], M[:, 2, 2] = c11 / det, c12 / det, c22 / det
    M[:, 1, 0], M[:, 2, 0], M[:, 2, 1] = M[:, 0, 1], M[:, 0, 2], M[:, 1, 2]
    return q, p - q, S, M


def gicp_sums(Pc, Qc, T, idx, d2, Np, Nq, eps):
    """(s, sabs): the 31 generalized sums for a float T (centred), the correspondences (idx, d2), the stored target normals
    Np and source normals Nq (uploaded order) and epsilon; sabs[k] = sum |term| of s[k] (the scale of its rounding)."""
    q, r, _, M = pair_terms(Pc, Qc, T, idx, Np, Nq, eps)
    hit = idx >= 0
    g = np.stack([(M[:, a, 0] * r[:, 0] + M[:, a, 1] * r[:, 1]) + M[:, a, 2] * r[:, 2] for a in range(3)], 1)
    B = np.empty_like(M)
    for c in range(3):
        B[:, 0, c] = q[:, 1] * M[:, 2, c] - q[:, 2] * M[:, 1, c]
        B[:, 1, c] = q[:, 2] * M[:, 0, c] - q[:, 0] * M[:, 2, c]
        B[:, 2, c] = q[:, 0] * M[:, 1, c] - q[:, 1] * M[:, 0, c]
    W = np.empty_like(M)
    for a in range(3):
        W[:, a, 0] = q[:, 1] * B[:, a, 2] - q[:, 2] * B[:, a, 1]
        W[:, a, 1] = q[:, 2] * B[:, a, 0] - q[:, 0] * B[:, a, 2]
        W[:, a, 2] = q[:, 0] * B[:, a, 1] - q[:, 1] * B[:, a, 0]
    h = np.stack([q[:, 1] * g[:, 2] - q[:, 2] * g[:, 1], q[:, 2] * g[:, 0] - q[:, 0] * g[:, 2], q[:, 0] * g[:, 1] - q[:, 1] * g[:, 0]], 1)
    n = len(q)
    one = np.ones(n)
    terms = [one, d2[hit].astype(np.float64), one, (r[:, 0] * g[:, 0] + r[:, 1] * g[:, 1]) + r[:, 2] * g[:, 2],
             W[:, 0, 0], W[:, 0, 1], W[:, 0, 2], B[:, 0, 0], B[:, 0, 1], B[:, 0, 2],
             W[:, 1, 1], W[:, 1, 2], B[:, 1, 0], B[:, 1, 1], B[:, 1, 2],
             W[:, 2, 2], B[:, 2, 0], B[:, 2, 1], B[:, 2, 2],
             M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2],
             h[:, 0], h[:, 1], h[:, 2], g[:, 0], g[:, 1], g[:, 2]]
    s = np.array([t.sum() for t in terms])
    sabs = np.array([np.abs(t).sum() for t in terms])
    return s, sabs


def sigma_spectrum(Pc, Qc, T, idx, Np, Nq, eps):
    """Eigenvalues (n, 3), ascending, of every pair's S = C(np) + C(nh)."""
    _, _, S, _ = pair_terms(Pc, Qc, T, idx, Np, Nq, eps)
    n = len(S[0, 0])
    F = np.empty((n, 3, 3))
    for (a, b), v in S.items():
        F[:, a, b] = v
        F[:, b, a] = v
    return np.linalg.eigvalsh(F)


def cpu_refine_gicp(cpu, solve_plane, Pc, Qc, Np, Nq, c, T0, d, eps=1e-3, max_iterations=30, rel_tol=1e-6, min_correspondences=3):
    """The refine loop of s4p_icp_refine_gicp on the CPU restatement: (T caller frame, iterations, status, history)."""
    def step(Tf):
        idx, d2, _ = cpu.pass_(Pc, Qc, Tf, d)
        s = gicp_sums(Pc, Qc, Tf, idx, d2, Np, Nq, eps)[0]
        return s, s[0]
    return H.refine_loop(step, solve_plane, c, T0, max_iterations, rel_tol, min_correspondences)[:4]
