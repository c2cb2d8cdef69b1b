"""Test-side restatement of the symmetric ICP contract (include/s4p_icp_symm.h) in numpy: the 31 symmetric sums, term by term
in the header's operation order, on top of the correspondence restatement (tests/icp_cpu); the symmetric step in numpy; the
refine loop on top of the sums with the library's host solve (s4p_icp_solve_symmetric); and the analytic bumpy pair of the
host tests."""
import numpy as np

from tests import icp_helpers as H


def pair_terms(Pc, Qc, T, idx, Np, Nq, ft=np.float32):
    """Per matched pair, in double and in the header's order: (u, v, n, dot, np, nh) with u = q^, v = p', n the sum of the
    two normals brought to one side, dot = np . nh.  ft: the type of the stored clouds, normals and T (float32 is the
    contract; float64 serves the analytic loop, where the pose is to be reached to 1e-9)."""
    T = np.asarray(T, ft).reshape(4, 4)
    Qc = np.asarray(Qc, ft)
    x, y, z = Qc[:, 0], Qc[:, 1], Qc[:, 2]
    qh = np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1)      # in ft
    hit = idx >= 0
    u = qh[hit].astype(np.float64)
    v = np.asarray(Pc, ft)[idx[hit]].astype(np.float64)
    n_p = np.asarray(Np, ft)[idx[hit]].astype(np.float64)
    m = np.asarray(Nq, ft)[hit].astype(np.float64)
    R = T[:3, :3].astype(np.float64)
    nh = np.stack([(R[a, 0] * m[:, 0] + R[a, 1] * m[:, 1]) + R[a, 2] * m[:, 2] for a in range(3)], 1)
    dot = (n_p[:, 0] * nh[:, 0] + n_p[:, 1] * nh[:, 1]) + n_p[:, 2] * nh[:, 2]
    n = np.where((dot < 0)[:, None], n_p - nh, n_p + nh)
    return u, v, n, dot, n_p, nh


def symm_sums(Pc, Qc, T, idx, d2, Np, Nq, ft=np.float32):
    """(s, sabs): the 31 symmetric sums for a float T (centred), the correspondences (idx, d2), the stored target normals Np
    and source normals Nq (uploaded order); sabs[k] = sum |term| of s[k] (the scale of its rounding)."""
    u, v, n, _, _, _ = pair_terms(Pc, Qc, T, idx, Np, Nq, ft)
    hit = idx >= 0
    dd = np.asarray(d2)[hit].astype(np.float64)
    has = (n != 0).any(1)
    u, v, n = u[has], v[has], n[has]
    e, h = v - u, u + v
    a = np.stack([h[:, 1] * n[:, 2] - h[:, 2] * n[:, 1], h[:, 2] * n[:, 0] - h[:, 0] * n[:, 2], h[:, 0] * n[:, 1] - h[:, 1] * n[:, 0]], 1)
    r = (e[:, 0] * n[:, 0] + e[:, 1] * n[:, 1]) + e[:, 2] * n[:, 2]
    J = np.concatenate([a, n], 1)
    terms = [np.ones(len(dd)), dd, np.ones(len(r)), r * r]
    for i in range(6):
        for k in range(i, 6):
            terms.append(J[:, i] * J[:, k])
    for i in range(6):
        terms.append(J[:, i] * r)
    s = np.array([t.sum() for t in terms])
    sabs = np.array([np.abs(t).sum() for t in terms])
    return s, sabs


def dot_is_decided(Pc, Qc, T, idx, Np, Nq):
    """The sign test's precondition: no matched pair has np . nh == 0 unless one of its two normals is zero."""
    _, _, _, dot, n_p, nh = pair_terms(Pc, Qc, T, idx, Np, Nq)
    return bool(np.all((dot != 0) | ~n_p.any(1) | ~nh.any(1)))


def plane_sums(Pc, Qc, T, idx, d2, Np, ft=np.float32):
    """The 31 point-to-plane sums (include/s4p_icp_plane.h) in the same style: a = q^ x np, n = np, r = (p' - q^) . np."""
    u, v, _, _, n_p, _ = pair_terms(Pc, Qc, T, idx, Np, np.zeros((len(Qc), 3), np.float32), ft)
    hit = idx >= 0
    dd = np.asarray(d2)[hit].astype(np.float64)
    has = n_p.any(1)
    u, v, n = u[has], v[has], n_p[has]
    a = np.cross(u, n)
    r = ((v - u) * n).sum(1)
    J = np.concatenate([a, n], 1)
    A = J.T @ J
    s = np.zeros(31)
    s[0], s[1], s[2], s[3] = len(dd), dd.sum(), len(r), (r * r).sum()
    s[4:25] = A[np.triu_indices(6)]
    s[25:31] = J.T @ r
    return s


def half_rotation(a):
    """Rh of include/s4p_icp_symm.h for a~ = a, and c = cos(atan |a|)."""
    a = np.asarray(a, np.float64)
    m2 = float(a @ a)
    c = 1.0 / np.sqrt(1.0 + m2)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + c * K + (c * c / (1.0 + c)) * (np.outer(a, a) - m2 * np.eye(3)), c


def solve_symmetric_numpy(s):
    """The symmetric step with numpy.linalg.solve on the 6x6 and the header's closed form: dT = [Rh Rh | Rh (c t~)]."""
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = s[4:25]
    A = A + A.T - np.diag(np.diag(A))
    x = np.linalg.solve(A, np.asarray(s[25:31], np.float64))
    Rh, c = half_rotation(x[:3])
    dT = np.eye(4)
    dT[:3, :3] = Rh @ Rh
    dT[:3, 3] = Rh @ (c * x[3:])
    return dT


def cpu_refine_symm(cpu, solve_symmetric, Pc, Qc, Np, Nq, c, T0, d, **kw):
    """The refine loop of s4p_icp_refine_symm on the CPU restatement: (T caller frame, iterations, status, history)."""
    def step(Tf):
        idx, d2, _ = cpu.pass_(Pc, Qc, Tf, d)
        s = symm_sums(Pc, Qc, Tf, idx, d2, Np, Nq)[0]
        return s, s[0]
    return H.refine_loop(step, solve_symmetric, c, T0, **kw)[:4]


def cpu_refine_plane(cpu, solve_plane, Pc, Qc, Np, c, T0, d, **kw):
    """The refine loop of s4p_icp_refine_plane on the same restatement (for iteration counts, not for bits)."""
    def step(Tf):
        idx, d2, _ = cpu.pass_(Pc, Qc, Tf, d)
        s = plane_sums(Pc, Qc, Tf, idx, d2, Np)
        return s, s[0]
    return H.refine_loop(step, solve_plane, c, T0, **kw)[:4]


motion = H.motion


def analytic_pair(n_p=6000, n_q=2500, seed=1):
    """A bumpy analytic surface z = f(x, y) with its analytic normals (float64): P, its normals, and Q = a rigidly moved
    subset of P with the moved normals under random signs.  (P, Np, Q, Nq, M, pick) with Q = M P[pick]: the pose to find
    is inv(M)."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-1.0, 1.0, size=(n_p, 2))
    x, y = xy[:, 0], xy[:, 1]
    z = 0.15 * np.sin(3.0 * x) * np.cos(2.5 * y) + 0.1 * np.cos(4.0 * x + 1.0) + 0.08 * x * y
    fx = 0.45 * np.cos(3.0 * x) * np.cos(2.5 * y) - 0.4 * np.sin(4.0 * x + 1.0) + 0.08 * y
    fy = -0.375 * np.sin(3.0 * x) * np.sin(2.5 * y) + 0.08 * x
    P = np.column_stack([x, y, z])
    Np = np.column_stack([-fx, -fy, np.ones(n_p)])
    Np /= np.linalg.norm(Np, axis=1)[:, None]
    pick = np.sort(rng.choice(n_p, n_q, replace=False))
    M = motion(7.0, [0.03, -0.02, 0.04], axis=(0.5, 0.2, -0.8))
    Q = P[pick] @ M[:3, :3].T + M[:3, 3]
    Nq = (Np[pick] @ M[:3, :3].T) * rng.choice([-1.0, 1.0], size=(n_q, 1))
    return P, Np, Q, Nq, M, pick


def brute_pass(Pc, Qc, T, d):
    """(idx, d2) of the nearest target within d for every q^ = T q' in float64 (the analytic loop needs no bit contract)."""
    T = np.asarray(T, np.float64)
    qh = Qc.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    idx = np.empty(len(qh), np.int64); d2 = np.empty(len(qh))
    Pd = Pc.astype(np.float64)
    for lo in range(0, len(qh), 512):
        D = ((qh[lo:lo + 512, None, :] - Pd[None, :, :]) ** 2).sum(2)
        j = D.argmin(1)
        idx[lo:lo + 512] = j; d2[lo:lo + 512] = D[np.arange(len(j)), j]
    idx[d2 > d * d] = -1
    return idx, d2
