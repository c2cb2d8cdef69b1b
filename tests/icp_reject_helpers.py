"""Test-side restatement of the correspondence-rejection contract (include/s4p_icp_reject.h) in numpy, on top of the
correspondence restatement (tests/icp_cpu through tests/icp_helpers.py, or numpy_brute on small clouds): the reverse search
is the same search with the roles swapped, the normal test a few lines in double.  Expected sums come from the existing
helpers of each metric fed the kept index array; this file adds only the sum of |term| of the point and plane sums, the
scale of their rounding."""
import numpy as np

from tests import icp_helpers as H
from tests import icp_robust_helpers as RH

KEPT, UNMATCHED, NORMALS, RECIPROCITY = 0, 1, 2, 3
I4 = np.eye(4, dtype=np.float32)


def reverse_map(T):
    """T- = [M^T | t-] as float32 4x4: the transposed float entries and t-_a = float(-((m_0a t_0 + m_1a t_1) + m_2a t_2)) in double."""
    T = np.asarray(T, np.float32).reshape(4, 4)
    R = np.eye(4, dtype=np.float32)
    R[:3, :3] = T[:3, :3].T
    m, t = T[:3, :3].astype(np.float64), T[:3, 3].astype(np.float64)
    for a in range(3):
        R[a, 3] = np.float32(-((m[0, a] * t[0] + m[1, a] * t[1]) + m[2, a] * t[2]))
    return R


def cpu_search(cpu):
    return lambda Pc, Qc, T, d: cpu.pass_(Pc, Qc, T, d)[:2]


def normal_cosines(T, idx, Np, Nq):
    """(c float64[n_Q], info bool[n_Q]) for the matched pairs of idx: c = np . (R nq) in the header's order, info False where
    either stored normal is zero (or the point is unmatched)."""
    T = np.asarray(T, np.float32).reshape(4, 4)
    R = T[:3, :3].astype(np.float64)
    hit = idx >= 0
    n_p = np.asarray(Np, np.float32)[np.maximum(idx, 0)].astype(np.float64)
    n_q = np.asarray(Nq, np.float32).astype(np.float64)
    nh = np.stack([(R[a, 0] * n_q[:, 0] + R[a, 1] * n_q[:, 1]) + R[a, 2] * n_q[:, 2] for a in range(3)], 1)
    c = (n_p[:, 0] * nh[:, 0] + n_p[:, 1] * nh[:, 1]) + n_p[:, 2] * nh[:, 2]
    info = hit & np.any(n_p != 0, axis=1) & np.any(n_q != 0, axis=1)
    return c, info


def reverse_search(search, Pc, Qc, T, d, targets):
    """r(i) for the target indices `targets`: the source index nearest to p~ = T- p'_i within d (ties to the smallest), or -1."""
    pt = RH.apply_f32(reverse_map(T), np.ascontiguousarray(Pc[targets], np.float32)).astype(np.float32)
    return search(Qc, pt, I4, d)[0]


def restate(search, Pc, Qc, T, d, reciprocal=False, normal_mode=0, normal_cos=0.0, Np=None, Nq=None, forward=None):
    """(idx, d2, why, counts) of s4p_icp_rejection and s4p_icp_rejection_counts for centred clouds and a float T.  forward:
    the one-way search's (idx, d2) for the same arguments, when the caller has it already."""
    fi, fd = search(Pc, Qc, T, d) if forward is None else forward
    why = np.where(fi >= 0, KEPT, UNMATCHED).astype(np.int32)
    if normal_mode:
        c, info = normal_cosines(T, fi, Np, Nq)
        ok = (np.abs(c) if normal_mode == 1 else c) >= normal_cos
        why[info & ~ok] = NORMALS
    if reciprocal:
        cand = np.flatnonzero(why == KEPT)
        targets = np.unique(fi[cand])
        if len(targets):
            back = np.full(len(Pc), -2, np.int64)
            back[targets] = reverse_search(search, Pc, Qc, T, d, targets)
            why[cand[back[fi[cand]] != cand]] = RECIPROCITY
    kept = why == KEPT
    idx = np.where(kept, fi, -1).astype(np.int32)
    d2 = np.where(kept, fd, np.float32(0)).astype(np.float32)
    counts = np.array([(fi >= 0).sum(), (why == NORMALS).sum(), (why == RECIPROCITY).sum(), kept.sum()], np.int64)
    return idx, d2, why, counts


def sums_abs(Pc, Qc, T, idx, d2, metric, Nc=None, loss=None, n_q=None, d=None, **kw):
    """Sum of |term| of every entry of the 17 point or 31 plane sums over the pairs of idx, weighted as
    RH.robust_sums weights them (loss None: every weight 1)."""
    qh = RH.apply_f32(T, Qc)
    hit = idx >= 0
    q = qh[hit].astype(np.float64); p = Pc[idx[hit]].astype(np.float64); dd = d2[hit].astype(np.float64)

    def weights(u):
        if loss is None:
            return np.ones(len(u))
        _, thr, s = RH.scale_and_k(u, loss, n_q, d, kw.get("trim_fraction"), kw.get("scale"))
        return RH.weights(u, loss, thr, s, kw.get("c"))

    if metric == "point":
        w = weights(d2[hit].astype(np.float32))
        terms = [w] + [q[:, a] * w for a in range(3)] + [p[:, a] * w for a in range(3)]
        terms += [q[:, a] * p[:, b] * w for a in range(3) for b in range(3)] + [dd * w]
        return np.array([np.abs(t).sum() for t in terms])
    nv = np.asarray(Nc, np.float32)[idx[hit]].astype(np.float64)
    nz = np.any(nv != 0, axis=1)
    qk, pk, nk = q[nz], p[nz], nv[nz]
    r = ((pk[:, 0] - qk[:, 0]) * nk[:, 0] + (pk[:, 1] - qk[:, 1]) * nk[:, 1]) + (pk[:, 2] - qk[:, 2]) * nk[:, 2]
    w = weights((r * r).astype(np.float32))
    a = np.concatenate([np.cross(qk, nk), nk], axis=1)
    out = [np.count_nonzero(~nz) + np.abs(w).sum(), dd[~nz].sum() + (dd[nz] * w).sum(), float(np.count_nonzero(w > 0)), (r * r * w).sum()]
    out += [np.abs(a[:, u] * a[:, v] * w).sum() for u in range(6) for v in range(u, 6)]
    out += [np.abs(a[:, u] * r * w).sum() for u in range(6)]
    return np.array(out, np.float64)


def cpu_refine_reject(cpu, solve, Pc, Qc, c, T0, d, max_iterations=30, rel_tol=1e-6, min_correspondences=3, **rej):
    """The loop of s4p_icp_refine under rejection on the restatement: (T caller frame, iterations, status, rmse history,
    count history)."""
    def step(Tf):
        idx, d2, _, _ = restate(cpu_search(cpu), Pc, Qc, Tf, d, **rej)
        s = RH.robust_sums(Pc, Qc, Tf, idx, d2, "point", "trimmed", len(Qc), d, trim_fraction=1.0)[0]    # every weight 1
        return s, s[0]
    return H.refine_loop(step, solve, c, T0, max_iterations, rel_tol, min_correspondences)


def cpu_refine_gicp_reject(cpu, solve_plane, Pc, Qc, Np, Nq, c, T0, d, eps=1e-3, max_iterations=30, rel_tol=1e-6, min_correspondences=3,
                           **rej):
    """The loop of s4p_icp_refine_gicp under rejection on the restatement (tests/icp_gicp_helpers.py's sums on the kept pairs)."""
    from tests import icp_gicp_helpers as GH

    def step(Tf):
        idx, d2, _, _ = restate(cpu_search(cpu), Pc, Qc, Tf, d, Np=Np, Nq=Nq, **rej)
        s = GH.gicp_sums(Pc, Qc, Tf, idx, d2, Np, Nq, eps)[0]
        return s, s[0]
    return H.refine_loop(step, solve_plane, c, T0, max_iterations, rel_tol, min_correspondences)
