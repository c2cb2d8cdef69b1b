"""Test-side restatement of the robust ICP contract (include/s4p_icp_robust.h) in numpy, on top of the correspondence
restatement (tests/icp_cpu) and the plane restatement (tests/icp_plane_helpers.py): residual keys, the exact order statistic
(np.partition), the weights, the weighted sums and info, and the refine loop with the library's host solves."""
import math

import numpy as np

from tests import icp_helpers as H

LOSSES = ("trimmed", "huber", "tukey")
C_DEFAULT = {"huber": 1.345, "tukey": 4.685}


def apply_f32(T, Qc):
    T = np.asarray(T, np.float32).reshape(4, 4)
    x, y, z = Qc[:, 0], Qc[:, 1], Qc[:, 2]
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1)


def select(u, k):
    """u_(k): the exact k-th smallest (1-based) of the float32 keys u."""
    return np.partition(np.asarray(u, np.float32), k - 1)[k - 1]


def scale_and_k(u, loss, n_q, d, trim_fraction=None, scale=None):
    """(k, threshold key or None, s) of the contract for the keys u (float32, one per keyed pair)."""
    M = len(u)
    if loss == "trimmed":
        k = min(M, max(1, math.ceil(trim_fraction * n_q)))
        return k, (select(u, k) if k > 0 else None), 0.0
    if scale is not None and scale > 0:
        return 0, None, float(scale)
    k = (M + 1) // 2
    smin = 1e-6 * float(np.float32(d))
    if k == 0:
        return 0, None, smin
    thr = select(u, k)
    return k, thr, max(1.4826 * math.sqrt(float(thr)), smin)


def weights(u, loss, thr, s, c=None):
    """w (float64) of the float32 keys u."""
    u = np.asarray(u, np.float32)
    if loss == "trimmed":
        return (u <= thr).astype(np.float64)
    c = C_DEFAULT[loss] if c is None else c
    cs = c * s
    cs2 = cs * cs
    ud = u.astype(np.float64)
    if loss == "huber":
        with np.errstate(divide="ignore"):
            return np.where(ud <= cs2, 1.0, cs / np.sqrt(np.where(ud > 0, ud, 1.0)))
    with np.errstate(divide="ignore", invalid="ignore"):
        t = 1.0 - ud / cs2 if cs2 > 0 else np.zeros_like(ud)
    return np.where(ud < cs2, t * t, 0.0)


def robust_sums(Pc, Qc, T, idx, d2, metric, loss, n_q, d, Nc=None, trim_fraction=None, scale=None, c=None):
    """(sums, info) of s4p_icp_robust_sums for a float T (centred), the correspondences (idx, d2) and, for the plane metric,
    the stored target normals Nc (uploaded order)."""
    qh = apply_f32(T, Qc)
    hit = idx >= 0
    q = qh[hit].astype(np.float64)
    p = Pc[idx[hit]].astype(np.float64)
    dd = d2[hit].astype(np.float64)
    if metric == "point":
        u = d2[hit].astype(np.float32)
        k, thr, s = scale_and_k(u, loss, n_q, d, trim_fraction, scale)
        w = weights(u, loss, thr, s, c)
        out = np.zeros(17)
        out[0] = w.sum()
        out[1:4] = (q * w[:, None]).sum(0)
        out[4:7] = (p * w[:, None]).sum(0)
        out[7:16] = ((q * w[:, None]).T @ p).reshape(9)
        out[16] = (dd * w).sum()
        count = int(np.count_nonzero(w > 0))
    else:
        nv = Nc[idx[hit]].astype(np.float64)
        nz = np.any(nv != 0, axis=1)
        qk, pk, nk = q[nz], p[nz], nv[nz]
        r = ((pk[:, 0] - qk[:, 0]) * nk[:, 0] + (pk[:, 1] - qk[:, 1]) * nk[:, 1]) + (pk[:, 2] - qk[:, 2]) * nk[:, 2]
        u = (r * r).astype(np.float32)
        k, thr, s = scale_and_k(u, loss, n_q, d, trim_fraction, scale)
        w = weights(u, loss, thr, s, c)
        a = np.concatenate([np.cross(qk, nk), nk], axis=1)
        out = np.zeros(31)
        n_free = int(np.count_nonzero(~nz))
        out[0] = n_free + w.sum()
        out[1] = dd[~nz].sum() + (dd[nz] * w).sum()
        out[2] = np.count_nonzero(w > 0)
        out[3] = (r * r * w).sum()
        out[4:25] = ((a * w[:, None]).T @ a)[np.triu_indices(6)]
        out[25:31] = (a * w[:, None]).T @ r
        count = n_free + int(np.count_nonzero(w > 0))
    thr_bits = int(np.float32(thr).view(np.uint32)) if thr is not None else 0
    info = np.array([len(u), k, thr_bits, s, count, out[0], 0.0, 0.0])
    return out, info


def cpu_refine_robust(cpu, solve, solve_plane, Pc, Qc, c, T0, d, metric, loss, Nc=None, trim_fraction=None, scale=None,
                      max_iterations=30, rel_tol=1e-6, min_correspondences=3):
    """The loop of s4p_icp_refine_robust on the restatement: (T caller frame, iterations, status, rmse history, count history)."""
    def step(Tf):
        idx, d2, _ = cpu.pass_(Pc, Qc, Tf, d)
        s, info = robust_sums(Pc, Qc, Tf, idx, d2, metric, loss, len(Qc), d, Nc, trim_fraction, scale)
        return s, info[4]
    return H.refine_loop(step, solve_plane if metric == "plane" else solve, c, T0, max_iterations, rel_tol, min_correspondences,
                         robust_point=metric == "point")


motion = H.motion


def outlier_scene(P, N, d, n_in=60_000, n_out=40_000, seed=31):
    """Source = a subset of the target P moved by M^-1 (so T_true = M maps it back exactly), plus clutter: target points
    pushed off the surface along +normal by 0.3 d .. 0.8 d (within d of P, one side only).  Returns (Q, T_true, inlier
    fraction)."""
    rng = np.random.default_rng(seed)
    P64 = P.astype(np.float64)
    ins = P64[np.sort(rng.choice(len(P), n_in, replace=False))]
    ok = np.flatnonzero(np.any(N != 0, axis=1))
    pick = ok[rng.choice(len(ok), n_out, replace=False)]
    out = P64[pick] + N[pick].astype(np.float64) * rng.uniform(0.3 * d, 0.8 * d, size=(n_out, 1))
    S = np.concatenate([ins, out])
    S = S[rng.permutation(len(S))]
    extent = float(np.linalg.norm(P64.max(0) - P64.min(0)))
    M = motion(0.5, 0.002 * extent * np.array([0.6, -0.8, 0.0]))
    Mi = np.linalg.inv(M)
    Q = (S @ Mi[:3, :3].T + Mi[:3, 3]).astype(np.float32)
    return Q, M, n_in / (n_in + n_out)
