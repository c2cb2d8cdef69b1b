"""Test-side restatement of the coloured ICP contract (include/s4p_icp_color.h) in numpy: the gradient neighbourhoods N(i)
(the float d2 of the correspondence contract, as tests/icp_plane_helpers.numpy_brute_cov states it, found through a grid of
the restatement's own instead of all pairs), the gradients and the 31 joint sums term by term in the header's operation
order, and the refine loop on top of them with the library's host solve (s4p_icp_solve_plane)."""
import numpy as np

from tests import icp_helpers as H

GATE = 1e-6                     # S4P_ICP_COLOR_GATE
LAMBDA = 0.968                  # S4P_ICP_COLOR_LAMBDA


def texture(X, scale=1.0):
    """The smooth intensity field of the planar check, evaluated at scale * (x, y): float32 in [0.05, 0.95]."""
    X = np.asarray(X, np.float64)
    x, y = scale * X[:, 0], scale * X[:, 1]
    v = 0.5 + 0.25 * np.sin(2 * np.pi * 1.5 * x + 0.3) * np.cos(2 * np.pi * 1.2 * y) + 0.2 * np.sin(2 * np.pi * (0.8 * x + 1.1 * y))
    return v.astype(np.float32)


def rot(axis, deg):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def planar_case(seed=3, n_p=20_000, n_q=5_000):
    """The case the metric exists for: 20 000 random points of z = 0 in the unit square with normals (0, 0, 1) and texture();
    the source is 5000 of them with their intensities, moved by 1 degree about z and 0.5 degrees about x around the patch
    centre plus (0.010, -0.008, 0.005).  Returns a dict: P, N, Ip, Q, Iq, T_true (maps Q onto P), d, r."""
    rng = np.random.default_rng(seed)
    P = np.column_stack([rng.uniform(0, 1, (n_p, 2)), np.zeros(n_p)]).astype(np.float32)
    N = np.tile(np.array([0, 0, 1], np.float32), (n_p, 1))
    Ip = texture(P)
    pick = np.sort(rng.choice(n_p, n_q, replace=False))
    R = rot((0, 0, 1), 1.0) @ rot((1, 0, 0), 0.5)
    ctr = np.array([0.5, 0.5, 0.0])
    M = np.eye(4); M[:3, :3] = R; M[:3, 3] = ctr - R @ ctr + np.array([0.010, -0.008, 0.005])
    Q = (P[pick].astype(np.float64) @ R.T + M[:3, 3]).astype(np.float32)
    return dict(P=P, N=N, Ip=Ip, Q=Q, Iq=Ip[pick].copy(), T_true=np.linalg.inv(M), d=0.03, r=0.03)


def neighbour_pairs(Pc, r, chunk=20_000, which=None):
    """N(i) of include/s4p_icp_plane.h / s4p_icp_color.h for the centred target Pc: yields (i, j) index arrays, i ascending,
    with float32 d2(p_i, p_j) = dx*dx + (dy*dy + dz*dz) <= fl(r*r), i itself included.  Candidates come from a grid of edge
    1.01 r (27 cells hold every point within r); the decision is the contract's float comparison.  which (sorted indices):
    only those i, from the same grid over all points and in the same order per i."""
    Pc = np.ascontiguousarray(Pc, np.float32)
    n = len(Pc)
    r2 = np.float32(r) * np.float32(r)
    h = 1.01 * float(r)
    lo = Pc.min(0).astype(np.float64)
    cell = np.floor((Pc.astype(np.float64) - lo) / h).astype(np.int64) + 1            # 1 cell of padding on every side
    dims = cell.max(0) + 2
    key = (cell[:, 2] * dims[1] + cell[:, 1]) * dims[0] + cell[:, 0]
    order = np.argsort(key, kind="stable")
    skey = key[order]
    offs = np.array([(dz * dims[1] + dy) * dims[0] + dx for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)], np.int64)
    rows = np.arange(n) if which is None else np.asarray(which, np.int64)
    for a in range(0, len(rows), chunk):
        ii = rows[a:a + chunk]
        nk = (key[ii][:, None] + offs[None, :]).ravel()
        b = np.searchsorted(skey, nk, "left"); e = np.searchsorted(skey, nk, "right")
        cnt = e - b
        tot = int(cnt.sum())
        i_rep = np.repeat(np.repeat(ii, 27), cnt)
        start = np.repeat(b - (np.cumsum(cnt) - cnt), cnt)
        j = order[start + np.arange(tot)]
        dx = Pc[i_rep, 0] - Pc[j, 0]; dy = Pc[i_rep, 1] - Pc[j, 1]; dz = Pc[i_rep, 2] - Pc[j, 2]
        keep = (dx * dx + (dy * dy + dz * dz)) <= r2
        yield i_rep[keep], j[keep]


def gradient_systems(Pc, Nc, I, r, which=None):
    """(k int64[n], A float64[n, 3, 3], b float64[n, 3]) of the header: S = sum u u^T, b = sum u dI over N(i), A = S + tr(S) n n^T.
    which (sorted indices): the rows of those points only (n = len(which)), the same terms in the same order."""
    rows = np.arange(len(Pc)) if which is None else np.asarray(which, np.int64)
    assert np.all(np.diff(rows) > 0)
    n = len(rows)
    P64 = np.asarray(Pc, np.float32).astype(np.float64); N64 = np.asarray(Nc, np.float32).astype(np.float64)
    I64 = np.asarray(I, np.float32).astype(np.float64)
    k = np.zeros(n, np.int64); S = np.zeros((n, 6)); b = np.zeros((n, 3))
    for i, j in neighbour_pairs(Pc, r, which=which):
        e = P64[j] - P64[i]
        nv = N64[i]
        en = (e[:, 0] * nv[:, 0] + e[:, 1] * nv[:, 1]) + e[:, 2] * nv[:, 2]
        u = e - en[:, None] * nv
        dI = I64[j] - I64[i]
        if which is not None:
            i = np.searchsorted(rows, i)                                # the point's row
        k += np.bincount(i, minlength=n)
        for c, (p, q) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            S[:, c] += np.bincount(i, weights=u[:, p] * u[:, q], minlength=n)
        for c in range(3):
            b[:, c] += np.bincount(i, weights=u[:, c] * dI, minlength=n)
    tr = (S[:, 0] + S[:, 3]) + S[:, 5]
    A = np.empty((n, 3, 3))
    N64 = N64[rows]
    for c, (p, q) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        A[:, p, q] = S[:, c] + tr * (N64[:, p] * N64[:, q])
        A[:, q, p] = A[:, p, q]
    return k, A, b


def color_gradients(Pc, Nc, I, r, min_neighbours, which=None):
    """(g float32[n, 3], ratio float64[n], k): the header's gradients, zero where k < min_neighbours, the normal is zero or
    ratio = lambda_min(A) / lambda_max(A) <= 1e-6 (numpy's eigvalsh for the device's Jacobi: the callers keep the ratio
    away from the gate).  ratio is nan where there is no system (zero normal or too few neighbours) or A = 0.  which (sorted
    indices): those points' rows only."""
    k, A, b = gradient_systems(Pc, Nc, I, r, which=which)
    Nc = np.asarray(Nc) if which is None else np.asarray(Nc)[np.asarray(which, np.int64)]
    has = np.any(np.asarray(Nc) != 0, axis=1) & (k >= min_neighbours)
    w = np.linalg.eigvalsh(A)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(has & (w[:, 2] > 0), w[:, 0] / w[:, 2], np.nan)
    ok = has & (w[:, 0] > GATE * w[:, 2])
    A00, A01, A02, A11, A12, A22 = A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2]
    c00 = A11 * A22 - A12 * A12; c01 = A02 * A12 - A01 * A22; c02 = A01 * A12 - A02 * A11
    c11 = A00 * A22 - A02 * A02; c12 = A01 * A02 - A00 * A12; c22 = A00 * A11 - A01 * A01
    det = (A00 * c00 + A01 * c01) + A02 * c02
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.stack([((c00 * b[:, 0] + c01 * b[:, 1]) + c02 * b[:, 2]) / det,
                      ((c01 * b[:, 0] + c11 * b[:, 1]) + c12 * b[:, 2]) / det,
                      ((c02 * b[:, 0] + c12 * b[:, 1]) + c22 * b[:, 2]) / det], 1)
    g[~ok] = 0.0
    return g.astype(np.float32), ratio, k


def color_sums(Pc, Qc, T, idx, d2, Nc, G, Ip, Iq, lam):
    """(s, sabs): the 31 joint sums for a float T (centred), the correspondences (idx, d2), the stored target normals Nc,
    gradients G and intensities Ip (uploaded order), the source intensities Iq and lambda; sabs[k] = sum |term| of s[k]."""
    T = np.asarray(T, np.float32).reshape(4, 4)
    x, y, z = Qc[:, 0], Qc[:, 1], Qc[:, 2]
    qh = np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1)      # float32
    hit = idx >= 0
    wg, wc = float(lam), 1.0 - float(lam)
    nv = np.asarray(Nc, np.float32)[idx[hit]].astype(np.float64)
    nz = np.any(nv != 0, axis=1)
    q = qh[hit].astype(np.float64)[nz]; p = np.asarray(Pc, np.float32)[idx[hit]].astype(np.float64)[nz]; nv = nv[nz]
    g = np.asarray(G, np.float32)[idx[hit]].astype(np.float64)[nz]
    ip = np.asarray(Ip, np.float32)[idx[hit]].astype(np.float64)[nz]
    iq = np.asarray(Iq, np.float32)[hit].astype(np.float64)[nz]
    r = p - q
    sg = (r[:, 0] * nv[:, 0] + r[:, 1] * nv[:, 1]) + r[:, 2] * nv[:, 2]
    gn = (g[:, 0] * nv[:, 0] + g[:, 1] * nv[:, 1]) + g[:, 2] * nv[:, 2]
    gp = g - gn[:, None] * nv
    rc = ((iq - ip) + ((g[:, 0] * r[:, 0] + g[:, 1] * r[:, 1]) + g[:, 2] * r[:, 2])) - sg * gn

    def six(v):
        return [q[:, 1] * v[:, 2] - q[:, 2] * v[:, 1], q[:, 2] * v[:, 0] - q[:, 0] * v[:, 2], q[:, 0] * v[:, 1] - q[:, 1] * v[:, 0],
                v[:, 0], v[:, 1], v[:, 2]]

    aG, aC = six(nv), six(gp)
    terms = [np.ones(np.count_nonzero(hit)), d2[hit].astype(np.float64), np.ones(len(q)), wg * (sg * sg) + wc * (rc * rc)]
    for u in range(6):
        for v in range(u, 6):
            terms.append(wg * (aG[u] * aG[v]) + wc * (aC[u] * aC[v]))
    for u in range(6):
        terms.append(wg * (aG[u] * sg) + wc * (aC[u] * rc))
    s = np.array([t.sum() for t in terms])
    sabs = np.array([np.abs(t).sum() for t in terms])
    return s, sabs


def cpu_refine_color(cpu, solve_plane, Pc, Qc, Nc, G, Ip, Iq, c, T0, d, lam=LAMBDA, max_iterations=30, rel_tol=1e-6,
                     min_correspondences=3):
    """The refine loop of s4p_icp_refine_color on the CPU restatement: (T caller frame, iterations, status, history)."""
    def step(Tf):
        idx, d2, _ = cpu.pass_(Pc, Qc, Tf, d)
        s = color_sums(Pc, Qc, Tf, idx, d2, Nc, G, Ip, Iq, lam)[0]
        return s, s[0]
    return H.refine_loop(step, solve_plane, c, T0, max_iterations, rel_tol, min_correspondences)[:4]
