"""Test-side restatement of the point-to-plane contract (include/s4p_icp_plane.h): the normal neighbourhoods through
tests/icp_plane_cpu/icp_plane_cpu.cpp, the normals and the 31 plane sums in numpy, and the refine loop on top of them with
the library's host solve (s4p_icp_solve_plane)."""
import ctypes as C

import numpy as np

from tests import icp_helpers as H
from tests import normals_suite as S


def build_plane_cpu(outdir):
    L = S.build_restatement("icp_plane_cpu/icp_plane_cpu.cpp", outdir, "libicp_plane_cpu")
    vp = C.c_void_p
    L.icp_plane_cpu_cov.restype = None
    L.icp_plane_cpu_cov.argtypes = [vp, vp, vp, C.c_int64, C.c_float, vp, vp, C.c_int32]
    return PlaneCPU(L)


class PlaneCPU:
    def __init__(self, L):
        self.L = L

    def cov(self, Pc, r, threads=0):
        """(k int32[n], C float64[n, 6] as xx xy xz yy yz zz) for the centred target Pc and radius r."""
        p = [np.ascontiguousarray(Pc[:, a], np.float32) for a in range(3)]
        n = p[0].shape[0]
        k = np.empty(n, np.int32); c6 = np.empty((n, 6), np.float64)
        self.L.icp_plane_cpu_cov(p[0].ctypes.data, p[1].ctypes.data, p[2].ctypes.data, n, float(r), k.ctypes.data, c6.ctypes.data,
                                 int(threads))
        return k, c6


def build_normals_literal(outdir):
    """tests/icp_plane_cpu/icp_normals_literal.cpp: k_normals restated term by term, for bit-for-bit comparison."""
    L = S.build_restatement("icp_plane_cpu/icp_normals_literal.cpp", outdir, "libicp_normals_literal")
    vp = C.c_void_p
    L.icp_normals_literal.restype = C.c_int32
    L.icp_normals_literal.argtypes = [vp, vp, vp, C.c_int64, C.c_float, C.c_float, C.c_int32, vp, C.c_int64, vp, vp, vp, C.c_int32]

    def normals(Pc, d, r, min_neighbours, which=None, threads=0):
        """(float32 (m, 3) normals of the target indices `which` (all when None), grid dims, cell edge) for the centred target
        Pc, set_target's max_distance d and estimate_normals' radius r."""
        p = [np.ascontiguousarray(Pc[:, a], np.float32) for a in range(3)]
        n = p[0].shape[0]
        w = np.arange(n, dtype=np.int64) if which is None else np.ascontiguousarray(which, np.int64)
        out = np.empty((len(w), 3), np.float32)
        dims = np.zeros(3, np.int32); h = np.zeros(1, np.float64)
        rc = L.icp_normals_literal(p[0].ctypes.data, p[1].ctypes.data, p[2].ctypes.data, n, float(d), float(r), int(min_neighbours),
                                   w.ctypes.data, len(w), out.ctypes.data, dims.ctypes.data, h.ctypes.data, int(threads))
        assert rc == 0
        return out, dims, float(h[0])

    return normals


def numpy_brute_cov(Pc, r):
    """The neighbourhood contract in numpy (float32 d2 in the contract's order): small clouds only."""
    Pc = np.asarray(Pc, np.float32)
    r2 = np.float32(r) * np.float32(r)
    dx = Pc[:, None, 0] - Pc[None, :, 0]; dy = Pc[:, None, 1] - Pc[None, :, 1]; dz = Pc[:, None, 2] - Pc[None, :, 2]
    M = (dx * dx + (dy * dy + dz * dz)) <= r2
    P64 = Pc.astype(np.float64)
    k = M.sum(1).astype(np.int32)
    c6 = np.zeros((len(Pc), 6))
    for i in range(len(Pc)):
        e = P64[M[i]] - P64[i]
        m = e.mean(0)
        C3 = e.T @ e / len(e) - np.outer(m, m)
        c6[i] = C3[[0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]
    return k, c6


def normals_from_cov(k, c6, min_neighbours):
    """(normals float32[n, 3], eigenvalues float64[n, 3] ascending): the eigenvector of the smallest eigenvalue, largest
    component positive (first on ties); zero where k < min_neighbours."""
    C3 = np.empty((len(k), 3, 3))
    C3[:, 0, 0], C3[:, 0, 1], C3[:, 0, 2], C3[:, 1, 1], C3[:, 1, 2], C3[:, 2, 2] = c6.T
    C3[:, 1, 0], C3[:, 2, 0], C3[:, 2, 1] = C3[:, 0, 1], C3[:, 0, 2], C3[:, 1, 2]
    w, V = np.linalg.eigh(C3)
    v = V[:, :, 0]
    lead = v[np.arange(len(v)), np.argmax(np.abs(v), axis=1)]
    v = v * np.where(lead < 0, -1.0, 1.0)[:, None]
    v[k < min_neighbours] = 0.0
    return v.astype(np.float32), w


def normalise(N):
    """set_target_normals' rule: normalised in double, rounded to float; zero or non-finite -> 0."""
    N = np.asarray(N, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ln = np.sqrt((N * N).sum(1))
        ok = np.isfinite(N).all(1) & (ln > 0) & np.isfinite(ln)
        out = np.where(ok[:, None], N / np.where(ok, ln, 1.0)[:, None], 0.0)
    return out.astype(np.float32)


def plane_sums(Pc, Qc, T, idx, d2, Nc):
    """The 31 plane sums in numpy for a float T (centred), the correspondences (idx, d2) and the target normals Nc
    (uploaded order, as stored)."""
    T = np.asarray(T, np.float32).reshape(4, 4)
    x, y, z = Qc[:, 0], Qc[:, 1], Qc[:, 2]
    qh = np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1)
    hit = idx >= 0
    s = np.zeros(31)
    s[0] = np.count_nonzero(hit)
    s[1] = d2[hit].astype(np.float64).sum()
    q = qh[hit].astype(np.float64); p = Pc[idx[hit]].astype(np.float64); nv = Nc[idx[hit]].astype(np.float64)
    nz = np.any(nv != 0, axis=1)
    q, p, nv = q[nz], p[nz], nv[nz]
    a = np.concatenate([np.cross(q, nv), nv], axis=1)
    r = ((p[:, 0] - q[:, 0]) * nv[:, 0] + (p[:, 1] - q[:, 1]) * nv[:, 1]) + (p[:, 2] - q[:, 2]) * nv[:, 2]
    s[2] = len(q)
    s[3] = (r * r).sum()
    A = a.T @ a
    s[4:25] = A[np.triu_indices(6)]
    s[25:31] = a.T @ r
    return s


def cpu_refine_plane(cpu, solve_plane, Pc, Qc, Nc, c, T0, d, max_iterations=30, rel_tol=1e-6, min_correspondences=3):
    """The refine loop of s4p_icp_refine_plane on the CPU restatement: (T caller frame, iterations, status, history)."""
    def step(Tf):
        idx, d2, _ = cpu.pass_(Pc, Qc, Tf, d)
        s = plane_sums(Pc, Qc, Tf, idx, d2, Nc)
        return s, s[0]
    return H.refine_loop(step, solve_plane, c, T0, max_iterations, rel_tol, min_correspondences)[:4]
