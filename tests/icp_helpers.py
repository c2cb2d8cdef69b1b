"""Test-side restatement of the ICP contract (include/s4p_icp.h): tests/icp_cpu/icp_cpu.cpp through ctypes, and the
refine loop on top of it with the library's host solve (s4p_icp_solve)."""
import ctypes as C

import numpy as np

from tests import normals_suite as S


def build_cpu(outdir):
    L = S.build_restatement("icp_cpu/icp_cpu.cpp", outdir, "libicp_cpu")
    fp, vp = C.POINTER(C.c_float), C.c_void_p
    L.icp_cpu_pass.restype = C.c_int64
    L.icp_cpu_pass.argtypes = [vp, vp, vp, C.c_int64, vp, vp, vp, C.c_int64, vp, C.c_float, vp, vp, vp, C.c_int32]
    L.icp_cpu_brute.restype = None
    L.icp_cpu_brute.argtypes = [vp, vp, vp, C.c_int64, vp, vp, vp, C.c_int64, vp, C.c_float, vp, vp]
    return CPU(L)


class CPU:
    def __init__(self, L):
        self.L = L

    @staticmethod
    def _cols(X):
        return [np.ascontiguousarray(X[:, k], np.float32) for k in range(3)]

    def pass_(self, Pc, Qc, T, d, want_idx=True, threads=0):
        """(idx, d2, sums[17]) for centred clouds and a float 4x4 T (centred frame)."""
        p, q = self._cols(Pc), self._cols(Qc)
        T12 = np.ascontiguousarray(np.asarray(T, np.float32).reshape(16)[:12])
        nq = q[0].shape[0]
        idx = np.empty(nq, np.int32) if want_idx else None
        d2 = np.empty(nq, np.float32) if want_idx else None
        sums = np.empty(17, np.float64)
        self.L.icp_cpu_pass(p[0].ctypes.data, p[1].ctypes.data, p[2].ctypes.data, p[0].shape[0], q[0].ctypes.data, q[1].ctypes.data,
                            q[2].ctypes.data, nq, T12.ctypes.data, float(d), idx.ctypes.data if want_idx else None,
                            d2.ctypes.data if want_idx else None, sums.ctypes.data, int(threads))
        return idx, d2, sums

    def brute(self, Pc, Qc, T, d):
        p, q = self._cols(Pc), self._cols(Qc)
        T12 = np.ascontiguousarray(np.asarray(T, np.float32).reshape(16)[:12])
        nq = q[0].shape[0]
        idx = np.empty(nq, np.int32); d2 = np.empty(nq, np.float32)
        self.L.icp_cpu_brute(p[0].ctypes.data, p[1].ctypes.data, p[2].ctypes.data, p[0].shape[0], q[0].ctypes.data, q[1].ctypes.data,
                             q[2].ctypes.data, nq, T12.ctypes.data, float(d), idx.ctypes.data, d2.ctypes.data)
        return idx, d2


def numpy_brute(Pc, Qc, T, d):
    """The contract in numpy (float32 throughout, same rounding order): small clouds only."""
    T = np.asarray(T, np.float32).reshape(4, 4)
    x, y, z = Qc[:, 0], Qc[:, 1], Qc[:, 2]
    qh = [((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)]
    dx = qh[0][:, None] - Pc[None, :, 0]; dy = qh[1][:, None] - Pc[None, :, 1]; dz = qh[2][:, None] - Pc[None, :, 2]
    D = dx * dx + (dy * dy + dz * dz)
    d2max = np.float32(d) * np.float32(d)
    D = np.where(D <= d2max, D, np.float32(np.inf))
    idx = np.argmin(D, axis=1).astype(np.int32)                 # first index of the minimum: ties to the smallest
    best = D[np.arange(len(idx)), idx]
    none = ~np.isfinite(best)
    idx[none] = -1
    return idx, np.where(none, np.float32(0), best).astype(np.float32)


def to_centred(T, c):
    Tc = np.array(T, np.float64).reshape(4, 4).copy()
    for r in range(3):
        Tc[r, 3] = T[r, 3] + (T[r, 0] * float(c[0]) + T[r, 1] * float(c[1]) + T[r, 2] * float(c[2])) - float(c[r])
    return Tc


def from_centred(Tc, c):
    T = np.array(Tc, np.float64).reshape(4, 4).copy()
    for r in range(3):
        T[r, 3] = Tc[r, 3] - (Tc[r, 0] * float(c[0]) + Tc[r, 1] * float(c[1]) + Tc[r, 2] * float(c[2])) + float(c[r])
    return T


def motion(angle_deg, shift, axis=(0.3, -0.5, 0.8)):
    """4x4: the rotation by angle_deg about axis (Rodrigues) and the translation shift."""
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(angle_deg)
    T = np.eye(4); T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K; T[:3, 3] = shift
    return T


def rot_err_deg(A, B):
    R = A[:3, :3] @ B[:3, :3].T
    return float(np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))))


def raw_normals(rng, n):
    """Caller normals: not unit length, some zero, one NaN."""
    raw = rng.normal(size=(n, 3)).astype(np.float32) * 3
    raw[::11] = 0
    if n > 5:
        raw[5, 0] = np.nan
    return raw


def refine_loop(step, solve, c, T0, max_iterations=30, rel_tol=1e-6, min_correspondences=3, robust_point=False):
    """s4p_icp_pass.inc's refine_loop on the CPU, comparison for comparison, for every metric: step(Tf) -> (sums, n) for the
    centred transform rounded to float32 (n = sums[0], or info[4] under a robust loss), solve(sums) -> dT or an ICPError
    with ERR_DEGENERATE.  robust_point: the robust point metric, where a weight sum below 1 is too few as well.
    (T caller frame, iterations, status, rmse history, count history)."""
    from super4pcs_amd import icp
    T = to_centred(np.asarray(T0, np.float64), c)
    prev, status, its, hist, hist_n = 0.0, icp.MAX_ITERATIONS, 0, [], []
    for k in range(max_iterations):
        s, n = step(T.astype(np.float32))
        sw = s[0]                                       # the weight sum of every family
        i_d2 = 16 if len(s) == 17 else 1                # sum (w) d2: [16] of the 17 point sums, [1] of the 31-sum families
        rmse = float(np.sqrt(s[i_d2] / sw)) if sw > 0 else 0.0
        hist.append(rmse)
        hist_n.append(int(n))
        if n < max(min_correspondences, 1) or (robust_point and not sw >= 1.0):
            status = icp.TOO_FEW
            break
        try:
            dT = solve(s)
        except icp.ICPError as e:
            if e.code != icp.ERR_DEGENERATE:
                raise
            status = icp.DEGENERATE
            break
        T = icp.compose(dT, T)
        its = k + 1
        if k + 1 == max_iterations:
            status = icp.MAX_ITERATIONS
            break
        if k > 0 and abs(rmse - prev) <= rel_tol * prev:
            status = icp.CONVERGED
            break
        prev = rmse
    return from_centred(T, c), its, status, hist, hist_n


def cpu_refine(cpu, solve, Pc, Qc, c, T0, d, max_iterations=30, rel_tol=1e-6, min_correspondences=3, threads=0):
    """The refine loop of s4p_icp_refine on the CPU restatement: (T caller frame, iterations, status, history)."""
    def step(Tf):
        s = cpu.pass_(Pc, Qc, Tf, d, want_idx=False, threads=threads)[2]
        return s, s[0]
    return refine_loop(step, solve, c, T0, max_iterations, rel_tol, min_correspondences)[:4]
