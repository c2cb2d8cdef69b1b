"""Test-side restatement of the normal-estimation contract (include/s4p_normals.h): tests/normals_cpu/normals_cpu.cpp through
ctypes (brute-force neighbour sets and normals), and a numpy brute force of the neighbour sets."""
import ctypes as C

import numpy as np

from tests import normals_suite as S


def build_cpu(outdir):
    L = S.build_restatement("normals_cpu/normals_cpu.cpp", outdir, "libnormals_cpu")
    vp = C.c_void_p
    L.normals_cpu_knn.restype = None
    L.normals_cpu_knn.argtypes = [vp, vp, vp, C.c_int64, vp, vp, vp, C.c_int64, C.c_int32, C.c_float, vp, vp, C.c_int32]
    L.normals_cpu_normals.restype = None
    L.normals_cpu_normals.argtypes = [vp, vp, vp, C.c_int64, vp, vp, vp, C.c_int64, C.c_int32, C.c_float, vp, C.c_int32]
    L.normals_cpu_normals_of_lists.restype = None
    L.normals_cpu_normals_of_lists.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int64, C.c_int32, vp, vp]
    return CPU(L)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_cols = S.cols


def _r(radius):
    return -1.0 if radius is None else float(radius)


class CPU:
    def __init__(self, L):
        self.L = L

    def knn(self, X, k, radius=None, queries=None, threads=0):
        """(idx int32[m, k] -1 padded, cnt int32[m]): N(q) in ascending (d2, index) order."""
        p = _cols(X)
        q = p if queries is None else _cols(queries)
        m = q[0].shape[0]
        idx = np.empty((m, k), np.int32); cnt = np.empty(m, np.int32)
        self.L.normals_cpu_knn(*S.xyzn(p), *S.xyzn(q), int(k), _r(radius), idx.ctypes.data, cnt.ctypes.data, int(threads))
        return idx, cnt

    def normals(self, X, k, radius=None, queries=None, threads=0):
        """float32 (m, 3): the contract's normal of every query (the cloud itself when queries is None)."""
        p = _cols(X)
        q = p if queries is None else _cols(queries)
        m = q[0].shape[0]
        out = np.empty((m, 3), np.float32)
        self.L.normals_cpu_normals(*S.xyzn(p), *S.xyzn(q), int(k), _r(radius), out.ctypes.data, int(threads))
        return out

    def normals_of_lists(self, X, idx, queries=None):
        """float32 (m, 3): the contract's normal of every query from the neighbour lists idx (m, k), -1 padded, in list order."""
        p = _cols(X)
        q = p if queries is None else _cols(queries)
        idx = np.ascontiguousarray(idx, np.int32)
        m, k = idx.shape
        assert q[0].shape[0] == m
        out = np.empty((m, 3), np.float32)
        self.L.normals_cpu_normals_of_lists(*S.xyzn(p)[:3], *S.xyzn(q), k, idx.ctypes.data, out.ctypes.data)
        return out


def numpy_knn(X, k, radius=None, queries=None):
    """The neighbour sets in numpy: float32 d2 in the contract's order, np.lexsort by (d2, index).  Small clouds only."""
    X = np.asarray(X, np.float32)
    Q = X if queries is None else np.asarray(queries, np.float32)
    dx = X[None, :, 0] - Q[:, None, 0]; dy = X[None, :, 1] - Q[:, None, 1]; dz = X[None, :, 2] - Q[:, None, 2]
    D = dx * dx + (dy * dy + dz * dz)
    r2 = np.float32(np.inf) if radius is None or radius <= 0 else np.float32(radius) * np.float32(radius)
    idx = np.full((len(Q), k), -1, np.int32)
    cnt = np.zeros(len(Q), np.int32)
    ids = np.arange(len(X))
    for i in range(len(Q)):
        ok = D[i] <= r2
        order = np.lexsort((ids[ok], D[i][ok]))[:k]
        sel = ids[ok][order]
        idx[i, :len(sel)] = sel
        cnt[i] = len(sel)
    return idx, cnt


def point3d_normalise(N):
    """Point3D::set_normal's float renormalisation (compat vector: z = x*x + (y*y + z*z), then n / sqrt(z)), so that a
    normal handed to the matcher through the facade can be reproduced in numpy."""
    N = np.asarray(N, np.float32)
    z = N[:, 0] * N[:, 0] + (N[:, 1] * N[:, 1] + N[:, 2] * N[:, 2])
    s = np.sqrt(z, dtype=np.float32)
    out = N.copy()
    nz = z > 0
    out[nz] = N[nz] / s[nz, None]
    return out
