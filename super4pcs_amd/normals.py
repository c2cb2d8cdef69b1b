"""ctypes binding of include/s4p_normals.h (libsuper4pcs_normals.so): k-nearest-neighbour normal estimation on the device.

    from super4pcs_amd import normals
    N = normals.estimate_normals(P, k=16)                      # (n, 3) float32, unoriented unit normals or zeros
    N = normals.estimate_normals(P, k=16, radius=0.05)         # hybrid: the 16 nearest within 0.05
    N = normals.estimate_normals(P, k=16, queries=Q)           # normals at Q's positions from P's points

Clouds are (N, 3) float32 numpy arrays, or (N, 3) float32 torch tensors on the GPU (they enter through the *_device entry
points, device to device, and the result is a torch tensor on the same device).  There is no CPU fallback: without a
device, Normals() raises NormalsError with code -2.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libsuper4pcs_normals.so")

MIN_K, MAX_K = 3, 32
ERR_NAMES = {0: "OK", -1: "BAD_ARG", -2: "NO_DEVICE", -3: "HIP", -4: "OOM", -7: "STATE"}

SYMBOLS = [
    "s4p_normals_create", "s4p_normals_destroy", "s4p_normals_last_error", "s4p_normals_set_cloud",
    "s4p_normals_set_cloud_device", "s4p_normals_estimate", "s4p_normals_estimate_device", "s4p_normals_estimate_at",
    "s4p_normals_estimate_at_device", "s4p_normals_grid",
]


class NormalsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("s4p_normals error %s (%d): %s" % (ERR_NAMES.get(code, "?"), code, msg))
        self.code = code


class GridInfo(C.Structure):
    _fields_ = [("cell", C.c_double), ("spacing", C.c_double), ("dims", C.c_int32 * 3), ("reserved", C.c_int32),
                ("cells", C.c_int64), ("nonempty", C.c_int64), ("mean_per_cell", C.c_double), ("p99_per_cell", C.c_int64),
                ("max_per_cell", C.c_int64)]

    def as_dict(self):
        return {"cell": self.cell, "spacing": self.spacing, "dims": list(self.dims), "cells": self.cells,
                "nonempty": self.nonempty, "mean_per_cell": self.mean_per_cell, "p99_per_cell": self.p99_per_cell,
                "max_per_cell": self.max_per_cell}


_LIB = None


def load_library():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise NormalsError(-7, "libsuper4pcs_normals.so not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.s4p_normals_create.restype = C.c_int32
    L.s4p_normals_create.argtypes = [C.c_int32, C.POINTER(vp)]
    L.s4p_normals_destroy.restype = None
    L.s4p_normals_destroy.argtypes = [vp]
    L.s4p_normals_last_error.restype = C.c_char_p
    L.s4p_normals_last_error.argtypes = [vp]
    for name in ("s4p_normals_set_cloud", "s4p_normals_set_cloud_device"):
        getattr(L, name).restype = C.c_int32
        getattr(L, name).argtypes = [vp, vp, vp, vp, C.c_int64]
    for name in ("s4p_normals_estimate", "s4p_normals_estimate_device"):
        getattr(L, name).restype = C.c_int32
        getattr(L, name).argtypes = [vp, C.c_int32, C.c_float, vp]
    for name in ("s4p_normals_estimate_at", "s4p_normals_estimate_at_device"):
        getattr(L, name).restype = C.c_int32
        getattr(L, name).argtypes = [vp, vp, vp, vp, C.c_int64, C.c_int32, C.c_float, vp]
    L.s4p_normals_grid.restype = C.c_int32
    L.s4p_normals_grid.argtypes = [vp, C.POINTER(GridInfo)]
    _LIB = L
    return L


def _is_torch(t):
    return type(t).__module__.startswith("torch")


def _cols(X):
    """(device?, three column pointers, n, keep-alive) of a numpy array or a GPU torch tensor."""
    if _is_torch(X):
        import torch
        if not (X.is_cuda and X.dtype == torch.float32 and X.dim() == 2 and X.shape[1] == 3):
            raise ValueError("torch input must be a (N, 3) float32 tensor on the GPU")
        cols = [X[:, k].contiguous() for k in range(3)]
        torch.cuda.synchronize(X.device)              # the copies run on torch's stream; the library reads on its own
        return True, [c.data_ptr() for c in cols], int(X.shape[0]), cols
    X = np.asarray(X)
    if X.ndim != 2 or X.shape[1] != 3:
        raise ValueError("clouds are (N, 3)")
    cols = [np.ascontiguousarray(X[:, k], dtype=np.float32) for k in range(3)]
    return False, [c.ctypes.data for c in cols], int(X.shape[0]), cols


def _radius(radius):
    return -1.0 if radius is None else float(radius)


class Normals:
    """One s4p_normals context (one GPU) holding one cloud and its grid."""

    def __init__(self, device=0):
        self.L = load_library()
        self.device = device
        h = C.c_void_p()
        rc = self.L.s4p_normals_create(device, C.byref(h))
        if rc != 0:
            raise NormalsError(rc, self.L.s4p_normals_last_error(None).decode())
        self.h = h
        self.n = 0

    def close(self):
        if getattr(self, "h", None):
            self.L.s4p_normals_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise NormalsError(rc, self.L.s4p_normals_last_error(self.h).decode())

    def set_cloud(self, X):
        dev, ptr, n, keep = _cols(X)
        fn = self.L.s4p_normals_set_cloud_device if dev else self.L.s4p_normals_set_cloud
        self._chk(fn(self.h, ptr[0], ptr[1], ptr[2], n))
        self.n = n
        del keep

    def _out(self, like_torch, like, m):
        if like_torch:
            import torch
            t = torch.empty((m, 3), dtype=torch.float32, device=like.device)
            torch.cuda.synchronize(like.device)
            return t, t.data_ptr()
        a = np.empty((m, 3), np.float32)
        return a, a.ctypes.data

    def estimate(self, k=16, radius=None, device_out=None):
        """(n, 3) float32 normals of the cloud itself; a torch tensor on the cloud's device when device_out is a tensor."""
        like_torch = device_out is not None
        out, ptr = self._out(like_torch, device_out, self.n)
        fn = self.L.s4p_normals_estimate_device if like_torch else self.L.s4p_normals_estimate
        self._chk(fn(self.h, int(k), _radius(radius), ptr))
        return out

    def estimate_at(self, Q, k=16, radius=None):
        """(m, 3) float32 normals at the query positions Q (numpy in, numpy out; GPU tensor in, GPU tensor out)."""
        dev, ptr, m, keep = _cols(Q)
        out, optr = self._out(dev, Q, m)
        fn = self.L.s4p_normals_estimate_at_device if dev else self.L.s4p_normals_estimate_at
        self._chk(fn(self.h, ptr[0], ptr[1], ptr[2], m, int(k), _radius(radius), optr))
        del keep
        return out

    def grid(self):
        g = GridInfo()
        self._chk(self.L.s4p_normals_grid(self.h, C.byref(g)))
        return g.as_dict()


def estimate_normals(xyz, k=16, radius=None, queries=None, device=0):
    """Unoriented unit normals from the k nearest neighbours (3 <= k <= 32) of each point of xyz, or of each query position
    when queries is given; radius > 0 restricts the neighbours to those within it (None or <= 0: unbounded).  A point with
    fewer than 3 neighbours, or whose neighbours all coincide, gets (0, 0, 0).  Returns the kind it was given: a numpy array,
    or a torch tensor on the input's GPU."""
    ctx = Normals(device)
    try:
        ctx.set_cloud(xyz)
        if queries is not None:
            return ctx.estimate_at(queries, k, radius)
        return ctx.estimate(k, radius, device_out=xyz if _is_torch(xyz) else None)
    finally:
        ctx.close()
