"""ctypes binding of include/s4p_normals.h (libsuper4pcs_normals.so): k-nearest-neighbour normal estimation on the device.

    from super4pcs_amd import normals
    N = normals.estimate_normals(P, k=16)                      # (n, 3) float32, unoriented unit normals or zeros
    N = normals.estimate_normals(P, k=16, radius=0.05)         # hybrid: the 16 nearest within 0.05
    N = normals.estimate_normals(P, k=16, queries=Q)           # normals at Q's positions from P's points
    N = normals.orient_normals(P, N, k=8)                      # one sign per surface: outward (include/s4p_normals_orient.h)
    N = normals.orient_normals(P, N, k=8, viewpoint=(0, 0, 0)) # ... or facing a viewpoint
    N = normals.estimate_normals(P, k=16, orient="outward")    # both steps on one context

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
ERR_NAMES = {0: "OK", -1: "BAD_ARG", -2: "NO_DEVICE", -3: "HIP", -4: "OOM", -7: "STATE", -8: "INTERNAL"}

SYMBOLS = [
    "s4p_normals_create", "s4p_normals_destroy", "s4p_normals_last_error", "s4p_normals_set_cloud",
    "s4p_normals_set_cloud_device", "s4p_normals_estimate", "s4p_normals_estimate_device", "s4p_normals_estimate_at",
    "s4p_normals_estimate_at_device", "s4p_normals_grid",
]

# include/s4p_normals_orient.h
ORIENT_SYMBOLS = ["s4p_orient_consistent", "s4p_orient_consistent_device", "s4p_orient_towards", "s4p_orient_towards_device"]
ORIENT_OUTWARD, ORIENT_VIEWPOINT = 0, 1


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


class OrientStats(C.Structure):
    _fields_ = [("vertices", C.c_int64), ("components", C.c_int64), ("flipped", C.c_int64), ("rounds", C.c_int32),
                ("max_jumps", C.c_int32)]

    def as_dict(self):
        return {"vertices": self.vertices, "components": self.components, "flipped": self.flipped, "rounds": self.rounds,
                "max_jumps": self.max_jumps}


_LIB = None
_ORIENT_DECLARED = False


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


def load_orient():
    """The library with the s4p_normals_orient.h entry points declared; a library without them is an error."""
    global _ORIENT_DECLARED
    L = load_library()
    if _ORIENT_DECLARED:
        return L
    missing = [s for s in ORIENT_SYMBOLS if not hasattr(L, s)]
    if missing:
        raise NormalsError(-7, "libsuper4pcs_normals.so lacks %s: rebuild it (build.build_normals())" % ", ".join(missing))
    vp = C.c_void_p
    for name in ("s4p_orient_consistent", "s4p_orient_consistent_device"):
        getattr(L, name).restype = C.c_int32
        getattr(L, name).argtypes = [vp, C.c_int32, C.c_float, C.c_int32, C.POINTER(C.c_float), vp, vp, vp, C.POINTER(OrientStats)]
    for name in ("s4p_orient_towards", "s4p_orient_towards_device"):
        getattr(L, name).restype = C.c_int32
        getattr(L, name).argtypes = [vp, vp, C.POINTER(C.c_float), vp]
    _ORIENT_DECLARED = True
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

    def _normals_copy(self, normals):
        """(torch?, a contiguous float32 (n, 3) copy of normals, its pointer): the library rewrites the copy in place."""
        if _is_torch(normals):
            import torch
            if not (normals.is_cuda and normals.dtype == torch.float32 and tuple(normals.shape) == (self.n, 3)):
                raise ValueError("torch normals must be a (n, 3) float32 tensor on the GPU, n the cloud's size")
            out = normals.contiguous().clone()
            return True, out, out.data_ptr()
        out = np.array(normals, dtype=np.float32, order="C", copy=True)
        if out.shape != (self.n, 3):
            raise ValueError("normals are (n, 3), n the cloud's size")
        return False, out, out.ctypes.data

    @staticmethod
    def _extra(dev, like, shape, np_dtype):
        if dev:
            import torch
            t = torch.empty(shape, dtype=getattr(torch, np.dtype(np_dtype).name), device=like.device)
            return t, t.data_ptr()
        a = np.empty(shape, np_dtype)
        return a, a.ctypes.data

    def orient(self, normals, k=8, radius=None, viewpoint=None, return_info=False):
        """The normals of the cloud's points with one consistent sign per connected component of the k-nearest-neighbour
        graph (include/s4p_normals_orient.h): signs spread along the minimum spanning tree of 1 - |n . n'| from an anchor
        that faces the viewpoint, or, with viewpoint=None, away from the centre of the cloud's bounds.  Returns a new
        (n, 3) array of the kind it was given; with return_info also a dict with the mask `flipped`, `component` (the
        anchor's index, -1 without a normal) and the counts of s4p_orient_stats."""
        L = load_orient()
        dev, out, ptr = self._normals_copy(normals)
        fl, pf = self._extra(dev, out, (self.n,), np.uint8) if return_info else (None, None)
        co, pc = self._extra(dev, out, (self.n,), np.int32) if return_info else (None, None)
        vp = None if viewpoint is None else (C.c_float * 3)(*[float(v) for v in viewpoint])
        st = OrientStats()
        if dev:
            import torch
            torch.cuda.synchronize(out.device)
        fn = L.s4p_orient_consistent_device if dev else L.s4p_orient_consistent
        self._chk(fn(self.h, int(k), _radius(radius), ORIENT_OUTWARD if viewpoint is None else ORIENT_VIEWPOINT, vp, ptr, pf, pc,
                     C.byref(st)))
        if not return_info:
            return out
        info = st.as_dict()
        info["flipped_count"] = info.pop("flipped")
        info["flipped"] = (fl != 0) if dev else fl.astype(bool)
        info["component"] = co
        return out, info

    def orient_towards(self, normals, viewpoint):
        """The normals of the cloud's points, each negated when it faces away from the viewpoint (n . (v - x) < 0)."""
        L = load_orient()
        dev, out, ptr = self._normals_copy(normals)
        vp = (C.c_float * 3)(*[float(v) for v in viewpoint])
        if dev:
            import torch
            torch.cuda.synchronize(out.device)
        fn = L.s4p_orient_towards_device if dev else L.s4p_orient_towards
        self._chk(fn(self.h, ptr, vp, None))
        return out


def estimate_normals(xyz, k=16, radius=None, queries=None, device=0, orient=None, orient_k=8):
    """Unit normals from the k nearest neighbours (3 <= k <= 32) of each point of xyz, or of each query position
    when queries is given; radius > 0 restricts the neighbours to those within it (None or <= 0: unbounded).  A point with
    fewer than 3 neighbours, or whose neighbours all coincide, gets (0, 0, 0).  Returns the kind it was given: a numpy array,
    or a torch tensor on the input's GPU.  The sign is arbitrary (the component of largest magnitude is positive) unless
    orient is given: "outward", or a viewpoint (x, y, z), orients the cloud's own normals consistently over the graph of the
    orient_k nearest neighbours (Normals.orient); the default None returns the estimate as it is."""
    if orient is not None and queries is not None:
        raise ValueError("orient applies to the cloud's own normals, not to queries")
    if isinstance(orient, str) and orient != "outward":
        raise ValueError('orient is None, "outward" or a viewpoint (x, y, z)')
    ctx = Normals(device)
    try:
        ctx.set_cloud(xyz)
        if queries is not None:
            return ctx.estimate_at(queries, k, radius)
        N = ctx.estimate(k, radius, device_out=xyz if _is_torch(xyz) else None)
        if orient is None:
            return N
        return ctx.orient(N, orient_k, None, None if isinstance(orient, str) else orient)
    finally:
        ctx.close()


def orient_normals(xyz, normals, k=8, radius=None, viewpoint=None, device=0):
    """normals of the points xyz with one consistent sign per connected component of the k-nearest-neighbour graph
    (1 <= k <= 32): facing the viewpoint, or outward (away from the centre of the bounds) when viewpoint is None.  Zero
    normals stay zero.  numpy in, numpy out; GPU tensors in, a GPU tensor out.  See Normals.orient."""
    ctx = Normals(device)
    try:
        ctx.set_cloud(xyz)
        return ctx.orient(normals, k, radius, viewpoint)
    finally:
        ctx.close()
