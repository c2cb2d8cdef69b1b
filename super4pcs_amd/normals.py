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
import contextlib
import ctypes as C
import os

import numpy as np

from . import _binding as _B
from ._binding import TWIN

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libsuper4pcs_normals.so")

MIN_K, MAX_K = 3, 32
ERR_NAMES = {0: "OK", -1: "BAD_ARG", -2: "NO_DEVICE", -3: "HIP", -4: "OOM", -7: "STATE", -8: "INTERNAL"}

ORIENT_OUTWARD, ORIENT_VIEWPOINT = 0, 1              # include/s4p_normals_orient.h


class NormalsError(RuntimeError):
    REBUILD = "build.build_normals()"

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


_VP = C.c_void_p
SIGNATURES = {                                         # include/s4p_normals.h
    "s4p_normals_create": [C.c_int32, C.POINTER(_VP)],
    "s4p_normals_destroy": (None, [_VP]),
    "s4p_normals_last_error": (C.c_char_p, [_VP]),
    "s4p_normals_set_cloud" + TWIN: [_VP, _VP, _VP, _VP, C.c_int64],
    "s4p_normals_estimate" + TWIN: [_VP, C.c_int32, C.c_float, _VP],
    "s4p_normals_estimate_at" + TWIN: [_VP, _VP, _VP, _VP, C.c_int64, C.c_int32, C.c_float, _VP],
    "s4p_normals_grid": [_VP, C.POINTER(GridInfo)],
}
ORIENT_SIGNATURES = {                                  # include/s4p_normals_orient.h
    "s4p_orient_consistent" + TWIN: [_VP, C.c_int32, C.c_float, C.c_int32, C.POINTER(C.c_float), _VP, _VP, _VP, C.POINTER(OrientStats)],
    "s4p_orient_towards" + TWIN: [_VP, _VP, C.POINTER(C.c_float), _VP],
}
SYMBOLS, ORIENT_SYMBOLS = _B.names(SIGNATURES), _B.names(ORIENT_SIGNATURES)

_LOADED = {}           # library path -> (the library, the tables declared on it): _binding.load


def load_library(path=None, *tables):
    """The library at path (default LIB_PATH), opened once per process, with s4p_normals.h and the tables of the families on top
    of it declared; a library without one of their functions is an error."""
    return _B.load(_LOADED, path or LIB_PATH, (SIGNATURES,) + tables, NormalsError, "libsuper4pcs_normals.so")


def load_orient(path=None):
    """The library with the s4p_normals_orient.h entry points declared; a library without them is an error."""
    return load_library(path, ORIENT_SIGNATURES)


@contextlib.contextmanager
def session(cls, xyz, device=0):
    """One context of cls (Normals or a class on it) for one convenience call, closed on every path; with the cloud xyz
    unless it is None."""
    ctx = cls(device)
    try:
        if xyz is not None:
            ctx.set_cloud(xyz)
        yield ctx
    finally:
        ctx.close()


def _radius(radius):
    return -1.0 if radius is None else float(radius)


class Normals:
    """One s4p_normals context (one GPU) holding one cloud and its grid."""
    _load = staticmethod(load_library)         # a class on this one names the loader of its own family

    def __init__(self, device=0, lib=None):
        """lib: the path of another copy or build of the library, bound next to the package's (None)."""
        self.lib = lib
        self.L = self._load(lib)
        self.device = device
        h = C.c_void_p()
        rc = self.L.s4p_normals_create(device, C.byref(h))
        if rc != 0:
            raise NormalsError(rc, self.L.s4p_normals_last_error(None).decode())
        self.h = h
        self.n = 0
        self._like = None

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

    def _sync(self):
        _B.sync(self._like)

    def _call(self, name, like, *args, synced=False):
        """The library's `name`(h, *args), or its _device twin when like is a tensor, after a synchronise of like's device
        (_binding.sync) unless cols() has just done it (synced); an error code raises."""
        if not synced:
            _B.sync(like)
        self._chk(getattr(self.L, name if like is None else name + "_device")(self.h, *args))

    def set_cloud(self, X):
        dev, ptr, n, keep = _B.cols(X)
        like = X if dev else None
        self._call("s4p_normals_set_cloud", like, *ptr, n, synced=True)
        self.n, self._like = n, like                      # device results follow the cloud's kind

    def estimate(self, k=16, radius=None, device_out=None):
        """(n, 3) float32 normals of the cloud itself; a torch tensor on the cloud's device when device_out is a tensor."""
        out, ptr = _B.empty(device_out, (self.n, 3), np.float32)
        self._call("s4p_normals_estimate", device_out, int(k), _radius(radius), ptr)
        return out

    def estimate_at(self, Q, k=16, radius=None):
        """(m, 3) float32 normals at the query positions Q (numpy in, numpy out; GPU tensor in, GPU tensor out)."""
        dev, ptr, m, keep = _B.cols(Q)
        like = Q if dev else None
        out, optr = _B.empty(like, (m, 3), np.float32)
        self._call("s4p_normals_estimate_at", like, *ptr, m, int(k), _radius(radius), optr)
        return out

    def grid(self):
        g = GridInfo()
        self._chk(self.L.s4p_normals_grid(self.h, C.byref(g)))
        return g.as_dict()

    def _normals_copy(self, normals):
        """(like, a contiguous float32 (n, 3) copy of normals, its pointer): the library rewrites the copy in place; like is
        the copy when it is a tensor, else None."""
        if _B.is_torch(normals):
            import torch
            if not (normals.is_cuda and normals.dtype == torch.float32 and tuple(normals.shape) == (self.n, 3)):
                raise ValueError("torch normals must be a (n, 3) float32 tensor on the GPU, n the cloud's size")
            out = normals.contiguous().clone()
            return out, out, out.data_ptr()
        out = np.array(normals, dtype=np.float32, order="C", copy=True)
        if out.shape != (self.n, 3):
            raise ValueError("normals are (n, 3), n the cloud's size")
        return None, out, out.ctypes.data

    def orient(self, normals, k=8, radius=None, viewpoint=None, return_info=False):
        """The normals of the cloud's points with one consistent sign per connected component of the k-nearest-neighbour
        graph (include/s4p_normals_orient.h): signs spread along the minimum spanning tree of 1 - |n . n'| from an anchor
        that faces the viewpoint, or, with viewpoint=None, away from the centre of the cloud's bounds.  Returns a new
        (n, 3) array of the kind it was given; with return_info also a dict with the mask `flipped`, `component` (the
        anchor's index, -1 without a normal) and the counts of s4p_orient_stats."""
        load_orient(self.lib)
        like, out, ptr = self._normals_copy(normals)
        fl, pf = _B.empty(like, (self.n,), np.uint8) if return_info else (None, None)
        co, pc = _B.empty(like, (self.n,), np.int32) if return_info else (None, None)
        vp = None if viewpoint is None else (C.c_float * 3)(*[float(v) for v in viewpoint])
        st = OrientStats()
        self._call("s4p_orient_consistent", like, int(k), _radius(radius), ORIENT_OUTWARD if viewpoint is None else ORIENT_VIEWPOINT,
                   vp, ptr, pf, pc, C.byref(st))
        if not return_info:
            return out
        info = st.as_dict()
        info["flipped_count"] = info.pop("flipped")
        info["flipped"] = (fl != 0) if like is not None else fl.astype(bool)
        info["component"] = co
        return out, info

    def orient_towards(self, normals, viewpoint):
        """The normals of the cloud's points, each negated when it faces away from the viewpoint (n . (v - x) < 0)."""
        load_orient(self.lib)
        like, out, ptr = self._normals_copy(normals)
        self._call("s4p_orient_towards", like, ptr, (C.c_float * 3)(*[float(v) for v in viewpoint]), None)
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
    with session(Normals, xyz, device) as ctx:
        if queries is not None:
            return ctx.estimate_at(queries, k, radius)
        N = ctx.estimate(k, radius, device_out=ctx._like)
        if orient is None:
            return N
        return ctx.orient(N, orient_k, None, None if isinstance(orient, str) else orient)


def orient_normals(xyz, normals, k=8, radius=None, viewpoint=None, device=0):
    """normals of the points xyz with one consistent sign per connected component of the k-nearest-neighbour graph
    (1 <= k <= 32): facing the viewpoint, or outward (away from the centre of the bounds) when viewpoint is None.  Zero
    normals stay zero.  numpy in, numpy out; GPU tensors in, a GPU tensor out.  See Normals.orient."""
    with session(Normals, xyz, device) as ctx:
        return ctx.orient(normals, k, radius, viewpoint)
