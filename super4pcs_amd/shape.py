"""ctypes binding of include/s4p_shape.h (libsuper4pcs_normals.so): normals from every point within a radius, with the
eigenvalues of the neighbourhood's covariance and the neighbour count, on the device.

    from super4pcs_amd import shape
    N, eig, cnt = shape.estimate_normals_radius(P, radius=0.02)                 # (n, 3), (n, 3) l1 >= l2 >= l3, (n,) int32
    N, eig, cnt = shape.estimate_normals_radius(P, 0.02, queries=Q)             # at Q's positions from P's points
    N, eig, cnt = shape.estimate_normals_radius(P, 0.02, orient="outward")      # one sign per surface (Normals.orient)
    curvature = shape.surface_variation(eig)                                    # l3 / (l1 + l2 + l3)
    ctx = shape.Shape(); ctx.set_cloud(P); N, eig, cnt = ctx.estimate(0.02, min_neighbours=10)

normals.estimate_normals takes at most 32 neighbours; on a dense, noisy scan those lie inside the noise.  Here the
neighbourhood is every point with d2 <= fl(r*r), the point itself included.  Clouds are (N, 3) float32 numpy arrays, or (N, 3)
float32 torch tensors on the GPU (they go through the *_device entry points and the results are torch tensors on the same
device); both give the same bits.  The result is unique: the moments are sums of integers (offsets quantised to r 2^-18),
which have no order.  A row with fewer than max(3, min_neighbours) neighbours, or whose neighbours all coincide, is all
zeros.  There is no CPU fallback: without a device, Shape() raises NormalsError with code -2.
"""
import ctypes as C

import numpy as np

from . import plane as _PL
from .knn import _empty
from .normals import NormalsError, _cols, _is_torch

SYMBOLS = ["s4p_shape_estimate", "s4p_shape_estimate_device", "s4p_shape_estimate_at", "s4p_shape_estimate_at_device"]

_DECLARED = False


def load_library():
    """The normals library with the s4p_shape.h entry points declared; a library without them is an error."""
    global _DECLARED
    L = _PL.load_library()
    if _DECLARED:
        return L
    vp = C.c_void_p
    missing = [s for s in SYMBOLS if not hasattr(L, s)]
    if missing:
        raise NormalsError(-7, "libsuper4pcs_normals.so lacks %s: rebuild it (build.build_normals())" % ", ".join(missing))
    for name in ("s4p_shape_estimate", "s4p_shape_estimate_device"):
        getattr(L, name).restype = C.c_int32
        getattr(L, name).argtypes = [vp, C.c_float, C.c_int32, vp, vp, vp]
    for name in ("s4p_shape_estimate_at", "s4p_shape_estimate_at_device"):
        getattr(L, name).restype = C.c_int32
        getattr(L, name).argtypes = [vp, vp, vp, vp, C.c_int64, C.c_float, C.c_int32, vp, vp, vp]
    _DECLARED = True
    return L


class Shape(_PL.Plane):
    """An s4p_normals context (one GPU, one cloud) with the radius-normals call; the plane, clustering, neighbour-list and
    orientation methods work on it too.  estimate here is the radius call: the k-nearest-neighbour estimate of the same
    context is normals.Normals.estimate(ctx, k)."""

    def __init__(self, device=0):
        load_library()
        super().__init__(device)

    def estimate(self, radius, min_neighbours=3, queries=None):
        """(normals (rows, 3) float32, eig (rows, 3) float32 l1 >= l2 >= l3, count (rows,) int32) of the cloud's own points,
        or of the query positions when queries is given.  The cloud's rows follow the cloud's kind, the queries' rows the
        queries' kind: numpy in, numpy out; a GPU tensor in, tensors out."""
        if queries is None:
            like, rows = self._like, self.n
        else:
            dev, ptr, rows, keep = _cols(queries)
            like = queries if dev else None
        normals, pn = _empty(like, (rows, 3), np.float32)
        eig, pe = _empty(like, (rows, 3), np.float32)
        count, pc = _empty(like, (rows,), np.int32)
        if like is not None:
            import torch
            torch.cuda.synchronize(like.device)           # torch's allocations before the library writes on its own stream
        if queries is None:
            fn = self.L.s4p_shape_estimate_device if like is not None else self.L.s4p_shape_estimate
            self._chk(fn(self.h, float(radius), int(min_neighbours), pn, pe, pc))
        else:
            fn = self.L.s4p_shape_estimate_at_device if like is not None else self.L.s4p_shape_estimate_at
            self._chk(fn(self.h, ptr[0], ptr[1], ptr[2], rows, float(radius), int(min_neighbours), pn, pe, pc))
            del keep
        return normals, eig, count


def estimate_normals_radius(xyz, radius, min_neighbours=3, queries=None, orient=None, device=0, orient_k=8):
    """Unit normals, eigenvalues and neighbour counts from every point of xyz within radius of each of its points, or of
    each query position when queries is given: (normals, eig, count) as Shape.estimate returns them.  The sign of a normal
    is arbitrary (its component of largest magnitude is positive) unless orient is given: "outward", or a viewpoint
    (x, y, z), orients the cloud's own normals consistently over the graph of the orient_k nearest neighbours
    (normals.Normals.orient)."""
    if orient is not None and queries is not None:
        raise ValueError("orient applies to the cloud's own normals, not to queries")
    if isinstance(orient, str) and orient != "outward":
        raise ValueError('orient is None, "outward" or a viewpoint (x, y, z)')
    ctx = Shape(device)
    try:
        ctx.set_cloud(xyz)
        N, eig, count = ctx.estimate(radius, min_neighbours, queries)
        if orient is not None:
            N = ctx.orient(N, orient_k, None, None if isinstance(orient, str) else orient)
        return N, eig, count
    finally:
        ctx.close()


def surface_variation(eig):
    """l3 / (l1 + l2 + l3) of every row of eig (rows, 3), 0 where the sum is not > 0: 0 on a plane, up to 1 / 3 where the
    neighbourhood has no direction.  float32; numpy in, numpy out; a tensor in, a tensor out."""
    if _is_torch(eig):
        import torch
        total = (eig[:, 0] + eig[:, 1]) + eig[:, 2]
        ok = total > 0
        return torch.where(ok, eig[:, 2] / torch.where(ok, total, torch.ones_like(total)), torch.zeros_like(total))
    eig = np.asarray(eig, np.float32)
    total = (eig[:, 0] + eig[:, 1]) + eig[:, 2]
    ok = total > 0
    return np.where(ok, eig[:, 2] / np.where(ok, total, np.float32(1)), np.float32(0)).astype(np.float32)
