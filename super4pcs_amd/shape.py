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

from . import _binding as _B
from . import plane as _PL
from ._binding import TWIN
from .normals import NormalsError, session

_VP = C.c_void_p
SIGNATURES = {                                         # include/s4p_shape.h
    "s4p_shape_estimate" + TWIN: [_VP, C.c_float, C.c_int32, _VP, _VP, _VP],
    "s4p_shape_estimate_at" + TWIN: [_VP, _VP, _VP, _VP, C.c_int64, C.c_float, C.c_int32, _VP, _VP, _VP],
}
SYMBOLS = _B.names(SIGNATURES)


def load_library(path=None, *tables):
    """The normals library with the s4p_shape.h entry points declared; a library without them is an error."""
    return _PL.load_library(path, SIGNATURES, *tables)


class Shape(_PL.Plane):
    """An s4p_normals context (one GPU, one cloud) with the radius-normals call; the plane, clustering, neighbour-list and
    orientation methods work on it too.  estimate here is the radius call: the k-nearest-neighbour estimate of the same
    context is normals.Normals.estimate(ctx, k)."""
    _load = staticmethod(load_library)

    def estimate(self, radius, min_neighbours=3, queries=None):
        """(normals (rows, 3) float32, eig (rows, 3) float32 l1 >= l2 >= l3, count (rows,) int32) of the cloud's own points,
        or of the query positions when queries is given.  The cloud's rows follow the cloud's kind, the queries' rows the
        queries' kind: numpy in, numpy out; a GPU tensor in, tensors out."""
        if queries is None:
            name, like, rows, where = "s4p_shape_estimate", self._like, self.n, ()
        else:
            dev, ptr, rows, keep = _B.cols(queries)
            name, like, where = "s4p_shape_estimate_at", queries if dev else None, (*ptr, rows)
        normals, pn = _B.empty(like, (rows, 3), np.float32)
        eig, pe = _B.empty(like, (rows, 3), np.float32)
        count, pc = _B.empty(like, (rows,), np.int32)
        self._call(name, like, *where, float(radius), int(min_neighbours), pn, pe, pc)
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
    with session(Shape, xyz, device) as ctx:
        N, eig, count = ctx.estimate(radius, min_neighbours, queries)
        if orient is not None:
            N = ctx.orient(N, orient_k, None, None if isinstance(orient, str) else orient)
        return N, eig, count


def surface_variation(eig):
    """l3 / (l1 + l2 + l3) of every row of eig (rows, 3), 0 where the sum is not > 0: 0 on a plane, up to 1 / 3 where the
    neighbourhood has no direction.  float32; numpy in, numpy out; a tensor in, a tensor out."""
    if _B.is_torch(eig):
        import torch
        total = (eig[:, 0] + eig[:, 1]) + eig[:, 2]
        ok = total > 0
        return torch.where(ok, eig[:, 2] / torch.where(ok, total, torch.ones_like(total)), torch.zeros_like(total))
    eig = np.asarray(eig, np.float32)
    total = (eig[:, 0] + eig[:, 1]) + eig[:, 2]
    ok = total > 0
    return np.where(ok, eig[:, 2] / np.where(ok, total, np.float32(1)), np.float32(0)).astype(np.float32)
