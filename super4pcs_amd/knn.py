"""ctypes binding of include/s4p_knn.h (libsuper4pcs_normals.so): exact k-nearest-neighbour lists and the two standard
outlier filters on the device, on the search that normal estimation uses.

    from super4pcs_amd import knn
    idx, d2, cnt = knn.knn(P, k=16)                                   # (n, 16) int32, (n, 16) float32, (n,) int32
    idx, d2, cnt = knn.knn(P, k=8, radius=0.05, exclude_self=True)     # rows padded with -1 / +inf where fewer are found
    idx, d2, cnt = knn.knn(P, k=8, queries=Q)                          # neighbours in P of the positions Q
    kept, mask, stats = knn.remove_statistical_outliers(P, k=16, std_ratio=2.0)
    kept, mask = knn.remove_radius_outliers(P, radius=0.05, min_neighbours=4)

Clouds are (N, 3) float32 numpy arrays, or (N, 3) float32 torch tensors on the GPU (they go through the *_device entry
points and the results are torch tensors on the same device); both give the same bits.  Neighbours are ordered by
(d2, index), d2 = dx*dx + (dy*dy + dz*dz) in float.  There is no CPU fallback: without a device, Knn() raises NormalsError
with code -2.
"""
import ctypes as C

import numpy as np

from . import _binding as _B
from . import normals as _N
from ._binding import TWIN
from .normals import NormalsError, _radius, session

MIN_K, MAX_K = 1, 32


class OutlierStats(C.Structure):
    _fields_ = [("n", C.c_int64), ("mean", C.c_double), ("stddev", C.c_double), ("threshold", C.c_double), ("kept", C.c_int64)]

    def as_dict(self):
        return {"n": self.n, "mean": self.mean, "stddev": self.stddev, "threshold": self.threshold, "kept": self.kept}


_VP = C.c_void_p
SIGNATURES = {                                         # include/s4p_knn.h
    "s4p_knn_search" + TWIN: [_VP, C.c_int32, C.c_float, C.c_int32, _VP, _VP, _VP],
    "s4p_knn_search_at" + TWIN: [_VP, _VP, _VP, _VP, C.c_int64, C.c_int32, C.c_float, _VP, _VP, _VP],
    "s4p_outliers_statistical" + TWIN: [_VP, C.c_int32, C.c_double, _VP, _VP, C.POINTER(OutlierStats)],
    "s4p_outliers_radius" + TWIN: [_VP, C.c_float, C.c_int32, _VP],
}
SYMBOLS = _B.names(SIGNATURES)


def load_library(path=None, *tables):
    """The normals library with the s4p_knn.h entry points declared; a library without them is an error."""
    return _N.load_library(path, SIGNATURES, *tables)


def _lists(like, rows, k):
    """((idx (rows, k) int32, d2 (rows, k) float32, cnt (rows,) int32), their pointers), empty, of like's kind."""
    idx, pi = _B.empty(like, (rows, max(k, 0)), np.int32)
    d2, pd = _B.empty(like, (rows, max(k, 0)), np.float32)
    cnt, pc = _B.empty(like, (rows,), np.int32)
    return (idx, d2, cnt), (pi, pd, pc)


class Knn(_N.Normals):
    """An s4p_normals context (one GPU, one cloud and its grid) with the neighbour queries and the outlier filters; the
    normals methods (estimate, estimate_at, grid) work on it too."""
    _load = staticmethod(load_library)

    def search(self, k, radius=None, exclude_self=False):
        """(idx (n, k) int32, d2 (n, k) float32, cnt (n,) int32) of the cloud's own points."""
        out, ptrs = _lists(self._like, self.n, int(k))
        self._call("s4p_knn_search", self._like, int(k), _radius(radius), 1 if exclude_self else 0, *ptrs)
        return out

    def search_at(self, Q, k, radius=None):
        """(idx (m, k), d2 (m, k), cnt (m,)) of the query positions Q (numpy in, numpy out; GPU tensor in, GPU tensor out)."""
        dev, ptr, m, keep = _B.cols(Q)
        like = Q if dev else None
        out, ptrs = _lists(like, m, int(k))
        self._call("s4p_knn_search_at", like, *ptr, m, int(k), _radius(radius), *ptrs)
        return out

    def statistical_outliers(self, k=16, std_ratio=2.0, want_mean_dist=True):
        """(keep (n,) bool, stats dict, mean_dist (n,) float64 or None): keep_j = (m_j <= mu + std_ratio * sigma)."""
        keep, pk = _B.empty(self._like, (self.n,), np.uint8)
        md, pm = _B.empty(self._like, (self.n,), np.float64) if want_mean_dist else (None, None)
        st = OutlierStats()
        self._call("s4p_outliers_statistical", self._like, int(k), float(std_ratio), pm, pk, C.byref(st))
        return _as_bool(keep), st.as_dict(), md

    def radius_outliers(self, radius, min_neighbours):
        """keep (n,) bool: at least min_neighbours other points within radius."""
        keep, pk = _B.empty(self._like, (self.n,), np.uint8)
        self._call("s4p_outliers_radius", self._like, float(radius), int(min_neighbours), pk)
        return _as_bool(keep)


def _as_bool(keep):
    if _B.is_torch(keep):
        return keep != 0
    return keep.astype(bool)


def knn(xyz, k, radius=None, queries=None, exclude_self=False, device=0):
    """The k nearest neighbours (1 <= k <= 32) in xyz of each of its own points, or of each query position when queries is
    given; radius > 0 keeps only neighbours with d2 <= fl(r*r).  exclude_self leaves the query's own index out (self form
    only).  Returns (idx, d2, cnt): rows in ascending (d2, index) order padded with -1 / +inf, and how many were found."""
    if queries is not None and exclude_self:
        raise ValueError("exclude_self applies to the cloud's own points, not to queries")
    with session(Knn, xyz, device) as ctx:
        if queries is not None:
            return ctx.search_at(queries, k, radius)
        return ctx.search(k, radius, exclude_self)


def remove_statistical_outliers(xyz, k=16, std_ratio=2.0, device=0):
    """Statistical outlier removal: a point is kept when the mean distance to its k nearest other points is at most
    mu + std_ratio * sigma of those means over the cloud.  Returns (kept_xyz, keep_mask, stats); kept_xyz = xyz[keep_mask]
    keeps the input order."""
    xyz = xyz if _B.is_torch(xyz) else np.asarray(xyz)
    with session(Knn, xyz, device) as ctx:
        keep, stats, _ = ctx.statistical_outliers(k, std_ratio, want_mean_dist=False)
        return xyz[keep], keep, stats


def remove_radius_outliers(xyz, radius, min_neighbours, device=0):
    """Radius outlier removal: a point is kept when at least min_neighbours (1..32) other points lie within radius.
    Returns (kept_xyz, keep_mask)."""
    xyz = xyz if _B.is_torch(xyz) else np.asarray(xyz)
    with session(Knn, xyz, device) as ctx:
        keep = ctx.radius_outliers(radius, min_neighbours)
        return xyz[keep], keep
