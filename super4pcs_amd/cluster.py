"""ctypes binding of include/s4p_cluster.h (libsuper4pcs_normals.so): density clustering (DBSCAN) and fixed-radius density on
the device.

    from super4pcs_amd import cluster
    labels, kind, stats = cluster.cluster_dbscan(P, eps=0.03, min_points=4)     # (n,) int32, -1 = noise; (n,) uint8 0 / 1 / 2
    kept, mask, labels = cluster.keep_clusters(P, eps=0.03, min_points=4)       # the largest cluster, input order kept
    ctx = cluster.Cluster(); ctx.set_cloud(P); counts = ctx.density(0.03)       # (n,) int32, the point itself included

Clouds are (N, 3) float32 numpy arrays, or (N, 3) float32 torch tensors on the GPU (they go through the *_device entry
points and the results are torch tensors on the same device); both give the same bits.  The result is unique: clusters are
numbered by their smallest core index, and a border point joins the cluster of its nearest core neighbour under (d2 bits,
index).  There is no CPU fallback: without a device, Cluster() raises NormalsError with code -2.
"""
import ctypes as C

import numpy as np

from . import _binding as _B
from . import knn as _K
from ._binding import TWIN
from .normals import NormalsError, session

NOISE, BORDER, CORE = 0, 1, 2


class ClusterStats(C.Structure):
    _fields_ = [("core", C.c_int64), ("border", C.c_int64), ("noise", C.c_int64), ("clusters", C.c_int64)]

    def as_dict(self):
        return {"core": self.core, "border": self.border, "noise": self.noise, "clusters": self.clusters}


_VP = C.c_void_p
SIGNATURES = {                                         # include/s4p_cluster.h
    "s4p_cluster_dbscan" + TWIN: [_VP, C.c_float, C.c_int32, _VP, _VP, C.POINTER(ClusterStats)],
    "s4p_cluster_density" + TWIN: [_VP, C.c_float, _VP],
}
SYMBOLS = _B.names(SIGNATURES)


def load_library(path=None, *tables):
    """The normals library with the s4p_cluster.h entry points declared; a library without them is an error."""
    return _K.load_library(path, SIGNATURES, *tables)


class Cluster(_K.Knn):
    """An s4p_normals context (one GPU, one cloud) with the clustering calls; the normals and the neighbour-list methods
    work on it too.  Results follow the cloud's kind: numpy for a numpy cloud, torch tensors on its device for a GPU tensor."""
    _load = staticmethod(load_library)

    def dbscan(self, eps, min_points=10):
        """(labels (n,) int32, kind (n,) uint8, stats dict): labels number the clusters from 0 in ascending order of their
        smallest core index, -1 is noise; kind is NOISE, BORDER or CORE."""
        labels, pl = _B.empty(self._like, (self.n,), np.int32)
        kind, pk = _B.empty(self._like, (self.n,), np.uint8)
        st = ClusterStats()
        self._call("s4p_cluster_dbscan", self._like, float(eps), int(min_points), pl, pk, C.byref(st))
        return labels, kind, st.as_dict()

    def density(self, radius):
        """(n,) int32: the number of points within radius of each point (d2 <= fl(r*r)), the point itself included."""
        count, pc = _B.empty(self._like, (self.n,), np.int32)
        self._call("s4p_cluster_density", self._like, float(radius), pc)
        return count


def cluster_dbscan(xyz, eps, min_points=10, device=0):
    """DBSCAN of the cloud: (labels, kind, stats) as Cluster.dbscan returns them."""
    with session(Cluster, xyz, device) as ctx:
        return ctx.dbscan(eps, min_points)


def largest_labels(labels, keep=1, min_size=1):
    """The labels of the `keep` largest clusters with at least min_size points, largest first; ties in size go to the smaller
    label.  labels: a numpy int array, -1 = noise."""
    if keep < 1 or min_size < 1:
        raise ValueError("keep and min_size must be at least 1")
    labels = np.asarray(labels)
    size = np.bincount(labels[labels >= 0]) if (labels >= 0).any() else np.zeros(0, np.int64)
    order = np.argsort(-size, kind="stable")
    return [int(c) for c in order if size[c] >= min_size][:keep]


def keep_clusters(xyz, eps, min_points=10, keep=1, min_size=1, device=0):
    """The cloud without everything but its `keep` largest clusters of at least min_size points (ties in size go to the
    smaller label).  Returns (kept_xyz, keep_mask, labels); kept_xyz = xyz[keep_mask] keeps the input order."""
    xyz = xyz if _B.is_torch(xyz) else np.asarray(xyz)
    labels, _, _ = cluster_dbscan(xyz, eps, min_points, device)
    host = labels.cpu().numpy() if _B.is_torch(labels) else labels
    mask = np.isin(host, np.asarray(largest_labels(host, keep, min_size), np.int64))
    if _B.is_torch(labels):
        import torch
        mask = torch.from_numpy(mask).to(labels.device)
    return xyz[mask], mask, labels
