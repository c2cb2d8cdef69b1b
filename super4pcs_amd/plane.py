"""ctypes binding of include/s4p_plane.h (libsuper4pcs_normals.so): RANSAC plane segmentation on the device, and ground removal
on top of it.

    from super4pcs_amd import plane
    pl, mask, info = plane.segment_plane(P, distance=0.15)                  # (4,) float32 n, d; (n,) uint8; dict
    planes, labels = plane.segment_planes(P, distance=0.05, max_planes=3)    # (p, 4) float32; (n,) int32, -1 = no plane
    kept, keep_mask, planes = plane.remove_planes(P, distance=0.15)          # the cloud without its dominant plane
    ctx = plane.Plane(); ctx.set_cloud(P); pl, mask, info = ctx.segment(0.15, exclude=mask0)

Clouds are (N, 3) float32 numpy arrays, or (N, 3) float32 torch tensors on the GPU (they go through the *_device entry point
and the results are torch tensors on the same device); both give the same bits.  The result is unique: candidate t samples
from a seeded splitmix64 stream, the largest count wins and ties go to the smallest t, every sum of the refit has one order
(the header states all of it).  The mask is defined by the residual in the centred frame (info["centre"],
info["d_centred"]), not by n . x + d evaluated in float.  There is no CPU fallback: without a device, Plane() raises
NormalsError with code -2.
"""
import ctypes as C

import numpy as np

from . import _binding as _B
from . import cluster as _CL
from ._binding import TWIN
from .normals import NormalsError, session

MAX_TRIALS, MAX_REFINE, SUM_BLOCK = 1 << 20, 16, 128


class PlaneOptions(C.Structure):
    _fields_ = [("distance", C.c_float), ("trials", C.c_int32), ("seed", C.c_uint64), ("refine", C.c_int32)]


class PlaneResult(C.Structure):
    _fields_ = [("normal", C.c_float * 3), ("d", C.c_float), ("centre", C.c_float * 3), ("d_centred", C.c_float),
                ("inliers", C.c_int64), ("alive", C.c_int64), ("trial", C.c_int32), ("valid_trials", C.c_int32)]

    def plane(self):
        return np.array([self.normal[0], self.normal[1], self.normal[2], self.d], np.float32)

    def as_dict(self):
        return {"centre": np.array(list(self.centre), np.float32), "d_centred": np.float32(self.d_centred), "inliers": self.inliers,
                "alive": self.alive, "trial": self.trial, "valid_trials": self.valid_trials}


_VP = C.c_void_p
SIGNATURES = {                                         # include/s4p_plane.h
    "s4p_plane_segment" + TWIN: [_VP, C.POINTER(PlaneOptions), _VP, C.POINTER(PlaneResult), _VP],
}
SYMBOLS = _B.names(SIGNATURES)


def load_library(path=None, *tables):
    """The normals library with the s4p_plane.h entry points declared; a library without them is an error."""
    return _CL.load_library(path, SIGNATURES, *tables)


class Plane(_CL.Cluster):
    """An s4p_normals context (one GPU, one cloud) with the plane call; the clustering, neighbour-list and normals methods work
    on it too.  Results follow the cloud's kind: numpy for a numpy cloud, torch tensors on its device for a GPU tensor."""
    _load = staticmethod(load_library)

    def _exclude(self, exclude):
        """(pointer or None, keep-alive) of an exclude mask of the cloud's kind, any integer or bool type, nonzero = excluded."""
        if exclude is None:
            return None, None
        if self._like is not None:
            import torch
            e = (torch.as_tensor(exclude, device=self._like.device) != 0).to(torch.uint8).contiguous()
            if e.shape != (self.n,):
                raise ValueError("exclude must have one entry per point")
            return e.data_ptr(), e
        e = np.ascontiguousarray(np.asarray(exclude) != 0, dtype=np.uint8)
        if e.shape != (self.n,):
            raise ValueError("exclude must have one entry per point")
        return e.ctypes.data, e

    def segment(self, distance, trials=1024, seed=0, refine=1, exclude=None):
        """(plane (4,) float32 = n, d with n . x + d = 0; mask (n,) uint8, 1 = inlier; info dict with centre, d_centred,
        inliers, alive, trial and valid_trials).  trial is -1, the plane zero and the mask empty when no candidate was
        valid."""
        pe, keep = self._exclude(exclude)
        mask, pm = _B.empty(self._like, (self.n,), np.uint8)
        opt = PlaneOptions(float(distance), int(trials), int(seed) & 0xFFFFFFFFFFFFFFFF, int(refine))
        res = PlaneResult()
        self._call("s4p_plane_segment", self._like, C.byref(opt), pe, C.byref(res), pm)
        return res.plane(), mask, res.as_dict()


def segment_plane(xyz, distance, trials=1024, seed=0, refine=1, exclude=None, device=0):
    """The dominant plane of the cloud: (plane, mask, info) as Plane.segment returns them."""
    with session(Plane, xyz, device) as ctx:
        return ctx.segment(distance, trials, seed, refine, exclude)


def peel_planes(segment, n, max_planes=4, min_inliers=3, like=None):
    """The peeling loop of segment_planes on any segment(p, exclude) -> (plane, mask, info): plane p is found on the points no
    earlier plane took, and the loop stops at the first plane with fewer than min_inliers inliers (that plane is dropped).
    Returns (planes (P, 4) float32, labels (n,) int32, -1 = no plane); the labels are a tensor on like's device when like is
    a GPU tensor, as the masks then are."""
    if max_planes < 1 or min_inliers < 1:
        raise ValueError("max_planes and min_inliers must be at least 1")
    labels, _ = _B.empty(like, (n,), np.int32)
    labels[:] = -1
    planes = []
    for p in range(max_planes):
        pl, mask, info = segment(p, (labels >= 0) if p else None)
        if info["trial"] < 0 or info["inliers"] < min_inliers:
            break
        labels[mask != 0] = p
        planes.append(pl)
    return np.array(planes, np.float32).reshape(-1, 4), labels


def segment_planes(xyz, distance, max_planes=4, min_inliers=3, trials=1024, seed=0, refine=1, device=0):
    """Up to max_planes planes peeled off one uploaded cloud, largest remaining first: plane p uses the seed seed + p and
    excludes the inliers of the planes before it; the loop stops at the first plane with fewer than min_inliers inliers.
    Returns (planes (P, 4) float32, labels (n,) int32, -1 = no plane); for a GPU tensor the labels are a tensor on its device."""
    with session(Plane, xyz, device) as ctx:
        return peel_planes(lambda p, ex: ctx.segment(distance, trials, seed + p, refine, ex), ctx.n, max_planes, min_inliers, ctx._like)


def remove_planes(xyz, distance, count=1, min_inliers=3, trials=1024, seed=0, refine=1, device=0):
    """The cloud without its `count` dominant planes (segment_planes with max_planes = count): returns (kept_xyz, keep_mask,
    planes); kept_xyz = xyz[keep_mask] keeps the input order."""
    xyz = xyz if _B.is_torch(xyz) else np.asarray(xyz)
    planes, labels = segment_planes(xyz, distance, count, min_inliers, trials, seed, refine, device)
    keep = labels < 0
    return xyz[keep], keep, planes
