"""ctypes binding of include/s4p_feature.h (libsuper4pcs_normals.so): Fast Point Feature Histograms (Rusu et al., ICRA 2009) of
a whole cloud and a feature-space matcher, on the device, and start poses from the matches on the host.

    from super4pcs_amd import features, icp
    Fp, cp = features.compute_fpfh(P, radius=0.08)                  # (n, 33) uint16 in [0, 4096], (n,) int32 accepted pairs
    Fq, cq = features.compute_fpfh(Q, radius=0.08)                  # normals within radius / 2, oriented outward
    M = features.match_features(Fp, Fq)                             # (k, 2) int32 of (row of P, row of Q), mutual best
    T0s = features.poses_from_matches(P, Q, M, max_distance=0.02)   # (<= 16, 4, 4) float64, each maps Q onto P
    T, res, i = icp.refine_best(P, Q, T0s, max_distance=0.02)       # the one the full clouds prefer

The descriptor needs CONSISTENTLY ORIENTED normals: with normals whose sign is arbitrary, as Shape.estimate and
Normals.estimate return them, the histograms of one surface patch differ between two clouds and almost no match is right.
compute_fpfh therefore orients by default.  The descriptor is defined to its last bit (histograms are sums of integers, the
feature distance is an integer), so two calls, the host and the device forms and a restatement on the CPU give the same
bits.  Clouds and normals are (n, 3) float32 numpy arrays or GPU torch tensors; descriptors are (n, 33) uint16 numpy arrays or
GPU torch tensors of dtype uint16; tensors go through the *_device entry points and the results are tensors on the same
device.  There is no CPU fallback: without a device, Features() raises NormalsError with code -2.
"""
import ctypes as C

import numpy as np

from . import _binding as _B
from . import shape as _SH
from ._binding import TWIN
from .normals import NormalsError, session

BINS = 33
MAX_VALUE = 4096

_VP = C.c_void_p
SIGNATURES = {                                         # include/s4p_feature.h
    "s4p_feature_fpfh" + TWIN: [_VP, _VP, C.c_float, _VP, _VP],
    "s4p_feature_match" + TWIN: [_VP, _VP, C.c_int64, _VP, C.c_int64, C.c_int32, _VP, _VP],
}
SYMBOLS = _B.names(SIGNATURES)


def load_library(path=None, *tables):
    """The normals library with the s4p_feature.h entry points declared; a library without them is an error."""
    return _SH.load_library(path, SIGNATURES, *tables)


def _table(F):
    """(tensor?, a contiguous (rows, 33) uint16 table, its pointer, rows)."""
    if _B.is_torch(F):
        import torch
        if not (F.is_cuda and F.dtype == torch.uint16 and F.dim() == 2 and F.shape[1] == BINS):
            raise ValueError("torch descriptors must be a (rows, 33) uint16 tensor on the GPU")
        F = F.contiguous()
        return True, F, F.data_ptr(), int(F.shape[0])
    F = np.ascontiguousarray(F)
    if F.dtype != np.uint16 or F.ndim != 2 or F.shape[1] != BINS:
        raise ValueError("descriptors are (rows, 33) uint16")
    return False, F, F.ctypes.data, int(F.shape[0])


class Features(_SH.Shape):
    """An s4p_normals context (one GPU, one cloud) with the descriptor and the matcher; every method of shape.Shape works on
    it too.  match needs no cloud."""
    _load = staticmethod(load_library)

    def fpfh(self, normals, radius):
        """(F (n, 33) uint16, count (n,) int32) of the cloud's points from their normals (n, 3), which must be consistently
        oriented (Normals.orient).  The results follow the normals' kind: numpy in, numpy out; a GPU tensor in, tensors out."""
        like, nrm, pn = self._normals_copy(normals)
        F, pf = _B.empty(like, (self.n, BINS), np.uint16)
        count, pc = _B.empty(like, (self.n,), np.int32)
        self._call("s4p_feature_fpfh", like, pn, float(radius), pf, pc)
        return F, count

    def match(self, fa, fb, mutual=True):
        """(idx (m,) int32, dist (m,) int32): for every row of fa the row of fb with the smallest (squared distance, index)
        among the rows of fb that are not all zeros, and that distance; -1 and -1 for a row of fa that is all zeros, when fb
        has no usable row, and, with mutual, when the row is not its partner's best in turn."""
        da, fa, pa, m = _table(fa)
        db, fb, pb, n = _table(fb)
        if da != db:
            raise ValueError("both tables are numpy arrays or both are GPU tensors")
        like = fa if da else None
        idx, pi = _B.empty(like, (m,), np.int32)
        dist, pd = _B.empty(like, (m,), np.int32)
        self._call("s4p_feature_match", like, pa, m, pb, n, 1 if mutual else 0, pi, pd)
        return idx, dist


def compute_fpfh(xyz, radius, normals=None, normal_radius=None, orient="outward", device=0, orient_k=8):
    """(F (n, 33) uint16, count (n,) int32): the FPFH of every point of xyz from the points within radius.  Without normals
    they are estimated on the same context from every point within normal_radius (default radius / 2, Shape.estimate) and
    oriented consistently (Normals.orient): orient is "outward" or a viewpoint (x, y, z).  Normals that are given are taken
    as they are, and must be oriented already.

    orient=None skips the orientation of estimated normals.  WARNING: their sign is then arbitrary (the component of largest
    magnitude is positive), one surface patch gets different histograms in two clouds, and matching such descriptors finds
    almost nothing; it is there for measuring exactly that."""
    if isinstance(orient, str) and orient != "outward":
        raise ValueError('orient is None, "outward" or a viewpoint (x, y, z)')
    if normals is not None and normal_radius is not None:
        raise ValueError("normal_radius applies to estimated normals only")
    with session(Features, xyz, device) as ctx:
        if normals is None:
            normals = ctx.estimate(float(normal_radius) if normal_radius is not None else float(radius) / 2)[0]
            if orient is not None:
                normals = ctx.orient(normals, orient_k, None, None if isinstance(orient, str) else orient)
        return ctx.fpfh(normals, radius)


def match_features(fa, fb, mutual=True, device=0):
    """(k, 2) int32 of (row of fa, row of fb), in ascending row of fa: Features.match without the rows that found no partner."""
    with session(Features, None, device) as ctx:
        idx, _ = ctx.match(fa, fb, mutual)
    if _B.is_torch(idx):
        import torch
        a = torch.nonzero(idx >= 0).flatten()
        return torch.stack([a.to(torch.int32), idx[a]], 1)
    a = np.flatnonzero(idx >= 0)
    return np.stack([a.astype(np.int32), idx[a]], 1).astype(np.int32).reshape(-1, 2)


def _kabsch(A, B):
    """The 4 x 4 rigid motion T with T B ~ A in the least-squares sense (A, B (k, 3) float64)."""
    ca, cb = A.mean(0), B.mean(0)
    U, _, Vt = np.linalg.svd((B - cb).T @ (A - ca))
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d if d != 0 else 1.0]) @ U.T
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = ca - R @ cb
    return T


def poses_from_matches(P, Q, matches, max_distance, trials=4096, starts=16, seed=0, min_edge=None):
    """Start poses for ICP from feature matches, on the host in float64: (starts', 4, 4), starts' <= starts, each mapping Q
    onto P, the best first.

    matches is (k, 2) of (row of P, row of Q) as match_features returns it.  trials triples of matches are drawn from
    np.random.default_rng(seed).  A triple is dropped when it repeats a match, when its shortest edge (in either cloud) is
    below min_edge (default max_distance), or when a pair of corresponding edges differs in length by more than 10 % of the
    longer one.  The others give a rigid motion (Kabsch); its score is the number of matches it brings within max_distance.
    The candidates are ordered by (score descending, trial ascending) and the first `starts` are returned, shaped for
    icp.refine_best:

        T0s = poses_from_matches(P, Q, M, max_distance=0.02)
        T, res, i = icp.refine_best(P, Q, T0s, max_distance=0.02)

    The order is a vote among the matches only.  On a cloud whose point spacing is as large as max_distance a wrong pose can
    collect more ICP correspondences than the right one: look at more than the first candidate."""
    P = np.asarray(P, np.float64); Q = np.asarray(Q, np.float64)
    M = np.asarray(matches).reshape(-1, 2).astype(np.int64)
    if not (max_distance > 0) or trials < 1 or starts < 1:
        raise ValueError("max_distance > 0, trials >= 1 and starts >= 1 are required")
    edge = float(max_distance if min_edge is None else min_edge)
    out = np.zeros((0, 4, 4))
    if len(M) < 3:
        return out
    A, B = P[M[:, 0]], Q[M[:, 1]]
    tri = np.random.default_rng(seed).integers(0, len(M), size=(int(trials), 3))
    cand = []
    for t, (i, j, k) in enumerate(tri):
        if i == j or j == k or i == k:
            continue
        ok = True
        for u, v in ((i, j), (j, k), (i, k)):
            la, lb = np.linalg.norm(A[u] - A[v]), np.linalg.norm(B[u] - B[v])
            if min(la, lb) < edge or abs(la - lb) > 0.1 * max(la, lb):
                ok = False
                break
        if not ok:
            continue
        T = _kabsch(A[[i, j, k]], B[[i, j, k]])
        moved = B @ T[:3, :3].T + T[:3, 3]
        score = int((np.linalg.norm(moved - A, axis=1) <= max_distance).sum())
        cand.append((-score, t, T))
    cand.sort(key=lambda c: (c[0], c[1]))
    if cand:
        out = np.stack([c[2] for c in cand[:int(starts)]])
    return out
