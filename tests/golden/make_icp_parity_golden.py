"""Records tests/golden/icp_parity.npz: what libsuper4pcs_icp.so returns, bit for bit, on every refine and sums path.

    python tests/golden/make_icp_parity_golden.py          (on the MI355X, by hand, with the library to be pinned)

record() is the one list of calls; tests/test_gpu_icp_parity.py runs it again and asks for equal arrays.  Every sum is a
fixed-order double sum without floating atomics, so a library that keeps the kernels and the refine loop's bookkeeping
returns the same bits.  Inputs come from tests/icp_edge_cases.py:
  small   box_faces: n_Q = 15 000 = 58 x 256 + 2 x 64 + 24 (59 workgroups, a partial last block and a partial last wave)
  large   full_launch, the source cut to 524 289 = 2048 x 256 + 1 (the first size whose lanes take two trips): sums only
  flat    a planar target with the normals (0, 0, 1): the plane metric's degenerate stop
Normals of the target are estimated on the device, the source normals and the intensities are fixed functions below."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import icp_edge_cases as E  # noqa: E402
from tests import icp_helpers as H  # noqa: E402

F = np.float32
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "icp_parity.npz")
REJECT = (("off", dict()), ("rej", dict(reciprocal=True, normal_angle=60.0)))
ROBUST = (("huber", dict(loss="huber")), ("trimmed", dict(loss="trimmed", trim_fraction=0.7)))


def _motion(angle_deg, shift):
    a = np.array([0.3, -0.5, 0.8]); a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(angle_deg)
    T = np.eye(4); T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K; T[:3, 3] = shift
    return T


def source_normals(Q, seed):
    """Random directions, every 11th zero (a source point without a normal)."""
    N = np.random.default_rng(seed).normal(size=Q.shape).astype(F)
    N[::11] = 0
    return N


def intensity(X):
    X = np.asarray(X, np.float64)
    return (np.sin(3.0 * X[:, 0]) + np.cos(5.0 * X[:, 1]) * X[:, 2]).astype(F)


def _context(icp, case, Q, seed, normals=None):
    ctx = icp.ICP(0)
    ctx.set_target(case.P, case.d)
    ctx.set_source(Q)
    if normals is None:
        ctx.estimate_normals(case.d)
    else:
        ctx.set_target_normals(normals)
    ctx.set_source_normals(source_normals(Q, seed))
    ctx.set_target_intensity(intensity(case.P))
    ctx.set_source_intensity(intensity(Q))
    ctx.estimate_color_gradients(case.d)
    return ctx


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def _result(r):
    return np.frombuffer(bytes(r), np.uint8).copy()


def _sums(ctx, Tc, out, tag):
    out[tag + "/sums/point"] = ctx.sums(Tc)
    out[tag + "/sums/plane"] = ctx.plane_sums(Tc)
    for metric in ("point", "plane"):
        for name, kw in ROBUST:
            s, info = ctx.robust_sums(Tc, metric, **kw)
            out["%s/sums/%s_%s" % (tag, name, metric)] = s
            out["%s/sums/%s_%s/info" % (tag, name, metric)] = info
    out[tag + "/sums/gicp"] = ctx.gicp_sums(Tc)
    out[tag + "/sums/color"] = ctx.color_sums(Tc)
    out[tag + "/sums/counts"] = ctx.rejection_counts()


def _refines(ctx, T0, out, tag, **kw):
    """Every metric's refine -> T, the Result's bytes, the robust info and the counters the final pass left."""
    runs = [("point", dict(metric="point")), ("plane", dict(metric="plane")), ("gicp", dict(metric="gicp")), ("color", dict(metric="color"))]
    runs += [("%s_%s" % (name, metric), dict(metric=metric, **rk)) for metric in ("point", "plane") for name, rk in ROBUST]
    for name, mk in runs:
        info = np.zeros(8, np.float64) if "loss" in mk else None
        T, r = ctx.refine(T0, info=info, **mk, **kw)
        key = "%s/%s" % (tag, name)
        out[key + "/T"] = T
        out[key + "/result"] = _result(r)
        out[key + "/counts"] = ctx.rejection_counts()
        if info is not None:
            out[key + "/info"] = info


def record(icp):
    """name -> array, for every call the parity check pins."""
    out = {}
    # the small case: everything
    case = E.box_faces()
    ctx = _context(icp, case, case.Q, 11)
    T0 = E.pose(case, _motion(0.3, 0.002))
    Tc = H.to_centred(T0, ctx.frame()).astype(F)
    for rname, rkw in REJECT:
        ctx.set_rejection(**rkw)
        tag = "small/" + rname
        _sums(ctx, Tc, out, tag)
        idx, d2, why = ctx.rejection(Tc)
        out[tag + "/rejection/sha256_idx_d2_why"] = _sha(idx, d2, why)                    # 15 000 answers each: their digest
        out[tag + "/rejection/why_histogram"] = np.bincount(why, minlength=4)
        out[tag + "/rejection/counts"] = ctx.rejection_counts()
        _refines(ctx, T0, out, tag + "/refine5", max_iterations=5, rel_tol=0.0)          # the max-iterations path
        _refines(ctx, T0, out, tag + "/refine")                                            # the converged path
        # too few: min_correspondences above the count
        for name, mk in (("point", dict()), ("plane", dict(metric="plane")), ("huber_point", dict(loss="huber")),
                         ("gicp", dict(metric="gicp"))):
            T, r = ctx.refine(T0, min_correspondences=10 ** 9, **mk)
            out["%s/too_few/%s/T" % (tag, name)] = T
            out["%s/too_few/%s/result" % (tag, name)] = _result(r)
        T, r = ctx.refine(T0, max_iterations=3, order_source=False)
        out[tag + "/unordered/T"], out[tag + "/unordered/result"] = T, _result(r)
        T, r = ctx.refine(T0, max_iterations=0)
        out[tag + "/zero_iterations/T"], out[tag + "/zero_iterations/result"] = T, _result(r)
    ctx.close()
    # the degenerate plane system: a planar target whose normals are all (0, 0, 1)
    case = E.flat()
    ctx = _context(icp, case, case.Q, 12, normals=np.tile(np.array([0, 0, 1], F), (len(case.P), 1)))
    for name, mk in (("plane", dict(metric="plane")), ("huber_plane", dict(metric="plane", loss="huber"))):
        T, r = ctx.refine(case.T0, **mk)
        out["flat/%s/T" % name], out["flat/%s/result" % name] = T, _result(r)
    ctx.close()
    # the grid-stride path: sums only
    case = E.full_launch_pair()
    Q = case.Q[:E.FULL_LAUNCH_N[1]]
    ctx = _context(icp, case, Q, 13)
    Tc = H.to_centred(E.pose(case, _motion(0.3, 0.002)), ctx.frame()).astype(F)
    for rname, rkw in REJECT:
        ctx.set_rejection(**rkw)
        _sums(ctx, Tc, out, "large/" + rname)
    ctx.close()
    return out


if __name__ == "__main__":
    from super4pcs_amd import build as B
    B.build_icp()
    from super4pcs_amd import icp as I
    arrays = record(I)
    np.savez_compressed(OUT, **arrays)
    print("%d arrays -> %s (%d bytes)" % (len(arrays), OUT, os.path.getsize(OUT)))
