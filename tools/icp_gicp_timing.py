"""Generalized ICP timing and pose errors ("Generalized ICP") -> profiles/icp_gicp_timing.json.

    python tools/icp_gicp_timing.py [--out profiles/icp_gicp_timing.json] [--parent-lib path/to/libsuper4pcs_icp.so]
                                    [--configs 2,3] [--no-register] [--noisy] [--quick]

Per configuration (BASELINE.json configs[2] / configs[3] clouds), max_distance d = 4 delta, target normals estimated within
d, source normals the 16 nearest neighbours' (super4pcs_amd.normals):
  - one iteration with the source ordered as refine orders it: median of 10 refine calls of one iteration minus the same
    with zero iterations, for the generalized and the plane metric of this library and, with --parent-lib, for the plane
    metric of that library (the parent commit's build) in the same process and session;
  - from a 1 degree / 0.2 % of the extent start: iterations, status and wall time of a whole refine for the plane and the
    generalized metric (rel_tol 1e-6, max 30 iterations), and the pose errors before and after;
  - unless --no-register (configs[2] only): Super4PCS at sample 2000, then both metrics, pose errors to the generator's pose.
--noisy: kept apart from the rows, a bumpy 1 M pair at 60 % overlap with sigma = delta noise on the source, from a 2 degree start.
--quick: the configs[2] one-iteration loop only, nothing written (for a kernel-trace run under rocprofv3).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _motion(angle_deg, shift):
    a = np.array([0.3, -0.5, 0.8]); a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(angle_deg)
    T = np.eye(4); T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K; T[:3, 3] = shift
    return T


def _errs(M, T):
    R = M[:3, :3] @ T[:3, :3].T
    return float(np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))), float(np.linalg.norm(M[:3, 3] - T[:3, 3]))


def _clock(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(np.min(ts))


def _iteration(refine):
    """(seconds of one iteration, (median, min) of one-iteration calls, of zero-iteration calls)."""
    refine(1)
    one_it = _clock(lambda: refine(1), 10)
    zero_it = _clock(lambda: refine(0), 10)
    return one_it[0] - zero_it[0], one_it, zero_it


def parent_plane_iteration(lib_path, P, Q, d, T0):
    """The plane iteration of another build of the library (include/s4p_icp.h and s4p_icp_plane.h only), through ctypes."""
    from super4pcs_amd import icp
    L = C.CDLL(lib_path)
    vp, dp = C.c_void_p, C.POINTER(C.c_double)
    L.s4p_icp_create.argtypes = [C.c_int32, C.POINTER(vp)]
    L.s4p_icp_destroy.argtypes = [vp]; L.s4p_icp_destroy.restype = None
    L.s4p_icp_set_target.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_float]
    L.s4p_icp_set_source.argtypes = [vp, vp, vp, vp, C.c_int64]
    L.s4p_icp_estimate_normals.argtypes = [vp, C.c_float, C.c_int32]
    L.s4p_icp_default_params.argtypes = [C.POINTER(icp.Params)]; L.s4p_icp_default_params.restype = None
    L.s4p_icp_refine_plane.argtypes = [vp, C.POINTER(icp.Params), dp, C.POINTER(icp.Result)]
    h = vp()
    assert L.s4p_icp_create(0, C.byref(h)) == 0
    pc = [np.ascontiguousarray(P[:, k], np.float32) for k in range(3)]
    qc = [np.ascontiguousarray(Q[:, k], np.float32) for k in range(3)]
    assert L.s4p_icp_set_target(h, pc[0].ctypes.data, pc[1].ctypes.data, pc[2].ctypes.data, len(P), float(d)) == 0
    assert L.s4p_icp_set_source(h, qc[0].ctypes.data, qc[1].ctypes.data, qc[2].ctypes.data, len(Q)) == 0
    assert L.s4p_icp_estimate_normals(h, float(d), icp.MIN_NEIGHBOURS) == 0

    def refine(k):
        p = icp.Params()
        L.s4p_icp_default_params(C.byref(p))
        p.max_iterations = k
        T = np.ascontiguousarray(T0, np.float64).reshape(16).copy()
        r = icp.Result()
        assert L.s4p_icp_refine_plane(h, C.byref(p), T.ctypes.data_as(dp), C.byref(r)) == 0

    out = _iteration(refine)
    L.s4p_icp_destroy(h)
    return out


def _whole(ctx, icp, T0, T_gt, metrics=("plane", "gicp")):
    out = {}
    for metric in metrics:
        ctx.refine(T0, max_iterations=1, metric=metric)
        t0 = time.perf_counter(); T, r = ctx.refine(T0, max_iterations=30, rel_tol=1e-6, metric=metric); secs = time.perf_counter() - t0
        out[metric] = {"iterations": r.iterations, "status": icp.STATUS_NAMES[r.status], "seconds": secs, "rmse": r.rmse,
                       "fitness": r.fitness, "err_before": _errs(T0, T_gt), "err_after": _errs(T, T_gt)}
    return out


def one(name, P, Q, T_gt, delta, overlap, sample, register, max_time, parent_lib, quick=False, start_deg=1.0):
    from super4pcs_amd import capi, icp, normals
    d = 4 * delta
    extent = float(np.linalg.norm(P.max(0) - P.min(0)))
    rec = {"config": name, "n_P": int(len(P)), "n_Q": int(len(Q)), "delta": delta, "max_distance": d, "normal_radius": d,
           "source_normal_k": 16, "gicp_epsilon": icp.GICP_EPSILON}
    t0 = time.perf_counter(); Nq = normals.estimate_normals(Q, k=16); rec["source_normals_s_incl_upload"] = time.perf_counter() - t0
    ctx = icp.ICP(0)
    ctx.set_target(P, d)
    ctx.set_source(Q)
    ctx.estimate_normals(d)
    ctx.set_source_normals(Nq)
    T0 = _motion(start_deg, 0.002 * extent) @ T_gt
    g = _iteration(lambda k: ctx.refine(T0, max_iterations=k, metric="gicp"))
    p = _iteration(lambda k: ctx.refine(T0, max_iterations=k, metric="plane"))
    rec["gicp_iteration_s"], rec["refine_gicp_1_iteration_s_median_min"], rec["refine_gicp_0_iterations_s_median_min"] = g
    rec["plane_iteration_s"], rec["refine_plane_1_iteration_s_median_min"], rec["refine_plane_0_iterations_s_median_min"] = p
    rec["gicp_over_plane"] = g[0] / p[0]
    if parent_lib:
        pp = parent_plane_iteration(parent_lib, P, Q, d, T0)
        rec["parent_plane_iteration_s"], rec["parent_refine_plane_1_iteration_s_median_min"], rec["parent_refine_plane_0_iterations_s_median_min"] = pp
        rec["gicp_over_parent_plane"] = g[0] / pp[0]
    if not quick:
        rec["from_start"] = _whole(ctx, icp, T0, T_gt)
    ctx.close()
    if register and not quick:
        gm = capi.Matcher(capi.make_options(delta, overlap, sample, max_time_seconds=max_time), device=0)
        lcp, M, Qm = gm.compute_transformation(P, Q)
        gm.close()
        M = M.astype(np.float64)
        reg = {"sample": sample, "overlap": overlap, "max_time_seconds": max_time, "lcp": lcp, "rot_deg_trans_super4pcs": _errs(M, T_gt)}
        for metric in ("plane", "gicp"):
            t0 = time.perf_counter()
            dT, rr = icp.refine(P, Qm, np.eye(4), max_distance=d, metric=metric)
            secs = time.perf_counter() - t0
            reg[metric] = {"seconds_incl_upload_grid_normals": secs, "iterations": rr.iterations, "status": icp.STATUS_NAMES[rr.status],
                           "rmse": rr.rmse, "fitness": rr.fitness, "rot_deg_trans_refined": _errs(icp.compose(dT, M), T_gt)}
        rec["after_super4pcs"] = reg
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_gicp_timing.json"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--configs", default="2,3")
    ap.add_argument("--no-register", action="store_true")
    ap.add_argument("--noisy", action="store_true")
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    from super4pcs_amd import build as B, datasets as D
    B.build_icp()
    B.build_normals()
    out = {"tool": "tools/icp_gicp_timing.py", "parent_lib": bool(a.parent_lib), "rows": []}
    t0 = time.perf_counter()
    cfgs = [2] if a.quick else [int(c) for c in a.configs.split(",") if c]
    if 2 in cfgs:
        P, Q, T = D.bumpy_pair(1_000_000, overlap=0.5, delta=0.004, seed=20140814)
        out["rows"].append(one("configs[2] bumpy 1M/1M", P, Q, T, 0.004, 0.5, 2000, not a.no_register, 30, a.parent_lib, a.quick))
    if 3 in cfgs:
        P, Q, T = D.lidar_pair(5_000_000, delta=0.05)
        out["rows"].append(one("configs[3] lidar 5M/5M", P, Q, T, 0.05, 0.4, 2000, False, 40, a.parent_lib))
    if a.noisy and not a.quick:
        P, Q, T = D.bumpy_pair(1_000_000, overlap=0.6, delta=0.004, noise_sigma=0.004, seed=7)
        out["noisy_60pct_overlap"] = one("bumpy 1M/1M, 60 % overlap, sigma = delta, 2 degree start", P, Q, T, 0.004, 0.6, 2000, False, 30,
                                         None, start_deg=2.0)
    out["wall_s"] = time.perf_counter() - t0
    if not a.quick:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print("written" if not a.quick else "quick run", a.out)


if __name__ == "__main__":
    main()
