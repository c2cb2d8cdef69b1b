"""Symmetric ICP timing and pose errors ("Symmetric ICP") -> profiles/icp_symm_timing.json.

    python tools/icp_symm_timing.py [--out profiles/icp_symm_timing.json] [--parent-lib path/to/libsuper4pcs_icp.so]
                                    [--configs 2,3] [--no-register] [--quick]

Per configuration (BASELINE.json configs[2] / configs[3] clouds), max_distance d = 4 delta, target normals estimated within
d, source normals the 16 nearest neighbours' (super4pcs_amd.normals):
  - one iteration with the source ordered as refine orders it, for the symmetric, the plane and the generalized metric of
    this library and, with --parent-lib, the plane and the generalized metric of that library (the parent commit's build):
    all in one process, interleaved (every repetition times every variant once, one-iteration and zero-iteration calls),
    10 repetitions; one iteration = median of the one-iteration calls minus median of the zero-iteration calls, with the
    range (min, max) of both;
  - whole refines (rel_tol 1e-6, max 30 iterations) from a 1 degree / 0.2 % of the extent start and from 5 and 10 degrees
    off: iterations, status, wall time and the pose errors before and after, for plane, gicp and symmetric;
  - unless --no-register (configs[2] only): Super4PCS at sample 2000, then the three metrics, pose errors to the generator's
    pose.
--quick: the configs[2] one-iteration loop of this library only, nothing written (for a kernel-trace run under rocprofv3).
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

METRICS = ("plane", "gicp", "symmetric")


def _motion(angle_deg, shift):
    a = np.array([0.3, -0.5, 0.8]); a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(angle_deg)
    T = np.eye(4); T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K; T[:3, 3] = shift
    return T


def _errs(M, T):
    R = M[:3, :3] @ T[:3, :3].T
    return float(np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))), float(np.linalg.norm(M[:3, 3] - T[:3, 3]))


class LibCtx:
    """One context of any build of the library through ctypes: target, source, estimated target normals, given source
    normals, and refine(metric, iterations) for plane / gicp / symmetric (the last only where the build exports it)."""

    def __init__(self, lib_path, P, Q, Nq, d):
        from super4pcs_amd import _binding, icp
        self.icp = icp
        L = self.L = C.CDLL(lib_path)
        for table in icp.TABLES:
            _binding.declare(L, table)                 # without an error class: a parent build may lack s4p_icp_refine_symm
        self.h = C.c_void_p()
        assert L.s4p_icp_create(0, C.byref(self.h)) == 0
        cols = lambda X: [np.ascontiguousarray(X[:, k], np.float32) for k in range(3)]
        pc, qc, nc = cols(P), cols(Q), cols(Nq)
        assert L.s4p_icp_set_target(self.h, pc[0].ctypes.data, pc[1].ctypes.data, pc[2].ctypes.data, len(P), float(d)) == 0
        assert L.s4p_icp_set_source(self.h, qc[0].ctypes.data, qc[1].ctypes.data, qc[2].ctypes.data, len(Q)) == 0
        assert L.s4p_icp_estimate_normals(self.h, float(d), icp.MIN_NEIGHBOURS) == 0
        assert L.s4p_icp_set_source_normals(self.h, nc[0].ctypes.data, nc[1].ctypes.data, nc[2].ctypes.data, len(Q)) == 0

    def refine(self, metric, T0, iterations, rel_tol=1e-6):
        icp, L = self.icp, self.L
        p = icp.Params()
        L.s4p_icp_default_params(C.byref(p))
        p.max_iterations, p.rel_tol = int(iterations), float(rel_tol)
        T = np.ascontiguousarray(T0, np.float64).reshape(16).copy()
        r = icp.Result()
        dp = T.ctypes.data_as(C.POINTER(C.c_double))
        if metric == "plane":
            rc = L.s4p_icp_refine_plane(self.h, C.byref(p), dp, C.byref(r))
        elif metric == "gicp":
            rc = L.s4p_icp_refine_gicp(self.h, C.byref(p), icp.GICP_EPSILON, dp, C.byref(r))
        else:
            rc = L.s4p_icp_refine_symm(self.h, C.byref(p), dp, C.byref(r))
        assert rc == 0, (metric, rc)
        return T.reshape(4, 4), r

    def close(self):
        self.L.s4p_icp_destroy(self.h)


def interleaved_iterations(variants, T0, reps=10):
    """variants: {name: (LibCtx, metric)}.  Every repetition times a one-iteration and a zero-iteration refine of every
    variant, in turn.  {name: {iteration_s, one: (median, min, max), zero: (median, min, max)}}."""
    for ctx, metric in variants.values():
        ctx.refine(metric, T0, 1)                      # first use: buffers, the source order's scratch
    t = {name: ([], []) for name in variants}
    for _ in range(reps):
        for name, (ctx, metric) in variants.items():
            for k in (1, 0):
                t0 = time.perf_counter(); ctx.refine(metric, T0, k); t[name][1 - k].append(time.perf_counter() - t0)
    out = {}
    for name, (one, zero) in t.items():
        stat = lambda v: (float(np.median(v)), float(np.min(v)), float(np.max(v)))
        out[name] = {"iteration_s": float(np.median(one) - np.median(zero)), "one_iteration_median_min_max_s": stat(one),
                     "zero_iterations_median_min_max_s": stat(zero)}
    return out


def _whole(ctx, icp, T0, T_gt):
    out = {}
    for metric in METRICS:
        ctx.refine(metric, T0, 1)
        t0 = time.perf_counter(); T, r = ctx.refine(metric, T0, 30); secs = time.perf_counter() - t0
        out[metric] = {"iterations": r.iterations, "status": icp.STATUS_NAMES[r.status], "seconds": secs, "rmse": r.rmse,
                       "fitness": r.fitness, "err_before": _errs(T0, T_gt), "err_after": _errs(T, T_gt)}
    return out


def one(name, P, Q, T_gt, delta, overlap, sample, register, max_time, parent_lib, quick=False):
    from super4pcs_amd import capi, icp, normals
    d = 4 * delta
    extent = float(np.linalg.norm(P.max(0) - P.min(0)))
    rec = {"config": name, "n_P": int(len(P)), "n_Q": int(len(Q)), "delta": delta, "max_distance": d, "normal_radius": d,
           "source_normal_k": 16, "gicp_epsilon": icp.GICP_EPSILON}
    Nq = normals.estimate_normals(Q, k=16)
    ctx = LibCtx(icp.LIB_PATH, P, Q, Nq, d)
    T0 = _motion(1.0, 0.002 * extent) @ T_gt
    variants = {m: (ctx, m) for m in METRICS}
    parent = None
    if parent_lib and not quick:
        parent = LibCtx(parent_lib, P, Q, Nq, d)
        variants["parent plane"] = (parent, "plane")
        variants["parent gicp"] = (parent, "gicp")
    rec["one_iteration"] = interleaved_iterations(variants, T0)
    if parent:
        parent.close()
    if not quick:
        rec["from_start"] = {"%g degrees" % a: _whole(ctx, icp, _motion(a, 0.002 * extent) @ T_gt, T_gt) for a in (1.0, 5.0, 10.0)}
    ctx.close()
    if register and not quick:
        gm = capi.Matcher(capi.make_options(delta, overlap, sample, max_time_seconds=max_time), device=0)
        lcp, M, Qm = gm.compute_transformation(P, Q)
        gm.close()
        M = M.astype(np.float64)
        reg = {"sample": sample, "overlap": overlap, "max_time_seconds": max_time, "lcp": lcp, "rot_deg_trans_super4pcs": _errs(M, T_gt)}
        for metric in METRICS:
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_symm_timing.json"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--configs", default="2,3")
    ap.add_argument("--no-register", action="store_true")
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    from super4pcs_amd import build as B, datasets as D
    B.build_icp()
    B.build_normals()
    out = {"tool": "tools/icp_symm_timing.py", "parent_lib": bool(a.parent_lib), "rows": []}
    t0 = time.perf_counter()
    cfgs = [2] if a.quick else [int(c) for c in a.configs.split(",") if c]
    if 2 in cfgs:
        P, Q, T = D.bumpy_pair(1_000_000, overlap=0.5, delta=0.004, seed=20140814)
        out["rows"].append(one("configs[2] bumpy 1M/1M", P, Q, T, 0.004, 0.5, 2000, not a.no_register, 30, a.parent_lib, a.quick))
    if 3 in cfgs:
        P, Q, T = D.lidar_pair(5_000_000, delta=0.05)
        out["rows"].append(one("configs[3] lidar 5M/5M", P, Q, T, 0.05, 0.4, 2000, False, 40, a.parent_lib))
    out["wall_s"] = time.perf_counter() - t0
    if not a.quick:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print("written" if not a.quick else "quick run", a.out)


if __name__ == "__main__":
    main()
