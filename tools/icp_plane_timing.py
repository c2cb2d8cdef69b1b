"""Point-to-plane ICP timing and pose errors ("Point-to-plane ICP") -> profiles/icp_plane_timing.json.

    python tools/icp_plane_timing.py [--out profiles/icp_plane_timing.json] [--quick] [--no-register]

Per configuration (BASELINE.json configs[2]-[4] clouds, the sizes of DESIGN.md section 11's table), max_distance d = 4 delta
and normal radius d:
  - estimate_normals: host clock around the synchronised call, median of 5 after a warm-up;
  - one plane pass (k_match_plane, k_final_plane, 31-double read-back) with the source ordered as refine orders it:
    median of 10 refine calls of one iteration minus the same with zero iterations (the final pass is one plane pass);
  - from a 1 degree / 0.2 % of the extent start: iterations, status and wall time of a whole refine for both metrics at
    the same rel_tol (1e-6, max 30 iterations), and the pose errors before and after;
  - unless --no-register: Super4PCS on the clouds, then both metrics, pose errors to the generator's pose.
--quick: 1 M-point pair only, no registration (for a kernel-trace run under rocprofv3).
"""
import argparse
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


def _refine_both(ctx, icp, T0, T_gt):
    out = {}
    for metric in ("point", "plane"):
        ctx.refine(T0, max_iterations=1, metric=metric)                 # warm-up of this metric's kernels
        t0 = time.perf_counter(); T, r = ctx.refine(T0, max_iterations=30, rel_tol=1e-6, metric=metric); secs = time.perf_counter() - t0
        out[metric] = {"iterations": r.iterations, "status": icp.STATUS_NAMES[r.status], "seconds": secs, "rmse": r.rmse,
                       "fitness": r.fitness, "err_before": _errs(T0, T_gt), "err_after": _errs(T, T_gt)}
    return out


def one(name, P, Q, T_gt, delta, overlap, sample, register, max_time):
    from super4pcs_amd import capi, icp
    d = 4 * delta
    extent = float(np.linalg.norm(P.max(0) - P.min(0)))
    rec = {"config": name, "n_P": int(len(P)), "n_Q": int(len(Q)), "delta": delta, "max_distance": d, "normal_radius": d,
           "min_neighbours": icp.MIN_NEIGHBOURS}
    ctx = icp.ICP(0)
    ctx.set_target(P, d)
    ctx.set_source(Q)
    ctx.estimate_normals(d)
    rec["estimate_normals_s_median_min"] = _clock(lambda: ctx.estimate_normals(d), 5)
    N = ctx.target_normals()
    rec["zero_normals"] = int(np.count_nonzero(~N.any(1)))
    T0 = _motion(1.0, 0.002 * extent) @ T_gt
    ctx.refine(T0, max_iterations=1, metric="plane")
    one_it = _clock(lambda: ctx.refine(T0, max_iterations=1, metric="plane"), 10)
    zero_it = _clock(lambda: ctx.refine(T0, max_iterations=0, metric="plane"), 10)
    rec["refine_plane_1_iteration_s_median_min"] = one_it
    rec["refine_plane_0_iterations_s_median_min"] = zero_it
    rec["plane_pass_ordered_s"] = one_it[0] - zero_it[0]
    rec["from_1deg"] = _refine_both(ctx, icp, T0, T_gt)
    ctx.close()
    if register:
        gm = capi.Matcher(capi.make_options(delta, overlap, sample, max_time_seconds=max_time), device=0)
        lcp, M, Qm = gm.compute_transformation(P, Q)
        gm.close()
        M = M.astype(np.float64)
        reg = {"sample": sample, "overlap": overlap, "max_time_seconds": max_time, "lcp": lcp, "rot_deg_trans_super4pcs": _errs(M, T_gt)}
        for metric in ("point", "plane"):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_plane_timing.json"))
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--no-register", action="store_true")
    a = ap.parse_args()
    from super4pcs_amd import build as B, datasets as D
    B.build_icp()
    out = {"tool": "tools/icp_plane_timing.py", "rows": []}
    t0 = time.perf_counter()
    reg = not (a.no_register or a.quick)
    P, Q, T = D.bumpy_pair(1_000_000, overlap=0.5, delta=0.004, seed=20140814)
    out["rows"].append(one("configs[2] bumpy 1M/1M", P, Q, T, 0.004, 0.5, 2000, reg, 30))
    if not a.quick:
        P, Q, T = D.lidar_pair(5_000_000, delta=0.05)
        out["rows"].append(one("configs[3] lidar 5M/5M", P, Q, T, 0.05, 0.4, 2000, reg, 40))
        P, Q, T = D.part_in_whole_pair(10_000_000, 100_000, delta=0.05)
        out["rows"].append(one("configs[4] part-in-whole 10M scene / 100k query", P, Q, T, 0.05, 0.2, 1000, reg, 40))
    out["wall_s"] = time.perf_counter() - t0
    if not a.quick:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print("written" if not a.quick else "quick run", a.out)


if __name__ == "__main__":
    main()
