"""Cost and effect of the ICP correspondence rejection ("Correspondence rejection") -> profiles/icp_reject_timing.json.

    python tools/icp_reject_timing.py [--out profiles/icp_reject_timing.json] [--quick]

Per pair (the 1 M bumpy pair and the 5 M lidar pair of DESIGN.md section 11's table), with target normals estimated on the
device and k = 16 nearest-neighbour source normals:
  - one iteration = one split pass (s4p_icp_gicp_sums: k_search, the sum kernel, the final sum, the read-back), host clock
    around the synchronised call, with the rejection off (the parent path), with reciprocity, and with both tests at 60
    degrees; the three are timed in turn, 12 rounds after 2 warm-up rounds, median and minimum per variant, so that a drift of
    the machine falls on all three alike;
  - the same per iteration inside a refine (source ordered by the T0-image, 10 iterations, tolerance 0);
  - the one-time cost of the source grid: the first pass after set_rejection minus a steady pass.
Pose errors: the 1 M bumpy pair at 60 % overlap from a start 1 degree / 0.2 % of the extent off, 100 iterations at most, point
and generalized metrics, with no filter, reciprocity, the normal test, and both.
--quick: the 1 M pair's timing only (for a kernel-trace run under rocprofv3); writes nothing.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ANGLE = 60.0
VARIANTS = (("off", dict()), ("reciprocal", dict(reciprocal=True)), ("reciprocal+normals60", dict(reciprocal=True, normal_angle=ANGLE)))


def _motion(angle_deg, shift):
    a = np.array([0.3, -0.5, 0.8]); a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(angle_deg)
    T = np.eye(4); T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K; T[:3, 3] = shift
    return T


def _errs(M, T):
    R = M[:3, :3] @ T[:3, :3].T
    return float(np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))), float(np.linalg.norm(M[:3, 3] - T[:3, 3]))


def _context(P, Q, d):
    from super4pcs_amd import icp, normals
    ctx = icp.ICP(0)
    ctx.set_target(P, d)
    ctx.set_source(Q)
    ctx.estimate_normals(d)
    ctx.set_source_normals(normals.estimate_normals(Q, k=16))
    return ctx


def timing(name, P, Q, T_gt, delta):
    from tests import icp_helpers as H
    d = 4 * delta
    extent = float(np.linalg.norm(P.max(0) - P.min(0)))
    rec = {"pair": name, "n_P": int(len(P)), "n_Q": int(len(Q)), "delta": delta, "max_distance": d, "normal_angle_deg": ANGLE}
    ctx = _context(P, Q, d)
    T0 = _motion(1.0, 0.002 * extent) @ T_gt
    Tc = H.to_centred(T0, ctx.frame()).astype(np.float32)
    ctx.gicp_sums(Tc)                                               # module load, first allocations
    # the source grid: first pass after set_rejection against a steady one
    ctx.set_rejection(reciprocal=True)
    t0 = time.perf_counter(); ctx.gicp_sums(Tc); first = time.perf_counter() - t0
    t0 = time.perf_counter(); ctx.gicp_sums(Tc); steady = time.perf_counter() - t0
    rec["source_grid_build_s"] = first - steady
    stage = {v: [] for v, _ in VARIANTS}
    counts = {}
    for rnd in range(14):
        for v, kw in VARIANTS:
            ctx.set_rejection(**kw)
            t0 = time.perf_counter(); s = ctx.gicp_sums(Tc); dt = time.perf_counter() - t0
            if rnd >= 2:
                stage[v].append(dt)
            counts[v] = ctx.rejection_counts().tolist() if kw else [int(s[0]), 0, 0, int(s[0])]
    rec["split_pass_s_median_min"] = {v: (float(np.median(t)), float(np.min(t))) for v, t in stage.items()}
    rec["counts_matched_normals_reciprocity_kept"] = counts
    off = rec["split_pass_s_median_min"]["off"][0]
    rec["split_pass_ratio_to_off"] = {v: rec["split_pass_s_median_min"][v][0] / off for v, _ in VARIANTS}
    loop = {}
    for v, kw in VARIANTS:
        ctx.set_rejection(**kw)
        ctx.refine(T0, metric="gicp", max_iterations=2, rel_tol=0.0)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter(); _, r = ctx.refine(T0, metric="gicp", max_iterations=10, rel_tol=0.0); ts.append(time.perf_counter() - t0)
        loop[v] = {"refine_10_iterations_s_median": float(np.median(ts)), "passes": r.iterations + 1,
                   "per_pass_s": float(np.median(ts)) / (r.iterations + 1)}
    rec["refine_ordered"] = loop
    rec["refine_per_pass_ratio_to_off"] = {v: loop[v]["per_pass_s"] / loop["off"]["per_pass_s"] for v, _ in VARIANTS}
    ctx.close()
    print(json.dumps(rec), flush=True)
    return rec


def pose_errors(P, Q, T_gt, delta, overlap):
    from super4pcs_amd import icp
    d = 4 * delta
    extent = float(np.linalg.norm(P.max(0) - P.min(0)))
    T0 = _motion(1.0, 0.002 * extent) @ T_gt
    ctx = _context(P, Q, d)
    rec = {"pair": "bumpy 1M/1M, overlap %.1f" % overlap, "max_distance": d, "start_rot_deg_trans": _errs(T0, T_gt), "max_iterations": 100,
           "normal_angle_deg": ANGLE, "runs": []}
    filters = (("none", dict()), ("reciprocal", dict(reciprocal=True)), ("normals60", dict(normal_angle=ANGLE)),
               ("reciprocal+normals60", dict(reciprocal=True, normal_angle=ANGLE)))
    for metric in ("point", "gicp"):
        for fname, kw in filters:
            ctx.set_rejection(**kw)
            T, r = ctx.refine(T0, metric=metric, max_iterations=100)
            rec["runs"].append({"metric": metric, "filter": fname, "iterations": r.iterations, "status": icp.STATUS_NAMES[r.status],
                                "n_corr": int(r.n_corr), "rmse": r.rmse, "rot_deg_trans": _errs(T, T_gt)})
            print(json.dumps(rec["runs"][-1]), flush=True)
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_reject_timing.json"))
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    from super4pcs_amd import build as B, datasets as D
    B.build_icp()
    B.build_normals()
    out = {"tool": "tools/icp_reject_timing.py", "timing": [], "pose": []}
    t0 = time.perf_counter()
    P, Q, T = D.bumpy_pair(1_000_000, overlap=0.5, delta=0.004, seed=20140814)
    out["timing"].append(timing("configs[2] bumpy 1M/1M", P, Q, T, 0.004))
    if not a.quick:
        P, Q, T = D.lidar_pair(5_000_000, delta=0.05)
        out["timing"].append(timing("configs[3] lidar 5M/5M", P, Q, T, 0.05))
        P, Q, T = D.bumpy_pair(1_000_000, overlap=0.6, delta=0.004, seed=20140814)
        out["pose"].append(pose_errors(P, Q, T, 0.004, 0.6))
    out["wall_s"] = time.perf_counter() - t0
    if not a.quick:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print("written" if not a.quick else "quick run", a.out)


if __name__ == "__main__":
    main()
