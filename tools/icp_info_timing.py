"""Information-pass timing ("Multiway registration") -> profiles/icp_info_timing.json.

    python tools/icp_info_timing.py [--out profiles/icp_info_timing.json] [--reps 20]

BASELINE.json configs[2] clouds (bumpy 1M/1M), max_distance d = 4 delta, target normals estimated within d, source normals the
16 nearest neighbours' (super4pcs_amd.normals), T = the generator's pose moved by 1 degree and 0.2 % of the extent.  One
information pass (ICP.information_sums: k_search, k_info_sum, k_final_info, one read-back) against one generalized pass of the
same library (ICP.gicp_sums: k_search, k_gicp_sum, k_final_plane, one read-back), both stage calls over the source as
uploaded: one process, a first call of each outside the clock, then every repetition times each call once, in turn.  Reported:
median, min and max of the wall time of a call, and of ICP.information (the pass plus the 6x6 matrix on the host).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_info_timing.json"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    from super4pcs_amd import build as B, datasets as D, icp, normals
    B.build_icp()
    B.build_normals()
    delta = 0.004
    d = 4 * delta
    P, Q, T_gt = D.bumpy_pair(1_000_000, overlap=0.5, delta=delta, seed=20140814)
    extent = float(np.linalg.norm(P.max(0) - P.min(0)))
    T = _motion(1.0, 0.002 * extent) @ T_gt
    ctx = icp.ICP(0)
    ctx.set_target(P, d)
    ctx.set_source(Q)
    ctx.estimate_normals(d)
    ctx.set_source_normals(normals.estimate_normals(Q, k=16))
    c = ctx.frame().astype(np.float64)
    Tc = T.copy()
    Tc[:3, 3] = T[:3, 3] + T[:3, :3] @ c - c
    Tc = Tc.astype(np.float32)
    calls = {"information_sums": lambda: ctx.information_sums(Tc), "gicp_sums": lambda: ctx.gicp_sums(Tc),
             "information": lambda: ctx.information(T)}
    first = {k: f() for k, f in calls.items()}
    t = {k: [] for k in calls}
    for _ in range(a.reps):
        for k, f in calls.items():
            t0 = time.perf_counter(); f(); t[k].append(time.perf_counter() - t0)
    stat = lambda v: [float(np.median(v)), float(np.min(v)), float(np.max(v))]
    out = {"tool": "tools/icp_info_timing.py", "config": "configs[2] bumpy 1M/1M", "n_P": int(len(P)), "n_Q": int(len(Q)),
           "delta": delta, "max_distance": d, "reps": a.reps, "n_matched": int(first["information_sums"][0]),
           "call_median_min_max_s": {k: stat(v) for k, v in t.items()},
           "information_minus_gicp_median_s": float(np.median(t["information_sums"]) - np.median(t["gicp_sums"]))}
    ctx.close()
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("written", a.out)


if __name__ == "__main__":
    main()
