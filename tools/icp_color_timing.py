"""Coloured ICP timing and pose errors ("Coloured ICP") -> profiles/icp_color_timing.json.

    python tools/icp_color_timing.py [--out profiles/icp_color_timing.json] [--parent-lib path/to/libsuper4pcs_icp.so]
                                     [--configs 2,3] [--quick]

Per configuration (BASELINE.json configs[2] / configs[3] clouds with a smooth synthetic intensity on both), max_distance
d = 4 delta, target normals estimated within d, gradients within d; everything in one process, each figure the median of
10 measurements:
  - one iteration with the source ordered as refine orders it: 10 refine calls of one iteration minus the same with zero
    iterations, for the coloured and the plane metric of this library and, with --parent-lib, for the plane metric of that
    library (the parent commit's build);
  - estimate_color_gradients beside estimate_normals at the same radius (both synchronise before they return);
  - from a 1 degree / 0.2 % of the extent start: iterations, status and wall time of a whole refine for the plane and the
    coloured metric (rel_tol 1e-6, max 30 iterations), and the pose errors before and after.
--quick: the configs[2] one-iteration loop only, nothing written (for a kernel-trace run under rocprofv3).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import icp_gicp_timing as G  # noqa: E402  (the shared clock, start motion, pose errors and the parent library's plane iteration)


def texture(X, scale):
    """A smooth intensity field in (x, y), as the tests' (tests/icp_color_helpers.texture)."""
    X = np.asarray(X, np.float64)
    x, y = scale * X[:, 0], scale * X[:, 1]
    v = 0.5 + 0.25 * np.sin(2 * np.pi * 1.5 * x + 0.3) * np.cos(2 * np.pi * 1.2 * y) + 0.2 * np.sin(2 * np.pi * (0.8 * x + 1.1 * y))
    return v.astype(np.float32)


def one(name, P, Q, T_gt, delta, scale, parent_lib, quick=False):
    from super4pcs_amd import icp
    d = 4 * delta
    extent = float(np.linalg.norm(P.max(0) - P.min(0)))
    rec = {"config": name, "n_P": int(len(P)), "n_Q": int(len(Q)), "delta": delta, "max_distance": d, "normal_radius": d,
           "color_radius": d, "color_lambda": icp.COLOR_LAMBDA, "texture_scale": scale}
    Ip = texture(P, scale)
    Iq = texture(Q.astype(np.float64) @ T_gt[:3, :3].T + T_gt[:3, 3], scale)
    ctx = icp.ICP(0)
    ctx.set_target(P, d)
    ctx.set_source(Q)
    ctx.estimate_normals(d)
    ctx.set_target_intensity(Ip)
    ctx.set_source_intensity(Iq)
    ctx.estimate_color_gradients(d)
    T0 = G._motion(1.0, 0.002 * extent) @ T_gt
    c = G._iteration(lambda k: ctx.refine(T0, max_iterations=k, metric="color"))
    p = G._iteration(lambda k: ctx.refine(T0, max_iterations=k, metric="plane"))
    rec["color_iteration_s"], rec["refine_color_1_iteration_s_median_min"], rec["refine_color_0_iterations_s_median_min"] = c
    rec["plane_iteration_s"], rec["refine_plane_1_iteration_s_median_min"], rec["refine_plane_0_iterations_s_median_min"] = p
    rec["color_over_plane"] = c[0] / p[0]
    if parent_lib:
        pp = G.parent_plane_iteration(parent_lib, P, Q, d, T0)
        rec["parent_plane_iteration_s"], rec["parent_refine_plane_1_iteration_s_median_min"], rec["parent_refine_plane_0_iterations_s_median_min"] = pp
        rec["color_over_parent_plane"] = c[0] / pp[0]
    if not quick:
        rec["from_start"] = G._whole(ctx, icp, T0, T_gt, metrics=("plane", "color"))
        # the gradients last: estimate_normals invalidates them, so each gradient call follows a normals call
        tn, tg = [], []
        for _ in range(10):
            t0 = time.perf_counter(); ctx.estimate_normals(d); tn.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); ctx.estimate_color_gradients(d); tg.append(time.perf_counter() - t0)
        rec["estimate_normals_s_median_min"] = [float(np.median(tn)), float(np.min(tn))]
        rec["estimate_color_gradients_s_median_min"] = [float(np.median(tg)), float(np.min(tg))]
        rec["gradients_over_normals"] = float(np.median(tg) / np.median(tn))
        g = ctx.target_color_gradients()
        rec["zero_gradients"] = int((~g.any(1)).sum())
    ctx.close()
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_color_timing.json"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--configs", default="2,3")
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    from super4pcs_amd import build as B, datasets as D
    B.build_icp()
    out = {"tool": "tools/icp_color_timing.py", "parent_lib": bool(a.parent_lib), "rows": []}
    t0 = time.perf_counter()
    cfgs = [2] if a.quick else [int(c) for c in a.configs.split(",") if c]
    if 2 in cfgs:
        P, Q, T = D.bumpy_pair(1_000_000, overlap=0.5, delta=0.004, seed=20140814)
        out["rows"].append(one("configs[2] bumpy 1M/1M", P, Q, T, 0.004, 4.0, a.parent_lib, a.quick))
    if 3 in cfgs:
        P, Q, T = D.lidar_pair(5_000_000, delta=0.05)
        out["rows"].append(one("configs[3] lidar 5M/5M", P, Q, T, 0.05, 0.2, a.parent_lib))
    out["wall_s"] = time.perf_counter() - t0
    if not a.quick:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print("written" if not a.quick else "quick run", a.out)


if __name__ == "__main__":
    main()
