#!/usr/bin/env python
"""What estimated normals buy the registration (-a, Match4PCSOptions::max_normal_difference) on the BASELINE workloads;
writes profiles/normals_registration.json.
Base selection reads positions only, so with and without normals the same RNG stream draws the same bases: the first
N_BASES bases are compared one by one (pairs, quads, candidates, ms per base).  Then a whole registration at -a 20 under
max_time_seconds = 60 (trials completed) and the pose error against the generator before and after point-to-plane ICP.
The no-normals side is capped at NO_NORMALS_BUDGET_S seconds of bases per configuration (configs[2] at n = 20 000 costs
about 17 s per base: VERDICT.md's figures stand for it).
usage: python tools/normals_registration.py [out.json]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from super4pcs_amd import capi, datasets as D, icp, normals  # noqa: E402
from benchlib.workload import DELTA, OVERLAP, SEED  # noqa: E402

N_BASES = 20
NO_NORMALS_BUDGET_S = 60.0
K = 16


def pose_err(M, T):
    R = np.asarray(M, np.float64)[:3, :3] @ np.asarray(T, np.float64)[:3, :3].T
    ang = float(np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))))
    return ang, float(np.linalg.norm(np.asarray(M, np.float64)[:3, 3] - np.asarray(T, np.float64)[:3, 3]))


def per_base(P, Q, Pn, Qn, delta, overlap, n, a, budget=None):
    gm = capi.Matcher(capi.make_options(delta, overlap, n, max_normal_difference=a))
    gm.init_full(P, Q, Pn, None, Qn, None)
    rows, t_all = [], 0.0
    for _ in range(N_BASES):
        t0 = time.perf_counter()
        ok, r = gm.try_one_base()
        dt = time.perf_counter() - t0
        t_all += dt
        rows.append({"pairs": int(r.n_pairs1 + r.n_pairs2), "quads": int(r.n_quads), "candidates": int(r.n_verified), "ms": dt * 1e3})
        if budget is not None and t_all > budget:
            break
    gm.close()
    return rows


def summary(rows):
    if not rows:
        return None
    return {k: float(np.mean([r[k] for r in rows])) for k in ("pairs", "quads", "candidates", "ms")} | {"bases": len(rows)}


def full_run(P, Q, T, Pn, Qn, delta, overlap, n, a):
    gm = capi.Matcher(capi.make_options(delta, overlap, n, max_time_seconds=60, max_normal_difference=a))
    t0 = time.perf_counter()
    lcp, M, _ = gm.compute_transformation(P, Q, Pn, None, Qn, None)
    wall = time.perf_counter() - t0
    info = gm.info()
    out = {"a": a, "lcp": float(lcp), "wall_s": wall, "trials_completed": int(info.current_trial), "trials": int(info.number_of_trials),
           "finished_inside_60s": int(info.current_trial) >= int(info.number_of_trials) or wall < 60.0}
    e0 = pose_err(M, T)
    Tr, r = icp.refine(P, Q, np.asarray(M, np.float64), max_distance=4 * delta, metric="plane",
                       target_normals=Pn if Pn is not None and Pn.any(1).all() else None)
    e1 = pose_err(Tr, T)
    out.update({"pose_error_deg": e0[0], "pose_error_trans": e0[1], "after_plane_icp_deg": e1[0], "after_plane_icp_trans": e1[1],
                "icp_status": icp.STATUS_NAMES[r.status], "icp_iterations": int(r.iterations)})
    print(json.dumps(out), flush=True)
    return out


def config(label, P, Q, T, delta, overlap, samples, full_n):
    t0 = time.perf_counter()
    Pn = normals.estimate_normals(P, k=K)
    Qn = normals.estimate_normals(Q, k=K)
    res = {"label": label, "delta": delta, "overlap": overlap, "n_P": len(P), "n_Q": len(Q), "k": K,
           "normals_s_both_clouds_incl_transfer": time.perf_counter() - t0, "per_base": [], "full": None}
    for n, skip_plain in samples:
        row = {"sample": n}
        row["no_normals"] = "not measured (see VERDICT.md)" if skip_plain else summary(per_base(P, Q, None, None, delta, overlap, n, -1.0,
                                                                                                  NO_NORMALS_BUDGET_S))
        for a in (10.0, 20.0):
            rows = per_base(P, Q, Pn, Qn, delta, overlap, n, a)
            row["a%d" % a] = summary(rows)
        print(json.dumps(row), flush=True)
        res["per_base"].append(row)
    if full_n:
        res["full"] = full_run(P, Q, T, Pn, Qn, delta, overlap, full_n, 20.0)
    return res


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "normals_registration.json")
    res = {"source": "tools/normals_registration.py", "bases_per_row": N_BASES, "k": K,
           "no_normals_budget_s": NO_NORMALS_BUDGET_S, "configs": []}
    P, Q, T = D.bumpy_pair(1_000_000, overlap=OVERLAP, delta=DELTA, seed=SEED)
    res["configs"].append(config("configs[2] 1 M-point pair", P, Q, T, DELTA, OVERLAP, [(2000, False), (20000, True)], 2000))
    P, Q, T = D.lidar_pair(5_000_000, delta=0.05)
    res["configs"].append(config("configs[3] 5 M-point LiDAR pair", P, Q, T, 0.05, 0.4, [(20000, False)], 20000))
    P, Q, T = D.part_in_whole_pair(10_000_000, 100_000, delta=0.05)
    res["configs"].append(config("configs[4] 100 k query in 10 M scene", P, Q, T, 0.05, 0.2, [(5000, False)], 5000))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    from super4pcs_amd import build as B
    B.build(); B.build_icp(); B.build_normals()
    main()
