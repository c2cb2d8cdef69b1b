"""Robust ICP timing and pose errors ("Robust ICP") -> profiles/icp_robust_timing.json.

    python tools/icp_robust_timing.py [--out profiles/icp_robust_timing.json] [--quick] [--kernel-stats stats.csv]

configs[2] bumpy 1 M / 1 M pair, d = 4 delta, target normals estimated within d:
  - one iteration of each metric, plain and with each loss: median of 10 refine calls of one iteration minus the same with
    zero iterations (the source ordered as refine orders it; the host solve included);
  - a whole refine (30 iterations at most, rel_tol 1e-6) per metric and loss from a 1 degree / 0.2 % start;
  - --kernel-stats: the per-kernel split of a robust iteration (search, selection, weighted sums) from the kernel_stats.csv
    of a `rocprofv3 --kernel-trace --stats` run of this tool with --quick;
  - pose errors after Super4PCS on configs[2] and on the 60 %-overlap bumpy pair of DESIGN.md section 11 (100 iterations
    there, as in that section): none vs trimmed (xi = the overlap) vs Tukey, both metrics.
--quick: the configs[2] iteration timings only (for the kernel-trace run).
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOSSES = ((None, {}), ("trimmed", {"trim_fraction": 0.5}), ("huber", {}), ("tukey", {}))


def _motion(angle_deg, shift):
    a = np.array([0.3, -0.5, 0.8]); a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(angle_deg)
    T = np.eye(4); T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K; T[:3, 3] = shift
    return T


def _errs(M, T):
    R = M[:3, :3] @ T[:3, :3].T
    return float(np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))), float(np.linalg.norm(M[:3, 3] - T[:3, 3]))


def _median(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def _name(loss):
    return loss or "none"


def iteration_times(ctx, T0, quick):
    out = {}
    for metric in ("point", "plane"):
        for loss, kw in LOSSES:
            ctx.refine(T0, max_iterations=1, metric=metric, loss=loss, **kw)
            one = _median(lambda: ctx.refine(T0, max_iterations=1, metric=metric, loss=loss, **kw), 10)
            zero = _median(lambda: ctx.refine(T0, max_iterations=0, metric=metric, loss=loss, **kw), 10)
            out["%s/%s" % (metric, _name(loss))] = {"one_iteration_s": one - zero, "refine_1_s": one, "refine_0_s": zero}
        plain = out["%s/none" % metric]["one_iteration_s"]
        for loss, _ in LOSSES[1:]:
            row = out["%s/%s" % (metric, loss)]
            row["ratio_to_plain"] = row["one_iteration_s"] / plain
    return out


def whole_refines(ctx, icp, T0, T_gt):
    out = {}
    for metric in ("point", "plane"):
        for loss, kw in LOSSES:
            t0 = time.perf_counter()
            T, r = ctx.refine(T0, max_iterations=30, rel_tol=1e-6, metric=metric, loss=loss, **kw)
            secs = time.perf_counter() - t0
            out["%s/%s" % (metric, _name(loss))] = {"seconds": secs, "iterations": r.iterations, "status": icp.STATUS_NAMES[r.status],
                                                    "rmse": r.rmse, "fitness": r.fitness, "err_before": _errs(T0, T_gt),
                                                    "err_after": _errs(T, T_gt)}
    return out


def after_registration(name, P, Q, T_gt, delta, overlap, sample, iterations):
    from super4pcs_amd import capi, icp
    d = 4 * delta
    gm = capi.Matcher(capi.make_options(delta, overlap, sample, max_time_seconds=30), device=0)
    lcp, M, Qm = gm.compute_transformation(P, Q)
    gm.close()
    M = M.astype(np.float64)
    rec = {"config": name, "sample": sample, "overlap": overlap, "max_iterations": iterations, "lcp": lcp,
           "rot_deg_trans_super4pcs": _errs(M, T_gt)}
    ctx = icp.ICP(0)
    ctx.set_target(P, d)
    ctx.set_source(Qm)
    ctx.estimate_normals(d)
    for metric in ("point", "plane"):
        for loss, kw in ((None, {}), ("trimmed", {"trim_fraction": overlap}), ("tukey", {})):
            t0 = time.perf_counter()
            dT, r = ctx.refine(np.eye(4), max_iterations=iterations, metric=metric, loss=loss, **kw)
            secs = time.perf_counter() - t0
            rec["%s/%s" % (metric, _name(loss))] = {"seconds": secs, "iterations": r.iterations, "status": icp.STATUS_NAMES[r.status],
                                                    "rmse": r.rmse, "fitness": r.fitness,
                                                    "rot_deg_trans_refined": _errs(icp.compose(dT, M), T_gt)}
    ctx.close()
    print(json.dumps(rec), flush=True)
    return rec


def kernel_split(path):
    """{kernel: (calls, average us)} of the ICP kernels in a rocprofv3 kernel_stats.csv, and the robust iteration's parts."""
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            if "s4p_icp::" not in name:
                continue
            short = name.split("s4p_icp::")[1].split("(")[0]
            rows[short] = {"calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) / 1e3}
    def avg(k):
        return rows.get(k, {}).get("average_us", 0.0)
    parts = {}
    for metric, t in (("point", "false"), ("plane", "true")):
        search = avg("k_search<%s>" % t)
        select = 4 * (avg("k_key_hist") + avg("k_key_digit"))
        sums = avg("k_wsum<%s>" % t) + avg("k_wfinal<%s>" % t)
        plain = avg("k_match<false>") + avg("k_final") if metric == "point" else avg("k_match_plane") + avg("k_final_plane")
        parts[metric] = {"search_us": search, "selection_us_4_digits": select, "weighted_sums_us": sums,
                         "robust_kernels_us": search + select + sums, "plain_kernels_us": plain,
                         "ratio": (search + select + sums) / plain if plain else None}
    return {"kernels": rows, "per_iteration": parts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_robust_timing.json"))
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    from super4pcs_amd import build as B, datasets as D, icp
    B.build_icp()
    out = {"tool": "tools/icp_robust_timing.py"}
    t0 = time.perf_counter()
    delta = 0.004
    P, Q, T_gt = D.bumpy_pair(1_000_000, overlap=0.5, delta=delta, seed=20140814)
    d = 4 * delta
    extent = float(np.linalg.norm(P.max(0) - P.min(0)))
    ctx = icp.ICP(0)
    ctx.set_target(P, d)
    ctx.set_source(Q)
    ctx.estimate_normals(d)
    T0 = _motion(1.0, 0.002 * extent) @ T_gt
    out["configs2"] = {"n_P": len(P), "n_Q": len(Q), "max_distance": d, "iteration": iteration_times(ctx, T0, a.quick)}
    print(json.dumps(out["configs2"]), flush=True)
    if not a.quick:
        out["configs2"]["whole_refine_from_1deg"] = whole_refines(ctx, icp, T0, T_gt)
    ctx.close()
    if a.kernel_stats:
        out["kernel_split_configs2"] = kernel_split(a.kernel_stats)
    if not a.quick:
        out["after_super4pcs"] = [after_registration("configs[2] bumpy 1M/1M 50 %", P, Q, T_gt, delta, 0.5, 2000, 30)]
        P6, Q6, T6 = D.bumpy_pair(1_000_000, overlap=0.6, delta=delta, seed=20140814)
        out["after_super4pcs"].append(after_registration("bumpy 1M/1M 60 % (section 11)", P6, Q6, T6, delta, 0.6, 2000, 100))
    out["wall_s"] = time.perf_counter() - t0
    if not a.quick:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print("written" if not a.quick else "quick run", a.out)


if __name__ == "__main__":
    main()
