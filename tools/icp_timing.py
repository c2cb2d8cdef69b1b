"""ICP refinement timing and pose errors ("ICP refinement") -> profiles/icp_refine_timing.json.

    python tools/icp_timing.py [--out profiles/icp_refine_timing.json] [--quick] [--no-register]

Per configuration (BASELINE.json configs[2]-[4] clouds):
  - set-target time (upload + frame + grid) and set-source time;
  - one iteration = one correspondence/sums pass (match kernel, final sum, 17-double read-back), host clock around the
    synchronised call, median of 10 after a warm-up, with the source ordered (refine's default) and unordered;
  - a whole refine (<= 30 iterations) from a pose 1 degree / 0.2 % of the extent off;
  - the CPU restatement (tests/icp_cpu/icp_cpu.cpp, 16 threads) for one pass on the same clouds (its grid build included);
  - unless --no-register: Super4PCS on the clouds, then refinement, rotation / translation error to the generator's pose.
--quick: 1 M-point pair only (for a kernel-trace run under rocprofv3).
"""
import argparse
import json
import os
import sys
import tempfile
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


def one(name, P, Q, T_gt, delta, overlap, sample, cpu, register, max_time):
    from super4pcs_amd import capi, icp
    from tests import icp_helpers as H
    d = 4 * delta
    extent = float(np.linalg.norm(P.max(0) - P.min(0)))
    rec = {"config": name, "n_P": int(len(P)), "n_Q": int(len(Q)), "delta": delta, "max_distance": d}
    ctx = icp.ICP(0)
    ctx.set_target(P, d)                                          # warm-up (module load, first allocations)
    t0 = time.perf_counter(); ctx.set_target(P, d); rec["set_target_s"] = time.perf_counter() - t0
    t0 = time.perf_counter(); ctx.set_source(Q); rec["set_source_s"] = time.perf_counter() - t0
    T0 = _motion(1.0, 0.002 * extent) @ T_gt
    c = ctx.frame()
    Tc = H.to_centred(T0, c).astype(np.float32)
    ctx.sums(Tc)
    rec["iteration_unordered_s_median_min"] = _clock(lambda: ctx.sums(Tc), 10)
    ctx.refine(T0, max_iterations=1)                              # orders the source by the T0-image (kept for the timing below)
    t0 = time.perf_counter(); T, r = ctx.refine(T0, max_iterations=30); whole = time.perf_counter() - t0
    ctx.refine(T0, max_iterations=1, order_source=False)
    t0 = time.perf_counter(); _, r_u = ctx.refine(T0, max_iterations=30, order_source=False); whole_u = time.perf_counter() - t0
    rec["refine_from_1deg"] = {"iterations": r.iterations, "status": icp.STATUS_NAMES[r.status], "rmse": r.rmse, "fitness": r.fitness,
                               "seconds_ordered": whole, "seconds_unordered": whole_u,
                               "per_iteration_ordered_s": whole / (r.iterations + 1), "per_iteration_unordered_s": whole_u / (r_u.iterations + 1),
                               "err_before": _errs(T0, T_gt), "err_after": _errs(T, T_gt)}
    rec["upload_grid_plus_refine_s"] = rec["set_target_s"] + rec["set_source_s"] + whole
    if cpu is not None:
        Pc, Qc = (P - c).astype(np.float32), (Q - c).astype(np.float32)
        cpu.pass_(Pc, Qc, Tc, d, want_idx=False, threads=16)
        rec["cpu_restatement_16t_pass_s_median_min"] = _clock(lambda: cpu.pass_(Pc, Qc, Tc, d, want_idx=False, threads=16), 3)
        rec["gpu_iteration_speedup_vs_cpu16"] = rec["cpu_restatement_16t_pass_s_median_min"][0] / rec["refine_from_1deg"]["per_iteration_ordered_s"]
    ctx.close()
    if register:
        gm = capi.Matcher(capi.make_options(delta, overlap, sample, max_time_seconds=max_time), device=0)
        t0 = time.perf_counter(); lcp, M, Qm = gm.compute_transformation(P, Q); reg_s = time.perf_counter() - t0
        gm.close()
        M = M.astype(np.float64)
        t0 = time.perf_counter(); dT, rr = icp.refine(P, Qm, np.eye(4), max_distance=d); ref_s = time.perf_counter() - t0
        Mr = icp.compose(dT, M)
        rec["after_super4pcs"] = {"sample": sample, "overlap": overlap, "max_time_seconds": max_time, "lcp": lcp, "register_s": reg_s,
                                  "refine_s": ref_s, "iterations": rr.iterations, "status": icp.STATUS_NAMES[rr.status],
                                  "rmse": rr.rmse, "fitness": rr.fitness,
                                  "rot_deg_trans_super4pcs": _errs(M, T_gt), "rot_deg_trans_refined": _errs(Mr, T_gt)}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_refine_timing.json"))
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--no-register", action="store_true")
    a = ap.parse_args()
    from super4pcs_amd import build as B, datasets as D
    from tests import icp_helpers as H
    B.build_icp()
    cpu = H.build_cpu(tempfile.mkdtemp())
    out = {"tool": "tools/icp_timing.py", "source_sha16": B.source_digest(), "rows": []}
    t0 = time.perf_counter()
    P, Q, T = D.bumpy_pair(1_000_000, overlap=0.5, delta=0.004, seed=20140814)
    out["rows"].append(one("configs[2] bumpy 1M/1M", P, Q, T, 0.004, 0.5, 2000, cpu, not a.no_register, 30))
    if not a.quick:
        P, Q, T = D.lidar_pair(5_000_000, delta=0.05)
        out["rows"].append(one("configs[3] lidar 5M/5M", P, Q, T, 0.05, 0.4, 2000, cpu, not a.no_register, 40))
        P, Q, T = D.part_in_whole_pair(10_000_000, 100_000, delta=0.05)
        out["rows"].append(one("configs[4] part-in-whole 10M scene / 100k query", P, Q, T, 0.05, 0.2, 1000, cpu, not a.no_register, 40))
        # 10 M source points: the scene against itself, moved
        Qs = (P.astype(np.float64) @ _motion(1.0, 0.0)[:3, :3].T).astype(np.float32)
        out["rows"].append(one("configs[4] scene 10M/10M (self, 1 degree)", P, Qs, np.linalg.inv(_motion(1.0, 0.0)), 0.05, 0.2, 0, cpu,
                               False, 0))
    out["wall_s"] = time.perf_counter() - t0
    if not a.quick:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print("written" if not a.quick else "quick run", a.out)


if __name__ == "__main__":
    main()
