"""Batched multi-start ICP against a loop of single refines ("Batched multi-start ICP") -> profiles/icp_batch_timing.json.

    python tools/icp_batch_timing.py [--out profiles/icp_batch_timing.json] [--quick]

Per pair, metric (point, plane) and B in {1, 4, 16, 64}, in one process and on one context: B starts within a degree or so of
the generator's pose, refined for exactly ITERATIONS iterations (rel_tol = 0, so every pose of both paths runs ITERATIONS + 1
passes) by ICP.refine_batch and by a loop of B ICP.refine calls, the two interleaved REPS times after a warm-up of each.
Host clock around the synchronised calls.  The loop of single calls is the baseline: the code path as it was before the
batch existed.  Recorded: the whole-call seconds of every repeat, their medians, the time per pass and pose, the ratio
loop / batch, and for B = 1 whether the batch's median lies inside the range of the loop's repeats.
Pairs: the configs[4] pair (10 M scene, 100 k query), the 1 M bumpy pair, and the bumpy pair voxel-downsampled to about 50 k.
--quick: the downsampled bumpy pair only, B in {1, 4, 16}, under a minute; writes nothing unless --out is given.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ITERATIONS = 10
REPS = 5


def _motion(angle_deg, shift):
    a = np.array([0.3, -0.5, 0.8]); a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(angle_deg)
    T = np.eye(4); T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K; T[:3, 3] = shift
    return T


def starts(T_gt, centre, extent, B):
    """B poses 0.2 to 1.2 degrees (about the source's centre) and up to 0.1 % of the extent off T_gt, all different."""
    S = np.eye(4); S[:3, 3] = centre
    Si = np.eye(4); Si[:3, 3] = -centre
    return np.stack([T_gt @ S @ _motion(0.2 + 1.0 * b / max(B - 1, 1), 0.001 * extent * ((b % 7) - 3) / 3.0) @ Si for b in range(B)])


def downsample_to(P, Q, target):
    """Both clouds at one voxel size chosen so that the source has about `target` points (two corrections of the edge)."""
    from super4pcs_amd import voxel
    v = float(np.linalg.norm(Q.max(0) - Q.min(0))) / 300.0
    for _ in range(3):
        Ql = voxel.voxel_downsample(Q, v)[0]
        if abs(len(Ql) - target) <= 0.1 * target:
            break
        v *= float(np.sqrt(len(Ql) / float(target)))           # a surface: the count goes with 1 / v^2
    return voxel.voxel_downsample(P, v)[0], Ql, v


def one(name, P, Q, T_gt, d, batches, reps):
    from super4pcs_amd import icp
    ctx = icp.ICP(0)
    ctx.set_target(P, d)
    ctx.set_source(Q)
    ctx.estimate_normals(d)
    centre = Q.astype(np.float64).mean(0)
    extent = float(np.linalg.norm(P.max(0) - P.min(0)))
    rows = []
    for metric in ("point", "plane"):
        for B in batches:
            T0s = starts(T_gt, centre, extent, B)
            kw = dict(max_iterations=ITERATIONS, rel_tol=0.0, metric=metric)

            def batch():
                return ctx.refine_batch(T0s, **kw)

            def loop():
                return [ctx.refine(T0, **kw) for T0 in T0s]

            _, res, _ = batch()                                   # warm-up of both, and the passes each pose ran
            single = loop()
            passes = sum(r.iterations + 1 for r in res)
            assert passes == sum(r.iterations + 1 for _, r in single)
            tb, tl = [], []
            for _ in range(reps):
                t0 = time.perf_counter(); batch(); tb.append(time.perf_counter() - t0)
                t0 = time.perf_counter(); loop(); tl.append(time.perf_counter() - t0)
            mb, ml = float(np.median(tb)), float(np.median(tl))
            row = {"pair": name, "n_P": int(len(P)), "n_Q": int(len(Q)), "max_distance": d, "metric": metric, "B": B,
                   "iterations": ITERATIONS, "passes_all_poses": passes, "batch_s": tb, "loop_s": tl, "batch_s_median": mb,
                   "loop_s_median": ml, "batch_ms_per_pass_per_pose": 1e3 * mb / passes, "loop_ms_per_pass_per_pose": 1e3 * ml / passes,
                   "loop_over_batch": ml / mb, "loop_s_range": [min(tl), max(tl)],
                   "batch_median_inside_loop_range": bool(min(tl) <= mb <= max(tl)), "batch_median_below_loop_max": bool(mb <= max(tl)),
                   "n_corr_first_pose": int(res[0].n_corr)}
            print(json.dumps(row), flush=True)
            rows.append(row)
    ctx.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    out_path = a.out or (None if a.quick else os.path.join(ROOT, "profiles", "icp_batch_timing.json"))
    from super4pcs_amd import build as B, datasets as D
    B.build_icp()
    out = {"tool": "tools/icp_batch_timing.py", "quick": bool(a.quick), "iterations": ITERATIONS, "rows": []}
    t0 = time.perf_counter()
    batches = (1, 4, 16) if a.quick else (1, 4, 16, 64)
    reps = 3 if a.quick else REPS
    P, Q, T = D.bumpy_pair(1_000_000, overlap=0.5, delta=0.004, seed=20140814)
    Pl, Ql, v = downsample_to(P, Q, 50_000)
    out["bumpy_voxel_size"] = v
    out["rows"] += one("bumpy 1M/1M voxel-downsampled", Pl, Ql, T, max(4 * 0.004, 3 * v), batches, reps)      # the multi-scale level distance
    if not a.quick:
        out["rows"] += one("configs[2] bumpy 1M/1M", P, Q, T, 4 * 0.004, batches, reps)
        P, Q, T = D.part_in_whole_pair(10_000_000, 100_000, delta=0.05)
        out["rows"] += one("configs[4] part-in-whole 10M scene / 100k query", P, Q, T, 4 * 0.05, batches, reps)
    out["wall_s"] = time.perf_counter() - t0
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
    print("written %s" % out_path if out_path else "quick run, nothing written")


if __name__ == "__main__":
    main()
