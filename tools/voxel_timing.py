#!/usr/bin/env python
"""Times the voxel-grid downsample (include/s4p_voxel.h, libsuper4pcs_normals.so) and multi-scale ICP
(super4pcs_amd/multiscale.py) on the BASELINE workloads and writes profiles/voxel_timing.json.  Host clock around
synchronised calls, median of 10 after a warm-up, device tensors in and out.  No target is fixed in advance.
  - downsample of configs[2] P (1 M) and configs[3] P (5 M) at voxel sizes that keep about 1/4 and 1/16 of the points (found
    by bisection on the device), without attributes and with 3 channels;
  - every point of the 5 M cloud in one voxel (the long-run path);
  - refine_multiscale with three levels ending at full resolution against the single-level 30-iteration refine of DESIGN.md
    section 11, on the same pairs from the same start (1 degree / 0.2 % of the extent off), times and pose errors side by side.
usage: python tools/voxel_timing.py [out.json]"""
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from super4pcs_amd import build as B, datasets as D, icp, multiscale, voxel  # noqa: E402

REPS = 10


def _med(f):
    ts = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def _motion(angle_deg, shift):
    a = np.array([0.3, -0.5, 0.8]); a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(angle_deg)
    T = np.eye(4); T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K; T[:3, 3] = shift
    return T


def _errs(M, T):
    R = M[:3, :3] @ T[:3, :3].T
    return [float(np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))), float(np.linalg.norm(M[:3, 3] - T[:3, 3]))]


def _size_for(ctx, Xt, fraction):
    """The voxel size at which about `fraction` of the points remain (geometric bisection, 14 steps)."""
    ext = float((Xt.max(0).values - Xt.min(0).values).max())
    lo, hi = ext * 2.0 ** -19, ext
    for _ in range(14):
        mid = float(np.sqrt(lo * hi))
        m = len(ctx.downsample(Xt, mid)[0])
        if m > fraction * len(Xt):
            lo = mid
        else:
            hi = mid
    return float(np.sqrt(lo * hi))


def time_downsample(label, X, one_voxel=False):
    ctx = voxel.VoxelGrid(0)
    Xt = torch.from_numpy(np.ascontiguousarray(X, np.float32)).cuda()
    At = torch.rand((len(X), 3), dtype=torch.float32, device="cuda")
    ctx.downsample(Xt, float((Xt.max(0).values - Xt.min(0).values).max()) / 100)          # warm-up (code-object load, arena)
    row = {"label": label, "n": len(X), "sizes": []}
    sizes = [("about 1/4", _size_for(ctx, Xt, 0.25), Xt), ("about 1/16", _size_for(ctx, Xt, 1.0 / 16), Xt)]
    if one_voxel:                                                 # shifted into the positive octant, one voxel around it all
        Xs = (Xt - Xt.min(0).values + 1.0).contiguous()
        sizes.append(("every point in one voxel (cloud shifted into the positive octant)", 2.0 * float(Xs.max()), Xs))
    for what, v, Xt in sizes:
        ctx.downsample(Xt, v, At)
        out = ctx.downsample(Xt, v)
        rec = {"what": what, "voxel": v, "m": len(out[0]), "largest_voxel": int(out[2].max()), "mean_members": len(X) / max(len(out[0]), 1),
               "ms": _med(lambda: ctx.downsample(Xt, v)), "ms_with_3_channels": _med(lambda: ctx.downsample(Xt, v, At))}
        row["sizes"].append(rec)
    ctx.close()
    print(json.dumps(row), flush=True)
    return row


def time_refine(label, P, Q, T_gt, delta, voxels):
    d = 4 * delta
    extent = float(np.linalg.norm(P.max(0) - P.min(0)))
    T0 = _motion(1.0, 0.002 * extent) @ T_gt
    Pt, Qt = torch.from_numpy(P).cuda(), torch.from_numpy(Q).cuda()
    rec = {"label": label, "n_P": len(P), "n_Q": len(Q), "max_distance": d, "voxel_sizes": list(voxels), "start_err_deg_trans": _errs(T0, T_gt)}
    # DESIGN.md section 11's figure: the refine call alone on a context that holds the clouds, source ordered
    ctx = icp.ICP(0)
    ctx.set_target(Pt, d); ctx.set_source(Qt)
    ctx.refine(T0, max_iterations=1)
    Ts, rs = ctx.refine(T0, max_iterations=30)
    rec["single_level"] = {"refine_call_ms": _med(lambda: ctx.refine(T0, max_iterations=30)), "iterations": rs.iterations,
                           "status": icp.STATUS_NAMES[rs.status], "rmse": rs.rmse, "err_deg_trans": _errs(Ts, T_gt)}
    ctx.close()
    one_shot = lambda: icp.refine(Pt, Qt, T0=T0, max_distance=d, max_iterations=30)                                       # noqa: E731
    one_shot()
    rec["single_level"]["one_shot_ms"] = _med(one_shot)
    multi = lambda: multiscale.refine_multiscale(Pt, Qt, T0=T0, voxel_sizes=voxels, max_distance=d, max_iterations=30)   # noqa: E731
    Tm, levels = multi()
    plan = multiscale.level_plan(voxels, max_distance=d)
    rec["multi_scale"] = {"one_shot_ms": _med(multi), "err_deg_trans": _errs(Tm, T_gt),
                          "levels": [{"voxel": v, "max_distance": dl, "iterations": r.iterations, "status": icp.STATUS_NAMES[r.status],
                                      "n_corr": r.n_corr, "rmse": r.rmse} for (v, dl, _), r in zip(plan, levels)]}
    down = lambda: [voxel.voxel_downsample(X, v) for v in voxels if v > 0 for X in (Pt, Qt)]                              # noqa: E731
    down()
    rec["multi_scale"]["of_which_downsampling_ms"] = _med(down)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "voxel_timing.json")
    h = hashlib.sha256()
    for f in ("s4p_normals.hip", "s4p_knn.inc", "s4p_voxel.inc"):
        h.update(open(os.path.join(ROOT, "super4pcs_amd", "normals_src", f), "rb").read())
    res = {"source": "tools/voxel_timing.py", "library_source_sha16": h.hexdigest()[:16],
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
           "method": "host perf_counter around torch.cuda.synchronize()-bracketed calls, median of %d after one warm-up; device "
                     "tensors in and out; one_shot rows include context creation, upload, grid and, for multi-scale, the "
                     "downsampling of both clouds at every level" % REPS,
           "downsample": [], "refine": []}
    P, Q, T = D.bumpy_pair(1_000_000, overlap=0.5, delta=0.004, seed=20140814)
    res["downsample"].append(time_downsample("configs[2] P, 1 M points", P))
    res["refine"].append(time_refine("configs[2] bumpy 1 M / 1 M", P, Q, T, 0.004, (0.016, 0.005, 0.0)))
    del P, Q
    P, Q, T = D.lidar_pair(5_000_000, delta=0.05)
    res["downsample"].append(time_downsample("configs[3] P, 5 M points", P, one_voxel=True))
    res["refine"].append(time_refine("configs[3] lidar 5 M / 5 M", P, Q, T, 0.05, (0.4, 0.15, 0.0)))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    B.build_normals()
    B.build_icp()
    main()
