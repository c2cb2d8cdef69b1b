#!/usr/bin/env python
"""What radius normals of the source do to the metrics that read them (DESIGN.md sections 23 and 34) ->
profiles/shape_registration.json.  configs[2] (bumpy 1 M / 1 M, sigma = delta = 0.004 on the source), the rows "5 degrees" and
"after Super4PCS at sample 2000" of tools/icp_symm_timing.py's whole refines (rel_tol 1e-6, at most 30 iterations, d = 4 delta,
target normals estimated within d), once with the source's normals from 16 neighbours as there and once from every point
within 0.02 (super4pcs_amd.shape): the rotation and translation distance of the fixed point to the generator's pose and the
iteration count, for plane (which does not read the source's normals), gicp and symmetric.  A record, not a test.
    python tools/shape_registration.py [out.json] [--no-register]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import icp_symm_timing as IS  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "shape_registration.json")
RADIUS = 0.02
START_DEG = 5.0


def main():
    a = [x for x in sys.argv[1:] if not x.startswith("--")]
    from super4pcs_amd import build as B, capi, datasets as D, icp, normals, shape
    B.build_icp()
    B.build_normals()
    delta, overlap, sample = 0.004, 0.5, 2000
    d = 4 * delta
    P, Q, T_gt = D.bumpy_pair(1_000_000, overlap=overlap, delta=delta, seed=20140814)
    extent = float(np.linalg.norm(P.max(0) - P.min(0)))

    def source_normals(Z):
        t0 = time.perf_counter()
        N16 = normals.estimate_normals(Z, k=16)
        t1 = time.perf_counter()
        Nr, _, cnt = shape.estimate_normals_radius(Z, RADIUS)
        t2 = time.perf_counter()
        return {"k = 16": N16, "radius %g" % RADIUS: Nr}, {"k16_seconds_incl_upload": t1 - t0, "radius_seconds_incl_upload": t2 - t1,
                                                          "median_neighbours": float(np.median(cnt)), "without_a_normal": int((~Nr.any(1)).sum())}
    out = {"tool": "tools/shape_registration.py", "config": "configs[2] bumpy 1M/1M", "delta": delta, "max_distance": d, "radius": RADIUS,
           "start_degrees": START_DEG, "from_start": {}, "after_super4pcs": {}}
    kinds, out["source_normals"] = source_normals(Q)
    T0 = IS._motion(START_DEG, 0.002 * extent) @ T_gt
    for kind, Nq in kinds.items():
        ctx = IS.LibCtx(icp.LIB_PATH, P, Q, Nq, d)
        out["from_start"][kind] = IS._whole(ctx, icp, T0, T_gt)
        ctx.close()
        print(kind, json.dumps(out["from_start"][kind]), flush=True)
    if "--no-register" not in sys.argv:
        gm = capi.Matcher(capi.make_options(delta, overlap, sample, max_time_seconds=30), device=0)
        lcp, M, Qm = gm.compute_transformation(P, Q)
        gm.close()
        M = M.astype(np.float64)
        out["after_super4pcs"] = {"sample": sample, "lcp": lcp, "rot_deg_trans_super4pcs": IS._errs(M, T_gt)}
        kinds_m, _ = source_normals(Qm)
        for kind, Nq in kinds_m.items():
            rec = {}
            for metric in IS.METRICS:
                dT, rr = icp.refine(P, Qm, np.eye(4), max_distance=d, metric=metric, source_normals=Nq)
                rec[metric] = {"iterations": rr.iterations, "status": icp.STATUS_NAMES[rr.status], "rmse": rr.rmse, "fitness": rr.fitness,
                               "rot_deg_trans_refined": IS._errs(icp.compose(dT, M), T_gt)}
            out["after_super4pcs"][kind] = rec
            print(kind, json.dumps(rec), flush=True)
    path = a[0] if a else OUT
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
