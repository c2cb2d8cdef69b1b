#!/usr/bin/env python
"""Times normal estimation (libsuper4pcs_normals.so) on the BASELINE workloads and writes profiles/normals_timing.json.
Host clock around synchronised calls, median of 10: the grid build (set_cloud from device tensors) and the estimation
(k = 16, into a device tensor) separately.  Also a 16-thread run of the CPU restatement (tests/normals_cpu, brute force)
on a sample of queries, labelled as such.
usage: python tools/normals_timing.py [out.json]"""
import hashlib
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from super4pcs_amd import build as B, datasets as D, normals  # noqa: E402

REPS = 10
K = 16


def _med(f):
    ts = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def time_cloud(label, X, queries=None):
    ctx = normals.Normals(0)
    Xt = torch.from_numpy(np.ascontiguousarray(X, np.float32)).cuda()
    ctx.set_cloud(Xt)                                             # warm-up (and code-object load)
    g_med, g_min, g_max = _med(lambda: ctx.set_cloud(Xt))
    out = torch.empty((len(X), 3), dtype=torch.float32, device="cuda")
    fn = ctx.L.s4p_normals_estimate_device
    ctx._chk(fn(ctx.h, K, -1.0, out.data_ptr()))
    e_med, e_min, e_max = _med(lambda: ctx._chk(fn(ctx.h, K, -1.0, out.data_ptr())))
    row = {"label": label, "n": len(X), "k": K, "grid_build_ms": {"median": g_med, "min": g_min, "max": g_max},
           "estimate_ms": {"median": e_med, "min": e_min, "max": e_max}, "grid": ctx.grid(),
           "zero_normals": int((~out.cpu().numpy().any(1)).sum())}
    row["estimate_ms_per_1M_points"] = e_med / (len(X) / 1e6)
    if queries is not None:
        Qt = torch.from_numpy(np.ascontiguousarray(queries, np.float32)).cuda()
        ctx.estimate_at(Qt, K)
        q_med, q_min, q_max = _med(lambda: ctx.estimate_at(Qt, K))
        row["estimate_at"] = {"m": len(queries), "ms": {"median": q_med, "min": q_min, "max": q_max},
                              "note": "includes the queries' cell sort and the torch output allocation"}
    ctx.close()
    print(json.dumps(row), flush=True)
    return row


def cpu_row(X, label, n_queries=2000):
    from tests import normals_helpers as NH
    cpu = NH.build_cpu(tempfile.mkdtemp(prefix="ncpu_"))
    rng = np.random.default_rng(0)
    Q = X[rng.choice(len(X), n_queries, replace=False)]
    t0 = time.perf_counter()
    cpu.normals(X, K, None, queries=Q, threads=16)
    dt = time.perf_counter() - t0
    row = {"label": label, "variant": "CPU restatement, brute force (all n points per query), 16 threads, a sample of %d queries"
           % n_queries, "n": len(X), "k": K, "seconds": dt, "ms_per_query": dt * 1e3 / n_queries,
           "extrapolated_ms_for_all_points": dt * 1e3 / n_queries * len(X)}
    print(json.dumps(row), flush=True)
    return row


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "normals_timing.json")
    src = os.path.join(ROOT, "super4pcs_amd", "normals_src", "s4p_normals.hip")
    res = {"source": "tools/normals_timing.py", "library_source_sha16": hashlib.sha256(open(src, "rb").read()).hexdigest()[:16],
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
           "method": "host perf_counter around torch.cuda.synchronize()-bracketed calls, median of %d after one warm-up" % REPS,
           "rows": []}
    P, Q, _ = D.bumpy_pair(1_000_000, overlap=0.5, delta=0.004, seed=20140814)
    res["rows"].append(time_cloud("configs[2] P, 1 M points", P))
    res["cpu"] = [cpu_row(P, "configs[2] P, 1 M points")]
    del P, Q
    P, Q, _ = D.lidar_pair(5_000_000, delta=0.05)
    res["rows"].append(time_cloud("configs[3] P, 5 M points", P))
    res["rows"].append(time_cloud("configs[3] Q, 5 M points", Q))
    del P, Q
    P, Q, _ = D.part_in_whole_pair(10_000_000, 100_000, delta=0.05)
    res["rows"].append(time_cloud("configs[4] scene P, 10 M points (and the 100 k query Q at its positions)", P, queries=Q))
    res["rows"].append(time_cloud("configs[4] query Q, 100 k points", Q))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    B.build_normals()
    main()
