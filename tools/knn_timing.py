#!/usr/bin/env python
"""Times the neighbour lists and the statistical outlier removal (include/s4p_knn.h, libsuper4pcs_normals.so) on the
BASELINE workloads and writes profiles/knn_timing.json.  Host clock around synchronised calls, median of 10 after a
warm-up, device tensors in and out: set_cloud, the lists at k = 16 and 32, statistical removal at k = 16 (with and without
the mean_dist output), and estimate(k) on the same context (the same walk, ending in the covariance instead of the
lists).  Also a 16-thread run of the CPU restatement (tests/normals_cpu, brute force) on a sample of queries, labelled
as such.  No target is fixed: the comparisons are lists against estimate at the same k, and the mean-only mode of the
statistical filter against the lists.
usage: python tools/knn_timing.py [out.json]"""
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

from super4pcs_amd import build as B, datasets as D, knn  # noqa: E402

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


def time_cloud(label, X):
    ctx = knn.Knn(0)
    Xt = torch.from_numpy(np.ascontiguousarray(X, np.float32)).cuda()
    n = len(X)
    ctx.set_cloud(Xt)                                             # warm-up (and code-object load)
    row = {"label": label, "n": n, "set_cloud_ms": _med(lambda: ctx.set_cloud(Xt)), "grid": ctx.grid()}
    L, h = ctx.L, ctx.h
    normals_out = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    keep = torch.empty((n,), dtype=torch.uint8, device="cuda")
    md = torch.empty((n,), dtype=torch.float64, device="cuda")
    cnt = torch.empty((n,), dtype=torch.int32, device="cuda")
    st = knn.OutlierStats()
    import ctypes as C
    for k in (16, 32):
        idx = torch.empty((n, k), dtype=torch.int32, device="cuda")
        d2 = torch.empty((n, k), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        lists = lambda: ctx._chk(L.s4p_knn_search_device(h, k, -1.0, 1, idx.data_ptr(), d2.data_ptr(), cnt.data_ptr()))      # noqa: E731
        est = lambda: ctx._chk(L.s4p_normals_estimate_device(h, k, -1.0, normals_out.data_ptr()))                          # noqa: E731
        lists(); est()
        row["k%d" % k] = {"lists_ms": _med(lists), "estimate_ms": _med(est), "list_bytes_written": n * (8 * k + 4)}
        row["k%d" % k]["lists_over_estimate"] = row["k%d" % k]["lists_ms"]["median"] / row["k%d" % k]["estimate_ms"]["median"]
        del idx, d2
    sor = lambda: ctx._chk(L.s4p_outliers_statistical_device(h, 16, 2.0, md.data_ptr(), keep.data_ptr(), C.byref(st)))      # noqa: E731
    sor_nomd = lambda: ctx._chk(L.s4p_outliers_statistical_device(h, 16, 2.0, None, keep.data_ptr(), C.byref(st)))        # noqa: E731
    sor(); sor_nomd()
    row["statistical_k16"] = {"ms": _med(sor), "ms_without_mean_dist_output": _med(sor_nomd), "stats": st.as_dict(),
                              "note": "the search in mean-only mode (8 bytes per point), two fixed-order reductions and the mask"}
    row["statistical_k16"]["over_lists_k16"] = row["statistical_k16"]["ms"]["median"] / row["k16"]["lists_ms"]["median"]
    ctx.close()
    print(json.dumps(row), flush=True)
    return row


def cpu_row(X, label, n_queries=2000):
    from tests import normals_helpers as NH
    cpu = NH.build_cpu(tempfile.mkdtemp(prefix="kcpu_"))
    rng = np.random.default_rng(0)
    Q = X[rng.choice(len(X), n_queries, replace=False)]
    t0 = time.perf_counter()
    cpu.knn(X, 17, None, queries=Q, threads=16)
    dt = time.perf_counter() - t0
    row = {"label": label, "variant": "CPU restatement, brute force (all n points per query), 16 threads, a sample of %d queries, "
           "the 17 nearest (16 without the point itself)" % n_queries, "n": len(X), "seconds": dt, "ms_per_query": dt * 1e3 / n_queries,
           "extrapolated_ms_for_all_points": dt * 1e3 / n_queries * len(X)}
    print(json.dumps(row), flush=True)
    return row


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "knn_timing.json")
    h = hashlib.sha256()
    for f in ("s4p_normals.hip", "s4p_knn.inc"):
        h.update(open(os.path.join(ROOT, "super4pcs_amd", "normals_src", f), "rb").read())
    res = {"source": "tools/knn_timing.py", "library_source_sha16": h.hexdigest()[:16],
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
           "method": "host perf_counter around torch.cuda.synchronize()-bracketed calls, median of %d after one warm-up; device "
                     "tensors in and out, unbounded radius, lists with exclude_self = 1" % REPS,
           "rows": [], "cpu": []}
    P = D.bumpy_pair(1_000_000, overlap=0.5, delta=0.004, seed=20140814)[0]
    res["rows"].append(time_cloud("configs[2] P, 1 M points", P))
    res["cpu"].append(cpu_row(P, "configs[2] P, 1 M points"))
    del P
    P = D.lidar_pair(5_000_000, delta=0.05)[0]
    res["rows"].append(time_cloud("configs[3] P, 5 M points", P))
    res["cpu"].append(cpu_row(P, "configs[3] P, 5 M points", n_queries=500))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    B.build_normals()
    main()
