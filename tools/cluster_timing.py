#!/usr/bin/env python
"""Times density clustering (include/s4p_cluster.h, libsuper4pcs_normals.so) on the BASELINE workloads and writes
profiles/cluster_timing.json.  Host clock around synchronised calls, median of 10 after a warm-up, device tensors in and
out, as tools/knn_timing.py: dbscan and density at eps = 3 x the context's reported spacing and min_points = 10, next to
set_cloud and the lists at k = 16 from the same run.  density is the grid build plus one full walk, so dbscan - density
bounds what the second walk, the union-find and the labelling add to a counting walk.  Also a 16-thread run of the CPU
restatement (tests/cluster_cpu: a plain grid DBSCAN, not a tuned baseline) on the same clouds, labelled as such.  No target
is fixed.
usage: python tools/cluster_timing.py [out.json] [--no-cpu]"""
import ctypes as C
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

from super4pcs_amd import build as B, cluster, datasets as D  # noqa: E402

REPS = 10
MIN_POINTS = 10


def _med(f):
    ts = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def time_cloud(label, X, with_cpu):
    ctx = cluster.Cluster(0)
    Xt = torch.from_numpy(np.ascontiguousarray(X, np.float32)).cuda()
    n = len(X)
    ctx.set_cloud(Xt)                                             # warm-up (and code-object load)
    row = {"label": label, "n": n, "set_cloud_ms": _med(lambda: ctx.set_cloud(Xt)), "grid": ctx.grid()}
    eps = float(np.float32(3.0 * row["grid"]["spacing"]))
    row["eps"] = eps
    row["min_points"] = MIN_POINTS
    L, h = ctx.L, ctx.h
    lab = torch.empty((n,), dtype=torch.int32, device="cuda")
    kind = torch.empty((n,), dtype=torch.uint8, device="cuda")
    cnt = torch.empty((n,), dtype=torch.int32, device="cuda")
    idx = torch.empty((n, 16), dtype=torch.int32, device="cuda")
    d2 = torch.empty((n, 16), dtype=torch.float32, device="cuda")
    st = cluster.ClusterStats()
    torch.cuda.synchronize()
    lists = lambda: ctx._chk(L.s4p_knn_search_device(h, 16, -1.0, 1, idx.data_ptr(), d2.data_ptr(), cnt.data_ptr()))            # noqa: E731
    dbscan = lambda: ctx._chk(L.s4p_cluster_dbscan_device(h, eps, MIN_POINTS, lab.data_ptr(), kind.data_ptr(), C.byref(st)))    # noqa: E731
    density = lambda: ctx._chk(L.s4p_cluster_density_device(h, eps, cnt.data_ptr()))                                            # noqa: E731
    lists(); dbscan(); density()
    row["lists_k16_ms"] = _med(lists)
    row["dbscan_ms"] = _med(dbscan)
    row["stats"] = st.as_dict()
    row["density_ms"] = _med(density)
    row["mean_density"] = float(cnt.double().mean().item())
    row["dbscan_minus_density_ms"] = row["dbscan_ms"]["median"] - row["density_ms"]["median"]
    ctx.close()
    if with_cpu:
        from tests import cluster_helpers as CH
        cpu = CH.build_cpu(tempfile.mkdtemp(prefix="ccpu_"))
        t0 = time.perf_counter()
        l, k, s = cpu.dbscan(X, eps, MIN_POINTS, threads=16)
        row["cpu"] = {"variant": "CPU restatement (tests/cluster_cpu): a plain grid DBSCAN on 16 threads, not a tuned baseline",
                      "seconds": time.perf_counter() - t0, "equal_to_device": bool(np.array_equal(l, lab.cpu().numpy()) and s == row["stats"])}
    print(json.dumps(row), flush=True)
    return row


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "cluster_timing.json")
    with_cpu = "--no-cpu" not in sys.argv
    h = hashlib.sha256()
    for f in ("s4p_normals.hip", "s4p_knn.inc", "s4p_cluster.inc"):
        h.update(open(os.path.join(ROOT, "super4pcs_amd", "normals_src", f), "rb").read())
    res = {"source": "tools/cluster_timing.py", "library_source_sha16": h.hexdigest()[:16],
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
           "method": "host perf_counter around torch.cuda.synchronize()-bracketed calls, median of %d after one warm-up; device "
                     "tensors in and out; eps = 3 x the context's spacing, min_points = %d; lists with exclude_self = 1, unbounded" % (REPS, MIN_POINTS),
           "rows": []}
    P = D.bumpy_pair(1_000_000, overlap=0.5, delta=0.004, seed=20140814)[0]
    res["rows"].append(time_cloud("configs[2] P, 1 M points", P, with_cpu))
    del P
    P = D.lidar_pair(5_000_000, delta=0.05)[0]
    res["rows"].append(time_cloud("configs[3] P, 5 M points", P, with_cpu))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    B.build_normals()
    main()
