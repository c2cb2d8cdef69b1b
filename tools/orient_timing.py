#!/usr/bin/env python
"""Times consistent normal orientation (include/s4p_normals_orient.h, libsuper4pcs_normals.so) on a 1 M-point bumpy cloud and
writes profiles/orient_timing.json.  Host clock around synchronised calls, median of 10 after a warm-up, device tensors
in and out: s4p_orient_consistent_device at k = 8 (outward), beside s4p_knn_search_device at the same k on the same context
in the same run (the list search is orient's first step), and s4p_orient_towards_device.  The normals are the library's own
estimate at k = 16; every timed orient call starts from a fresh copy of them.  No target is fixed.
usage: python tools/orient_timing.py [out.json]
       python tools/orient_timing.py --quick            (3 orient calls, nothing written: for rocprofv3 --kernel-trace --stats)
       python tools/orient_timing.py --stats kernel_stats.csv [out.json]     (adds the per-kernel split of such a run to out.json)"""
import csv
import ctypes as C
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 10
N_POINTS = 1_000_000
K = 8
OUT = os.path.join(ROOT, "profiles", "orient_timing.json")


def _med(torch, f, before=None):
    ts = []
    for _ in range(REPS):
        if before:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def run(quick, out_path):
    import numpy as np
    import torch
    from super4pcs_amd import build as B, datasets as D, normals as NM
    B.build_normals()
    X = D.bumpy_pair(N_POINTS, overlap=0.5, delta=0.004, seed=20140814)[0]
    n = len(X)
    ctx = NM.Normals(0)
    Xt = torch.from_numpy(np.ascontiguousarray(X, np.float32)).cuda()
    ctx.set_cloud(Xt)
    L, h = NM.load_orient(), ctx.h
    from super4pcs_amd import knn
    knn.load_library()
    N0 = ctx.estimate(16, device_out=Xt)
    work = N0.clone()
    idx = torch.empty((n, K), dtype=torch.int32, device="cuda")
    d2 = torch.empty((n, K), dtype=torch.float32, device="cuda")
    st = NM.OrientStats()
    v = (C.c_float * 3)(0.0, 0.0, 0.0)
    torch.cuda.synchronize()
    reset = lambda: work.copy_(N0)                                                                                        # noqa: E731
    orient = lambda: ctx._chk(L.s4p_orient_consistent_device(h, K, -1.0, NM.ORIENT_OUTWARD, None, work.data_ptr(), None, None, C.byref(st)))   # noqa: E731
    lists = lambda: ctx._chk(L.s4p_knn_search_device(h, K, -1.0, 1, idx.data_ptr(), d2.data_ptr(), None))               # noqa: E731
    towards = lambda: ctx._chk(L.s4p_orient_towards_device(h, work.data_ptr(), v, None))                                # noqa: E731
    if quick:
        for _ in range(3):
            reset(); orient()
        torch.cuda.synchronize()
        print(json.dumps({"quick": True, "n": n, "stats": st.as_dict()}))
        return
    reset(); orient(); lists(); towards()                                                                               # warm-up
    row = {"label": "configs[2] P, 1 M points", "n": n, "k": K, "grid": ctx.grid(),
           "orient_ms": _med(torch, orient, reset), "lists_ms": _med(torch, lists), "towards_ms": _med(torch, towards, reset)}
    reset(); orient()
    row["stats"] = st.as_dict()
    row["orient_over_lists"] = row["orient_ms"]["median"] / row["lists_ms"]["median"]
    row["outward_share"] = float(((work.cpu().numpy().astype(np.float64) * X).sum(1) > 0).mean())
    row["outward_share_before"] = float(((N0.cpu().numpy().astype(np.float64) * X).sum(1) > 0).mean())
    hs = hashlib.sha256()
    for f in ("s4p_normals.hip", "s4p_knn.inc", "s4p_orient.inc"):
        hs.update(open(os.path.join(ROOT, "super4pcs_amd", "normals_src", f), "rb").read())
    res = {"source": "tools/orient_timing.py", "library_source_sha16": hs.hexdigest()[:16], "device": torch.cuda.get_device_name(0),
           "torch": torch.__version__, "hip": torch.version.hip,
           "method": "host perf_counter around torch.cuda.synchronize()-bracketed calls, median of %d after one warm-up; device tensors "
                     "in and out, unbounded radius, outward mode; the normals are restored from a copy before every orient call, outside "
                     "the timed window" % REPS,
           "rows": [row]}
    print(json.dumps(row), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)
    ctx.close()


def add_stats(csv_path, out_path):
    """The k_orient_* / k_knn_search rows of a rocprofv3 kernel_stats.csv (a --quick run: 3 orient calls) into out.json."""
    rows = []
    with open(csv_path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            if "k_orient_" in name or "k_knn_search" in name:
                rows.append({"kernel": name.split("(")[0].replace("void ", "").replace("s4p_nrm::", ""), "calls": int(r["Calls"]),
                             "total_us": float(r["TotalDurationNs"]) / 1e3, "average_us": float(r["AverageNs"]) / 1e3})
    rows.sort(key=lambda r: -r["total_us"])
    res = json.load(open(out_path))
    res["kernel_split"] = {"source": "rocprofv3 --kernel-trace --stats -- python tools/orient_timing.py --quick (3 orient calls, a run of its own)",
                           "orient_calls": 3, "kernels": rows, "kernel_total_us_per_call": sum(r["total_us"] for r in rows) / 3}
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["kernel_split"], indent=1))


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "--stats":
        add_stats(a[1], a[2] if len(a) > 2 else OUT)
    elif a and a[0] == "--quick":
        run(True, None)
    else:
        run(False, a[0] if a else OUT)
