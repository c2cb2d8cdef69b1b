#!/usr/bin/env python
"""Times the descriptors and the matcher (include/s4p_feature.h, libsuper4pcs_normals.so) and writes
profiles/feature_timing.json.  Host clock around synchronised calls, median of 10 after a warm-up with min and max, device
tensors in and out, as tools/shape_timing.py: Features.fpfh on configs[2] P (1 M points) at the two radii of section 34's table
(about 150 and 600 neighbours) with radial normals, and Features.match on random tables of 20 000 x 20 000 and
100 000 x 100 000 rows, mutual.  Beside each the 16-thread run of the CPU restatement (tests/feature_cpu: a plain grid and a
brute-force matcher, not tuned baselines), labelled as such, and whether it equals the device's result.
    python tools/feature_timing.py [out.json] [--no-cpu] [--lib PATH]      --lib: another build of the library (the same sources
                                                                           with -DS4P_FEATURE_COUNT_BITS=16) in the package's place
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/feature_timing.py --quick     (2 fpfh calls and 2 match calls, nothing written)
    python tools/feature_timing.py --stats DIR/.../*_kernel_stats.csv [out.json]          (merges the kernel rows)
No target is fixed: the parent of this feature has no such call."""
import csv
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

from super4pcs_amd import build as B, datasets as D, features  # noqa: E402

LIB = None                                      # --lib: the path every context of this run binds (Features(0, lib=LIB))
if "--lib" in sys.argv:
    LIB = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
    del sys.argv[sys.argv.index("--lib"):sys.argv.index("--lib") + 2]

REPS = 10
OUT = os.path.join(ROOT, "profiles", "feature_timing.json")
RADII = (0.0055079106241464615, 0.011046895757317543)        # profiles/shape_timing.json, configs[2] P: 150 and 601 neighbours
MATCH_SIZES = (20_000, 100_000)
QUICK_CALLS = 2


def _med(f, reps=REPS):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def cloud():
    X = D.bumpy_pair(1_000_000, overlap=0.5, delta=0.004, seed=20140814)[0]
    v = X.astype(np.float64) - X.astype(np.float64).mean(0)
    return X, (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def tables(rows):
    rng = np.random.default_rng(rows)
    fa = rng.integers(0, 4097, size=(rows, 33)).astype(np.uint16)
    fb = rng.integers(0, 4097, size=(rows, 33)).astype(np.uint16)
    fb[rng.permutation(rows)[:rows // 4]] = fa[rng.permutation(rows)[:rows // 4]]
    return fa, fb


def _cpu():
    from tests import feature_helpers as FH
    return FH, FH.build_cpu(tempfile.mkdtemp(prefix="fcpu_"))


def time_fpfh(with_cpu):
    X, N = cloud()
    ctx = features.Features(0, lib=LIB)
    ctx.set_cloud(torch.from_numpy(X).cuda())
    Nt = torch.from_numpy(N).cuda()
    rows = []
    for r in RADII:
        F, cnt = ctx.fpfh(Nt, r)                                   # warm-up, and the result that is recorded
        ms = _med(lambda: ctx.fpfh(Nt, r))
        pairs = int(cnt.sum(dtype=torch.int64))
        e = {"label": "configs[2] P, 1 M points", "n": len(X), "radius": r, "median_pairs": float(cnt.float().median()), "max_pairs": int(cnt.max()),
             "rows_of_zeros": int((~(F.view(torch.int16) != 0).any(1)).sum()), "fpfh_ms": ms, "accepted_pairs": pairs, "pairs_per_second": pairs / (ms["median"] * 1e-3)}
        if with_cpu:
            FH, cpu = _cpu()
            t0 = time.perf_counter()
            want = cpu.fpfh(X, N, r, threads=16)
            e["cpu"] = {"variant": "CPU restatement (tests/feature_cpu): a plain grid of edge 1.001 r on 16 threads, not a tuned baseline",
                        "seconds": time.perf_counter() - t0, "equal_to_device": bool(FH.same((F, cnt), want))}
        rows.append(e)
        print(json.dumps(e), flush=True)
    ctx.close()
    return rows


def time_match(with_cpu):
    ctx = features.Features(0, lib=LIB)
    rows = []
    for m in MATCH_SIZES:
        fa, fb = tables(m)
        ta, tb = torch.from_numpy(fa).cuda(), torch.from_numpy(fb).cuda()
        idx, dist = ctx.match(ta, tb, True)
        ms = _med(lambda: ctx.match(ta, tb, True))
        e = {"rows": m, "columns": m, "mutual": True, "matched": int((idx >= 0).sum()), "match_ms": ms,
             "pairs_per_second": 2.0 * m * m / (ms["median"] * 1e-3)}          # mutual: both directions are computed
        if with_cpu:
            FH, cpu = _cpu()
            t0 = time.perf_counter()
            want = cpu.match(fa, fb, True, threads=16)
            e["cpu"] = {"variant": "CPU restatement (tests/feature_cpu): brute force on 16 threads, not a tuned baseline",
                        "seconds": time.perf_counter() - t0,
                        "equal_to_device": bool(np.array_equal(idx.cpu().numpy(), want[0]) and np.array_equal(dist.cpu().numpy(), want[1]))}
        rows.append(e)
        print(json.dumps(e), flush=True)
    ctx.close()
    return rows


def _digest():
    h = hashlib.sha256()
    for f in ("s4p_normals.hip", "s4p_cluster.inc", "s4p_shape.inc", "s4p_feature.inc"):
        h.update(open(os.path.join(ROOT, "super4pcs_amd", "normals_src", f), "rb").read())
    return h.hexdigest()[:16]


def run(out_path, with_cpu):
    prop = torch.cuda.get_device_properties(0)
    res = {"source": "tools/feature_timing.py", "library": LIB or "the package's", "library_source_sha16": _digest(), "device": torch.cuda.get_device_name(0),
           "compute_units": prop.multi_processor_count, "torch": torch.__version__, "hip": torch.version.hip,
           "method": "host perf_counter around torch.cuda.synchronize()-bracketed calls, median of %d after one warm-up; device tensors in "
                     "and out; radial normals; random descriptor tables, a quarter of the rows shared" % REPS,
           "fpfh": time_fpfh(with_cpu), "match": time_match(with_cpu)}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


def quick():
    X, N = cloud()
    ctx = features.Features(0, lib=LIB)
    ctx.set_cloud(torch.from_numpy(X).cuda())
    Nt = torch.from_numpy(N).cuda()
    fa, fb = tables(MATCH_SIZES[0])
    ta, tb = torch.from_numpy(fa).cuda(), torch.from_numpy(fb).cuda()
    for _ in range(QUICK_CALLS):
        ctx.fpfh(Nt, RADII[1])
        ctx.match(ta, tb, True)
    ctx.close()


def add_stats(csv_path, out_path):
    """The rows of a rocprofv3 kernel_stats.csv (a --quick run) into out.json."""
    rows = []
    with open(csv_path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            rows.append({"kernel": name.split("(")[0].replace("void ", "").replace("s4p_nrm::", "")[:80], "calls": int(r["Calls"]),
                         "total_us": float(r["TotalDurationNs"]) / 1e3, "average_us": float(r["AverageNs"]) / 1e3})
    rows.sort(key=lambda r: -r["total_us"])
    res = json.load(open(out_path))
    res["kernel_split"] = {"source": "rocprofv3 --kernel-trace --stats -- python tools/feature_timing.py --quick (%d fpfh calls on configs[2] P at "
                                     "the larger radius and %d mutual match calls at %d x %d; a run of its own)"
                                     % (QUICK_CALLS, QUICK_CALLS, MATCH_SIZES[0], MATCH_SIZES[0]), "kernels": rows[:16]}
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["kernel_split"], indent=1))


if __name__ == "__main__":
    a = [x for x in sys.argv[1:] if x != "--no-cpu"]
    if LIB is None:
        B.build_normals()
    if a and a[0] == "--stats":
        add_stats(a[1], a[2] if len(a) > 2 else OUT)
    elif a and a[0] == "--quick":
        quick()
    else:
        run(a[0] if a else OUT, "--no-cpu" not in sys.argv)
