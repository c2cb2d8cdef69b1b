#!/usr/bin/env python
"""Times radius normals (include/s4p_shape.h, libsuper4pcs_normals.so) on the BASELINE workloads and writes
profiles/shape_timing.json.  Host clock around synchronised calls, median of 10 after a warm-up, device tensors in and out, as
tools/plane_timing.py: Shape.estimate on the configs[2] and configs[3] clouds at two radii each, found by bisection on the
median neighbour count (about 150 and about 600), next to set_cloud, the k = 32 estimate_normals of the same cloud and a
16-thread run of the CPU restatement (tests/shape_cpu: a plain grid, not a tuned baseline), labelled as such.  The distance
tests of a call are counted on the host from the cell occupancy of a grid of the kernel's edge; the accepted neighbours are the
sum of the counts the call returns.
    python tools/shape_timing.py [out.json] [--no-cpu]
    python tools/shape_timing.py --variants DIR [out.json]     other builds of the library (DIR/libshape_<name>.so, the same
                                                               sources with -DS4P_SHAPE_RINGS=1 or 2, or with
                                                               profiles/shape_acc_double.patch), timed in alternation with
                                                               the package's library in one process and compared with it bit
                                                               for bit; merged into out.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/shape_timing.py --quick     (3 calls on configs[2] P, nothing written)
    python tools/shape_timing.py --stats DIR/.../*_kernel_stats.csv [out.json]          (merges the kernel rows)
No target is fixed: the parent of this feature has no such call."""
import csv
import glob
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

from super4pcs_amd import build as B, datasets as D, normals, shape  # noqa: E402

REPS = 10
OUT = os.path.join(ROOT, "profiles", "shape_timing.json")
TARGETS = (150, 600)                 # median neighbours
QUICK_CALLS = 3
EDGE_MARGIN = 1.0 + 2.0 ** -16       # the kernel's cell edge is r (1 + 2^-16) / rings


def _med(f, reps=REPS):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def clouds():
    yield "configs[2] P, 1 M points", D.bumpy_pair(1_000_000, overlap=0.5, delta=0.004, seed=20140814)[0], 0.006
    yield "configs[3] P, 5 M points", D.lidar_pair(5_000_000, delta=0.05)[0], 0.15


def radius_for(ctx, target, start):
    """A radius whose median neighbour count is within 3 % of the target: the counts of one point in 64 at each step."""
    q = ctx._like[::64].contiguous()
    r = start
    for _ in range(8):
        med = float(ctx.estimate(r, queries=q)[2].float().median())
        if abs(med / target - 1) < 0.03:
            break
        r *= (target / max(med, 1.0)) ** 0.5
    return float(np.float32(r)), med


def distance_tests(X, radius, rings):
    """How many d2 the walk computes: for every point, the points in the (2 rings + 1)^3 cells around its cell, on the grid
    the kernel uses when nothing enlarges it (edge r (1 + 2^-16) / rings over the cloud's bounds); None when that grid
    passes the cell cap."""
    h = float(np.float32(radius)) * EDGE_MARGIN / rings
    lo = X.min(0).astype(np.float64)
    c = np.floor((X.astype(np.float64) - lo) / h).astype(np.int64)
    dim = c.max(0) + 1
    if float(dim[0]) * float(dim[1]) * float(dim[2]) > min(1 << 28, max(1 << 20, 4 * len(X))):
        return None
    code = (c[:, 2] * dim[1] + c[:, 1]) * dim[0] + c[:, 0]
    cells, occ = np.unique(code, return_counts=True)
    cz, rem = np.divmod(cells, dim[0] * dim[1])
    cy, cx = np.divmod(rem, dim[0])
    total = 0
    span = range(-rings, rings + 1)
    for dz in span:
        for dy in span:
            for dx in span:
                x, y, z = cx + dx, cy + dy, cz + dz
                ok = (x >= 0) & (x < dim[0]) & (y >= 0) & (y < dim[1]) & (z >= 0) & (z < dim[2])
                want = (z[ok] * dim[1] + y[ok]) * dim[0] + x[ok]
                at = np.searchsorted(cells, want)
                hit = (at < len(cells)) & (cells[np.minimum(at, len(cells) - 1)] == want)
                total += int((occ[ok][hit] * occ[at[hit]]).sum())
    return total


# ---- other builds of the library: shape.Shape(0, lib=path), next to the package's in one process ----------------------------------

def _equal(a, b):
    return bool(torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and
                torch.equal(a[2], b[2]))


def time_variants(label, Xt, radii, libs):
    """Every build on every radius: REPS rounds, the builds in turn within a round."""
    rows = []
    for lib in libs.values():
        lib.set_cloud(Xt)
    for r in radii:
        ref = None
        times = {name: [] for name in libs}
        same = {}
        for name, lib in libs.items():                     # warm-up, and the bits
            got = lib.estimate(r)
            ref = got if ref is None else ref
            same[name] = _equal(got, ref)
        for _ in range(REPS):
            for name, lib in libs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                lib.estimate(r)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
        rows.append({"label": label, "radius": r,
                     "builds": {name: {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "bits_equal_to_first": same[name]}
                                for name, t in times.items()}})
        print(json.dumps(rows[-1]), flush=True)
    return rows


# ---- the package's library --------------------------------------------------------------------------------------------------------

def time_cloud(label, X, start, with_cpu):
    ctx = shape.Shape(0)
    Xt = torch.from_numpy(np.ascontiguousarray(X, np.float32)).cuda()
    ctx.set_cloud(Xt)
    row = {"label": label, "n": len(X), "set_cloud_ms": _med(lambda: ctx.set_cloud(Xt)),
           "knn_normals_k32_ms": _med(lambda: normals.Normals.estimate(ctx, 32, None, device_out=Xt)), "estimate": []}
    for target in TARGETS:
        r, _ = radius_for(ctx, target, start * (target / TARGETS[0]) ** 0.5)
        N, E, cnt = ctx.estimate(r)                                  # warm-up, and the result that is recorded
        accepted = int(cnt.sum(dtype=torch.int64))
        tests, rings = distance_tests(X, r, 2), 2              # the library's rule: the finer grid when it fits as it is
        if tests is None:
            tests, rings = distance_tests(X, r, 1), 1
        ms = _med(lambda: ctx.estimate(r))
        e = {"target": target, "radius": r, "rings": rings, "median_neighbours": float(cnt.float().median()), "max_neighbours": int(cnt.max()),
             "without_a_normal": int((~N.any(1)).sum()), "estimate_ms": ms, "distance_tests": tests, "accepted_neighbours": accepted,
             "tests_per_accepted": tests / accepted if tests else None, "tests_per_second": tests / (ms["median"] * 1e-3) if tests else None,
             "accepted_per_second": accepted / (ms["median"] * 1e-3)}
        if with_cpu:
            from tests import shape_helpers as SH
            cpu = SH.build_cpu(tempfile.mkdtemp(prefix="scpu_"))
            t0 = time.perf_counter()
            want = cpu.estimate(X, r, threads=16)
            e["cpu"] = {"variant": "CPU restatement (tests/shape_cpu): a plain grid of edge 1.001 r on 16 threads, not a tuned baseline",
                        "seconds": time.perf_counter() - t0, "equal_to_device": bool(SH.same((N, E, cnt), want)), "largest_u": cpu.umax}
        row["estimate"].append(e)
        print(json.dumps(e), flush=True)
    ctx.close()
    return row, Xt


def _digest():
    h = hashlib.sha256()
    for f in ("s4p_normals.hip", "s4p_cluster.inc", "s4p_shape.inc"):
        h.update(open(os.path.join(ROOT, "super4pcs_amd", "normals_src", f), "rb").read())
    return h.hexdigest()[:16]


def run(out_path, with_cpu, variants_dir):
    prop = torch.cuda.get_device_properties(0)
    res = {"source": "tools/shape_timing.py", "library_source_sha16": _digest(), "device": torch.cuda.get_device_name(0),
           "compute_units": prop.multi_processor_count, "clock_mhz": getattr(prop, "clock_rate", 0) / 1e3, "torch": torch.__version__,
           "hip": torch.version.hip,
           "method": "host perf_counter around torch.cuda.synchronize()-bracketed calls, median of %d after one warm-up; device tensors in "
                     "and out; min_neighbours 3; radii by bisection on the median count of one point in 64" % REPS,
           "rows": [], "variants": []}
    libs = {}
    if variants_dir:
        libs["package"] = shape.Shape(0)
        for path in sorted(glob.glob(os.path.join(variants_dir, "libshape_*.so"))):
            libs[os.path.basename(path)[len("libshape_"):-3]] = shape.Shape(0, lib=path)
    for label, X, start in clouds():
        row, Xt = time_cloud(label, X, start, with_cpu)
        res["rows"].append(row)
        if libs:
            res["variants"] += time_variants(label, Xt, [e["radius"] for e in row["estimate"]], libs)
        del Xt
    for lib in libs.values():
        lib.close()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


def quick():
    label, X, start = next(clouds())
    ctx = shape.Shape(0)
    ctx.set_cloud(torch.from_numpy(np.ascontiguousarray(X, np.float32)).cuda())
    r, _ = radius_for(ctx, TARGETS[1], start * 2)
    for _ in range(QUICK_CALLS):
        ctx.estimate(r)
    ctx.close()


def add_stats(csv_path, out_path):
    """The rows of a rocprofv3 kernel_stats.csv (a --quick run) into out.json: k_shape_walk and the grid's kernels."""
    rows = []
    with open(csv_path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            rows.append({"kernel": name.split("(")[0].replace("void ", "").replace("s4p_nrm::", "")[:80], "calls": int(r["Calls"]),
                         "total_us": float(r["TotalDurationNs"]) / 1e3, "average_us": float(r["AverageNs"]) / 1e3})
    rows.sort(key=lambda r: -r["total_us"])
    res = json.load(open(out_path))
    res["kernel_split"] = {"source": "rocprofv3 --kernel-trace --stats -- python tools/shape_timing.py --quick (the radius search, then %d estimate "
                                     "calls on configs[2] P at about %d neighbours; a run of its own)" % (QUICK_CALLS, TARGETS[1]), "kernels": rows[:16]}
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["kernel_split"], indent=1))


if __name__ == "__main__":
    a = [x for x in sys.argv[1:] if x != "--no-cpu"]
    B.build_normals()
    if a and a[0] == "--stats":
        add_stats(a[1], a[2] if len(a) > 2 else OUT)
    elif a and a[0] == "--quick":
        quick()
    else:
        vdir = None
        if a and a[0] == "--variants":
            vdir, a = a[1], a[2:]
        run(a[0] if a else OUT, "--no-cpu" not in sys.argv, vdir)
