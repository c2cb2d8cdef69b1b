#!/usr/bin/env python
"""Times plane segmentation (include/s4p_plane.h, libsuper4pcs_normals.so) on the BASELINE workloads and writes
profiles/plane_timing.json.  Host clock around synchronised calls, median of 10 after a warm-up, device tensors in and out, as
tools/cluster_timing.py: segment at 1024 and 4096 trials with one refit and with none, on the configs[2] and configs[3]
clouds, next to a 16-thread run of the CPU restatement (tests/plane_cpu: a plain loop with std::fmaf, not a tuned baseline),
labelled as such.  k_plane_count alone comes from a kernel trace in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/plane_timing.py --quick      (3 calls at 4096 trials, nothing written)
    python tools/plane_timing.py --stats DIR/.../*_kernel_stats.csv [out.json]           (merges the k_plane_* rows)
The vector instructions per (point, candidate) pair are read from the ISA of k_plane_count's inner loop (COUNT_ISA below);
the share of the issue peak is pairs per second times that count against one wave64 vector instruction per SIMD every 2
cycles.  No target is fixed.
usage: python tools/plane_timing.py [out.json] [--no-cpu]"""
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

from super4pcs_amd import build as B, datasets as D, plane  # noqa: E402

REPS = 10
OUT = os.path.join(ROOT, "profiles", "plane_timing.json")
TRIALS = (1024, 4096)
QUICK_CALLS, QUICK_TRIALS = 3, 4096
# k_plane_count's loop over one candidate record, per lane and 16 points (hipcc of ROCm 7.2, -O3 -ffp-contract=off): the
# compiler packs the three fmaf of two points into v_pk_fma_f32; next to them 37 scalar ALU instructions, 6 s_nop and a wait
COUNT_ISA = {"points_per_lane": 16, "v_pk_fma_f32": 24, "v_cmp_le_f32": 16, "v_mov_b64": 1, "s_load_dwordx4": 1, "s_bcnt1_i32_b64": 16,
             "s_add_i32": 15, "lds_atomic_per_wave_when_nonzero": 1}
VECTOR_PER_PAIR = (COUNT_ISA["v_pk_fma_f32"] + COUNT_ISA["v_cmp_le_f32"] + COUNT_ISA["v_mov_b64"]) / COUNT_ISA["points_per_lane"]


def _med(f):
    ts = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def _distance(label):
    return 0.15 if "configs[3]" in label else 0.004


def time_cloud(label, X, with_cpu):
    ctx = plane.Plane(0)
    Xt = torch.from_numpy(np.ascontiguousarray(X, np.float32)).cuda()
    ctx.set_cloud(Xt)
    dist = _distance(label)
    row = {"label": label, "n": len(X), "distance": dist, "set_cloud_ms": _med(lambda: ctx.set_cloud(Xt)), "segment": []}
    for trials in TRIALS:
        pl, mask, info = ctx.segment(dist, trials, 0, 1)              # warm-up, and the result that is recorded
        r = {"trials": trials, "plane": [float(v) for v in pl], "inliers": info["inliers"], "trial": info["trial"],
             "valid_trials": info["valid_trials"], "refine1_ms": _med(lambda: ctx.segment(dist, trials, 0, 1)),
             "refine0_ms": _med(lambda: ctx.segment(dist, trials, 0, 0)), "pairs": len(X) * trials}
        if with_cpu:
            from tests import plane_helpers as PH
            cpu = PH.build_cpu(tempfile.mkdtemp(prefix="pcpu_"))
            t0 = time.perf_counter()
            want = cpu.segment(X, dist, trials, 0, 1, threads=16)
            r["cpu"] = {"variant": "CPU restatement (tests/plane_cpu): a plain loop with std::fmaf on 16 threads, not a tuned baseline",
                        "seconds": time.perf_counter() - t0, "equal_to_device": bool(PH.same((pl, mask, info), want))}
        row["segment"].append(r)
    ctx.close()
    print(json.dumps(row), flush=True)
    return row


def clouds():
    yield "configs[2] P, 1 M points", D.bumpy_pair(1_000_000, overlap=0.5, delta=0.004, seed=20140814)[0]
    yield "configs[3] P, 5 M points", D.lidar_pair(5_000_000, delta=0.05)[0]


def run(out_path, with_cpu):
    h = hashlib.sha256()
    for f in ("s4p_normals.hip", "s4p_plane.inc"):
        h.update(open(os.path.join(ROOT, "super4pcs_amd", "normals_src", f), "rb").read())
    prop = torch.cuda.get_device_properties(0)
    res = {"source": "tools/plane_timing.py", "library_source_sha16": h.hexdigest()[:16], "device": torch.cuda.get_device_name(0),
           "compute_units": prop.multi_processor_count, "clock_mhz": getattr(prop, "clock_rate", 0) / 1e3, "torch": torch.__version__,
           "hip": torch.version.hip,
           "method": "host perf_counter around torch.cuda.synchronize()-bracketed calls, median of %d after one warm-up; device tensors in "
                     "and out; seed 0; distance 0.004 (configs[2]) / 0.15 (configs[3])" % REPS,
           "count_isa": COUNT_ISA, "vector_instructions_per_pair": VECTOR_PER_PAIR, "rows": [time_cloud(l, X, with_cpu) for l, X in clouds()]}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


def quick():
    label, X = next(clouds())
    ctx = plane.Plane(0)
    ctx.set_cloud(torch.from_numpy(np.ascontiguousarray(X, np.float32)).cuda())
    for _ in range(QUICK_CALLS):
        ctx.segment(_distance(label), QUICK_TRIALS, 0, 1)
    ctx.close()


def add_stats(csv_path, out_path):
    """The k_plane_* rows of a rocprofv3 kernel_stats.csv (a --quick run) into out.json, and k_plane_count's rate."""
    rows = []
    with open(csv_path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            if "k_plane_" in name:
                rows.append({"kernel": name.split("(")[0].replace("void ", "").replace("s4p_nrm::", ""), "calls": int(r["Calls"]),
                             "total_us": float(r["TotalDurationNs"]) / 1e3, "average_us": float(r["AverageNs"]) / 1e3})
    rows.sort(key=lambda r: -r["total_us"])
    res = json.load(open(out_path))
    split = {"source": "rocprofv3 --kernel-trace --stats -- python tools/plane_timing.py --quick (%d segment calls on configs[2] P at %d trials, "
                       "one refit; a run of its own)" % (QUICK_CALLS, QUICK_TRIALS), "kernels": rows}
    count = [r for r in rows if r["kernel"].endswith("k_plane_count")]
    if count:
        pairs = res["rows"][0]["n"] * QUICK_TRIALS
        per_s = pairs / (count[0]["average_us"] * 1e-6)
        cus, mhz = res.get("compute_units", 256), res.get("clock_mhz") or 2400.0
        peak_lane_instr = cus * 4 * (mhz * 1e6 / 2.0) * 64                  # one wave64 vector instruction per SIMD every 2 cycles
        split["k_plane_count"] = {"average_us": count[0]["average_us"], "pairs": pairs, "clock_mhz_used": mhz, "pairs_per_second": per_s,
                                  "vector_instructions_per_pair": VECTOR_PER_PAIR,
                                  "issue_peak_lane_instructions_per_second": peak_lane_instr,
                                  "share_of_issue_peak": per_s * VECTOR_PER_PAIR / peak_lane_instr,
                                  "fma_tflops": per_s * 6 / 1e12,
                                  "note": "the issue peak counts a packed instruction as one 2-cycle issue like any other; in FLOPs "
                                          "(3 FMA per pair) the figure compares with the 157.3 TF vector peak"}
    res["kernel_split"] = split
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(split, indent=1))


if __name__ == "__main__":
    a = [x for x in sys.argv[1:] if x != "--no-cpu"]
    B.build_normals()
    if a and a[0] == "--stats":
        add_stats(a[1], a[2] if len(a) > 2 else OUT)
    elif a and a[0] == "--quick":
        quick()
    else:
        run(a[0] if a else OUT, "--no-cpu" not in sys.argv)
