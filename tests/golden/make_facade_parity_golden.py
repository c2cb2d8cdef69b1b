"""Records tests/golden/facade_parity.json: what the facade programs under tests/*_app print on the MI355X, line by line.

    python tests/golden/make_facade_parity_golden.py [--include DIR] [--out FILE]
        (on the MI355X, by hand; DIR: the include/ tree whose facade headers are to be pinned, default this tree's)

CASES is the one list of runs; tests/test_gpu_facade_parity.py builds the programs from this tree's headers, runs the same
list and asks for equal strings.  The programs print every number as %.9g of a float or %.17g of a double, the host
arithmetic of the headers is plain C++ in a fixed order and the libraries sum in a fixed order, so headers that make the same
calls with the same arguments print the same characters.

Inputs: the hippo fixture (tests/golden/hippo_config1.npz, 5281 / 3820 points).  No run calls the matcher: Q is moved on the
host by the fixture's registration followed by a fixed motion of 1 degree and 0.2 % of P's extent, and every ICP run starts
from the identity.  Normals, where a case wants the files to carry them, are the directions from the cloud's centroid, and
colours a fixed function of the position: host arithmetic of +, *, /, sqrt and floor only, the same bits wherever it runs.
A line of numbers only (one per point: normals, masks, moved points) is not stored: such lines are replaced, in place, by
one line with their count and SHA-256.  Every matrix, count and status line is stored as printed."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import apps  # noqa: E402

F = np.float32
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "facade_parity.json")
NORMALS_LIBS = ("super4pcs_normals",)
PROGRAMS = {"icp_facade_app": apps.ICP_FACADE_LIBS, "multiway_app": apps.ICP_FACADE_LIBS,
            "icp_multiscale_app": ("super4pcs_icp", "super4pcs_normals", "dl"), "normals_facade_app": NORMALS_LIBS}
COS1, SIN1 = 0.9998476951563913, 0.01745240643728351          # of one degree


def _icp(name, p, q, *flags):
    return (name, "icp_facade_app", (p, q, "0.01", "0.7", "200") + flags)


# (case, program, arguments; a name of write_inputs' files stands for its path)
CASES = [_icp("icp/" + m, "P.xyz", "Q.xyz", "--identity", "--metric", m) for m in ("point", "plane", "gicp", "symmetric")]
CASES += [_icp("icp/color", "P_rgb.xyz", "Q_rgb.xyz", "--identity", "--metric", "color", "--rgb")]
for _m in ("plane", "gicp", "symmetric"):
    CASES += [_icp("icp/%s/own_normals" % _m, "P_n.xyz", "Q_n.xyz", "--identity", "--metric", _m),
              # the last point of Q has no normal: icp_own_normals' boundary, the estimated path
              _icp("icp/%s/last_of_Q_without" % _m, "P_n.xyz", "Q_n_but_last.xyz", "--identity", "--metric", _m)]
CASES += [_icp("icp/trimmed", "P.xyz", "Q.xyz", "--identity", "--loss", "trimmed", "--trim-fraction", "0.7"),
          _icp("icp/huber", "P.xyz", "Q.xyz", "--identity", "--loss", "huber"),
          _icp("icp/point/rejection", "P.xyz", "Q.xyz", "--identity", "--metric", "point", "--reciprocal", "--normal-angle-deg", "60"),
          _icp("icp/gicp/rejection", "P.xyz", "Q.xyz", "--identity", "--metric", "gicp", "--reciprocal", "--normal-angle-deg", "60"),
          _icp("icp/batch", "P.xyz", "Q.xyz", "--batch"),
          _icp("icp/batch/plane", "P.xyz", "Q.xyz", "--batch", "--metric", "plane"),
          ("multiway/plane", "multiway_app", ("poses.txt", "0.04", "0.3", "scan0.xyz", "scan1.xyz", "scan2.xyz")),
          ("multiway/gicp", "multiway_app", ("poses.txt", "0.04", "0.3", "scan0.xyz", "scan1.xyz", "scan2.xyz", "--metric", "gicp")),
          ("multiscale/point", "icp_multiscale_app", ("P.xyz", "Q_own_frame.xyz", "T0.txt", "point", "0.02:0.06:20", "0:0.04:20")),
          ("normals", "normals_facade_app", ("normals", "P.xyz", "16")),
          ("orient", "normals_facade_app", ("orient", "P_n_mixed.txt", "8", "-1")),
          ("outliers", "normals_facade_app", ("outliers", "P.xyz", "stat", "16", "2.0")),
          ("voxel", "normals_facade_app", ("voxel", "P_n_rgb.txt", "0.02", "attrs"))]


def _radial(X):
    d = X.astype(np.float64) - X.astype(np.float64).mean(0)
    return (d / np.sqrt((d * d).sum(1))[:, None]).astype(F)


def _rgb(X):
    v = X.astype(np.float64) * 37.0
    return np.floor(255.0 * (v - np.floor(v))).astype(F)


def write_inputs(d):
    """Every input file of CASES under the directory d: name -> path."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "hippo_config1.npz"))
    Ps, Qu = g["Ps"].astype(F), g["Qu"].astype(F)
    motion = np.eye(4)
    motion[:2, :2] = [[COS1, -SIN1], [SIN1, COS1]]
    motion[:3, 3] = 0.002 * (Ps.max(0).astype(np.float64) - Ps.min(0).astype(np.float64))
    T0 = (motion @ g["M"].astype(np.float64)).astype(F)
    Q = apps.move_f32(T0, Qu)
    Np, Nq = _radial(Ps), _radial(Q)
    Np_mixed = Np.copy()
    Np_mixed[::3] *= -1                                                                # every third normal points inward: OrientNormals flips
    Nq_but_last = [tuple(r) for r in np.column_stack([Q, Nq])[:-1]] + [tuple(Q[-1])]
    order = np.argsort(Ps[:, 0], kind="stable")
    n = len(order)
    scans = [Ps[np.sort(order[a * n // 5:(a + 3) * n // 5])] for a in range(3)]        # three overlapping slabs of P along x
    tilt = np.eye(4)
    tilt[1:3, 1:3] = [[COS1, -SIN1], [SIN1, COS1]]
    poses = [np.eye(4), motion, tilt @ motion, np.eye(4)]                              # the start poses, then the pose of the information
    rows = {"P.xyz": Ps, "Q.xyz": Q, "Q_own_frame.xyz": Qu, "P_n.xyz": np.column_stack([Ps, Np]), "Q_n.xyz": np.column_stack([Q, Nq]),
            "Q_n_but_last.xyz": Nq_but_last, "P_rgb.xyz": np.column_stack([Ps, _rgb(Ps)]), "Q_rgb.xyz": np.column_stack([Q, _rgb(Q)]),
            "P_n_rgb.txt": np.column_stack([Ps, Np, _rgb(Ps)]), "P_n_mixed.txt": np.column_stack([Ps, Np_mixed]), "T0.txt": [T0.reshape(16)],
            "scan0.xyz": scans[0], "scan1.xyz": scans[1], "scan2.xyz": scans[2]}
    files = {}
    for name, r in rows.items():
        files[name] = os.path.join(str(d), name)
        apps.write_xyz(files[name], r)
    files["poses.txt"] = os.path.join(str(d), "poses.txt")
    with open(files["poses.txt"], "w") as f:
        f.write("".join(" ".join("%.17g" % v for v in X.reshape(16)) + "\n" for X in poses))
    return files


def build(outdir, include=None):
    """The programs against the facade headers under `include` (default: this tree's): program -> path."""
    return {name: apps.build_app(outdir, name, libs, ("-Werror",), include=include) for name, libs in PROGRAMS.items()}


def _fold(lines):
    """The lines as stored: each run of number-only lines becomes "<count> lines sha256 <digest>"."""
    out, run = [], []

    def flush():
        if run:
            out.append("%d lines sha256 %s" % (len(run), hashlib.sha256("\n".join(run).encode()).hexdigest()))
            del run[:]
    for ln in lines:
        if ln[:1].isalpha():
            flush()
            out.append(ln)
        else:
            run.append(ln)
    flush()
    return out


def run_case(case, programs, files):
    """{"returncode", "lines"} of one entry of CASES."""
    name, program, args = case
    r = subprocess.run([programs[program]] + [files.get(a, a) for a in args], capture_output=True, text=True, timeout=apps.TIMEOUT)
    return {"returncode": r.returncode, "lines": _fold((r.stdout + r.stderr).splitlines())}


def record(programs, files):
    return {case[0]: run_case(case, programs, files) for case in CASES}


if __name__ == "__main__":
    import tempfile
    from super4pcs_amd import build as B
    B.build(); B.build_icp(); B.build_normals()
    arg = dict(zip(sys.argv[1::2], sys.argv[2::2]))
    with tempfile.TemporaryDirectory() as d:
        got = record(build(d, arg.get("--include")), write_inputs(d))
    bad = [k for k, v in got.items() if v["returncode"] != 0]
    out = arg.get("--out", OUT)
    with open(out, "w") as f:
        json.dump(got, f, indent=1)
        f.write("\n")
    print("%d cases -> %s (%d bytes); nonzero exit: %s" % (len(got), out, os.path.getsize(out), bad))
    sys.exit(1 if bad else 0)
