"""The scaffolding the tests share around the programs under tests/*_app and the command line: one compiler line, the text
and OBJ writers, the float move of a cloud in the facade's order, the run of tests/icp_facade_app with its parsed output,
and the run of `Super4PCS ... -m` with its parsed matrix.  Plain functions; the assertions on what comes back stay in the
tests."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "super4pcs_amd", "lib")
TIMEOUT = 300
ICP_FACADE_LIBS = ("super4pcs_amd", "super4pcs_icp")        # not the normals library: RefineICP binds it at run time


def build_app(outdir, name, libs, extra=(), include=None):
    """tests/<name>/main.cpp against the facade headers and the libraries `libs` of super4pcs_amd/lib; extra: further
    compiler flags (-Werror, -g, -D..., sanitizers); include: another include/ tree than this one's (the recorders under
    tests/golden pin an earlier tree's headers with it).  Returns the program's path under outdir."""
    exe = os.path.join(str(outdir), name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + (include or os.path.join(ROOT, "include"))] + list(extra) +
                          [os.path.join(ROOT, "tests", name, "main.cpp"), "-L" + LIBDIR] + ["-l" + lib for lib in libs] +
                          ["-Wl,-rpath," + LIBDIR, "-o", exe])
    return exe


def write_xyz(path, rows):
    """One "%.9g ..." line per row, as np.savetxt(fmt="%.9g") writes it; the rows need not have one length."""
    with open(path, "w") as f:
        for row in rows:
            f.write(" ".join("%.9g" % v for v in row) + "\n")


def write_obj(path, pts, faces=()):
    with open(path, "w") as f:
        f.write("# points\n")
        for p in pts:
            f.write("v %.9g %.9g %.9g\n" % (p[0], p[1], p[2]))
        for t in faces:
            f.write("f %d %d %d\n" % tuple(t))
        f.write("# End of File\n")


def move_f32(M, X):
    """float32 (n, 3): X moved by the float matrix in k_apply's and the facade's order, ((m0 * x + m1 * y) + m2 * z) + m3."""
    M = np.asarray(M, np.float32); X = np.asarray(X, np.float32)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    return np.stack([((M[k, 0] * x + M[k, 1] * y) + M[k, 2] * z) + M[k, 3] for k in range(3)], 1).astype(np.float32)


def start_icp_app(exe, P_rows, Q_rows, delta, overlap, samples, *flags):
    """Writes P.xyz and Q.xyz next to the program and runs `exe P.xyz Q.xyz delta overlap samples flags...`: the finished
    process, whatever its exit status."""
    d = os.path.dirname(exe)
    p, q = os.path.join(d, "P.xyz"), os.path.join(d, "Q.xyz")
    write_xyz(p, P_rows); write_xyz(q, Q_rows)
    return subprocess.run([exe, p, q, str(delta), str(overlap), str(samples)] + [str(f) for f in flags], capture_output=True, text=True,
                          timeout=TIMEOUT)


def run_icp_app(exe, P_rows, Q_rows, delta, overlap, samples, *flags):
    """start_icp_app, exit status 0 required: ({"registered": float32 4x4, "refined": float32 4x4}, the words of the
    "icp iterations ..." line)."""
    out = start_icp_app(exe, P_rows, Q_rows, delta, overlap, samples, *flags)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = {ln.split()[0]: np.array([float(v) for v in ln.split()[1:17]], np.float32).reshape(4, 4)
            for ln in out.stdout.splitlines() if ln.startswith(("registered", "refined"))}
    stats = [ln for ln in out.stdout.splitlines() if ln.startswith("icp iterations")][0].split()
    return rows, stats


def run_cli(cli, P_obj, Q_obj, delta, overlap, samples, extra_args=()):
    """`Super4PCS -i P Q -o overlap -d delta -t 1000 -n samples extra_args... -m mat.txt`, exit status 0 required: (the 4x4
    of the matrix file, stdout + stderr)."""
    mat = os.path.join(os.path.dirname(str(Q_obj)), "mat.txt")
    rc = subprocess.run([cli, "-i", str(P_obj), str(Q_obj), "-o", str(overlap), "-d", str(delta), "-t", "1000", "-n", str(samples)] +
                        [str(a) for a in extra_args] + ["-m", mat], capture_output=True, text=True, timeout=TIMEOUT)
    assert rc.returncode == 0, rc.stderr
    lines = open(mat).read().splitlines()
    assert lines[:2] == ["VERSION\t=\t1", "MATRIX\t="]
    return np.array([[float(v) for v in ln.split()] for ln in lines[2:6]]), rc.stdout + rc.stderr
