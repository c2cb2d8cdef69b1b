"""The scaffolding the suites of libsuper4pcs_normals.so share (normals, neighbour lists and outliers, voxel grid, orientation,
clustering, planes): the host checks every feature repeats with its own constants, the one compiler line of the CPU
restatements, the column and pointer helpers of their ctypes classes, the run of tests/normals_facade_app with its parsed
output, and the "command line with a filter against the Python path" block.  Plain functions: a test module keeps its test
names, its literal lists and every assertion that is its own, and calls these for what is the same everywhere."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from tests import apps

ROOT = apps.ROOT
INCLUDE = os.path.join(ROOT, "include")
NORMALS_LIBS = ("super4pcs_normals",)
FACADE_APP = "normals_facade_app"


def gpu_visible():
    from tests.conftest import _gpu_visible
    return _gpu_visible()


def normals_module(name):
    """super4pcs_amd.<name> with libsuper4pcs_normals.so built."""
    from super4pcs_amd import build as B
    B.build_normals()
    return importlib.import_module("super4pcs_amd." + name)


def lib_path():
    return normals_module("normals").LIB_PATH


def cli():
    from super4pcs_amd import build as B
    return B.build_cli()


# ---- the CPU restatements ------------------------------------------------------------------------------------------------------

def build_restatement(src, outdir, libname, openmp=True):
    """tests/<src> as <outdir>/<libname>.so, without contraction: the ctypes library."""
    so = os.path.join(str(outdir), libname + ".so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off"] + (["-fopenmp"] if openmp else []) +
                          ["-fPIC", "-shared", "-std=c++17", os.path.join(ROOT, "tests", src), "-o", so])
    return ctypes.CDLL(so)


def cols(X):
    """The three float32 coordinate columns of an (n, 3) cloud, each contiguous."""
    return [np.ascontiguousarray(np.asarray(X)[:, a], np.float32) for a in range(3)]


def ptr(a):
    return None if a is None else a.ctypes.data


def xyzn(p):
    """The four leading arguments of every restatement entry: the column pointers and the point count."""
    return [p[0].ctypes.data, p[1].ctypes.data, p[2].ctypes.data, p[0].shape[0]]


# ---- host and device forms -----------------------------------------------------------------------------------------------------

def to_device(X):
    import torch
    return None if X is None else torch.from_numpy(X).cuda()


def to_host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


# ---- the host checks -------------------------------------------------------------------------------------------------------------

def declared(header, prefix_regex, txt=None):
    """The functions include/<header> declares under the prefix, comments stripped; sorted."""
    if txt is None:
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(%s\w+)\s*\(" % prefix_regex, txt)))


def check_header(header, prefix_regex, symbols, binding, closed_prefixes=None, restype=ctypes.c_int32):
    """The header's declarations under the prefix are the binding's symbol list and the library's defined exports under it;
    nothing is declared under closed_prefixes; every function of the loaded binding has argtypes and the restype (None: not
    asked, for a header with functions that return a pointer).  Returns (the header without comments, the declared names,
    nm's output) for what a header pins of its own."""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, header)).read(), flags=re.S)
    decl = declared(header, prefix_regex, txt)
    assert decl == sorted(symbols), decl
    if closed_prefixes:
        assert not declared(header, closed_prefixes, txt)                       # the older prefixes stay closed sets
    for s in decl:
        fn = getattr(binding, s)
        assert fn.argtypes is not None and (restype is None or fn.restype is restype), s
    exported = subprocess.run(["nm", "-D", "--defined-only", lib_path()], capture_output=True, text=True).stdout
    got = sorted(set(re.findall(r"\b(%s\w+)" % prefix_regex, exported)))
    assert got == decl, got
    return txt, decl, exported


def check_kernels_in_namespace(names, stray=None):
    """Every kernel of `names` is in the library as s4p_nrm::<name>; nothing matches the regex `stray` (a family's kernel
    outside the namespace).  Returns nm -C's output."""
    out = subprocess.run(["nm", "-C", lib_path()], capture_output=True, text=True).stdout
    for name in names:
        assert "s4p_nrm::" + name in out, name
    if stray:
        assert not re.search(stray, out)
    return out


def check_no_device(error_type, calls, code=-2, text="no HIP device"):
    for i, call in enumerate(calls):
        with pytest.raises(error_type) as e:
            call()
        assert e.value.code == code and text in str(e.value), (i, str(e.value))


def check_cli_flags(tmp_path, bad, good, usage_word, usage_order=None):
    """Every list of `bad` is a usage error that names usage_word; every list of `good` passes the parser and fails at the
    missing input; with usage_order = (earlier, later) the usage text has the two in that order."""
    exe = cli()
    base = [exe, "-i", "a.obj", "b.obj"]
    for flags in bad:
        r = subprocess.run(base + flags, capture_output=True, text=True)
        assert r.returncode == 1 and "Usage:" in r.stderr and usage_word in r.stderr, (flags, r.returncode, r.stderr)
    for flags in good:
        r = subprocess.run([exe, "-i", str(tmp_path / "none1.obj"), str(tmp_path / "none2.obj")] + flags, capture_output=True, text=True)
        assert r.returncode == 255 and "Can't read input set1" in r.stderr, (flags, r.stderr)
    if usage_order:
        r = subprocess.run(base + ["-h"], capture_output=True, text=True)
        assert r.stderr.index(usage_order[0]) < r.stderr.index(usage_order[1])       # the older usage lines come first


def _two_inputs(tmp_path):
    pts = np.random.default_rng(1).uniform(size=(50, 3))
    apps.write_obj(tmp_path / "P.obj", pts); apps.write_obj(tmp_path / "Q.obj", pts)
    return pts


def check_cli_refuses_faces(tmp_path, flag_args):
    """Faces index the vertex list: either input with faces is refused before any device work, with exit status -2, the
    flag's name and no matrix file."""
    pts = _two_inputs(tmp_path)
    apps.write_obj(tmp_path / "Q.obj", pts, faces=[(1, 2, 3), (2, 3, 4)])
    for first, second in (("P.obj", "Q.obj"), ("Q.obj", "P.obj")):
        r = subprocess.run([cli(), "-i", str(tmp_path / first), str(tmp_path / second)] + flag_args + ["-m", str(tmp_path / "m.txt")],
                           capture_output=True, text=True, timeout=120)
        out = r.stdout + r.stderr
        assert r.returncode == 254 and flag_args[0] in out and "faces" in out, (r.returncode, r.stdout, r.stderr)
        assert not (tmp_path / "m.txt").exists()


def check_cli_no_device(tmp_path, flag_args, facade_name=None):
    """A valid command reaches the device call and ends with its error: exit status -2, the facade call's name where the
    command line prints one."""
    _two_inputs(tmp_path)
    r = subprocess.run([cli(), "-i", str(tmp_path / "P.obj"), str(tmp_path / "Q.obj")] + flag_args + ["-m", str(tmp_path / "m.txt")],
                       capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 254, (r.returncode, r.stdout, r.stderr)
    assert "Unknown flag" not in r.stderr and "no HIP device" in out and (facade_name is None or facade_name in out), (r.stdout, r.stderr)


def build_facade_app(outdir, extra=()):
    """tests/normals_facade_app/main.cpp with -Werror against the facade headers and libsuper4pcs_normals.so."""
    return apps.build_app(outdir, FACADE_APP, NORMALS_LIBS, ("-Werror",) + tuple(extra))


def check_header_alone(tmp_path, header, eigen):
    """include/super4pcs/algorithms/<header>, included alone, compiles up to the probe's #error and sees Eigen exactly when it
    is there.  Returns the compiler flags of that choice."""
    extra = ["-I" + os.path.join(ROOT, "oracle", "eigen_shim")] if eigen else ["-DS4P_NO_EIGEN"]
    probe = tmp_path / "probe.cpp"
    probe.write_text('#include "super4pcs/algorithms/%s"\n#ifdef S4P_HAVE_EIGEN\n#error have\n#else\n#error none\n#endif\n' % header)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + INCLUDE] + extra + [str(probe)], capture_output=True, text=True)
    assert re.search(r"#error (have|none)", r.stderr).group(1) == ("have" if eigen else "none"), r.stderr
    return extra


def check_facade_header(tmp_path, header, eigen, command, rows, no_device_args, no_device_text, bad_args, bad_text):
    """check_header_alone; the facade program compiles with -Werror either way; `command` (the subcommand's word) on a file of
    `rows` ends with status 1 and every text of no_device_text without a device, and with status 1 and bad_text for every
    argument list of bad_args.  Returns the program and the file."""
    extra = check_header_alone(tmp_path, header, eigen)
    exe = build_facade_app(tmp_path, extra)
    assert os.path.exists(exe)
    path = str(tmp_path / "P.txt")
    apps.write_xyz(path, rows)
    if not gpu_visible():
        r = subprocess.run([exe, command, path] + no_device_args, capture_output=True, text=True)
        assert r.returncode == 1 and not [t for t in no_device_text if t not in r.stderr], r.stderr
    for bad in bad_args:
        r = subprocess.run([exe, command, path] + bad, capture_output=True, text=True)
        assert r.returncode == 1 and bad_text in r.stderr, (bad, r.stderr)
    return exe, path


# ---- the GPU-side blocks ---------------------------------------------------------------------------------------------------------

def run_points_app(exe, args, rows):
    """Writes the rows next to the program, runs `exe args[0] file args[1:]` under the time limit, exit status 0 required.
    Returns (heads, counts, points): the lines that begin with a word ("removed 3", "plane ..."), after each of them the
    one-number lines that follow it (counts, masks, labels, rows) as an int64 array, and the point lines at the end as a
    float64 array with one row per line (no columns when there is none)."""
    path = os.path.join(os.path.dirname(exe), "points.txt")
    apps.write_xyz(path, rows)
    r = subprocess.run([exe, args[0], path] + [str(a) for a in args[1:]], capture_output=True, text=True, timeout=apps.TIMEOUT)
    assert r.returncode == 0, r.stderr
    heads, counts, points = [], [], []
    for ln in r.stdout.splitlines():
        words = ln.split()
        if ln[:1].isalpha() and words[0] not in ("nan", "inf"):
            heads.append(ln); counts.append([])
        elif len(words) == 1:
            counts[-1].append(int(words[0]))
        else:
            points.append([float(v) for v in words])
    return heads, [np.array(c, np.int64) for c in counts], np.array(points, np.float64).reshape(len(points), -1)


def cli_filter_equals_python(tmp_path, P, Q, flag_args, python_filter, banner):
    """`Super4PCS ... flag_args -m -r` on the pair against the Python path: python_filter on both clouds, then
    capi.Matcher with the same options.  The matrix file is text of limited precision and is compared within 1e-5; the -r
    file holds binary floats, the filtered and registered Q, and is compared bit for bit.  Returns (the filtered P, the
    filtered Q)."""
    from super4pcs_amd import capi
    delta, overlap, n_s = 0.01, 0.6, 200
    apps.write_obj(tmp_path / "P.obj", P); apps.write_obj(tmp_path / "Q.obj", Q)
    got, out = apps.run_cli(cli(), tmp_path / "P.obj", tmp_path / "Q.obj", delta, overlap, n_s, list(flag_args) + ["-r", tmp_path / "reg.obj"])
    Pk, Qk = python_filter(P), python_filter(Q)
    gm = capi.Matcher(capi.make_options(delta, overlap, n_s))
    _, M, gQ = gm.compute_transformation(Pk, Qk)
    print("kept %d of %d, %d of %d\ncli:\n%s\npython:\n%s" % (len(Pk), len(P), len(Qk), len(Q), got, M))
    assert np.max(np.abs(got - np.asarray(M, np.float64))) <= 1e-5
    assert banner in out
    head, body = (tmp_path / "reg.ply").read_bytes().split(b"end_header\n", 1)
    assert b"element vertex %d\n" % len(Qk) in head
    assert np.array_equal(np.frombuffer(body, "<f4").reshape(-1, 3), gQ)
    return Pk, Qk
