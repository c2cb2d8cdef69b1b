"""Point-to-plane ICP (include/s4p_icp_plane.h) on the host: exports and binding, the plane solve against numpy, its
degenerate cases, the CPU restatement of the normals and of the plane sums against numpy brute force, the command line's
new flags."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import icp_helpers as H
from tests import icp_plane_helpers as PH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def icp_lib(s4p_lib_built):
    from super4pcs_amd import build as B
    B.build_icp()
    from super4pcs_amd import icp
    return icp


@pytest.fixture(scope="module")
def pcpu(tmp_path_factory):
    return PH.build_plane_cpu(tmp_path_factory.mktemp("icp_plane_cpu"))


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return H.build_cpu(tmp_path_factory.mktemp("icp_cpu"))


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(s4p_icp_\w+)\s*\(", txt)))


def test_plane_functions_are_exported_and_bound(icp_lib):
    decl = _declared("s4p_icp_plane.h")
    assert len(decl) == 7, decl
    assert set(decl) == set(icp_lib.PLANE_SYMBOLS) and not set(decl) & set(icp_lib.SYMBOLS)
    L = ctypes.CDLL(icp_lib.LIB_PATH)
    assert not [s for s in decl if not hasattr(L, s)]
    Lb = icp_lib.load_library()
    for s in decl:
        assert getattr(Lb, s).argtypes is not None
    assert icp_lib.STATUS_NAMES[icp_lib.DEGENERATE] and icp_lib.DEGENERATE == 3


def test_plane_kernels_live_in_the_icp_namespace(icp_lib):
    out = subprocess.run(["nm", "-C", icp_lib.LIB_PATH], capture_output=True, text=True).stdout
    for k in ("k_normals", "k_match_plane", "k_final_plane"):
        assert re.search(r"s4p_icp::%s\b" % k, out), k
    assert "_ZN3s4p" not in subprocess.run(["nm", "-D", "--defined-only", icp_lib.LIB_PATH], capture_output=True, text=True).stdout


def _rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _sums_from_system(A, b, n_plane=100):
    s = np.zeros(31)
    s[0] = n_plane; s[1] = 1.0; s[2] = n_plane; s[3] = 1.0
    s[4:25] = A[np.triu_indices(6)]
    s[25:31] = b
    return s


@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3])
def test_solve_plane_equals_numpy_solve_and_rodrigues(icp_lib, scale):
    rng = np.random.default_rng(int(scale * 1000) + 1)
    for _ in range(30):
        M = rng.normal(size=(6, 6))
        A = M @ M.T + 6 * np.eye(6)
        D = np.diag([scale] * 3 + [1.0] * 3)                    # rotation rows carry a length: unit-free degeneracy test
        A = D @ A @ D
        b = rng.normal(size=6) * np.array([scale] * 3 + [1.0] * 3) * 0.05
        got = icp_lib.solve_plane(_sums_from_system(A, b))
        x = np.linalg.solve(A, b)
        want = np.eye(4); want[:3, :3] = _rodrigues(x[:3]); want[:3, 3] = x[3:]
        assert np.max(np.abs(got - want)) <= 1e-10 * max(1.0, np.max(np.abs(want))), (got, want)
        R = got[:3, :3]
        assert np.max(np.abs(R @ R.T - np.eye(3))) <= 1e-14 and abs(np.linalg.det(R) - 1.0) <= 1e-14
        assert np.array_equal(got[3], [0, 0, 0, 1])
    # zero step: the identity exactly
    assert np.array_equal(icp_lib.solve_plane(_sums_from_system(np.eye(6), np.zeros(6))), np.eye(4))


def _planar_sums(rng, n=500):
    """The plane sums of a planar target (z = 0, normals (0, 0, 1)) for a source near it: rotation about z and sliding in
    the plane are unobservable."""
    q = np.column_stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.normal(scale=0.01, size=n)])
    p = q.copy(); p[:, 2] = 0.0
    nv = np.tile([0.0, 0.0, 1.0], (n, 1))
    a = np.concatenate([np.cross(q, nv), nv], axis=1)
    r = ((p - q) * nv).sum(1)
    return _sums_from_system(a.T @ a, a.T @ r, n_plane=n)


def test_solve_plane_reports_degenerate_systems(icp_lib):
    rng = np.random.default_rng(3)
    for s in (_planar_sums(rng), _planar_sums(rng, 20)):
        with pytest.raises(icp_lib.ICPError) as e:
            icp_lib.solve_plane(s)
        assert e.value.code == icp_lib.ERR_DEGENERATE
    # a well-conditioned system with n_plane < 6
    M = rng.normal(size=(6, 6))
    s = _sums_from_system(M @ M.T + 6 * np.eye(6), np.zeros(6), n_plane=5)
    with pytest.raises(icp_lib.ICPError) as e:
        icp_lib.solve_plane(s)
    assert e.value.code == icp_lib.ERR_DEGENERATE
    s[2] = 6
    icp_lib.solve_plane(s)
    # nearly planar: the smallest balanced eigenvalue below 1e-10 of the largest
    A = np.diag([1.0, 1.0, 1e-12, 1.0, 1.0, 1.0])
    with pytest.raises(icp_lib.ICPError):
        icp_lib.solve_plane(_sums_from_system(A, np.zeros(6)))
    icp_lib.solve_plane(_sums_from_system(np.diag([1.0, 1.0, 1e-8, 1.0, 1.0, 1.0]), np.zeros(6)))


def _surface(rng, n):
    """A bumpy height field with duplicated points and a few isolated ones (zero normals)."""
    xy = rng.uniform(-0.5, 0.5, size=(n, 2))
    z = 0.05 * np.sin(6 * xy[:, 0]) * np.cos(5 * xy[:, 1])
    P = np.column_stack([xy, z]).astype(np.float32)
    P[n // 2:n // 2 + n // 20] = P[:n // 20]
    P[-5:] = np.array([[3.0, 3.0, 3.0]], np.float32) + np.arange(5, dtype=np.float32)[:, None]
    return P


@pytest.mark.parametrize("seed", [1, 2])
def test_normal_restatement_equals_numpy_brute_force(pcpu, seed):
    rng = np.random.default_rng(seed)
    P = _surface(rng, 1500)
    c = P.mean(0).astype(np.float32)
    Pc = (P - c).astype(np.float32)
    r = 0.06 if seed == 1 else 0.045
    k, c6 = pcpu.cov(Pc, r)
    kb, cb = PH.numpy_brute_cov(Pc, r)
    assert np.array_equal(k, kb)
    assert np.all(np.abs(c6 - cb) <= 1e-12 * max(1.0, np.max(np.abs(cb))))
    assert k.min() == 1 and k.max() > 20                         # isolated points see only themselves
    N, w = PH.normals_from_cov(k, c6, 6)
    assert np.all(N[k < 6] == 0) and np.all(np.abs(np.linalg.norm(N[k >= 6], axis=1) - 1) < 1e-6)
    lead = N[np.arange(len(N)), np.argmax(np.abs(N), axis=1)]
    assert np.all(lead[k >= 6] > 0)
    # on a height field of small slope the normal is close to +z
    assert np.median(N[k >= 6, 2]) > 0.9


def test_plane_sum_restatement_equals_a_direct_loop(cpu):
    rng = np.random.default_rng(9)
    P = _surface(rng, 1200)
    c = P.mean(0).astype(np.float32)
    Pc = (P - c).astype(np.float32)
    Qc = (Pc[rng.integers(0, len(Pc), 700)] + rng.normal(scale=0.01, size=(700, 3))).astype(np.float32)
    N = PH.normalise(rng.normal(size=(len(Pc), 3)))
    N[::7] = 0
    d = 0.03
    T = np.eye(4); T[:3, 3] = [0.004, -0.002, 0.001]
    idx, d2 = H.numpy_brute(Pc, Qc, T, d)
    s = PH.plane_sums(Pc, Qc, T, idx, d2, N)
    ref = np.zeros(31)
    Tf = T.astype(np.float32)
    for j in range(len(Qc)):
        if idx[j] < 0:
            continue
        x, y, z = Qc[j]
        q = np.array([((Tf[r, 0] * x + Tf[r, 1] * y) + Tf[r, 2] * z) + Tf[r, 3] for r in range(3)], np.float64)
        ref[0] += 1; ref[1] += float(d2[j])
        nv = N[idx[j]].astype(np.float64)
        if not nv.any():
            continue
        a = np.array([q[1] * nv[2] - q[2] * nv[1], q[2] * nv[0] - q[0] * nv[2], q[0] * nv[1] - q[1] * nv[0], *nv])
        r = float(np.dot(Pc[idx[j]].astype(np.float64) - q, nv))
        ref[2] += 1; ref[3] += r * r
        ref[4:25] += np.outer(a, a)[np.triu_indices(6)]
        ref[25:31] += a * r
    assert s[0] == ref[0] and s[2] == ref[2] and 0 < s[2] < s[0]
    assert np.all(np.abs(s - ref) <= 1e-12 * np.maximum(1.0, np.abs(ref)))


def test_normalise_rule():
    N = np.array([[3, 4, 0], [0, 0, 0], [np.nan, 1, 0], [np.inf, 0, 0], [1e-30, 0, 0], [-2, 0, 0]], np.float32)
    out = PH.normalise(N)
    assert np.array_equal(out, np.array([[0.6, 0.8, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [1, 0, 0], [-1, 0, 0]], np.float32))


def test_cli_icp_metric_flags_parse_and_bad_values_exit_with_usage(s4p_lib_built, tmp_path):
    from super4pcs_amd import build as B
    cli = B.build_cli()
    for bad in (["--icp-metric", "planar"], ["--icp-metric", ""], ["--icp-normal-radius", "0"], ["--icp-normal-radius", "-1"],
                ["--icp-normal-radius", "nan"], ["--icp-normal-radius", "inf"], ["--icp-normal-radius", "1x"]):
        r = subprocess.run([cli, "-i", "a.obj", "b.obj", "--icp", "30"] + bad, capture_output=True, text=True)
        assert r.returncode == 1 and "Usage:" in r.stderr and "--icp-metric" in r.stderr, (bad, r.returncode, r.stderr)
    for good in (["--icp-metric", "plane", "--icp-normal-radius", "0.03"], ["--icp-metric", "point"]):
        r = subprocess.run([cli, "-i", str(tmp_path / "none1.obj"), str(tmp_path / "none2.obj"), "--icp", "30"] + good,
                           capture_output=True, text=True)
        assert r.returncode == 255 and "Can't read input set1" in r.stderr, (good, r.stderr)
