"""Generalized ICP (include/s4p_icp_gicp.h) on the host: exports and binding, the numpy restatement of the generalized sums
against the point-to-point Gauss-Newton system and against numpy's solve, the command line's new flags, and the Python
argument checks that need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import icp_gicp_helpers as GH
from tests import icp_helpers as H
from tests import icp_plane_helpers as PH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def icp_lib(s4p_lib_built):
    from super4pcs_amd import build as B
    B.build_icp()
    from super4pcs_amd import icp
    return icp


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(s4p_icp_\w+)\s*\(", txt)))


def test_gicp_functions_are_exported_and_bound(icp_lib):
    decl = _declared("s4p_icp_gicp.h")
    assert len(decl) == 5, decl
    assert set(decl) == set(icp_lib.GICP_SYMBOLS)
    others = set(icp_lib.SYMBOLS) | set(icp_lib.PLANE_SYMBOLS) | set(icp_lib.ROBUST_SYMBOLS)
    assert not set(decl) & others
    L = ctypes.CDLL(icp_lib.LIB_PATH)
    assert not [s for s in decl if not hasattr(L, s)]
    Lb = icp_lib.load_library()
    for s in decl:
        assert getattr(Lb, s).argtypes is not None
    out = subprocess.run(["nm", "-C", icp_lib.LIB_PATH], capture_output=True, text=True).stdout
    for k in ("k_gicp_sum", "k_gather_source_normals"):
        assert re.search(r"s4p_icp::%s\b" % k, out), k


def _surface(rng, n):
    xy = rng.uniform(-0.5, 0.5, size=(n, 2))
    z = 0.05 * np.sin(6 * xy[:, 0]) * np.cos(5 * xy[:, 1])
    return np.column_stack([xy, z]).astype(np.float32)


def _pair(seed=9, n_p=1200, n_q=700):
    rng = np.random.default_rng(seed)
    P = _surface(rng, n_p)
    c = P.mean(0).astype(np.float32)
    Pc = (P - c).astype(np.float32)
    Qc = (Pc[rng.integers(0, len(Pc), n_q)] + rng.normal(scale=0.01, size=(n_q, 3))).astype(np.float32)
    Np = PH.normalise(rng.normal(size=(n_p, 3)))
    Np[::7] = 0
    Nq = PH.normalise(rng.normal(size=(n_q, 3)))
    Nq[::5] = 0
    th = np.deg2rad(0.7)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]]
    T[:3, 3] = [0.004, -0.002, 0.001]
    d = 0.03
    idx, d2 = H.numpy_brute(Pc, Qc, T, d)
    assert (idx >= 0).sum() > 300 and (idx < 0).sum() > 0
    # the worst conditioning: some pairs whose rotated source normal is the target's
    same = np.flatnonzero((idx >= 0) & Np[np.maximum(idx, 0)].any(1))[:60]
    Nq[same] = PH.normalise(Np[idx[same]].astype(np.float64) @ T[:3, :3])
    return Pc, Qc, T, idx, d2, Np, Nq


def _point_system(Pc, Qc, T, idx):
    """The point-to-point Gauss-Newton system of the matched pairs: A = sum J^T J, b = sum J^T r, J = [-[q^]x | I], with
    the sum of |term| of every entry."""
    Tf = np.asarray(T, np.float32)
    x, y, z = Qc[:, 0], Qc[:, 1], Qc[:, 2]
    qh = np.stack([((Tf[r, 0] * x + Tf[r, 1] * y) + Tf[r, 2] * z) + Tf[r, 3] for r in range(3)], 1)
    hit = idx >= 0
    q = qh[hit].astype(np.float64); p = Pc[idx[hit]].astype(np.float64)
    A = np.zeros((6, 6)); Aa = np.zeros((6, 6)); b = np.zeros(6); ba = np.zeros(6)
    for qi, pi in zip(q, p):
        X = np.array([[0, -qi[2], qi[1]], [qi[2], 0, -qi[0]], [-qi[1], qi[0], 0]])
        JT = np.vstack([X, np.eye(3)])                       # J^T = [[q^]x ; I]
        t = JT @ JT.T
        A += t; Aa += np.abs(t)
        v = JT @ (pi - qi)
        b += v; ba += np.abs(v)
    iu = np.triu_indices(6)
    return np.concatenate([A[iu], b]), np.concatenate([Aa[iu], ba])


def test_restated_sums_with_isotropic_covariances_are_half_the_point_system():
    """M = I / 2 exactly when every normal is zero, and when the source normals are zero and epsilon = 1."""
    Pc, Qc, T, idx, d2, Np, Nq = _pair()
    ref, ref_abs = _point_system(Pc, Qc, T, idx)
    zp, zq = np.zeros_like(Np), np.zeros_like(Nq)
    for np_, nq_, eps in ((zp, zq, 1e-3), (zp, zq, 1.0), (Np, zq, 1.0)):
        s, sabs = GH.gicp_sums(Pc, Qc, T, idx, d2, np_, nq_, eps)
        assert s[0] == s[2] == np.count_nonzero(idx >= 0)
        assert s[1] == d2[idx >= 0].astype(np.float64).sum()
        assert np.all(np.abs(s[4:31] - 0.5 * ref) <= 1e-12 * 0.5 * ref_abs), (s[4:31], 0.5 * ref)
        assert np.all(sabs[4:31] <= 0.5 * ref_abs * (1 + 1e-12) + 1e-300)
        # [3] = sum r^T M r = half the sum of squared double distances
        hit = idx >= 0
        q, r, _, _ = GH.pair_terms(Pc, Qc, T, idx, np_, nq_, eps)
        assert abs(s[3] - 0.5 * (r * r).sum()) <= 1e-12 * 0.5 * (r * r).sum()
        assert len(q) == hit.sum()


@pytest.mark.parametrize("eps", [1e-3, 1e-2, 1.0])
def test_every_pair_covariance_is_positive_definite_and_bounded(eps):
    """S = C(np) + C(nh): eigenvalues in [2 eps - 2e-7, 2] up to rounding, condition number <= 1.01 / eps."""
    Pc, Qc, T, idx, d2, Np, Nq = _pair()
    w = GH.sigma_spectrum(Pc, Qc, T, idx, Np, Nq, eps)
    assert np.all(w[:, 0] > 0)
    cond = w[:, 2] / w[:, 0]
    print("eps %g: lambda in [%.6g, %.6g], max condition %.6g" % (eps, w[:, 0].min(), w[:, 2].max(), cond.max()))
    assert cond.max() <= 1.01 / eps
    assert w[:, 0].min() >= 2 * eps - 4e-7 and w[:, 2].max() <= 2 + 1e-6
    # the cofactor inverse is the inverse: M S = I to rounding times the condition number
    _, _, S, M = GH.pair_terms(Pc, Qc, T, idx, Np, Nq, eps)
    F = np.empty_like(M)
    for (a, b), v in S.items():
        F[:, a, b] = v; F[:, b, a] = v
    assert np.max(np.abs(M @ F - np.eye(3))) <= 50 * (1 / eps) * 2.0 ** -53


def _rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


@pytest.mark.parametrize("eps", [1e-3, 1e-2, 1.0])
def test_solve_plane_on_the_restated_sums_equals_numpy(icp_lib, eps):
    Pc, Qc, T, idx, d2, Np, Nq = _pair()
    s, _ = GH.gicp_sums(Pc, Qc, T, idx, d2, Np, Nq, eps)
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = s[4:25]
    A = A + A.T - np.diag(np.diag(A))
    assert np.all(np.linalg.eigvalsh(A) > 0)
    x = np.linalg.solve(A, s[25:31])
    want = np.eye(4); want[:3, :3] = _rodrigues(x[:3]); want[:3, 3] = x[3:]
    got = icp_lib.solve_plane(s)
    assert np.max(np.abs(got - want)) <= 1e-10 * max(1.0, np.max(np.abs(want))), (got, want)
    # and the restatement's 6x6 is the explicit sum of J^T M J, its right side the sum of J^T M r
    q, r, _, M = GH.pair_terms(Pc, Qc, T, idx, Np, Nq, eps)
    Ad = np.zeros((6, 6)); bd = np.zeros(6); Aa = np.zeros((6, 6)); ba = np.zeros(6)
    for qi, ri, Mi in zip(q, r, M):
        X = np.array([[0, -qi[2], qi[1]], [qi[2], 0, -qi[0]], [-qi[1], qi[0], 0]])
        JT = np.vstack([X, np.eye(3)])
        t = JT @ Mi @ JT.T; v = JT @ (Mi @ ri)
        Ad += t; Aa += np.abs(t); bd += v; ba += np.abs(v)
    iu = np.triu_indices(6)
    assert np.all(np.abs(s[4:25] - Ad[iu]) <= 1e-12 * np.maximum(Aa[iu], 1e-300))
    assert np.all(np.abs(s[25:31] - bd) <= 1e-12 * np.maximum(ba, 1e-300))


def test_cli_gicp_flags_parse_and_bad_values_exit_with_usage(s4p_lib_built, tmp_path):
    from super4pcs_amd import build as B
    cli = B.build_cli()
    g = ["--icp-metric", "gicp"]
    for bad in (g + ["--icp-gicp-epsilon", "0"], g + ["--icp-gicp-epsilon", "-1"], g + ["--icp-gicp-epsilon", "1e-7"],
                g + ["--icp-gicp-epsilon", "1.5"], g + ["--icp-gicp-epsilon", "nan"], g + ["--icp-gicp-epsilon", "inf"],
                g + ["--icp-gicp-epsilon", "1x"], g + ["--icp-gicp-epsilon", ""], ["--icp-gicp-epsilon", "0.01"],
                ["--icp-metric", "plane", "--icp-gicp-epsilon", "0.01"], ["--icp-metric", "gicp2"],
                g + ["--icp-loss", "huber"], g + ["--icp-loss", "trimmed", "--icp-trim", "0.5"], ["--icp-loss", "tukey"] + g):
        r = subprocess.run([cli, "-i", "a.obj", "b.obj", "--icp", "30"] + bad, capture_output=True, text=True)
        assert r.returncode == 1 and "Usage:" in r.stderr and "--icp-gicp-epsilon" in r.stderr, (bad, r.returncode, r.stderr)
    for good in (g, g + ["--icp-gicp-epsilon", "0.01"], g + ["--icp-gicp-epsilon", "1e-6"], g + ["--icp-gicp-epsilon", "1"],
                 g + ["--icp-loss", "none"], g + ["--icp-normal-radius", "0.03", "--estimate-normals", "16"]):
        r = subprocess.run([cli, "-i", str(tmp_path / "none1.obj"), str(tmp_path / "none2.obj"), "--icp", "30"] + good,
                           capture_output=True, text=True)
        assert r.returncode == 255 and "Can't read input set1" in r.stderr, (good, r.stderr)


def test_python_argument_checks_need_no_device(icp_lib):
    P = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match="loss"):
        icp_lib.refine(P, P, max_distance=1.0, metric="gicp", loss="huber")
    with pytest.raises(ValueError, match="loss"):
        icp_lib.refine(P, P, max_distance=1.0, metric="gicp", loss="trimmed", trim_fraction=0.5)
    with pytest.raises(ValueError, match="metric"):
        icp_lib.refine(P, P, max_distance=1.0, metric="generalised")
    ctx = object.__new__(icp_lib.ICP)                       # no context: the checks come before any library call
    ctx.h = None
    with pytest.raises(ValueError, match="loss"):
        ctx.refine(metric="gicp", loss="tukey")
    with pytest.raises(ValueError, match="metric"):
        ctx.refine(metric="planes")
    assert "gicp" in icp_lib.REFINE_METRICS and icp_lib.METRICS == ("point", "plane")
