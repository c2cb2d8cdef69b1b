"""Symmetric ICP (include/s4p_icp_symm.h) on the host: exports and binding, s4p_icp_solve_symmetric against a numpy
restatement, s4p_icp_solve_plane's bits across the shared 6x6 path, the restated loop on an analytic pair, the command line's
new metric, the facade application's build, and the Python argument checks that need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import apps
from tests import icp_symm_helpers as SH

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


def test_symm_functions_are_exported_and_bound(icp_lib):
    decl = _declared("s4p_icp_symm.h")
    assert len(decl) == 3, decl
    assert set(decl) == set(icp_lib.SYMM_SYMBOLS)
    others = (set(icp_lib.SYMBOLS) | set(icp_lib.PLANE_SYMBOLS) | set(icp_lib.ROBUST_SYMBOLS) | set(icp_lib.GICP_SYMBOLS) |
              set(icp_lib.COLOR_SYMBOLS) | set(icp_lib.REJECT_SYMBOLS) | set(icp_lib.BATCH_SYMBOLS))
    assert not set(decl) & others
    L = ctypes.CDLL(icp_lib.LIB_PATH)
    assert not [s for s in decl if not hasattr(L, s)]
    Lb = icp_lib.load_library()
    for s in decl:
        assert getattr(Lb, s).argtypes is not None
    out = subprocess.run(["nm", "-C", icp_lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"s4p_icp::k_symm_sum\b", out)
    assert icp_lib.SYMM_NSUMS == icp_lib.PLANE_NSUMS == 31


def _random_sums(rng, n=200, scale=1.0, tilt=0.3):
    """Well-conditioned symmetric-shaped sums: J = (h x n, n) of random points and normals, r from a small true step."""
    h = rng.normal(size=(n, 3)) * scale
    nn = rng.normal(size=(n, 3))
    J = np.concatenate([np.cross(h, nn), nn], 1)
    x = np.concatenate([rng.normal(size=3) * tilt, rng.normal(size=3) * scale * 0.1])
    r = J @ x + rng.normal(size=n) * 1e-3 * scale
    s = np.zeros(31)
    s[0], s[1], s[2], s[3] = n, 1.0, n, (r * r).sum()
    s[4:25] = (J.T @ J)[np.triu_indices(6)]
    s[25:31] = J.T @ r
    return s


def test_solve_symmetric_equals_numpy_solve_plus_the_closed_form(icp_lib):
    rng = np.random.default_rng(12)
    for k in range(40):
        s = _random_sums(rng, n=int(rng.integers(20, 400)), scale=10.0 ** rng.uniform(-2, 2), tilt=10.0 ** rng.uniform(-3, 0))
        got = icp_lib.solve_symmetric(s)
        want = SH.solve_symmetric_numpy(s)
        assert np.max(np.abs(got - want)) <= 1e-12 * max(1.0, np.max(np.abs(want))), (k, got, want)
        assert np.array_equal(got[3], [0, 0, 0, 1])


def test_solve_symmetric_zero_right_side_is_the_identity(icp_lib):
    s = _random_sums(np.random.default_rng(3))
    s[25:31] = 0.0
    assert np.array_equal(icp_lib.solve_symmetric(s), np.eye(4))


def _sums_for_step(x):
    """Sums whose solution is x up to rounding: A = a well-conditioned J^T J, b = A x."""
    rng = np.random.default_rng(5)
    h = rng.normal(size=(300, 3)); nn = rng.normal(size=(300, 3))
    J = np.concatenate([np.cross(h, nn), nn], 1)
    A = J.T @ J
    s = np.zeros(31)
    s[0] = s[2] = 300
    s[4:25] = A[np.triu_indices(6)]
    s[25:31] = A @ x
    return s


@pytest.mark.parametrize("m", [0.0, 1e-9, 0.1, 1.0, 10.0])
def test_solve_symmetric_rotates_by_twice_atan(icp_lib, m):
    """a~ = m * axis, t~ = 0: dT's rotation is the rotation by 2 atan m about the axis, orthonormal, both to 1e-14."""
    axis = np.array([0.36, -0.48, 0.8])
    dT = icp_lib.solve_symmetric(_sums_for_step(np.concatenate([m * axis, np.zeros(3)])))
    R = dT[:3, :3]
    th = 2.0 * np.arctan(m)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    want = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    print("m %g: |R - R(2 atan m)| %.3g, |R R^T - I| %.3g, |t| %.3g" % (m, np.max(np.abs(R - want)), np.max(np.abs(R @ R.T - np.eye(3))),
                                                                       np.max(np.abs(dT[:3, 3]))))
    assert np.max(np.abs(R - want)) <= 1e-14
    assert np.max(np.abs(R @ R.T - np.eye(3))) <= 1e-14


def _code(fn, s):
    L_out = np.full(16, -77.0)
    dp = ctypes.POINTER(ctypes.c_double)
    s = np.ascontiguousarray(s, np.float64)
    return fn(s.ctypes.data_as(dp), L_out.ctypes.data_as(dp)), L_out


def test_solve_symmetric_is_degenerate_where_solve_plane_is(icp_lib):
    L = icp_lib.load_library()
    rng = np.random.default_rng(7)
    good = _random_sums(rng)
    few = good.copy(); few[2] = 5
    P3 = rng.normal(size=(50, 3)); P3[:, 2] = 0
    J3 = np.concatenate([np.cross(P3, np.tile([0, 0, 1.0], (50, 1))), np.tile([0, 0, 1.0], (50, 1))], 1)    # planar: rank 3
    assert np.linalg.matrix_rank(J3) == 3
    rank3 = np.zeros(31); rank3[0] = rank3[2] = 50
    rank3[4:25] = (J3.T @ J3)[np.triu_indices(6)]; rank3[25:31] = J3.T @ rng.normal(size=50)
    nan = good.copy(); nan[9] = np.nan
    inf = good.copy(); inf[4] = np.inf
    for name, s in (("few", few), ("rank3", rank3), ("nan", nan), ("inf", inf)):
        rp, _ = _code(L.s4p_icp_solve_plane, s)
        rs, out = _code(L.s4p_icp_solve_symmetric, s)
        assert rp == rs == icp_lib.ERR_DEGENERATE, (name, rp, rs)
        assert np.all(out == -77.0)                                    # nothing written
        with pytest.raises(icp_lib.ICPError) as e:
            icp_lib.solve_symmetric(s)
        assert e.value.code == icp_lib.ERR_DEGENERATE
    assert _code(L.s4p_icp_solve_plane, good)[0] == _code(L.s4p_icp_solve_symmetric, good)[0] == 0
    assert L.s4p_icp_solve_symmetric(None, None) == -1


def test_solve_plane_returns_the_recorded_bits(icp_lib):
    """tests/golden/icp_solve_plane_bits.npz: 48 sums (well-conditioned at several scales, [2] < 6, planar, NaN, inf, b = 0)
    and what s4p_icp_solve_plane returned for them before its 6x6 path became a function shared with
    s4p_icp_solve_symmetric."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "icp_solve_plane_bits.npz"))
    L = icp_lib.load_library()
    assert len(g["sums"]) == 48 and np.count_nonzero(g["rc"] == 0) >= 30 and np.count_nonzero(g["rc"] == -8) >= 10
    for s, want, rc in zip(g["sums"], g["dT"], g["rc"]):
        got_rc, got = _code(L.s4p_icp_solve_plane, s)
        assert got_rc == rc
        assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("start_deg", [5.0, 20.0])
def test_restated_loop_reaches_the_pose_of_an_analytic_pair(icp_lib, start_deg):
    """A bumpy analytic surface with analytic normals on both clouds, a rigidly moved subset, random signs on the source
    normals, d = 0.15: restated sums + icp.solve_symmetric reach max |T q - p| <= 1e-9 within 10 iterations."""
    P, Np, Q, Nq, M, pick = SH.analytic_pair()
    T = SH.motion(start_deg, [0, 0, 0], axis=(0.2, 0.9, 0.4)) @ np.linalg.inv(M)
    errs = []
    for k in range(10):
        idx, d2 = SH.brute_pass(P, Q, T, 0.15)
        s, _ = SH.symm_sums(P, Q, T, idx, d2, Np, Nq, ft=np.float64)
        T = icp_lib.compose(icp_lib.solve_symmetric(s), T)
        errs.append(float(np.max(np.abs(Q @ T[:3, :3].T + T[:3, 3] - P[pick]))))
        if errs[-1] <= 1e-9:
            break
    print("analytic pair from %g degrees: max |T q - p| per iteration %s" % (start_deg, ["%.2g" % e for e in errs]))
    assert errs[-1] <= 1e-9, errs


def test_restated_sums_ignore_the_normals_signs():
    """The restatement itself: negating any subset of either cloud's normals leaves every one of the 31 sums' bits."""
    P, Np, Q, Nq, M, pick = SH.analytic_pair(n_p=1500, n_q=600)
    P, Np, Q, Nq = (a.astype(np.float32) for a in (P, Np, Q, Nq))
    T = (SH.motion(3.0, [0.01, 0, 0]) @ np.linalg.inv(M)).astype(np.float32)
    idx, d2 = SH.brute_pass(P, Q, T, 0.15)
    assert SH.dot_is_decided(P, Q, T, idx, Np, Nq)
    s0, _ = SH.symm_sums(P, Q, T, idx, d2, Np, Nq)
    rng = np.random.default_rng(2)
    fp = np.where(rng.random(len(P)) < 0.5, -1.0, 1.0).astype(np.float32)[:, None]
    fq = np.where(rng.random(len(Q)) < 0.5, -1.0, 1.0).astype(np.float32)[:, None]
    for a, b in ((Np * fp, Nq), (Np, Nq * fq), (Np * fp, Nq * fq), (-Np, -Nq)):
        assert SH.symm_sums(P, Q, T, idx, d2, a, b)[0].tobytes() == s0.tobytes()


def test_cli_symmetric_metric_parses_and_bad_combinations_exit_with_usage(s4p_lib_built, tmp_path):
    from super4pcs_amd import build as B
    cli = B.build_cli()
    g = ["--icp-metric", "symmetric"]
    for bad in (g + ["--icp-loss", "huber"], g + ["--icp-loss", "trimmed", "--icp-trim", "0.5"], ["--icp-loss", "tukey"] + g,
                g + ["--icp-starts", "4"], g + ["--icp-gicp-epsilon", "0.01"], g + ["--icp-color-lambda", "0.9"],
                ["--icp-metric", "symmetrical"], ["--icp-metric", "symm"], ["--icp-metric"]):
        r = subprocess.run([cli, "-i", "a.obj", "b.obj", "--icp", "30"] + bad, capture_output=True, text=True)
        assert r.returncode == 1 and "Usage:" in r.stderr and "point|plane|gicp|symmetric|color" in r.stderr, (bad, r.returncode, r.stderr)
    for good in (g, g + ["--icp-loss", "none"], g + ["--icp-normal-radius", "0.03", "--estimate-normals", "16"],
                 g + ["--icp-reciprocal", "--icp-normal-angle", "60"], g + ["--icp-scales", "0.2,0"],
                 ["--icp-metric", "gicp"] + g, g + ["--icp-dist", "0.05"]):
        r = subprocess.run([cli, "-i", str(tmp_path / "none1.obj"), str(tmp_path / "none2.obj"), "--icp", "10"] + good,
                           capture_output=True, text=True)
        assert r.returncode == 255 and "Can't read input set1" in r.stderr, (good, r.stderr)
    head = open(os.path.join(ROOT, "demos", "Super4PCS", "super4pcs_cli.cc")).read().split("#include")[0]
    assert "point|plane|gicp|symmetric|color" in head and "s4p_icp_symm.h" in head


@pytest.mark.parametrize("eigen", [False, True])
def test_facade_application_compiles_with_and_without_eigen(icp_lib, tmp_path, eigen):
    """tests/icp_facade_app builds against the facade either way; the symmetric metric with a loss and in a batch is refused
    before a device is asked for."""
    extra = ["-I" + os.path.join(ROOT, "oracle", "eigen_shim")] if eigen else ["-DS4P_NO_EIGEN"]
    probe = tmp_path / "probe.cpp"
    probe.write_text('#include "super4pcs/algorithms/icp.h"\n#ifdef S4P_HAVE_EIGEN\n#error have\n#else\n#error none\n#endif\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include")] + extra + [str(probe)],
                       capture_output=True, text=True)
    assert re.search(r"#error (have|none)", r.stderr).group(1) == ("have" if eigen else "none"), r.stderr
    exe = apps.build_app(tmp_path, "icp_facade_app", apps.ICP_FACADE_LIBS, extra)
    P = np.random.default_rng(1).uniform(size=(8, 3))
    for flags, word in ((("--identity", "--loss", "huber"), "symmetric metric takes no loss"), (("--batch",), "no batch form")):
        r = apps.start_icp_app(exe, P, P, "0.01", "0.7", "8", "--metric", "symmetric", "--max-iterations", "5", *flags)
        # the program prints "invalid: " and exits with 5 for std::invalid_argument alone
        assert r.returncode == 5 and r.stdout.splitlines()[-1].startswith("invalid: ") and word in r.stdout, (flags, r.returncode, r.stdout)


def test_python_argument_checks_need_no_device(icp_lib):
    from super4pcs_amd import multiscale
    P = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match="loss"):
        icp_lib.refine(P, P, max_distance=1.0, metric="symmetric", loss="huber")
    with pytest.raises(ValueError, match="loss"):
        icp_lib.refine(P, P, max_distance=1.0, metric="symmetric", loss="trimmed", trim_fraction=0.5)
    with pytest.raises(ValueError, match="metric"):
        icp_lib.refine(P, P, max_distance=1.0, metric="symm")
    ctx = object.__new__(icp_lib.ICP)                       # no context: the checks come before any library call
    ctx.h = None
    with pytest.raises(ValueError, match="loss"):
        ctx.refine(metric="symmetric", loss="tukey")
    with pytest.raises(ValueError, match="batch"):
        ctx.refine_batch(np.eye(4)[None], metric="symmetric")
    with pytest.raises(ValueError, match="batch"):
        ctx.sums_batch(np.eye(4)[None], metric="symmetric")
    with pytest.raises(ValueError, match="batch"):
        icp_lib.refine_best(P, P, np.eye(4)[None], max_distance=1.0, metric="symmetric")
    with pytest.raises(ValueError, match="starts="):
        multiscale.refine_multiscale(P, P, voxel_sizes=(0,), max_distance=1.0, metric="symmetric", starts=np.eye(4)[None])
    with pytest.raises(ValueError, match="loss"):
        multiscale.refine_multiscale(P, P, voxel_sizes=(0,), max_distance=1.0, metric="symmetric", loss="huber")
    assert icp_lib.REFINE_METRICS == ("point", "plane", "gicp", "symmetric", "color")
    assert icp_lib.REFINE_METRICS[-1] == "color" and icp_lib.METRICS == ("point", "plane")
