"""Coloured ICP (include/s4p_icp_color.h) on the host: exports and binding, the numpy restatement of the joint sums against
the point-to-plane restatement and against numpy's solve, the planar textured case on the CPU loop (the colour term pins
what point-to-plane leaves free), the gate condition on the gradient inputs, the command line's new flags, and the Python
argument checks that need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import icp_color_helpers as CH
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
def cpu(tmp_path_factory):
    return H.build_cpu(tmp_path_factory.mktemp("icp_cpu"))


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(s4p_icp_\w+)\s*\(", txt)))


def test_color_functions_are_exported_and_bound(icp_lib):
    decl = _declared("s4p_icp_color.h")
    assert len(decl) == 8, decl
    assert set(decl) == set(icp_lib.COLOR_SYMBOLS) and len(icp_lib.COLOR_SYMBOLS) == 8
    others = set(icp_lib.SYMBOLS) | set(icp_lib.PLANE_SYMBOLS) | set(icp_lib.ROBUST_SYMBOLS) | set(icp_lib.GICP_SYMBOLS)
    assert not set(decl) & others
    L = ctypes.CDLL(icp_lib.LIB_PATH)
    assert not [s for s in decl if not hasattr(L, s)]
    Lb = icp_lib.load_library()
    for s in decl:
        assert getattr(Lb, s).argtypes is not None
    out = subprocess.run(["nm", "-C", icp_lib.LIB_PATH], capture_output=True, text=True).stdout
    for k in ("k_color_gradient", "k_color_sum", "k_gather_target_intensity", "k_gather_source_intensity"):
        assert re.search(r"s4p_icp::%s\b" % k, out), k
    assert icp_lib.COLOR_LAMBDA == 0.968 and icp_lib.COLOR_NSUMS == icp_lib.PLANE_NSUMS == 31


def _surface(rng, n):
    xy = rng.uniform(-0.5, 0.5, size=(n, 2))
    z = 0.05 * np.sin(6 * xy[:, 0]) * np.cos(5 * xy[:, 1])
    return np.column_stack([xy, z]).astype(np.float32)


def _pair(seed=9, n_p=1200, n_q=700):
    """A small bumpy pair with analytic normals (some zero), restated gradients (some zero) and intensities."""
    rng = np.random.default_rng(seed)
    P = _surface(rng, n_p)
    c = P.mean(0).astype(np.float32)
    Pc = (P - c).astype(np.float32)
    pick = rng.integers(0, len(Pc), n_q)
    Qc = (Pc[pick] + rng.normal(scale=0.01, size=(n_q, 3))).astype(np.float32)
    x, y = P[:, 0].astype(np.float64), P[:, 1].astype(np.float64)
    Np = PH.normalise(np.column_stack([-0.3 * np.cos(6 * x) * np.cos(5 * y), 0.25 * np.sin(6 * x) * np.sin(5 * y), np.ones(n_p)]))
    Np[::7] = 0
    Ip = CH.texture(P, 2.0)
    Iq = (Ip[pick] + rng.normal(scale=0.01, size=n_q)).astype(np.float32)
    G, ratio, k = CH.color_gradients(Pc, Np, Ip, 0.08, 6)
    assert G.any(1).sum() > 0.7 * n_p and (~G.any(1)).sum() >= n_p // 7
    th = np.deg2rad(0.7)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]]
    T[:3, 3] = [0.004, -0.002, 0.001]
    d = 0.03
    idx, d2 = H.numpy_brute(Pc, Qc, T, d)
    assert (idx >= 0).sum() > 300 and (idx < 0).sum() > 0
    return Pc, Qc, T, idx, d2, Np, G, Ip, Iq


def test_restated_sums_at_lambda_one_are_the_plane_sums():
    Pc, Qc, T, idx, d2, Np, G, Ip, Iq = _pair()
    s, sabs = CH.color_sums(Pc, Qc, T, idx, d2, Np, G, Ip, Iq, 1.0)
    ref = PH.plane_sums(Pc, Qc, T, idx, d2, Np)
    assert s[0] == ref[0] and s[2] == ref[2] and 0 < s[2] < s[0]
    assert np.all(np.abs(s - ref) <= 1e-12 * sabs), (s, ref)


@pytest.mark.parametrize("lam", [0.0, 0.5, 0.968])
def test_restated_sums_without_colour_information_are_lambda_times_the_plane_sums(lam):
    """All gradients zero and I_q = I_p: a_C = 0 and r_C = 0, so [3..30] are lambda times point-to-plane's."""
    Pc, Qc, T, idx, d2, Np, G, Ip, Iq = _pair()
    Iq = np.where(idx >= 0, Ip[np.maximum(idx, 0)], Iq).astype(np.float32)
    s, sabs = CH.color_sums(Pc, Qc, T, idx, d2, Np, np.zeros_like(G), Ip, Iq, lam)
    ref = PH.plane_sums(Pc, Qc, T, idx, d2, Np)
    _, ref_abs = CH.color_sums(Pc, Qc, T, idx, d2, Np, np.zeros_like(G), Ip, Iq, 1.0)
    assert np.array_equal(s[:3], ref[:3])
    assert np.all(np.abs(s[3:] - lam * ref[3:]) <= 1e-12 * ref_abs[3:]), (s, ref)


def _rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


@pytest.mark.parametrize("lam", [0.5, 0.968, 1.0])
def test_solve_plane_on_the_restated_sums_equals_numpy(icp_lib, lam):
    Pc, Qc, T, idx, d2, Np, G, Ip, Iq = _pair()
    s, _ = CH.color_sums(Pc, Qc, T, idx, d2, Np, G, Ip, Iq, lam)
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = s[4:25]
    A = A + A.T - np.diag(np.diag(A))
    assert np.all(np.linalg.eigvalsh(A) > 0)
    x = np.linalg.solve(A, s[25:31])
    want = np.eye(4); want[:3, :3] = _rodrigues(x[:3]); want[:3, 3] = x[3:]
    got = icp_lib.solve_plane(s)
    assert np.max(np.abs(got - want)) <= 1e-10 * max(1.0, np.max(np.abs(want))), (got, want)
    # and the restatement's system is the explicit sum over the pairs of the two weighted rank-one terms
    Tf = np.asarray(T, np.float32)
    x_, y_, z_ = Qc[:, 0], Qc[:, 1], Qc[:, 2]
    qh = np.stack([((Tf[r, 0] * x_ + Tf[r, 1] * y_) + Tf[r, 2] * z_) + Tf[r, 3] for r in range(3)], 1).astype(np.float64)
    Ad = np.zeros((6, 6)); bd = np.zeros(6); Aa = np.zeros((6, 6)); ba = np.zeros(6); e = 0.0
    for j in np.flatnonzero(idx >= 0):
        n = Np[idx[j]].astype(np.float64)
        if not n.any():
            continue
        q, p, g = qh[j], Pc[idx[j]].astype(np.float64), G[idx[j]].astype(np.float64)
        r = p - q
        gp = g - (g @ n) * n
        aG = np.concatenate([np.cross(q, n), n]); aC = np.concatenate([np.cross(q, gp), gp])
        sg = r @ n
        rc = (float(Iq[j]) - float(Ip[idx[j]])) + gp @ r                  # g.r - (r.n)(g.n) = g_perp . r
        t = lam * np.outer(aG, aG) + (1 - lam) * np.outer(aC, aC); v = lam * aG * sg + (1 - lam) * aC * rc
        Ad += t; Aa += np.abs(lam * np.outer(aG, aG)) + np.abs((1 - lam) * np.outer(aC, aC))
        bd += v; ba += np.abs(lam * aG * sg) + np.abs((1 - lam) * aC * rc)
        e += lam * sg * sg + (1 - lam) * rc * rc
    iu = np.triu_indices(6)
    assert np.all(np.abs(s[4:25] - Ad[iu]) <= 1e-12 * np.maximum(Aa[iu], 1e-300))
    assert np.all(np.abs(s[25:31] - bd) <= 1e-11 * np.maximum(ba, 1e-300))
    assert abs(s[3] - e) <= 1e-11 * e


def _planar_setup():
    c = CH.planar_case()
    ctr = c["P"].astype(np.float64).mean(0).astype(np.float32)
    Pc, Qc = (c["P"] - ctr).astype(np.float32), (c["Q"] - ctr).astype(np.float32)
    G, ratio, k = CH.color_gradients(Pc, c["N"], c["Ip"], c["r"], 6)
    return c, ctr, Pc, Qc, G, ratio, k


def test_planar_gradients_are_well_conditioned_and_away_from_the_gate():
    """The condition on the inputs of the gradient tests: no target point's lambda_min / lambda_max lies in
    [0.5e-6, 2e-6], so the zero pattern cannot flip between device and restatement.  With the trace weight on the normal
    row the healthy neighbourhoods of the plane sit far above the gate."""
    c, ctr, Pc, Qc, G, ratio, k = _planar_setup()
    print("planar: k in [%d, %d] (mean %.1f), lambda_min / lambda_max >= %.3g, %d zero gradients"
          % (k.min(), k.max(), k.mean(), np.nanmin(ratio), (~G.any(1)).sum()))
    assert not np.any((ratio >= 0.5e-6) & (ratio <= 2e-6))
    assert np.nanmin(ratio) > 0.05 and k.min() >= 6 and G.any(1).all()
    assert np.max(np.abs(G[:, 2])) == 0.0                       # in the tangent plane z = 0, exactly: u_z = 0 for every neighbour


@pytest.mark.parametrize("lam", [0.968, 0.5])
def test_cpu_loop_recovers_the_planar_pose_where_plane_is_degenerate(icp_lib, cpu, lam):
    c, ctr, Pc, Qc, G, ratio, k = _planar_setup()
    T0 = np.eye(4)
    start = np.max(np.abs(T0 - c["T_true"]))
    T, its, status, hist = CH.cpu_refine_color(cpu, icp_lib.solve_plane, Pc, Qc, c["N"], G, c["Ip"], c["Iq"], ctr, T0, c["d"], lam=lam)
    err = np.max(np.abs(T - c["T_true"]))
    print("planar, lambda %g: |T0 - T_true| %.2g -> %.2g in %d iterations (%s); rmse %s"
          % (lam, start, err, its, icp_lib.STATUS_NAMES[status], ["%.2g" % h for h in hist[:4]]))
    assert start > 1e-2 and err <= 1e-5
    Tp, its_p, status_p, _ = PH.cpu_refine_plane(cpu, icp_lib.solve_plane, Pc, Qc, c["N"], ctr, T0, c["d"])
    assert status_p == icp_lib.DEGENERATE and its_p == 0 and np.array_equal(Tp, T0)
    # lambda = 1 is point-to-plane: the same three free directions
    _, its_1, status_1, _ = CH.cpu_refine_color(cpu, icp_lib.solve_plane, Pc, Qc, c["N"], G, c["Ip"], c["Iq"], ctr, T0, c["d"], lam=1.0)
    assert status_1 == icp_lib.DEGENERATE and its_1 == 0


def test_rgb_to_intensity_is_the_facades_formula(icp_lib):
    rng = np.random.default_rng(1)
    rgb = rng.integers(0, 256, size=(1000, 3))
    want = np.array([np.float32(((float(r) + float(g)) + float(b)) / 765.0) for r, g, b in rgb], np.float32)
    for arr in (rgb, rgb.astype(np.uint8), rgb.astype(np.float32)):
        got = icp_lib.rgb_to_intensity(arr)
        assert got.dtype == np.float32 and np.array_equal(got, want)
    assert icp_lib.rgb_to_intensity(np.array([[255, 255, 255], [0, 0, 0]]))[0] == 1.0
    with pytest.raises(ValueError):
        icp_lib.rgb_to_intensity(np.zeros((4, 2)))


def test_cli_color_flags_parse_and_bad_values_exit_with_usage(s4p_lib_built, tmp_path):
    from super4pcs_amd import build as B
    cli = B.build_cli()
    g = ["--icp-metric", "color"]
    for bad in (g + ["--icp-color-lambda", "-0.1"], g + ["--icp-color-lambda", "1.01"], g + ["--icp-color-lambda", "nan"],
                g + ["--icp-color-lambda", "inf"], g + ["--icp-color-lambda", "0.5x"], g + ["--icp-color-lambda", ""],
                ["--icp-color-lambda", "0.5"], ["--icp-metric", "plane", "--icp-color-lambda", "0.5"],
                ["--icp-metric", "gicp", "--icp-color-lambda", "0.5"], ["--icp-metric", "colour"],
                g + ["--icp-metric", "point", "--icp-color-lambda", "0.5"],
                g + ["--icp-loss", "huber"], g + ["--icp-loss", "trimmed", "--icp-trim", "0.5"], ["--icp-loss", "tukey"] + g,
                g + ["--icp-gicp-epsilon", "0.01"]):
        r = subprocess.run([cli, "-i", "a.obj", "b.obj", "--icp", "30"] + bad, capture_output=True, text=True)
        assert r.returncode == 1 and "Usage:" in r.stderr and "--icp-color-lambda" in r.stderr, (bad, r.returncode, r.stderr)
    for good in (g, g + ["--icp-color-lambda", "0.5"], g + ["--icp-color-lambda", "0"], g + ["--icp-color-lambda", "1"],
                 g + ["--icp-loss", "none"], g + ["--icp-normal-radius", "0.03", "--estimate-normals", "16"],
                 ["--icp-metric", "gicp"] + g + ["--icp-color-lambda", "0.9"]):
        r = subprocess.run([cli, "-i", str(tmp_path / "none1.obj"), str(tmp_path / "none2.obj"), "--icp", "30"] + good,
                           capture_output=True, text=True)
        assert r.returncode == 255 and "Can't read input set1" in r.stderr, (good, r.stderr)


def test_python_argument_checks_need_no_device(icp_lib):
    P = np.zeros((4, 3), np.float32)
    I = np.zeros(4, np.float32)
    with pytest.raises(ValueError, match="loss"):
        icp_lib.refine(P, P, max_distance=1.0, metric="color", target_intensity=I, source_intensity=I, loss="huber")
    with pytest.raises(ValueError, match="loss"):
        icp_lib.refine(P, P, max_distance=1.0, metric="color", target_intensity=I, source_intensity=I, loss="trimmed", trim_fraction=0.5)
    with pytest.raises(ValueError, match="intensity"):
        icp_lib.refine(P, P, max_distance=1.0, metric="color")
    with pytest.raises(ValueError, match="intensity"):
        icp_lib.refine(P, P, max_distance=1.0, metric="color", target_intensity=I)
    with pytest.raises(ValueError, match="intensity"):
        icp_lib.refine(P, P, max_distance=1.0, metric="color", source_intensity=I)
    with pytest.raises(ValueError, match="color"):
        icp_lib.refine(P, P, max_distance=1.0, metric="plane", target_intensity=I, source_intensity=I)
    with pytest.raises(ValueError):
        icp_lib.refine(P, P, max_distance=1.0, metric="color", target_intensity=np.zeros((4, 2)), source_intensity=I)
    with pytest.raises(ValueError, match="metric"):
        icp_lib.refine(P, P, max_distance=1.0, metric="colour")
    ctx = object.__new__(icp_lib.ICP)                       # no context: the checks come before any library call
    ctx.h = None
    with pytest.raises(ValueError, match="loss"):
        ctx.refine(metric="color", loss="tukey")
    assert icp_lib.REFINE_METRICS[-1] == "color" and icp_lib.METRICS == ("point", "plane")
    assert "gicp" in icp_lib.REFINE_METRICS
