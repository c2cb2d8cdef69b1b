"""ICP refinement on the MI355X (libsuper4pcs_icp.so): correspondences bit-exact against the CPU restatement
(tests/icp_cpu/icp_cpu.cpp), sums, determinism, convergence to an exact pose, the refine trajectory against the CPU loop,
refinement after a registration on the full clouds, and the facade / command line / torch entry points."""
import os
import time

import numpy as np
import pytest

from tests import apps
from tests import icp_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def icp(s4p_lib_built):
    from super4pcs_amd import build as B
    B.build_icp()
    from super4pcs_amd import icp as I
    return I


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return H.build_cpu(tmp_path_factory.mktemp("icp_cpu"))


@pytest.fixture(scope="module")
def bumpy():
    from super4pcs_amd import datasets as D
    P, Q, T = D.bumpy_pair(200_000, overlap=0.5, delta=0.004, seed=11)
    return P, Q, T


@pytest.fixture(scope="module")
def lidar():
    from super4pcs_amd import datasets as D
    P, Q, T = D.lidar_pair_scaled(0.02, delta=0.05)
    return P, Q, T


def _check_pass(ctx, cpu, P, Q, T_caller, d):
    c = ctx.frame()
    Pc, Qc = (P - c).astype(np.float32), (Q - c).astype(np.float32)
    Tc = H.to_centred(T_caller, c).astype(np.float32)
    gi, gd = ctx.correspondences(Tc)
    ci, cd, cs = cpu.pass_(Pc, Qc, Tc, d)
    assert np.array_equal(gi, ci) and np.array_equal(gd, cd)
    gs = ctx.sums(Tc)
    assert gs[0] == cs[0] == np.count_nonzero(ci >= 0)
    # relative 1e-10 against each sum's scale (the centred first moments cancel: their scale is n times the extent)
    R = float(np.max(np.abs(Pc)))
    scale = np.maximum(np.abs(cs), np.array([cs[0]] + [cs[0] * R] * 6 + [cs[0] * R * R] * 9 + [abs(cs[16])]))
    assert np.all(np.abs(gs - cs) <= 1e-10 * scale), (gs, cs)
    return int(gs[0])


def test_correspondences_and_sums_are_the_contract(icp, cpu, bumpy, lidar):
    """1 + 2: idx and d2 equal the CPU restatement bit for bit, the sums to relative 1e-10, n exactly -- two pairs, several
    transforms around the generator's pose, target duplicates (ties)."""
    rng = np.random.default_rng(4)
    for (P, Q, T_gt), d in ((bumpy, 4 * 0.004), (lidar, 4 * 0.05)):
        P = np.concatenate([P, P[rng.integers(0, len(P), 5000)]])                    # duplicates: ties by construction
        ctx = icp.ICP(0)
        ctx.set_target(P, d)
        ctx.set_source(Q)
        for k, (ang, sh) in enumerate(((0.0, 0.0), (0.3, 0.002), (-1.0, 0.01), (2.0, -0.02))):
            n = _check_pass(ctx, cpu, P, Q, H.motion(ang, sh) @ T_gt, d)
            assert n > 1000, (k, n)
        ctx.close()


def test_correspondences_at_exactly_d_and_ties_on_a_dyadic_cloud(icp, cpu):
    """Coordinates on a 2^-10 lattice, P symmetric about 0: the frame is exactly 0, so source points can be put exactly at d
    (2^-6) and one float step beyond it; duplicated and lattice-equidistant targets tie."""
    rng = np.random.default_rng(7)
    A = rng.integers(-512, 512, size=(20000, 3)).astype(np.float32) / 1024
    P = np.concatenate([A, -A, A[:3000], -A[:3000]])
    d = np.float32(2.0 ** -6)
    Q = P[rng.integers(0, len(A), 30000)].copy()
    Q[:5000, 0] += d
    Q[5000:10000, 1] = np.nextafter(Q[5000:10000, 1] + d, np.float32(np.inf))
    Q[10000:] += rng.integers(-16, 17, size=(20000, 3)).astype(np.float32) / 1024
    ctx = icp.ICP(0)
    ctx.set_target(P, float(d))
    ctx.set_source(Q)
    assert np.array_equal(ctx.frame(), np.zeros(3, np.float32))
    gi, gd = ctx.correspondences(np.eye(4, dtype=np.float32))
    ii, dd = cpu.brute(P, Q, np.eye(4), float(d))
    assert np.array_equal(gi, ii) and np.array_equal(gd, dd)
    assert np.any(gd == d * d) and np.count_nonzero(gi >= 0) < len(Q)
    _check_pass(ctx, cpu, P, Q, np.eye(4), float(d))


def test_refine_is_deterministic_and_converges_to_an_exact_pose(icp, bumpy):
    """3 + 4: two calls give identical bits; Q = a 100 k subset of P moved by 2 degrees and 1 % of the extent is brought
    back to 1e-5; started at the exact pose, T stays put."""
    P = bumpy[0]
    rng = np.random.default_rng(5)
    sub = P[np.sort(rng.choice(len(P), 100_000, replace=False))].astype(np.float64)
    extent = float(np.linalg.norm(P.max(0) - P.min(0)))
    M = H.motion(2.0, 0.01 * extent * np.array([0.6, -0.8, 0.0]))
    Q = (sub @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
    T_true = np.linalg.inv(M)
    ctx = icp.ICP(0)
    ctx.set_target(P, 0.05 * extent)
    ctx.set_source(Q)
    T1, r1 = ctx.refine(np.eye(4), max_iterations=64, rel_tol=0.0)
    T2, r2 = ctx.refine(np.eye(4), max_iterations=64, rel_tol=0.0)
    assert np.array_equal(T1, T2) and bytes(r1) == bytes(r2)
    print("exact-pose refine: iterations %d rmse %.3g fitness %.4f  |T - T_true| %.2g" % (r1.iterations, r1.rmse, r1.fitness,
                                                                                         np.max(np.abs(T1 - T_true))))
    assert np.max(np.abs(T1 - T_true)) <= 1e-5 and r1.rmse < 1e-5 * extent and r1.fitness == 1.0
    T3, r3 = ctx.refine(T_true, max_iterations=30)
    assert np.max(np.abs(T3 - T_true)) <= 1e-6


def test_refine_trajectory_equals_the_cpu_loop(icp, cpu, bumpy):
    """5: the CPU restatement plus s4p_icp_solve, from a start 1.5 degrees off the generator's pose."""
    P, Q, T_gt = bumpy
    d = 4 * 0.004
    T0 = H.motion(1.5, 0.004) @ T_gt
    ctx = icp.ICP(0)
    ctx.set_target(P, d)
    ctx.set_source(Q)
    T, r = ctx.refine(T0)
    c = ctx.frame()
    Tc, its, status, hist = H.cpu_refine(cpu, icp.solve, (P - c).astype(np.float32), (Q - c).astype(np.float32), c, T0, d)
    print("trajectory: gpu %d its (%s) rmse %.6g; cpu %d its (%s) |dT| %.2g" % (r.iterations, icp.STATUS_NAMES[r.status], r.rmse, its,
                                                                                icp.STATUS_NAMES[status], np.max(np.abs(T - Tc))))
    assert np.max(np.abs(T - Tc)) <= 1e-5
    assert abs(r.iterations - its) <= 1 and r.status == status
    assert np.allclose(list(r.history_rmse[:min(r.history_len, len(hist), 3)]), hist[:min(r.history_len, len(hist), 3)], rtol=1e-9)


def _register(P, Q, delta, overlap, n_s):
    from super4pcs_amd import capi
    gm = capi.Matcher(capi.make_options(delta, overlap, n_s), device=0)
    _lcp, M, Qm = gm.compute_transformation(P, Q)
    gm.close()
    return M.astype(np.float64), Qm


@pytest.mark.parametrize("which", ["bumpy_1m", "lidar"])
def test_refinement_after_registration_is_closer_to_the_generator(icp, which, lidar):
    """6: Super4PCS pose, then refinement on the full clouds: rotation and translation error strictly below."""
    from super4pcs_amd import datasets as D
    if which == "bumpy_1m":                                      # configs[2] (bench.py's pair), sample 2000
        delta = 0.004
        P, Q, T_gt = D.bumpy_pair(1_000_000, overlap=0.5, delta=delta, seed=20140814)
        M, Qm = _register(P, Q, delta, 0.5, 2000)
    else:
        delta = 0.05
        P, Q, T_gt = lidar
        M, Qm = _register(P, Q, delta, 0.4, 400)
    t0 = time.perf_counter()
    dT, r = icp.refine(P, Qm, np.eye(4), max_distance=4 * delta)
    secs = time.perf_counter() - t0
    Mr = icp.compose(dT, M)
    e0 = (H.rot_err_deg(M, T_gt), float(np.linalg.norm(M[:3, 3] - T_gt[:3, 3])))
    e1 = (H.rot_err_deg(Mr, T_gt), float(np.linalg.norm(Mr[:3, 3] - T_gt[:3, 3])))
    print("%s: n_P %d n_Q %d  Super4PCS rot %.4g deg trans %.4g -> ICP rot %.4g deg trans %.4g (%d its, %s, rmse %.4g, fitness %.3f, %.3f s)"
          % (which, len(P), len(Q), e0[0], e0[1], e1[0], e1[1], r.iterations, icp.STATUS_NAMES[r.status], r.rmse, r.fitness, secs))
    assert e1[0] < e0[0] and e1[1] < e0[1]


def test_facade_cli_and_torch_agree_with_the_python_binding(icp, tmp_path, s4p_lib_built):
    """7: the hippo fixture through MatchSuper4PCS + RefineICP (tests/icp_facade_app), through `Super4PCS ... --icp 30 -m`, and
    through icp.py from the same Super4PCS result; then torch device tensors against numpy input."""
    import torch
    from super4pcs_amd import build as B
    g = np.load(os.path.join(ROOT, "tests", "golden", "hippo_config1.npz"))
    Ps, Qu = g["Ps"].astype(np.float32), g["Qu"].astype(np.float32)
    delta, overlap, n_s = 0.01, 0.7, 200
    # facade application: MatchSuper4PCS + RefineICP
    exe = apps.build_app(tmp_path, "icp_facade_app", apps.ICP_FACADE_LIBS)
    rows, _ = apps.run_icp_app(exe, Ps, Qu, delta, overlap, n_s)
    # icp.py from the same Super4PCS result: Q moved by it in k_apply's order
    M = rows["registered"].astype(np.float64)
    Mf = rows["registered"]
    Qm = apps.move_f32(Mf, Qu)
    ctx = icp.ICP(0)
    ctx.set_target(Ps, np.float32(4.0 * delta))
    ctx.set_source(Qm)
    dT, r = ctx.refine(np.eye(4))
    want = icp.compose(dT, M).astype(np.float32)
    print("hippo: facade refined == icp.py bit for bit: %s (max diff %.2g), %d iterations, rmse %.4g"
          % (np.array_equal(rows["refined"], want), np.max(np.abs(rows["refined"] - want)), r.iterations, r.rmse))
    assert np.max(np.abs(rows["refined"] - want)) <= 1e-6
    assert np.max(np.abs(rows["refined"] - Mf)) > 0               # the refinement moved the pose
    # command line
    cli = B.build_cli()
    apps.write_obj(tmp_path / "P.obj", Ps); apps.write_obj(tmp_path / "Q.obj", Qu)
    got, said = apps.run_cli(cli, tmp_path / "P.obj", tmp_path / "Q.obj", delta, overlap, n_s, ["--icp", "30"])
    assert "ICP: " in said
    assert np.max(np.abs(got - want)) <= 2e-6
    # torch device tensors: the same bits as numpy input
    dev = torch.device("cuda:0")
    ctx2 = icp.ICP(0)
    ctx2.set_target(torch.from_numpy(Ps).to(dev), np.float32(4.0 * delta))
    ctx2.set_source(torch.from_numpy(np.ascontiguousarray(Qm)).to(dev))
    dT2, r2 = ctx2.refine(np.eye(4))
    assert np.array_equal(dT2, dT) and bytes(r2) == bytes(r)
    assert np.array_equal(ctx2.frame(), ctx.frame())
    # apply: k_apply's rounding order
    Qa = ctx.apply(dT, Qm)
    exp = apps.move_f32(dT.astype(np.float32), Qm)
    assert np.array_equal(Qa, exp)
