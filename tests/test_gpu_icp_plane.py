"""Point-to-plane ICP on the MI355X (include/s4p_icp_plane.h): estimated normals against the CPU restatement
(tests/icp_plane_cpu), plane sums against the numpy restatement, determinism, convergence to an exact pose in fewer
iterations than point-to-point, the trajectory against the CPU loop, a degenerate planar target, refinement after a
registration, and the facade / command line / Python binding agreeing."""
import os

import numpy as np
import pytest

from tests import apps
from tests import icp_helpers as H
from tests import icp_plane_helpers as PH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
MIN_NB = 6


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
def pcpu(tmp_path_factory):
    return PH.build_plane_cpu(tmp_path_factory.mktemp("icp_plane_cpu"))


@pytest.fixture(scope="module")
def bumpy():
    from super4pcs_amd import datasets as D
    return D.bumpy_pair(200_000, overlap=0.5, delta=0.004, seed=11)


@pytest.fixture(scope="module")
def lidar():
    from super4pcs_amd import datasets as D
    return D.lidar_pair_scaled(0.02, delta=0.05)


def _check_normals(ctx, pcpu, P, r):
    c = ctx.frame()
    Pc = (P - c).astype(np.float32)
    ctx.estimate_normals(r, MIN_NB)
    G = ctx.target_normals()
    k, c6 = pcpu.cov(Pc, r)
    N, w = PH.normals_from_cov(k, c6, MIN_NB)
    zero_g, zero_c = ~G.any(1), ~N.any(1)
    assert np.array_equal(zero_g, zero_c) and np.array_equal(zero_c, k < MIN_NB)
    sep = (w[:, 1] >= 4 * w[:, 0]) & ~zero_c
    dots = np.abs((G[sep].astype(np.float64) * N[sep].astype(np.float64)).sum(1))
    print("normals: n %d, separated %d, zero %d, min |dot| %.9f" % (len(P), sep.sum(), zero_c.sum(), dots.min()))
    assert sep.sum() > 0.1 * len(P) and dots.min() >= 1 - 1e-6
    assert np.all(np.abs(np.linalg.norm(G[~zero_g].astype(np.float64), axis=1) - 1) < 1e-6)
    ctx.estimate_normals(r, MIN_NB)
    assert np.array_equal(ctx.target_normals(), G)                 # two calls, identical bits
    return G


def test_estimated_normals_are_the_contract(icp, pcpu, bumpy, lidar):
    """1: against the CPU restatement on the bumpy and the lidar pair (|dot| >= 1 - 1e-6 where the two smallest eigenvalues
    differ by 4x; zeros in the same places); on a sphere within 1 degree of the analytic normal; deterministic."""
    for (P, _, _), d in ((bumpy, 4 * 0.004), (lidar, 4 * 0.05)):
        ctx = icp.ICP(0)
        ctx.set_target(P, d)
        _check_normals(ctx, pcpu, P, d)
        with pytest.raises(icp.ICPError) as e:
            ctx.estimate_normals(d * 1.01, MIN_NB)                  # radius above max_distance
        assert e.value.code == -1
        with pytest.raises(icp.ICPError):
            ctx.estimate_normals(d, 2)
        ctx.close()
    rng = np.random.default_rng(2)
    u = rng.normal(size=(200_000, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    ctx = icp.ICP(0)
    ctx.set_target(u.astype(np.float32), 0.05)
    G = _check_normals(ctx, pcpu, u.astype(np.float32), 0.05)
    ang = np.degrees(np.arccos(np.clip(np.abs((G.astype(np.float64) * u).sum(1)), 0, 1)))
    print("sphere: max angle to the analytic normal %.3f deg" % ang.max())
    assert ang.max() < 1.0
    ctx.close()


def _check_plane_sums(ctx, cpu, P, Q, N, T_caller, d):
    c = ctx.frame()
    Pc, Qc = (P - c).astype(np.float32), (Q - c).astype(np.float32)
    Tc = H.to_centred(T_caller, c).astype(np.float32)
    gi, gd = ctx.correspondences(Tc)
    ci, cd, _ = cpu.pass_(Pc, Qc, Tc, d)
    assert np.array_equal(gi, ci) and np.array_equal(gd, cd)
    gs = ctx.plane_sums(Tc)
    cs = PH.plane_sums(Pc, Qc, Tc, ci, cd, N)
    assert gs[0] == cs[0] and gs[2] == cs[2]
    R = float(np.max(np.abs(Pc)))
    # relative 1e-10 against each sum's scale: a carries one length in its rotation half, r one length
    w = np.array([R, R, R, 1.0, 1.0, 1.0])
    tri = np.outer(w, w)[np.triu_indices(6)]
    scale = np.maximum(np.abs(cs), np.concatenate([[cs[0], abs(cs[1]), cs[0], abs(cs[3])], cs[2] * tri, cs[2] * w * R]))
    assert np.all(np.abs(gs - cs) <= 1e-10 * scale), (gs, cs)
    return int(gs[2])


def test_plane_sums_are_the_contract(icp, cpu, bumpy, lidar):
    """2: correspondences bit for bit, n and n_plane exactly, the rest to relative 1e-10; caller normals (some zero, not
    unit length) and estimated normals; several transforms around the generator's pose."""
    rng = np.random.default_rng(4)
    for (P, Q, T_gt), d in ((bumpy, 4 * 0.004), (lidar, 4 * 0.05)):
        ctx = icp.ICP(0)
        ctx.set_target(P, d)
        ctx.set_source(Q)
        with pytest.raises(icp.ICPError) as e:
            ctx.plane_sums(np.eye(4))
        assert e.value.code == -7                                    # no normals yet
        raw = rng.normal(size=P.shape).astype(np.float32) * 3
        raw[::11] = 0
        raw[5, 0] = np.nan
        ctx.set_target_normals(raw)
        Nu = PH.normalise(raw)
        assert np.array_equal(ctx.target_normals(), Nu)
        for ang, sh in ((0.0, 0.0), (0.3, 0.002), (-1.0, 0.01)):
            assert _check_plane_sums(ctx, cpu, P, Q, Nu, H.motion(ang, sh) @ T_gt, d) > 1000
        ctx.estimate_normals(d, MIN_NB)
        Ne = ctx.target_normals()
        for ang, sh in ((0.0, 0.0), (0.5, -0.004), (2.0, -0.02)):
            assert _check_plane_sums(ctx, cpu, P, Q, Ne, H.motion(ang, sh) @ T_gt, d) > 1000
        ctx.set_target(P, d)                                          # set_target invalidates the normals
        with pytest.raises(icp.ICPError) as e:
            ctx.refine(T_gt, metric="plane")
        assert e.value.code == -7
        ctx.close()


def _exact_pose_setup(bumpy):
    P = bumpy[0]
    rng = np.random.default_rng(5)
    sub = P[np.sort(rng.choice(len(P), 100_000, replace=False))].astype(np.float64)
    extent = float(np.linalg.norm(P.max(0) - P.min(0)))
    M = H.motion(2.0, 0.01 * extent * np.array([0.6, -0.8, 0.0]))
    Q = (sub @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
    return P, Q, np.linalg.inv(M), extent


def test_plane_refine_is_deterministic_and_torch_agrees(icp, bumpy):
    """3: two calls give identical bits; numpy and torch device inputs (clouds and normals) too."""
    import torch
    P, Q, T_true, extent = _exact_pose_setup(bumpy)
    d = 0.05 * extent
    ctx = icp.ICP(0)
    ctx.set_target(P, d)
    ctx.set_source(Q)
    ctx.estimate_normals(d)
    T1, r1 = ctx.refine(np.eye(4), metric="plane")
    T2, r2 = ctx.refine(np.eye(4), metric="plane")
    assert np.array_equal(T1, T2) and bytes(r1) == bytes(r2)
    N = ctx.target_normals()
    dev = torch.device("cuda:0")
    ctx2 = icp.ICP(0)
    ctx2.set_target(torch.from_numpy(P).to(dev), d)
    ctx2.set_source(torch.from_numpy(Q).to(dev))
    ctx2.estimate_normals(d)
    assert np.array_equal(ctx2.target_normals(), N)
    T3, r3 = ctx2.refine(np.eye(4), metric="plane")
    assert np.array_equal(T3, T1) and bytes(r3) == bytes(r1)
    raw = (N * 2.5).astype(np.float32)
    ctx.set_target_normals(raw)
    ctx2.set_target_normals(torch.from_numpy(raw).to(dev))
    assert np.array_equal(ctx2.target_normals(), ctx.target_normals())
    T4, r4 = ctx.refine(np.eye(4), metric="plane")
    T5, r5 = ctx2.refine(np.eye(4), metric="plane")
    assert np.array_equal(T4, T5) and bytes(r4) == bytes(r5)


def _first_below(hist, thr):
    for k, v in enumerate(hist):
        if v <= thr:
            return k
    return None


def test_plane_refine_reaches_an_exact_pose_in_fewer_iterations(icp, bumpy):
    """4: a 100 k subset of P moved by 2 degrees and 1 % of the extent: point-to-plane with estimated normals comes back to
    1e-5, and its rmse history falls below 1e-6 of the extent in fewer iterations than point-to-point's."""
    P, Q, T_true, extent = _exact_pose_setup(bumpy)
    d = 0.05 * extent
    ctx = icp.ICP(0)
    ctx.set_target(P, d)
    ctx.set_source(Q)
    ctx.estimate_normals(d)
    Tl, rl = ctx.refine(np.eye(4), max_iterations=64, rel_tol=0.0, metric="plane")
    Tp, rp = ctx.refine(np.eye(4), max_iterations=64, rel_tol=0.0)
    thr = 1e-6 * extent
    kl, kp = _first_below(rl.as_dict()["history_rmse"], thr), _first_below(rp.as_dict()["history_rmse"], thr)
    print("exact pose: rmse <= 1e-6 extent after %s plane / %s point iterations; |T - T_true| plane %.2g point %.2g"
          % (kl, kp, np.max(np.abs(Tl - T_true)), np.max(np.abs(Tp - T_true))))
    assert np.max(np.abs(Tl - T_true)) <= 1e-5 and rl.fitness == 1.0
    assert kl is not None and (kp is None or kl < kp)


def test_plane_refine_trajectory_equals_the_cpu_loop(icp, cpu, bumpy):
    """5: the CPU restatement of the plane sums plus s4p_icp_solve_plane, from 1.5 degrees off the generator's pose."""
    P, Q, T_gt = bumpy
    d = 4 * 0.004
    T0 = H.motion(1.5, 0.004) @ T_gt
    ctx = icp.ICP(0)
    ctx.set_target(P, d)
    ctx.set_source(Q)
    ctx.estimate_normals(d)
    T, r = ctx.refine(T0, metric="plane")
    c = ctx.frame()
    Tc, its, status, hist = PH.cpu_refine_plane(cpu, icp.solve_plane, (P - c).astype(np.float32), (Q - c).astype(np.float32),
                                                ctx.target_normals(), c, T0, d)
    print("plane trajectory: gpu %d its (%s) rmse %.6g; cpu %d its (%s) |dT| %.2g; rot err %.4g -> %.4g deg"
          % (r.iterations, icp.STATUS_NAMES[r.status], r.rmse, its, icp.STATUS_NAMES[status], np.max(np.abs(T - Tc)),
             H.rot_err_deg(T0, T_gt), H.rot_err_deg(T, T_gt)))
    assert np.max(np.abs(T - Tc)) <= 1e-5
    assert abs(r.iterations - its) <= 1 and r.status == status
    k = min(r.history_len, len(hist), 3)
    assert np.allclose(list(r.history_rmse[:k]), hist[:k], rtol=1e-9)


def test_planar_target_is_degenerate(icp):
    """6: z = 0: rotation about z and sliding in the plane are unobservable; the refine stops at T0 with DEGENERATE."""
    rng = np.random.default_rng(8)
    P = np.column_stack([rng.uniform(-1, 1, (50_000, 2)), np.zeros(50_000)]).astype(np.float32)
    Q = P[rng.choice(len(P), 20_000, replace=False)] + np.array([0, 0, 0.01], np.float32)
    T0 = H.motion(0.5, np.array([0.01, -0.02, 0.0]), axis=(0, 0, 1))
    ctx = icp.ICP(0)
    ctx.set_target(P, 0.08)
    ctx.set_source(Q)
    ctx.estimate_normals(0.08)
    N = ctx.target_normals()
    assert np.array_equal(N, np.tile(np.array([0, 0, 1], np.float32), (len(P), 1)))
    s = ctx.plane_sums(H.to_centred(T0, ctx.frame()).astype(np.float32))
    assert s[2] > 10_000
    T, r = ctx.refine(T0, metric="plane")
    print("planar target: status %s, iterations %d" % (icp.STATUS_NAMES[r.status], r.iterations))
    assert r.status == icp.DEGENERATE and r.iterations == 0
    assert np.array_equal(T, T0)


def _register(P, Q, delta, overlap, n_s):
    from super4pcs_amd import capi
    gm = capi.Matcher(capi.make_options(delta, overlap, n_s), device=0)
    _lcp, M, Qm = gm.compute_transformation(P, Q)
    gm.close()
    return M.astype(np.float64), Qm


def test_plane_refinement_after_registration_is_closer_to_the_generator(icp):
    """7: configs[2] (bumpy 1 M, sample 2000): Super4PCS pose, then point-to-plane on the full clouds."""
    from super4pcs_amd import datasets as D
    delta = 0.004
    P, Q, T_gt = D.bumpy_pair(1_000_000, overlap=0.5, delta=delta, seed=20140814)
    M, Qm = _register(P, Q, delta, 0.5, 2000)
    dT, r = icp.refine(P, Qm, np.eye(4), max_distance=4 * delta, metric="plane")
    Mr = icp.compose(dT, M)
    e0 = (H.rot_err_deg(M, T_gt), float(np.linalg.norm(M[:3, 3] - T_gt[:3, 3])))
    e1 = (H.rot_err_deg(Mr, T_gt), float(np.linalg.norm(Mr[:3, 3] - T_gt[:3, 3])))
    print("configs[2] plane: Super4PCS rot %.4g deg trans %.4g -> rot %.4g deg trans %.4g (%d its, %s, rmse %.4g, fitness %.3f)"
          % (e0[0], e0[1], e1[0], e1[1], r.iterations, icp.STATUS_NAMES[r.status], r.rmse, r.fitness))
    assert e1[0] < e0[0] and e1[1] < e0[1]


def test_facade_cli_and_binding_agree_on_the_hippo(icp, tmp_path, s4p_lib_built):
    """8: the hippo fixture through MatchSuper4PCS + RefineICP(PointToPlane) (tests/icp_facade_app), through
    `Super4PCS ... --icp 30 --icp-metric plane -m`, and through icp.py from the same Super4PCS result; then the facade
    with P's own normals against set_target_normals."""
    from super4pcs_amd import build as B
    g = np.load(os.path.join(ROOT, "tests", "golden", "hippo_config1.npz"))
    Ps, Qu = g["Ps"].astype(np.float32), g["Qu"].astype(np.float32)
    delta, overlap, n_s = 0.01, 0.7, 200
    exe = apps.build_app(tmp_path, "icp_facade_app", apps.ICP_FACADE_LIBS)

    def app(p_rows):
        return apps.run_icp_app(exe, p_rows, Qu, delta, overlap, n_s, "--metric", "plane")[0]

    rows = app(Ps)
    M, Mf = rows["registered"].astype(np.float64), rows["registered"]
    Qm = apps.move_f32(Mf, Qu)
    ctx = icp.ICP(0)
    ctx.set_target(Ps, np.float32(4.0 * delta))
    ctx.set_source(Qm)
    ctx.estimate_normals(np.float32(4.0 * delta))
    dT, r = ctx.refine(np.eye(4), metric="plane")
    want = icp.compose(dT, M).astype(np.float32)
    print("hippo plane: facade == icp.py max diff %.2g, %d iterations (%s), rmse %.4g"
          % (np.max(np.abs(rows["refined"] - want)), r.iterations, icp.STATUS_NAMES[r.status], r.rmse))
    assert np.max(np.abs(rows["refined"] - want)) <= 1e-6
    assert np.max(np.abs(rows["refined"] - Mf)) > 0
    # command line
    cli = B.build_cli()
    apps.write_obj(tmp_path / "P.obj", Ps); apps.write_obj(tmp_path / "Q.obj", Qu)
    got, _ = apps.run_cli(cli, tmp_path / "P.obj", tmp_path / "Q.obj", delta, overlap, n_s, ["--icp", "30", "--icp-metric", "plane"])
    assert np.max(np.abs(got - want)) <= 2e-6
    # the facade with P's own (nonzero) normals uploads them
    N = ctx.target_normals()
    N[~N.any(1)] = np.array([0, 0, 1], np.float32)
    rows2 = app(np.column_stack([Ps, N]))
    assert np.array_equal(rows2["registered"], rows["registered"])
    ctx.set_target_normals(N)
    dT2, _ = ctx.refine(np.eye(4), metric="plane")
    want2 = icp.compose(dT2, M).astype(np.float32)
    assert np.max(np.abs(rows2["refined"] - want2)) <= 1e-6
