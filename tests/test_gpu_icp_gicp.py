"""Generalized ICP on the MI355X (include/s4p_icp_gicp.h): the generalized sums against the numpy restatement
(tests/icp_gicp_helpers.py), state and argument errors, determinism, the trajectory against the CPU loop, an exact pose, a
planar target at the smallest epsilon, the facade / command line / Python binding agreeing, and edge sizes."""
import os

import numpy as np
import pytest

from tests import icp_gicp_helpers as GH
from tests import apps
from tests import icp_helpers as H
from tests import icp_plane_helpers as PH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
MIN_NB = 6
EPSILONS = (1e-3, 1e-2, 1.0)


@pytest.fixture(scope="module")
def icp(s4p_lib_built):
    from super4pcs_amd import build as B
    B.build_icp()
    B.build_normals()
    from super4pcs_amd import icp as I
    return I


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return H.build_cpu(tmp_path_factory.mktemp("icp_cpu"))


@pytest.fixture(scope="module")
def bumpy():
    from super4pcs_amd import datasets as D
    return D.bumpy_pair(200_000, overlap=0.5, delta=0.004, seed=11)


@pytest.fixture(scope="module")
def lidar():
    from super4pcs_amd import datasets as D
    return D.lidar_pair_scaled(0.02, delta=0.05)


def _check_gicp_sums(ctx, cpu, P, Q, Np, Nq, T_caller, d, eps_list=EPSILONS):
    """Correspondences bit for bit, [0] and [2] exactly, every other entry within 1e-10 of its sum of |term|."""
    c = ctx.frame()
    Pc, Qc = (P - c).astype(np.float32), (Q - c).astype(np.float32)
    Tc = H.to_centred(T_caller, c).astype(np.float32)
    gi, gd = ctx.correspondences(Tc)
    ci, cd, _ = cpu.pass_(Pc, Qc, Tc, d)
    assert np.array_equal(gi, ci) and np.array_equal(gd, cd)
    for eps in eps_list:
        gs = ctx.gicp_sums(Tc, eps)
        cs, cabs = GH.gicp_sums(Pc, Qc, Tc, ci, cd, Np, Nq, eps)
        assert gs[0] == cs[0] and gs[2] == cs[2] and gs[0] == gs[2] == np.count_nonzero(ci >= 0)
        err = np.abs(gs - cs)
        worst = float(np.max(err / np.maximum(cabs, 1e-300)))
        print("gicp sums: n_Q %d, n %d, eps %g: max |gpu - cpu| / sum|term| %.3g" % (len(Q), int(gs[0]), eps, worst))
        assert np.all(err <= 1e-10 * cabs), (eps, gs, cs)
    return int(cs[0])


def test_gicp_sums_are_the_contract(icp, cpu, bumpy, lidar):
    """1: caller source normals (some zero, not unit length, one NaN); caller target normals, then estimated ones; three
    transforms around the generator's pose; epsilon 1e-3, 1e-2, 1."""
    rng = np.random.default_rng(4)
    for (P, Q, T_gt), d in ((bumpy, 4 * 0.004), (lidar, 4 * 0.05)):
        ctx = icp.ICP(0)
        ctx.set_target(P, d)
        ctx.set_source(Q)
        raw_q = H.raw_normals(rng, len(Q))
        ctx.set_source_normals(raw_q)
        Nq = PH.normalise(raw_q)
        assert np.array_equal(ctx.source_normals(), Nq)
        assert not Nq[::11].any() and not Nq[5].any() and Nq.any(1).sum() > 0.8 * len(Q)
        raw_p = H.raw_normals(rng, len(P))
        ctx.set_target_normals(raw_p)
        Np = PH.normalise(raw_p)
        assert np.array_equal(ctx.target_normals(), Np)
        for ang, sh in ((0.0, 0.0), (0.3, 0.002), (-1.0, 0.01)):
            assert _check_gicp_sums(ctx, cpu, P, Q, Np, Nq, H.motion(ang, sh) @ T_gt, d) > 1000
        ctx.estimate_normals(d, MIN_NB)
        Ne = ctx.target_normals()
        assert np.array_equal(ctx.source_normals(), Nq)              # untouched by the target's normals
        for ang, sh in ((0.0, 0.0), (0.5, -0.004), (2.0, -0.02)):
            assert _check_gicp_sums(ctx, cpu, P, Q, Ne, Nq, H.motion(ang, sh) @ T_gt, d) > 1000
        ctx.close()


def test_gicp_state_and_argument_errors(icp, bumpy):
    """2: -7 without target or source normals, -1 for a wrong count or an epsilon outside [1e-6, 1]; set_source invalidates."""
    P, Q, T_gt = bumpy
    P, Q = P[:20_000], Q[:5_000]
    d = 4 * 0.004
    rng = np.random.default_rng(6)
    Nq = rng.normal(size=Q.shape).astype(np.float32)
    ctx = icp.ICP(0)
    ctx.set_target(P, d)
    ctx.set_source(Q)

    def code(fn):
        with pytest.raises(icp.ICPError) as e:
            fn()
        return e.value.code

    assert code(lambda: ctx.gicp_sums(np.eye(4))) == -7               # neither
    assert code(lambda: ctx.source_normals()) == -7
    ctx.set_source_normals(Nq)
    assert code(lambda: ctx.gicp_sums(np.eye(4))) == -7               # no target normals
    assert code(lambda: ctx.refine(T_gt, metric="gicp")) == -7
    ctx.estimate_normals(d)
    ctx.gicp_sums(np.eye(4))
    ctx.set_source(Q)                                                 # invalidates the source normals
    assert code(lambda: ctx.gicp_sums(np.eye(4))) == -7
    assert code(lambda: ctx.refine(T_gt, metric="gicp")) == -7
    assert code(lambda: ctx.source_normals()) == -7
    assert code(lambda: ctx.set_source_normals(Nq[:-1])) == -1
    assert code(lambda: ctx.set_source_normals(np.concatenate([Nq, Nq[:1]]))) == -1
    ctx.set_source_normals(Nq)
    for eps in (0.0, -1e-3, 9.9e-7, 1.0000001, 2.0, float("nan"), float("inf")):
        assert code(lambda: ctx.gicp_sums(np.eye(4), eps)) == -1, eps
        assert code(lambda: ctx.refine(T_gt, metric="gicp", gicp_epsilon=eps)) == -1, eps
    for eps in (1e-6, 1.0):
        ctx.gicp_sums(np.eye(4), eps)
    ctx.set_target(P, d)                                              # invalidates the target normals, keeps the source's
    assert code(lambda: ctx.gicp_sums(np.eye(4))) == -7
    assert np.array_equal(ctx.source_normals(), PH.normalise(Nq))
    with pytest.raises(ValueError):
        ctx.refine(T_gt, metric="gicp", loss="huber")
    ctx.close()


def _exact_pose_setup(icp, bumpy):
    """Q: a 100 k subset of P moved rigidly; normals of P estimated once, Q's the same normals moved with it."""
    P = bumpy[0]
    rng = np.random.default_rng(5)
    pick = np.sort(rng.choice(len(P), 100_000, replace=False))
    extent = float(np.linalg.norm(P.max(0) - P.min(0)))
    d = 0.05 * extent
    ctx = icp.ICP(0)
    ctx.set_target(P, d)
    ctx.estimate_normals(d)
    Np = ctx.target_normals()
    ctx.close()
    M = H.motion(2.0, 0.01 * extent * np.array([0.6, -0.8, 0.0]))
    Q = (P[pick].astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
    Nq = (Np[pick].astype(np.float64) @ M[:3, :3].T).astype(np.float32)
    return P, Q, Np, Nq, np.linalg.inv(M), d


def test_gicp_is_deterministic_and_torch_agrees(icp, bumpy):
    """3: two calls and a second context give identical sums, T and Result bytes; numpy and torch device inputs too;
    order_source on and off see the same correspondences."""
    import torch
    P, Q, Np, Nq, T_true, d = _exact_pose_setup(icp, bumpy)
    T0 = H.motion(1.0, 0.002) @ T_true
    ctx = icp.ICP(0)
    ctx.set_target(P, d); ctx.set_source(Q)
    ctx.set_target_normals(Np); ctx.set_source_normals(Nq * 2.5)
    Tc = H.to_centred(T0, ctx.frame()).astype(np.float32)
    s1, s2 = ctx.gicp_sums(Tc), ctx.gicp_sums(Tc)
    assert s1.tobytes() == s2.tobytes()
    T1, r1 = ctx.refine(T0, metric="gicp")
    T2, r2 = ctx.refine(T0, metric="gicp")
    assert np.array_equal(T1, T2) and bytes(r1) == bytes(r2)
    assert ctx.gicp_sums(Tc).tobytes() == s1.tobytes()               # the refine's source order leaves the stage call alone
    dev = torch.device("cuda:0")
    ctx2 = icp.ICP(0)
    ctx2.set_target(torch.from_numpy(P).to(dev), d); ctx2.set_source(torch.from_numpy(Q).to(dev))
    ctx2.set_target_normals(torch.from_numpy(Np).to(dev)); ctx2.set_source_normals(torch.from_numpy(Nq * 2.5).to(dev))
    assert np.array_equal(ctx2.source_normals(), ctx.source_normals())
    assert ctx2.gicp_sums(Tc).tobytes() == s1.tobytes()
    T3, r3 = ctx2.refine(T0, metric="gicp")
    assert np.array_equal(T3, T1) and bytes(r3) == bytes(r1)
    # order_source: another summation order, the same pairs
    Ta, ra = ctx.refine(T0, metric="gicp", max_iterations=1, order_source=True)
    Tb, rb = ctx.refine(T0, metric="gicp", max_iterations=1, order_source=False)
    assert ra.history_n[0] == rb.history_n[0] == int(s1[0]) and ra.n_corr == rb.n_corr
    assert np.isclose(ra.history_rmse[0], rb.history_rmse[0], rtol=1e-12) and np.max(np.abs(Ta - Tb)) <= 1e-9
    ctx.close(); ctx2.close()


def test_gicp_refine_trajectory_equals_the_cpu_loop(icp, cpu, bumpy):
    """4: the CPU restatement of the generalized sums plus s4p_icp_solve_plane, from 1.5 degrees off the generator's pose;
    estimated target normals, k-nearest-neighbour source normals."""
    from super4pcs_amd import normals
    P, Q, T_gt = bumpy
    d = 4 * 0.004
    T0 = H.motion(1.5, 0.004) @ T_gt
    ctx = icp.ICP(0)
    ctx.set_target(P, d)
    ctx.set_source(Q)
    ctx.estimate_normals(d)
    ctx.set_source_normals(normals.estimate_normals(Q, k=16))
    T, r = ctx.refine(T0, metric="gicp")
    c = ctx.frame()
    Tc, its, status, hist = GH.cpu_refine_gicp(cpu, icp.solve_plane, (P - c).astype(np.float32), (Q - c).astype(np.float32),
                                               ctx.target_normals(), ctx.source_normals(), c, T0, d)
    print("gicp trajectory: gpu %d its (%s) rmse %.6g; cpu %d its (%s) |dT| %.2g; rot err %.4g -> %.4g deg"
          % (r.iterations, icp.STATUS_NAMES[r.status], r.rmse, its, icp.STATUS_NAMES[status], np.max(np.abs(T - Tc)),
             H.rot_err_deg(T0, T_gt), H.rot_err_deg(T, T_gt)))
    assert np.max(np.abs(T - Tc)) <= 1e-5
    assert abs(r.iterations - its) <= 1 and r.status == status
    k = min(r.history_len, len(hist), 3)
    assert np.allclose(list(r.history_rmse[:k]), hist[:k], rtol=1e-9)
    ctx.close()


def test_gicp_refine_reaches_an_exact_pose(icp, bumpy):
    """5: a rigidly moved subset of P with the same normals on both clouds, from 1 degree off: back to 1e-5, fitness 1."""
    P, Q, Np, Nq, T_true, d = _exact_pose_setup(icp, bumpy)
    T0 = H.motion(1.0, 0.002) @ T_true
    ctx = icp.ICP(0)
    ctx.set_target(P, d); ctx.set_source(Q)
    ctx.set_target_normals(Np); ctx.set_source_normals(Nq)
    T, r = ctx.refine(T0, max_iterations=64, rel_tol=0.0, metric="gicp")
    print("gicp exact pose: |T0 - T_true| %.2g -> |T - T_true| %.2g, %d iterations (%s), rmse %.3g, fitness %.6f"
          % (np.max(np.abs(T0 - T_true)), np.max(np.abs(T - T_true)), r.iterations, icp.STATUS_NAMES[r.status], r.rmse, r.fitness))
    assert np.max(np.abs(T - T_true)) <= 1e-5 and r.fitness == 1.0
    ctx.close()


def test_gicp_planar_target_at_the_smallest_epsilon(icp, cpu):
    """6: z = 0 with every normal along z and epsilon 1e-6: the in-plane directions carry weight epsilon only.  No crash;
    s4p_icp_solve_plane decides, and decides the same on the CPU loop's sums."""
    rng = np.random.default_rng(8)
    P = np.column_stack([rng.uniform(-1, 1, (50_000, 2)), np.zeros(50_000)]).astype(np.float32)
    Q = P[rng.choice(len(P), 20_000, replace=False)] + np.array([0, 0, 0.01], np.float32)
    T0 = H.motion(0.5, np.array([0.01, -0.02, 0.0]), axis=(0, 0, 1))
    up = np.array([0, 0, 1], np.float32)
    Np, Nq = np.tile(up, (len(P), 1)), np.tile(up, (len(Q), 1))
    eps = 1e-6
    ctx = icp.ICP(0)
    ctx.set_target(P, 0.08); ctx.set_source(Q)
    ctx.set_target_normals(Np); ctx.set_source_normals(Nq)
    c = ctx.frame()
    Pc, Qc = (P - c).astype(np.float32), (Q - c).astype(np.float32)
    Tc = H.to_centred(T0, c).astype(np.float32)
    gs = ctx.gicp_sums(Tc, eps)
    ci, cd, _ = cpu.pass_(Pc, Qc, Tc, 0.08)
    cs, _ = GH.gicp_sums(Pc, Qc, Tc, ci, cd, Np, Nq, eps)
    assert np.all(np.isfinite(gs)) and gs[0] == cs[0] > 10_000

    def decide(s):
        try:
            icp.solve_plane(s)
            return 0
        except icp.ICPError as e:
            return e.code

    assert decide(gs) == decide(cs)
    T, r = ctx.refine(T0, metric="gicp", gicp_epsilon=eps)
    Tcpu, its, status, hist = GH.cpu_refine_gicp(cpu, icp.solve_plane, Pc, Qc, Np, Nq, c, T0, 0.08, eps=eps)
    print("gicp planar target, eps 1e-6: first solve %s; gpu %d its (%s), cpu %d its (%s), |dT| %.2g"
          % ("degenerate" if decide(gs) else "ok", r.iterations, icp.STATUS_NAMES[r.status], its, icp.STATUS_NAMES[status],
             np.max(np.abs(T - Tcpu))))
    assert np.all(np.isfinite(T)) and r.status == status
    if r.status == icp.DEGENERATE and r.iterations == 0:
        assert np.array_equal(T, T0)
    ctx.close()


def test_facade_cli_and_binding_agree_on_the_hippo(icp, tmp_path, s4p_lib_built):
    """7: the hippo fixture through MatchSuper4PCS + RefineICP(Generalized) (tests/icp_facade_app), through
    `Super4PCS ... --icp 30 --icp-metric gicp -m`, and through icp.refine from the same Super4PCS result; then the facade
    with both clouds' own normals (Q's rotated by the registration) against the binding."""
    from super4pcs_amd import build as B
    from super4pcs_amd import normals
    g = np.load(os.path.join(ROOT, "tests", "golden", "hippo_config1.npz"))
    Ps, Qu = g["Ps"].astype(np.float32), g["Qu"].astype(np.float32)
    delta, overlap, n_s = 0.01, 0.7, 200
    exe = apps.build_app(tmp_path, "icp_facade_app", apps.ICP_FACADE_LIBS)

    def app(p_rows, q_rows):
        return apps.run_icp_app(exe, p_rows, q_rows, delta, overlap, n_s, "--metric", "gicp")[0]

    rows = app(Ps, Qu)
    M, Mf = rows["registered"].astype(np.float64), rows["registered"]
    Qm = apps.move_f32(Mf, Qu)
    dT, r = icp.refine(Ps, Qm, np.eye(4), max_distance=np.float32(4.0 * delta), metric="gicp")
    want = icp.compose(dT, M).astype(np.float32)
    print("hippo gicp: facade == icp.py max diff %.2g, %d iterations (%s), rmse %.4g"
          % (np.max(np.abs(rows["refined"] - want)), r.iterations, icp.STATUS_NAMES[r.status], r.rmse))
    assert np.max(np.abs(rows["refined"] - want)) <= 1e-6
    assert np.max(np.abs(rows["refined"] - Mf)) > 0
    # command line
    cli = B.build_cli()
    apps.write_obj(tmp_path / "P.obj", Ps); apps.write_obj(tmp_path / "Q.obj", Qu)
    got, _ = apps.run_cli(cli, tmp_path / "P.obj", tmp_path / "Q.obj", delta, overlap, n_s, ["--icp", "30", "--icp-metric", "gicp"])
    assert np.max(np.abs(got - want)) <= 2e-6
    # the facade with both clouds' own (nonzero) normals uploads them, Q's rotated by the registration's linear part
    Np = normals.estimate_normals(Ps, k=16); Nq = normals.estimate_normals(Qu, k=16)
    Np[~Np.any(1)] = np.array([0, 0, 1], np.float32); Nq[~Nq.any(1)] = np.array([0, 0, 1], np.float32)
    rows2 = app(np.column_stack([Ps, Np]), np.column_stack([Qu, Nq]))
    assert np.array_equal(rows2["registered"], rows["registered"])
    Mr = Mf[:3, :3].astype(np.float64); nq = Nq.astype(np.float64)
    Nq_moved = np.stack([(Mr[a, 0] * nq[:, 0] + Mr[a, 1] * nq[:, 1]) + Mr[a, 2] * nq[:, 2] for a in range(3)], 1).astype(np.float32)
    dT2, _ = icp.refine(Ps, Qm, np.eye(4), max_distance=np.float32(4.0 * delta), metric="gicp", target_normals=Np,
                        source_normals=Nq_moved)
    want2 = icp.compose(dT2, M).astype(np.float32)
    assert np.max(np.abs(rows2["refined"] - want2)) <= 1e-6


@pytest.fixture(scope="module")
def first_hit(cpu, bumpy):
    """The first source point of the bumpy pair with a correspondence at the edge test's transform (CPU restatement)."""
    P, Q, T_gt = bumpy
    c = P.astype(np.float64).mean(0).astype(np.float32)
    idx, _, _ = cpu.pass_((P - c).astype(np.float32), (Q - c).astype(np.float32), H.to_centred(H.motion(0.3, 0.002) @ T_gt, c).astype(np.float32),
                          4 * 0.004)
    return int(np.flatnonzero(idx >= 0)[0])


@pytest.mark.parametrize("n_q", [1, 63, 64, 65, 257, 524_289])
def test_gicp_sums_at_edge_sizes(icp, cpu, bumpy, first_hit, n_q):
    """8: one lane, a ragged wave, exactly one wave, one lane more, a ragged second workgroup; and 524 289 source points:
    one more than the 2048 x 256 lanes of a full launch, so the grid-stride loop runs a second, ragged round."""
    P, Q, T_gt = bumpy
    d = 4 * 0.004
    rng = np.random.default_rng(n_q)
    if first_hit + n_q <= len(Q):
        Qn = Q[first_hit:first_hit + n_q]             # starts at a point that has a match
    else:
        reps = -(-n_q // len(Q))
        Qn = np.concatenate([Q] * reps)[:n_q].astype(np.float64)
        Qn[len(Q):] += rng.normal(scale=0.001, size=(n_q - len(Q), 3))
        Qn = Qn.astype(np.float32)
    assert len(Qn) == n_q
    ctx = icp.ICP(0)
    ctx.set_target(P, d)
    ctx.set_source(Qn)
    raw_q = H.raw_normals(rng, n_q)
    ctx.set_source_normals(raw_q)
    Nq = PH.normalise(raw_q)
    assert np.array_equal(ctx.source_normals(), Nq)
    ctx.estimate_normals(d, MIN_NB)
    Np = ctx.target_normals()
    n = _check_gicp_sums(ctx, cpu, P, Qn, Np, Nq, H.motion(0.3, 0.002) @ T_gt, d)
    print("edge size %d: %d pairs" % (n_q, n))
    assert n >= (1 if n_q < 1000 else 1000)
    T, r = ctx.refine(T_gt, metric="gicp", max_iterations=2)
    assert np.all(np.isfinite(T)) and r.history_n[0] >= 1
    ctx.close()
