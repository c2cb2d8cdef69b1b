"""Robust ICP on the MI355X (include/s4p_icp_robust.h): weighted sums and info against the numpy restatement
(tests/icp_robust_helpers.py), the selection's edge cases, unit weights reducing to the plain path bit for bit, determinism
and torch inputs, the trajectory against the CPU loop, an outlier scene where plain point-to-plane stays off the pose and
trimmed / Tukey reach it, and the facade / command line / Python binding agreeing."""
import os

import numpy as np
import pytest

from tests import apps
from tests import icp_helpers as H
from tests import icp_plane_helpers as PH
from tests import icp_robust_helpers as RH

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


CASES = [dict(loss="trimmed", trim_fraction=0.7), dict(loss="trimmed", trim_fraction=0.3), dict(loss="huber"),
         dict(loss="tukey"), dict(loss="tukey", scale=0.01), dict(loss="huber", scale=0.002)]


def _check(ctx, cpu, P, Q, Nc, Tc, d, metric, kw):
    c = ctx.frame()
    Pc, Qc = (P - c).astype(np.float32), (Q - c).astype(np.float32)
    ci, cd, _ = cpu.pass_(Pc, Qc, Tc, d)
    gs, gi = ctx.robust_sums(Tc, metric, **kw)
    cs, ii = RH.robust_sums(Pc, Qc, Tc, ci, cd, metric, n_q=len(Q), d=d, Nc=Nc, **kw)
    assert np.array_equal(gi[[0, 1, 2, 4, 6, 7]], ii[[0, 1, 2, 4, 6, 7]]), (metric, kw, gi, ii)
    assert gi[3] == ii[3] and gi[5] == gs[0], (gi, ii)
    R = float(np.max(np.abs(Pc)))
    if metric == "point":
        n = float(np.count_nonzero(ci >= 0))
        scale = np.maximum(np.abs(cs), np.array([n] + [n * R] * 6 + [n * R * R] * 9 + [n * float(d) ** 2]))
    else:
        assert gs[2] == cs[2]
        n = float(np.count_nonzero(ci >= 0))
        w = np.array([R, R, R, 1.0, 1.0, 1.0])
        tri = np.outer(w, w)[np.triu_indices(6)]
        scale = np.maximum(np.abs(cs), np.concatenate([[n, n * float(d) ** 2, n, n * float(d) ** 2], n * tri, n * w * float(d)]))
    assert np.all(np.abs(gs - cs) <= 1e-10 * scale), (metric, kw, gs, cs)
    return gi


def test_robust_sums_are_the_contract(icp, cpu, bumpy, lidar):
    """1: each loss x both metrics x transforms around the generator's pose, caller-supplied and estimated normals: M, k,
    the threshold bits, s and the count exactly; the sums to relative 1e-10."""
    rng = np.random.default_rng(4)
    for (P, Q, T_gt), d in ((bumpy, 4 * 0.004), (lidar, 4 * 0.05)):
        ctx = icp.ICP(0)
        ctx.set_target(P, d)
        ctx.set_source(Q)
        with pytest.raises(icp.ICPError) as e:
            ctx.robust_sums(np.eye(4), "plane", "huber")
        assert e.value.code == -7                                     # no normals yet
        raw = rng.normal(size=P.shape).astype(np.float32)
        raw[::11] = 0
        ctx.set_target_normals(raw)
        Nu = PH.normalise(raw)
        c = ctx.frame()
        for normals in ("caller", "estimated"):
            if normals == "estimated":
                ctx.estimate_normals(d)
                Nu = ctx.target_normals()
            for ang, sh in ((0.0, 0.0), (0.5, 0.002)):
                Tc = H.to_centred(RH.motion(ang, sh) @ T_gt, c).astype(np.float32)
                for kw in CASES:
                    for metric in ("point", "plane"):
                        gi = _check(ctx, cpu, P, Q, Nu, Tc, d, metric, kw)
                        assert gi[0] > 1000 and gi[4] > 0
        ctx.close()


def test_selection_edge_cases(icp, cpu):
    """2: all residuals equal (every pair tied at the threshold is kept), k = 1 and k = M, M below min_correspondences, and
    an exact pose where every key is 0 and s_min applies."""
    g = np.arange(64, dtype=np.float32) * np.float32(0.125)
    X, Y = np.meshgrid(g, g)
    P = np.column_stack([X.ravel(), Y.ravel(), np.zeros(X.size)]).astype(np.float32)
    Q = P + np.array([0, 0, 0.0625], np.float32)
    d = 0.1
    ctx = icp.ICP(0)
    ctx.set_target(P, d)
    ctx.set_source(Q)
    ctx.set_target_normals(np.tile(np.array([0, 0, 1], np.float32), (len(P), 1)))
    key = int(np.float32(0.0625 * 0.0625).view(np.uint32))
    for metric in ("point", "plane"):
        s, info = ctx.robust_sums(np.eye(4), metric, "trimmed", trim_fraction=0.5)
        assert info[:5].tolist() == [len(P), len(P) // 2, key, 0.0, len(P)]          # ties: every pair weighs 1
        s, info = ctx.robust_sums(np.eye(4), metric, "tukey")
        assert info[:3].tolist() == [len(P), len(P) // 2, key] and info[4] == len(P)
        assert info[3] == max(1.4826 * 0.0625, 1e-6 * float(np.float32(d)))
    # k = 1 and k = M on distinct keys
    rng = np.random.default_rng(3)
    P2 = rng.uniform(-1, 1, (20_000, 3)).astype(np.float32)
    Q2 = (P2[:5000] + rng.normal(scale=0.01, size=(5000, 3))).astype(np.float32)
    ctx2 = icp.ICP(0)
    ctx2.set_target(P2, 0.05)
    ctx2.set_source(Q2)
    c = ctx2.frame()
    ci, cd, _ = cpu.pass_((P2 - c).astype(np.float32), (Q2 - c).astype(np.float32), np.eye(4, dtype=np.float32), 0.05)
    u = cd[ci >= 0]
    for xi, k in ((1e-9, 1), (1.0, len(u))):
        s, info = ctx2.robust_sums(np.eye(4), "point", "trimmed", trim_fraction=xi)
        thr = RH.select(u, k)
        assert info[:3].tolist() == [len(u), k, int(thr.view(np.uint32))]
        assert info[4] == np.count_nonzero(u <= thr)
    # M below min_correspondences: two matches only
    Q3 = np.concatenate([P2[:2], P2[2:1000] + np.float32(50.0)]).astype(np.float32)
    ctx2.set_source(Q3)
    s, info = ctx2.robust_sums(np.eye(4), "point", "tukey")
    assert info[0] == 2 and info[1] == 1 and info[4] == 2
    T, r = ctx2.refine(np.eye(4), loss="tukey")
    assert r.status == icp.TOO_FEW and r.iterations == 0 and r.n_corr == 2 and np.array_equal(T, np.eye(4))
    # exact pose: every key 0, s = s_min, every Tukey weight 1
    ctx2.set_source(P2[:5000])
    for metric_loss in ("tukey", "huber"):
        s, info = ctx2.robust_sums(np.eye(4), "point", metric_loss)
        assert info[:5].tolist() == [5000, 2500, 0, 1e-6 * float(np.float32(0.05)), 5000] and s[0] == 5000
    T, r = ctx2.refine(np.eye(4), loss="tukey")
    assert r.n_corr == 5000 and r.rmse == 0.0 and np.max(np.abs(T - np.eye(4))) <= 1e-6


def test_unit_weights_reduce_to_the_plain_path(icp, bumpy):
    """3: trimmed with xi = 1 and Huber with a huge fixed scale weigh every pair 1: sums bit-identical to sums() /
    plane_sums(), and the whole refine returns the plain refine's T and result bytes, for both metrics."""
    P, Q, T_gt = bumpy
    d = 4 * 0.004
    ctx = icp.ICP(0)
    ctx.set_target(P, d)
    ctx.set_source(Q)
    ctx.estimate_normals(d)
    c = ctx.frame()
    for ang, sh in ((0.0, 0.0), (1.0, 0.003)):
        Tc = H.to_centred(RH.motion(ang, sh) @ T_gt, c).astype(np.float32)
        plain = {"point": ctx.sums(Tc), "plane": ctx.plane_sums(Tc)}
        for kw in (dict(loss="trimmed", trim_fraction=1.0), dict(loss="huber", scale=1e3)):
            for metric in ("point", "plane"):
                s, info = ctx.robust_sums(Tc, metric, **kw)
                assert np.array_equal(s, plain[metric]), (metric, kw)
                assert info[4] == plain[metric][0]
    T0 = RH.motion(1.5, 0.004) @ T_gt
    for metric in ("point", "plane"):
        Tp, rp = ctx.refine(T0, metric=metric)
        for kw in (dict(loss="trimmed", trim_fraction=1.0), dict(loss="huber", loss_scale=1e3)):
            Tr, rr = ctx.refine(T0, metric=metric, **kw)
            assert np.array_equal(Tr, Tp) and bytes(rr) == bytes(rp), (metric, kw)


def test_robust_is_deterministic_and_torch_agrees(icp, bumpy):
    """4: two calls give identical bits; numpy and torch device inputs agree."""
    import torch
    P, Q, T_gt = bumpy
    d = 4 * 0.004
    T0 = RH.motion(1.0, 0.002) @ T_gt
    dev = torch.device("cuda:0")
    ctx, ctx2 = icp.ICP(0), icp.ICP(0)
    ctx.set_target(P, d); ctx.set_source(Q); ctx.estimate_normals(d)
    ctx2.set_target(torch.from_numpy(P).to(dev), d); ctx2.set_source(torch.from_numpy(Q).to(dev)); ctx2.estimate_normals(d)
    Tc = H.to_centred(T0, ctx.frame()).astype(np.float32)
    for metric in ("point", "plane"):
        for kw in (dict(loss="trimmed", trim_fraction=0.6), dict(loss="tukey")):
            a = ctx.robust_sums(Tc, metric, **kw)
            b = ctx.robust_sums(Tc, metric, **kw)
            t = ctx2.robust_sums(Tc, metric, **kw)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)) and all(np.array_equal(x, y) for x, y in zip(a, t))
            i1, i2 = np.zeros(8), np.zeros(8)
            T1, r1 = ctx.refine(T0, metric=metric, info=i1, **kw)
            T2, r2 = ctx.refine(T0, metric=metric, **kw)
            T3, r3 = ctx2.refine(T0, metric=metric, info=i2, **kw)
            assert np.array_equal(T1, T2) and np.array_equal(T1, T3) and bytes(r1) == bytes(r2) == bytes(r3)
            assert np.array_equal(i1, i2) and i1[4] == r1.n_corr


def test_robust_trajectory_equals_the_cpu_loop(icp, cpu, bumpy):
    """5: history_rmse against the CPU restatement's loop (rtol 1e-9), from 1.5 degrees off the generator's pose."""
    P, Q, T_gt = bumpy
    d = 4 * 0.004
    T0 = RH.motion(1.5, 0.004) @ T_gt
    ctx = icp.ICP(0)
    ctx.set_target(P, d)
    ctx.set_source(Q)
    ctx.estimate_normals(d)
    c = ctx.frame()
    N = ctx.target_normals()
    Pc, Qc = (P - c).astype(np.float32), (Q - c).astype(np.float32)
    for metric, kw in (("point", dict(loss="trimmed", trim_fraction=0.5)), ("plane", dict(loss="tukey")), ("plane", dict(loss="trimmed", trim_fraction=0.5)),
                       ("point", dict(loss="huber"))):
        T, r = ctx.refine(T0, metric=metric, **{("loss_scale" if k == "scale" else k): v for k, v in kw.items()})
        Tc, its, status, hist, hist_n = RH.cpu_refine_robust(cpu, icp.solve, icp.solve_plane, Pc, Qc, c, T0, d, metric, Nc=N, **kw)
        print("robust trajectory %s %s: gpu %d its (%s) rmse %.6g; cpu %d its (%s) |dT| %.2g; rot err %.4g -> %.4g deg"
              % (metric, kw, r.iterations, icp.STATUS_NAMES[r.status], r.rmse, its, icp.STATUS_NAMES[status], np.max(np.abs(T - Tc)),
                 H.rot_err_deg(T0, T_gt), H.rot_err_deg(T, T_gt)))
        k = min(r.history_len, len(hist), 3)
        assert np.allclose(list(r.history_rmse[:k]), hist[:k], rtol=1e-9, atol=0)
        assert list(r.history_n[:k]) == hist_n[:k]
        assert np.max(np.abs(T - Tc)) <= 1e-5 and abs(r.iterations - its) <= 1


def test_trimmed_and_tukey_reach_the_pose_in_clutter(icp, pcpu, bumpy):
    """6: a 60 k subset of the bumpy target moved by 0.5 degrees, plus 40 k clutter points 0.3 d .. 0.8 d off the surface
    on one side.  The CPU restatement's loop (same normals) gives: plain point-to-plane 0.43 degrees / 0.0049 off, trimmed
    (xi = 0.6) and Tukey within 1e-8.  Bounds: plain > 0.1 degrees off, robust within 1e-6."""
    P = bumpy[0]
    d = 4 * 0.004
    ctx = icp.ICP(0)
    ctx.set_target(P, d)
    c = ctx.frame()
    k, c6 = pcpu.cov((P - c).astype(np.float32), d)
    N, _ = PH.normals_from_cov(k, c6, 6)
    N = PH.normalise(N)
    Q, M, frac = RH.outlier_scene(P, N, d)
    ctx.set_source(Q)
    ctx.set_target_normals(N)
    Tp, rp = ctx.refine(np.eye(4), metric="plane")
    Tt, rt = ctx.refine(np.eye(4), metric="plane", loss="trimmed", trim_fraction=frac)
    Tk, rk = ctx.refine(np.eye(4), metric="plane", loss="tukey")
    print("clutter: plain %.4g deg / %.3g, trimmed %.3g, tukey %.3g (max |T - T_true|); fitness %.3f %.3f %.3f"
          % (H.rot_err_deg(Tp, M), np.linalg.norm(Tp[:3, 3] - M[:3, 3]), np.max(np.abs(Tt - M)), np.max(np.abs(Tk - M)),
             rp.fitness, rt.fitness, rk.fitness))
    assert H.rot_err_deg(Tp, M) > 0.1 and np.max(np.abs(Tp - M)) > 1e-3
    assert np.max(np.abs(Tt - M)) <= 1e-6 and np.max(np.abs(Tk - M)) <= 1e-6
    assert abs(rt.fitness - frac) < 0.01


def test_facade_cli_and_binding_agree_on_the_hippo_with_trimmed_loss(icp, tmp_path, s4p_lib_built):
    """7: the hippo fixture through MatchSuper4PCS + RefineICP(loss Trimmed, xi = the overlap) (tests/icp_facade_app),
    through `Super4PCS ... --icp 30 --icp-loss trimmed -m` (xi defaults to -o), and through icp.py from the same result."""
    from super4pcs_amd import build as B
    g = np.load(os.path.join(ROOT, "tests", "golden", "hippo_config1.npz"))
    Ps, Qu = g["Ps"].astype(np.float32), g["Qu"].astype(np.float32)
    delta, overlap, n_s = 0.01, 0.7, 200
    exe = apps.build_app(tmp_path, "icp_facade_app", apps.ICP_FACADE_LIBS)
    rows, _ = apps.run_icp_app(exe, Ps, Qu, delta, overlap, n_s, "--loss", "trimmed", "--trim-fraction", overlap)
    M, Mf = rows["registered"].astype(np.float64), rows["registered"]
    Qm = apps.move_f32(Mf, Qu)
    ctx = icp.ICP(0)
    ctx.set_target(Ps, np.float32(4.0 * delta))
    ctx.set_source(Qm)
    dT, r = ctx.refine(np.eye(4), loss="trimmed", trim_fraction=overlap)
    want = icp.compose(dT, M).astype(np.float32)
    print("hippo trimmed: facade == icp.py max diff %.2g, %d iterations (%s), rmse %.4g, fitness %.3f"
          % (np.max(np.abs(rows["refined"] - want)), r.iterations, icp.STATUS_NAMES[r.status], r.rmse, r.fitness))
    assert np.max(np.abs(rows["refined"] - want)) <= 1e-6
    assert np.max(np.abs(rows["refined"] - Mf)) > 0
    cli = B.build_cli()
    apps.write_obj(tmp_path / "P.obj", Ps); apps.write_obj(tmp_path / "Q.obj", Qu)
    got, _ = apps.run_cli(cli, tmp_path / "P.obj", tmp_path / "Q.obj", delta, overlap, n_s, ["--icp", "30", "--icp-loss", "trimmed"])
    assert np.max(np.abs(got - want)) <= 2e-6
