"""Coloured ICP on the MI355X (include/s4p_icp_color.h): the gradients and the joint sums against the numpy restatement
(tests/icp_color_helpers.py), state and argument errors, determinism, the trajectory against the CPU loop, the planar
textured case the metric exists for, the facade / command line / Python binding agreeing, and edge sizes."""
import os

import numpy as np
import pytest

from tests import icp_color_helpers as CH
from tests import apps
from tests import icp_helpers as H
from tests import icp_plane_helpers as PH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
MIN_NB = 6
LAMBDAS = (0.0, 0.5, 0.968, 1.0)


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
    return D.bumpy_pair(200_000, overlap=0.5, delta=0.004, seed=11)


@pytest.fixture(scope="module")
def lidar():
    from super4pcs_amd import datasets as D
    return D.lidar_pair_scaled(0.02, delta=0.05)


def _textured(pair, scale):
    """(P, Q, T_gt, Ip, Iq): texture() on P, and on Q where the generator's pose puts it, so both clouds carry one field."""
    P, Q, T_gt = pair
    Qm = Q.astype(np.float64) @ T_gt[:3, :3].T + T_gt[:3, 3]
    return P, Q, T_gt, CH.texture(P, scale), CH.texture(Qm, scale)


def _check_gradients(ctx, P, Np, Ip, r, min_nb, what, which=None):
    """The device's gradients against the restatement: the input condition (no eigenvalue ratio within a factor 2 of the
    gate), the same zero pattern, every component within 2^-23 of the point's largest restated component.  which (sorted
    indices): the rule on those points only (the restatement of a large target costs seconds per 40 k points); the returned
    gradients are the whole target's, the zero pattern the compared points'."""
    c = ctx.frame()
    Pc = (P - c).astype(np.float32)
    want, ratio, k = CH.color_gradients(Pc, Np, Ip, r, min_nb, which=which)
    assert not np.any((ratio >= 0.5e-6) & (ratio <= 2e-6)), "input condition: an eigenvalue ratio next to the gate"
    full = ctx.target_color_gradients()
    got = full if which is None else full[which]
    Np = np.asarray(Np) if which is None else np.asarray(Np)[which]
    zw, zg = ~want.any(1), ~got.any(1)
    scale = np.max(np.abs(want.astype(np.float64)), axis=1)
    err = np.max(np.abs(got.astype(np.float64) - want.astype(np.float64)), axis=1)
    nzr = scale > 0
    worst = float(np.max(err[nzr] / scale[nzr])) if nzr.any() else 0.0
    print("%s: n %d, k mean %.1f max %d, %d zero gradients (%d zero normals, %d with k < %d), min ratio %.3g, "
          "max |gpu - cpu| / max|g| = %.3g (2^-23 = %.3g)"
          % (what, len(want), k.mean(), k.max(), zw.sum(), (~np.asarray(Np).any(1)).sum(), (k < min_nb).sum(), min_nb,
             np.nanmin(ratio) if np.isfinite(ratio).any() else np.nan, worst, 2.0 ** -23))
    assert np.array_equal(zw, zg)
    assert np.all(err <= 2.0 ** -23 * scale)
    return full, zw


def test_gradients_are_the_contract(icp, bumpy, lidar):
    """1: the planar input with caller normals; the bumpy 200 k pair with caller normals (some zero, non-unit, a NaN)
    and with estimated ones; the 2 % LiDAR pair with estimated normals.  Two calls give the same bits, and so do numpy
    and torch uploads of the caller's inputs."""
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(2)
    pc = CH.planar_case()
    cases = [("planar", pc["P"], pc["Ip"], pc["d"], pc["r"], pc["N"]),
             ("bumpy, caller normals", bumpy[0], CH.texture(bumpy[0], 4.0), 4 * 0.004, 2 * 0.004, "scaled"),
             ("bumpy, estimated normals", bumpy[0], CH.texture(bumpy[0], 4.0), 4 * 0.004, 2 * 0.004, None),
             ("lidar, estimated normals", lidar[0], CH.texture(lidar[0], 1.0), 4 * 0.05, 2 * 0.05, None)]
    for what, P, Ip, d, r, raw in cases:
        ctx = icp.ICP(0)
        ctx.set_target(P, d)
        ctx.estimate_normals(d, MIN_NB)
        if raw is not None and not isinstance(raw, np.ndarray):
            # the surface's normals at other lengths, some zero, one NaN.  (Random directions would put some tangent planes
            # edge-on to the surface, and some of those next to the gate: the input condition of _check_gradients.)
            raw = ctx.target_normals() * rng.uniform(0.5, 3.0, size=(len(P), 1)).astype(np.float32)
            raw[::11] = 0
            raw[5, 0] = np.nan
        if raw is not None:
            ctx.set_target_normals(raw)
        Np = ctx.target_normals()
        if raw is not None:
            assert np.array_equal(Np, PH.normalise(raw))
        ctx.set_target_intensity(Ip)
        ctx.estimate_color_gradients(r, MIN_NB)
        G, zero = _check_gradients(ctx, P, Np, Ip, r, MIN_NB, what)
        assert (~zero).sum() > 0.5 * len(P)
        ctx.estimate_color_gradients(r, MIN_NB)
        assert ctx.target_color_gradients().tobytes() == G.tobytes()
        if raw is not None:                       # the same caller input from the device (an upload normalises what it is given)
            ctx2 = icp.ICP(0)
            ctx2.set_target(torch.from_numpy(P).to(dev), d)
            ctx2.set_target_normals(torch.from_numpy(raw).to(dev))
            ctx2.set_target_intensity(torch.from_numpy(Ip).to(dev))
            ctx2.estimate_color_gradients(r, MIN_NB)
            assert ctx2.target_color_gradients().tobytes() == G.tobytes()
            ctx2.close()
        ctx.close()


def _check_color_sums(ctx, cpu, P, Q, Np, G, Ip, Iq, T_caller, d, lams=LAMBDAS):
    """Correspondences bit for bit, [0] and [2] exactly, every other entry within 1e-10 of its sum of |term|; at lambda = 1
    also against the library's own plane sums."""
    c = ctx.frame()
    Pc, Qc = (P - c).astype(np.float32), (Q - c).astype(np.float32)
    Tc = H.to_centred(T_caller, c).astype(np.float32)
    gi, gd = ctx.correspondences(Tc)
    ci, cd, _ = cpu.pass_(Pc, Qc, Tc, d)
    assert np.array_equal(gi, ci) and np.array_equal(gd, cd)
    for lam in lams:
        gs = ctx.color_sums(Tc, lam)
        cs, cabs = CH.color_sums(Pc, Qc, Tc, ci, cd, Np, G, Ip, Iq, lam)
        assert gs[0] == cs[0] == np.count_nonzero(ci >= 0) and gs[2] == cs[2] <= gs[0]
        err = np.abs(gs - cs)
        worst = float(np.max(err / np.maximum(cabs, 1e-300)))
        print("color sums: n_Q %d, n %d, n_term %d, lambda %g: max |gpu - cpu| / sum|term| %.3g" % (len(Q), int(gs[0]), int(gs[2]), lam, worst))
        assert np.all(err <= 1e-10 * cabs), (lam, gs, cs)
        if lam == 1.0:
            ps = ctx.plane_sums(Tc)
            assert ps[0] == gs[0] and ps[2] == gs[2]
            assert np.all(np.abs(gs - ps) <= 1e-10 * cabs), (gs, ps)
    return int(cs[0]), int(cs[2])


def _flatten_stretches(I, X):
    """Constant stretches in an intensity: a slab of the cloud set to one value (exactly zero gradients inside it)."""
    I = I.copy()
    lo, hi = np.quantile(X[:, 0], [0.3, 0.45])
    I[(X[:, 0] >= lo) & (X[:, 0] <= hi)] = np.float32(0.25)
    return I


def test_color_sums_are_the_contract(icp, cpu, bumpy, lidar):
    """2: caller target normals (some zero: zero gradients, pairs without a term), then estimated ones; intensities with a
    constant stretch (gradients exactly zero inside it); three transforms around the generator's pose; lambda 0, 0.5,
    0.968, 1."""
    rng = np.random.default_rng(4)
    for pair, d, scale in ((bumpy, 4 * 0.004, 4.0), (lidar, 4 * 0.05, 1.0)):
        P, Q, T_gt, Ip, Iq = _textured(pair, scale)
        Ip = _flatten_stretches(Ip, P)
        ctx = icp.ICP(0)
        ctx.set_target(P, d)
        ctx.set_source(Q)
        ctx.set_source_intensity(Iq)
        ctx.set_target_intensity(Ip)
        ctx.set_target_normals(H.raw_normals(rng, len(P)))
        Np = ctx.target_normals()
        ctx.estimate_color_gradients(d / 2, MIN_NB)
        G = ctx.target_color_gradients()
        assert not G[::11].any() and G.any(1).sum() > 0.5 * len(P)
        for ang, sh in ((0.0, 0.0), (0.3, 0.002), (-1.0, 0.01)):
            n, nt = _check_color_sums(ctx, cpu, P, Q, Np, G, Ip, Iq, H.motion(ang, sh) @ T_gt, d)
            assert n > 1000 and 0.8 * n < nt < n
        ctx.estimate_normals(d, MIN_NB)
        Ne = ctx.target_normals()
        ctx.estimate_color_gradients(d / 2, MIN_NB)
        G = ctx.target_color_gradients()
        slab = Ip == np.float32(0.25)
        assert slab.sum() > 1000 and (~G[slab & Ne.any(1)].any(1)).sum() > 100         # exactly zero inside the stretch
        for ang, sh in ((0.0, 0.0), (0.5, -0.004), (2.0, -0.02)):
            n, nt = _check_color_sums(ctx, cpu, P, Q, Ne, G, Ip, Iq, H.motion(ang, sh) @ T_gt, d)
            assert n > 1000
        ctx.close()


def test_color_state_and_argument_errors(icp, bumpy):
    """3: -7 without target normals, target intensity, gradients or source intensity; -1 for a wrong count, a non-finite
    intensity, a bad radius / min_neighbours or a lambda outside [0, 1]; what set_source, set_target, a normals replacement
    and a new target intensity invalidate."""
    P, Q, T_gt, Ip, Iq = _textured(bumpy, 4.0)
    P, Q, Ip, Iq = P[:20_000], Q[:5_000], Ip[:20_000], Iq[:5_000]
    d = 4 * 0.004
    E = np.eye(4)

    def code(fn):
        with pytest.raises(icp.ICPError) as e:
            fn()
        return e.value.code

    ctx = icp.ICP(0)
    assert code(lambda: ctx.set_target_intensity(Ip)) == -7           # no target yet
    assert code(lambda: ctx.set_source_intensity(Iq)) == -7
    ctx.set_target(P, d)
    ctx.set_source(Q)
    assert code(lambda: ctx.color_sums(E)) == -7                      # nothing
    assert code(lambda: ctx.estimate_color_gradients(d)) == -7        # no normals
    assert code(lambda: ctx.target_color_gradients()) == -7
    ctx.estimate_normals(d)
    assert code(lambda: ctx.estimate_color_gradients(d)) == -7        # no target intensity
    assert code(lambda: ctx.color_sums(E)) == -7
    ctx.set_target_intensity(Ip)
    assert code(lambda: ctx.color_sums(E)) == -7                      # no gradients
    assert code(lambda: ctx.refine(T_gt, metric="color")) == -7
    ctx.estimate_color_gradients(d)
    assert code(lambda: ctx.color_sums(E)) == -7                      # no source intensity
    assert code(lambda: ctx.refine(T_gt, metric="color")) == -7
    ctx.set_source_intensity(Iq)
    ctx.color_sums(E)
    G = ctx.target_color_gradients()
    # arguments
    assert code(lambda: ctx.set_target_intensity(Ip[:-1])) == -1
    assert code(lambda: ctx.set_source_intensity(np.concatenate([Iq, Iq[:1]]))) == -1
    for bad in (np.nan, np.inf, -np.inf):
        v = Iq.copy(); v[17] = bad
        assert code(lambda: ctx.set_source_intensity(v)) == -1
        w = Ip.copy(); w[-1] = bad
        assert code(lambda: ctx.set_target_intensity(w)) == -1
    ctx.color_sums(E)                                                 # a rejected upload changes nothing
    assert np.array_equal(ctx.target_color_gradients(), G)
    for r in (0.0, -1.0, float("nan"), d * 1.001):
        assert code(lambda: ctx.estimate_color_gradients(r)) == -1, r
    for m in (3, 0, -1):
        assert code(lambda: ctx.estimate_color_gradients(d, m)) == -1, m
    ctx.estimate_color_gradients(d, 4)
    for lam in (-1e-9, 1.0000001, 2.0, float("nan"), float("inf")):
        assert code(lambda: ctx.color_sums(E, lam)) == -1, lam
        assert code(lambda: ctx.refine(T_gt, metric="color", color_lambda=lam)) == -1, lam
    for lam in (0.0, 1.0):
        ctx.color_sums(E, lam)
    # invalidation
    ctx.set_source(Q)                                                 # the source intensity goes, the target side stays
    assert code(lambda: ctx.color_sums(E)) == -7
    ctx.target_color_gradients()
    ctx.set_source_intensity(Iq)
    ctx.color_sums(E)
    ctx.estimate_normals(d)                                           # a normals replacement: the gradients go
    assert code(lambda: ctx.color_sums(E)) == -7 and code(lambda: ctx.target_color_gradients()) == -7
    ctx.estimate_color_gradients(d)
    ctx.set_target_normals(ctx.target_normals())
    assert code(lambda: ctx.color_sums(E)) == -7
    ctx.estimate_color_gradients(d)
    ctx.set_target_intensity(Ip)                                      # a new target intensity: the gradients go
    assert code(lambda: ctx.color_sums(E)) == -7
    ctx.estimate_color_gradients(d)
    ctx.color_sums(E)
    ctx.set_target(P, d)                                              # normals, target intensity and gradients go; the source's stays
    assert code(lambda: ctx.estimate_color_gradients(d)) == -7
    ctx.estimate_normals(d)
    assert code(lambda: ctx.estimate_color_gradients(d)) == -7
    ctx.set_target_intensity(Ip)
    ctx.estimate_color_gradients(d)
    ctx.color_sums(E)
    with pytest.raises(ValueError):
        ctx.refine(T_gt, metric="color", loss="huber")
    ctx.close()


def _subset_setup(icp, bumpy):
    """Q: a 100 k subset of P with its intensities, moved rigidly; normals of P estimated once."""
    P = bumpy[0]
    rng = np.random.default_rng(5)
    pick = np.sort(rng.choice(len(P), 100_000, replace=False))
    d = 4 * 0.004
    Ip = CH.texture(P, 4.0)
    M = H.motion(0.5, np.array([0.0012, -0.0016, 0.0]))
    Q = (P[pick].astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
    return P, Q, Ip, Ip[pick].copy(), np.linalg.inv(M), d


def test_color_is_deterministic_and_torch_agrees(icp, bumpy):
    """4: two calls and a second context give identical sums, T and Result bytes; numpy and torch device inputs too;
    order_source on and off see the same correspondences."""
    import torch
    P, Q, Ip, Iq, T_true, d = _subset_setup(icp, bumpy)
    T0 = H.motion(0.3, 0.001) @ T_true
    ctx = icp.ICP(0)
    ctx.set_target(P, d); ctx.set_source(Q)
    ctx.estimate_normals(d)
    Np = ctx.target_normals()
    ctx.set_target_normals(Np)                                       # both contexts are given the same normals (an upload normalises)
    ctx.set_target_intensity(Ip); ctx.set_source_intensity(Iq)
    ctx.estimate_color_gradients(d / 2)
    Tc = H.to_centred(T0, ctx.frame()).astype(np.float32)
    s1, s2 = ctx.color_sums(Tc), ctx.color_sums(Tc)
    assert s1.tobytes() == s2.tobytes()
    T1, r1 = ctx.refine(T0, metric="color")
    T2, r2 = ctx.refine(T0, metric="color")
    assert np.array_equal(T1, T2) and bytes(r1) == bytes(r2)
    assert ctx.color_sums(Tc).tobytes() == s1.tobytes()              # the refine's source order leaves the stage call alone
    dev = torch.device("cuda:0")
    ctx2 = icp.ICP(0)
    ctx2.set_target(torch.from_numpy(P).to(dev), d); ctx2.set_source(torch.from_numpy(Q).to(dev))
    ctx2.set_target_normals(torch.from_numpy(Np).to(dev))
    ctx2.set_target_intensity(torch.from_numpy(Ip).to(dev)); ctx2.set_source_intensity(torch.from_numpy(Iq).to(dev))
    ctx2.estimate_color_gradients(d / 2)
    assert ctx2.target_color_gradients().tobytes() == ctx.target_color_gradients().tobytes()
    assert ctx2.color_sums(Tc).tobytes() == s1.tobytes()
    T3, r3 = ctx2.refine(T0, metric="color")
    assert np.array_equal(T3, T1) and bytes(r3) == bytes(r1)
    # order_source: another summation order, the same pairs
    Ta, ra = ctx.refine(T0, metric="color", max_iterations=1, order_source=True)
    Tb, rb = ctx.refine(T0, metric="color", max_iterations=1, order_source=False)
    assert ra.history_n[0] == rb.history_n[0] == int(s1[0]) and ra.n_corr == rb.n_corr
    assert np.isclose(ra.history_rmse[0], rb.history_rmse[0], rtol=1e-12) and np.max(np.abs(Ta - Tb)) <= 1e-9
    print("color determinism: %d iterations (%s), |T - T_true| %.2g" % (r1.iterations, icp.STATUS_NAMES[r1.status], np.max(np.abs(T1 - T_true))))
    ctx.close(); ctx2.close()


def test_color_refine_trajectory_equals_the_cpu_loop(icp, cpu, bumpy):
    """5: the CPU restatement of the joint sums plus s4p_icp_solve_plane, on the textured bumpy 200 k pair from 1.5 degrees
    off the generator's pose; estimated target normals, gradients within half the search distance."""
    P, Q, T_gt, Ip, Iq = _textured(bumpy, 4.0)
    d = 4 * 0.004
    T0 = H.motion(1.5, 0.004) @ T_gt
    ctx = icp.ICP(0)
    ctx.set_target(P, d)
    ctx.set_source(Q)
    ctx.estimate_normals(d)
    ctx.set_target_intensity(Ip); ctx.set_source_intensity(Iq)
    ctx.estimate_color_gradients(d / 2)
    T, r = ctx.refine(T0, metric="color")
    c = ctx.frame()
    Tc, its, status, hist = CH.cpu_refine_color(cpu, icp.solve_plane, (P - c).astype(np.float32), (Q - c).astype(np.float32),
                                                ctx.target_normals(), ctx.target_color_gradients(), Ip, Iq, c, T0, d)
    print("color trajectory: gpu %d its (%s) rmse %.6g; cpu %d its (%s) |dT| %.2g; rot err %.4g -> %.4g deg"
          % (r.iterations, icp.STATUS_NAMES[r.status], r.rmse, its, icp.STATUS_NAMES[status], np.max(np.abs(T - Tc)),
             H.rot_err_deg(T0, T_gt), H.rot_err_deg(T, T_gt)))
    assert np.max(np.abs(T - Tc)) <= 1e-5
    assert abs(r.iterations - its) <= 1
    k = min(r.history_len, len(hist), 3)
    assert np.allclose(list(r.history_rmse[:k]), hist[:k], rtol=1e-9)
    ctx.close()


def test_color_pins_a_planar_target_where_plane_is_degenerate(icp):
    """6: the case the metric exists for.  z = 0 with a texture: point-to-plane has three free directions, answers
    DEGENERATE and returns the start pose; the coloured metric returns the true pose to 1e-5 with fitness 1, through the
    context and through icp.refine with rgb input.  The status is not asserted: at noise-level rmse the relative test may
    or may not fire."""
    c = CH.planar_case()
    T0 = np.eye(4)
    ctx = icp.ICP(0)
    ctx.set_target(c["P"], c["d"]); ctx.set_source(c["Q"])
    ctx.set_target_normals(c["N"])
    Tp, rp = ctx.refine(T0, metric="plane")
    assert rp.status == icp.DEGENERATE and rp.iterations == 0 and np.array_equal(Tp, T0)
    ctx.set_target_intensity(c["Ip"]); ctx.set_source_intensity(c["Iq"])
    ctx.estimate_color_gradients(c["r"])
    for lam in (icp.COLOR_LAMBDA, 0.5):
        T, r = ctx.refine(T0, metric="color", color_lambda=lam)
        print("planar, lambda %g: |T0 - T_true| %.2g -> |T - T_true| %.2g, %d iterations (%s), rmse %.3g, fitness %.6f"
              % (lam, np.max(np.abs(T0 - c["T_true"])), np.max(np.abs(T - c["T_true"])), r.iterations, icp.STATUS_NAMES[r.status],
                 r.rmse, r.fitness))
        assert np.max(np.abs(T - c["T_true"])) <= 1e-5 and r.fitness == 1.0
    T1, r1 = ctx.refine(T0, metric="color", color_lambda=1.0)          # lambda = 1 is point-to-plane
    assert r1.status == icp.DEGENERATE and np.array_equal(T1, T0)
    ctx.close()
    # the convenience call; an (n, 1) intensity and an (n,) one are the same input
    T2, r2 = icp.refine(c["P"], c["Q"], T0, max_distance=c["d"], metric="color", target_normals=c["N"], target_intensity=c["Ip"][:, None],
                        source_intensity=c["Iq"], color_radius=c["r"])
    assert np.max(np.abs(T2 - c["T_true"])) <= 1e-5 and r2.fitness == 1.0
    Tpl, rpl = icp.refine(c["P"], c["Q"], T0, max_distance=c["d"], metric="plane", target_normals=c["N"])
    assert rpl.status == icp.DEGENERATE and np.array_equal(Tpl, T0)


def _write_ply(path, pts, grey):
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % len(pts))
        f.write("property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
        for p, g in zip(pts, grey):
            f.write("%.9g %.9g %.9g %d %d %d\n" % (p[0], p[1], p[2], g, g, g))


def test_facade_cli_and_binding_agree_on_the_textured_hippo(icp, tmp_path, s4p_lib_built):
    """7: the hippo fixture with a grey texture through MatchSuper4PCS + RefineICP(Colored) (tests/icp_facade_app), through
    `Super4PCS ... --icp 30 --icp-metric color -m` on coloured PLY files, and through icp.refine with rgb input from the same
    Super4PCS result; then what the facade rejects."""
    import torch
    from super4pcs_amd import build as B
    g = np.load(os.path.join(ROOT, "tests", "golden", "hippo_config1.npz"))
    Ps, Qu, Mg = g["Ps"].astype(np.float32), g["Qu"].astype(np.float32), g["M"].astype(np.float64)
    grey_p = np.rint(255 * CH.texture(Ps, 3.0)).astype(np.int64)
    grey_q = np.rint(255 * CH.texture(Qu.astype(np.float64) @ Mg[:3, :3].T + Mg[:3, 3], 3.0)).astype(np.int64)
    rgb_p, rgb_q = np.repeat(grey_p[:, None], 3, 1), np.repeat(grey_q[:, None], 3, 1)
    delta, overlap, n_s = 0.01, 0.7, 200
    exe = apps.build_app(tmp_path, "icp_facade_app", apps.ICP_FACADE_LIBS)
    flags = ("--metric", "color", "--rgb")
    rows, _ = apps.run_icp_app(exe, np.column_stack([Ps, rgb_p]), np.column_stack([Qu, rgb_q]), delta, overlap, n_s, *flags)
    M, Mf = rows["registered"].astype(np.float64), rows["registered"]
    Qm = apps.move_f32(Mf, Qu)
    dT, r = icp.refine(Ps, Qm, np.eye(4), max_distance=np.float32(4.0 * delta), metric="color", target_intensity=rgb_p,
                       source_intensity=rgb_q)
    want = icp.compose(dT, M).astype(np.float32)
    print("hippo color: facade == icp.py max diff %.2g, %d iterations (%s), rmse %.4g"
          % (np.max(np.abs(rows["refined"] - want)), r.iterations, icp.STATUS_NAMES[r.status], r.rmse))
    assert np.max(np.abs(rows["refined"] - want)) <= 1e-6
    assert np.max(np.abs(rows["refined"] - Mf)) > 0
    # torch rgb on the device is the same input
    dev = torch.device("cuda:0")
    dT_t, _ = icp.refine(torch.from_numpy(Ps).to(dev), torch.from_numpy(Qm).to(dev), np.eye(4), max_distance=np.float32(4.0 * delta),
                         metric="color", target_intensity=torch.from_numpy(rgb_p).to(dev), source_intensity=torch.from_numpy(rgb_q).to(dev))
    assert np.array_equal(dT_t, dT)
    # and it is not the plane refinement
    dT_p, _ = icp.refine(Ps, Qm, np.eye(4), max_distance=np.float32(4.0 * delta), metric="plane")
    assert np.max(np.abs(dT_p - dT)) > 0
    # command line
    cli = B.build_cli()
    _write_ply(tmp_path / "P.ply", Ps, grey_p); _write_ply(tmp_path / "Q.ply", Qu, grey_q)
    got, _ = apps.run_cli(cli, tmp_path / "P.ply", tmp_path / "Q.ply", delta, overlap, n_s, ["--icp", "30", "--icp-metric", "color"])
    assert np.max(np.abs(got - want)) <= 2e-6
    # the facade rejects a cloud with a point that has no colour, and a loss
    q_rows = [row[:3] if k == 7 else row for k, row in enumerate(np.column_stack([Qu, rgb_q]))]
    out = apps.start_icp_app(exe, np.column_stack([Ps, rgb_p]), q_rows, delta, overlap, n_s, *flags)
    assert out.returncode == 5 and "invalid:" in out.stdout and "colour" in out.stdout, out.stdout + out.stderr
    out = apps.start_icp_app(exe, np.column_stack([Ps, rgb_p]), np.column_stack([Qu, rgb_q]), delta, overlap, n_s, *flags,
                             "--color-lambda", "0.968", "--loss", "huber")
    assert out.returncode == 5 and "invalid:" in out.stdout and "loss" in out.stdout, out.stdout + out.stderr


@pytest.fixture(scope="module")
def first_hit(cpu, bumpy):
    """The first source point of the bumpy pair with a correspondence at the edge test's transform (CPU restatement)."""
    P, Q, T_gt = bumpy
    c = P.astype(np.float64).mean(0).astype(np.float32)
    idx, _, _ = cpu.pass_((P - c).astype(np.float32), (Q - c).astype(np.float32), H.to_centred(H.motion(0.3, 0.002) @ T_gt, c).astype(np.float32),
                          4 * 0.004)
    return int(np.flatnonzero(idx >= 0)[0])


@pytest.fixture(scope="module")
def edge_target(icp, bumpy):
    """One target context for the edge sizes: caller normals with zeros, a texture with a constant stretch, gradients."""
    P = bumpy[0]
    d = 4 * 0.004
    Ip = _flatten_stretches(CH.texture(P, 4.0), P)
    ctx = icp.ICP(0)
    ctx.set_target(P, d)
    ctx.estimate_normals(d, MIN_NB)
    Np = ctx.target_normals()
    Np[::13] = 0
    ctx.set_target_normals(Np)
    Np = ctx.target_normals()
    ctx.set_target_intensity(Ip)
    ctx.estimate_color_gradients(d / 2, MIN_NB)
    yield ctx, Np, ctx.target_color_gradients(), Ip
    ctx.close()


@pytest.mark.parametrize("n_q", [1, 63, 64, 65, 257, 524_289])
def test_color_sums_at_edge_sizes(icp, cpu, bumpy, first_hit, edge_target, n_q):
    """8: one lane, a ragged wave, exactly one wave, one lane more, a ragged second workgroup; and 524 289 source points:
    one more than the 2048 x 256 lanes of a full launch, so the grid-stride loop runs a second, ragged round."""
    P, Q, T_gt = bumpy
    ctx, Np, G, Ip = edge_target
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
    Iq = CH.texture(Qn.astype(np.float64) @ T_gt[:3, :3].T + T_gt[:3, 3], 4.0)
    ctx.set_source(Qn)
    ctx.set_source_intensity(Iq)
    n, nt = _check_color_sums(ctx, cpu, P, Qn, Np, G, Ip, Iq, H.motion(0.3, 0.002) @ T_gt, d)
    print("edge size %d: %d pairs, %d with a term" % (n_q, n, nt))
    assert n >= (1 if n_q < 1000 else 1000)
    T, r = ctx.refine(T_gt, metric="color", max_iterations=2)
    assert np.all(np.isfinite(T)) and r.history_n[0] >= 1
