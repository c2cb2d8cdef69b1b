"""Correspondence rejection on the MI355X (include/s4p_icp_reject.h): the per-point answers and the counts against the numpy
restatement (tests/icp_reject_helpers.py) bit for bit, every sums call on the kept pairs, weight-1 equality with the fused
kernels, ties / duplicates / the bound d on a dyadic lattice, edge sizes and degenerate source grids, determinism, the refine
trajectory against the CPU loop, state errors, the facade / command line / Python binding agreeing, and multi-scale."""
import ctypes
import os

import numpy as np
import pytest

from tests import icp_color_helpers as CH
from tests import icp_gicp_helpers as GH
from tests import apps
from tests import icp_helpers as H
from tests import icp_plane_helpers as PH
from tests import icp_reject_helpers as JH
from tests import icp_robust_helpers as RH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
MIN_NB = 6
COS60 = float(np.cos(np.deg2rad(60.0)))


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


def _set(ctx, kw):
    ctx.set_rejection(reciprocal=kw.get("reciprocal", False), oriented=kw.get("normal_mode", 0) == 2,
                      normal_cos=kw["normal_cos"] if kw.get("normal_mode", 0) else None)


def _check_contract(ctx, cpu, Pc, Qc, Tc, d, kw, Np=None, Nq=None, forward=None):
    """idx, d2, why and the four counts equal the restatement bit for bit; returns the restatement."""
    _set(ctx, kw)
    gi, gd, gw = ctx.rejection(Tc)
    gc = ctx.rejection_counts()
    ci, cd, cw, cc = JH.restate(JH.cpu_search(cpu), Pc, Qc, Tc, d, Np=Np, Nq=Nq, forward=forward, **kw)
    assert np.array_equal(gw, cw), (kw, np.flatnonzero(gw != cw)[:10])
    assert np.array_equal(gi, ci) and gd.tobytes() == cd.tobytes(), kw
    assert np.array_equal(gc, cc), (kw, gc, cc)
    return ci, cd, cw, cc


def test_rejection_is_the_contract_per_point(icp, cpu, bumpy, lidar):
    """1: reciprocal only, normals only in each mode, both together; raw caller normals (zeros, a NaN, not unit length) at 60
    degrees and estimated normals of both clouds at 30 degrees (45 for the oriented test: the estimates' signs are set per
    cloud, in its own frame); the generator's pose and two perturbed ones.  Every case both keeps and rejects more than 1000
    pairs: at the generator's pose the two clouds' estimated normals agree within 30 degrees up to sign on 34 % of the bumpy
    pairs and 44 % of the lidar pairs, and within 45 degrees with sign on 6 % and 56 %."""
    from super4pcs_amd import normals
    rng = np.random.default_rng(4)
    cos30, cos45 = float(np.cos(np.deg2rad(30.0))), float(np.cos(np.deg2rad(45.0)))
    for name, (P, Q, T_gt), d in (("bumpy", bumpy, 4 * 0.004), ("lidar", lidar, 4 * 0.05)):
        ctx = icp.ICP(0)
        ctx.set_target(P, d)
        ctx.set_source(Q)
        c = ctx.frame()
        Pc, Qc = (P - c).astype(np.float32), (Q - c).astype(np.float32)
        raw_p, raw_q = H.raw_normals(rng, len(P)), H.raw_normals(rng, len(Q))
        Nq_est = normals.estimate_normals(Q, k=16)
        for ang, sh in ((0.0, 0.0), (0.3, 0.002), (-1.0, 0.01)):
            Tc = H.to_centred(RH.motion(ang, sh) @ T_gt, c).astype(np.float32)
            fwd = JH.cpu_search(cpu)(Pc, Qc, Tc, d)
            gi, gd = ctx.correspondences(Tc)
            assert np.array_equal(gi, fwd[0]) and np.array_equal(gd, fwd[1])       # the forward search is unchanged
            for kind in ("raw", "estimated"):
                if kind == "raw":
                    ctx.set_target_normals(raw_p); ctx.set_source_normals(raw_q)
                    cos = cos_o = COS60
                else:
                    ctx.estimate_normals(d, MIN_NB); ctx.set_source_normals(Nq_est)
                    cos, cos_o = cos30, cos45
                Np, Nq = ctx.target_normals(), ctx.source_normals()
                cases = [dict(normal_mode=1, normal_cos=cos), dict(normal_mode=2, normal_cos=cos_o),
                         dict(reciprocal=True, normal_mode=1, normal_cos=cos)]
                if kind == "raw":
                    cases.insert(0, dict(reciprocal=True))
                for kw in cases:
                    _, _, _, cc = _check_contract(ctx, cpu, Pc, Qc, Tc, d, kw, Np, Nq, forward=fwd)
                    print("%s %+.1f deg, %s normals, %s: matched %d, by normals %d, by reciprocity %d, kept %d"
                          % (name, ang, kind, kw, cc[0], cc[1], cc[2], cc[3]))
                    assert cc[3] > 1000 and cc[1] + cc[2] > 1000, (name, ang, kind, kw, cc)
            assert np.array_equal(ctx.correspondences(Tc)[0], fwd[0])               # and stays the raw one-way search
        ctx.close()


def _close(gs, cs, cabs):
    err = np.abs(gs - cs)
    assert np.all(err <= 1e-10 * np.maximum(cabs, 1e-300)), (gs, cs, err / np.maximum(cabs, 1e-300))


ROBUST_CASES = [dict(loss="trimmed", trim_fraction=0.7), dict(loss="trimmed", trim_fraction=0.1), dict(loss="huber"), dict(loss="tukey"),
                dict(loss="tukey", scale=0.01)]


def test_every_sums_call_runs_over_the_kept_pairs(icp, cpu, bumpy):
    """2: s4p_icp_sums, _plane_sums, _gicp_sums, _color_sums and _robust_sums (each loss, both metrics) under rejection equal
    the helpers of each metric fed the kept index array: counts exactly, M / k / threshold bits / s / count of the robust info
    exactly, every sum within 1e-10 of its sum of |term|."""
    P, Q, T_gt = bumpy
    d = 4 * 0.004
    rng = np.random.default_rng(9)
    ctx = icp.ICP(0)
    ctx.set_target(P, d); ctx.set_source(Q)
    c = ctx.frame()
    Pc, Qc = (P - c).astype(np.float32), (Q - c).astype(np.float32)
    ctx.estimate_normals(d, MIN_NB)
    ctx.set_source_normals(H.raw_normals(rng, len(Q)))
    Ip, Iq = CH.texture(P, 4.0), CH.texture(Q, 4.0)
    ctx.set_target_intensity(Ip); ctx.set_source_intensity(Iq)
    ctx.estimate_color_gradients(d / 2, MIN_NB)
    Np, Nq, G = ctx.target_normals(), ctx.source_normals(), ctx.target_color_gradients()
    Tc = H.to_centred(RH.motion(0.5, 0.002) @ T_gt, c).astype(np.float32)
    fwd = JH.cpu_search(cpu)(Pc, Qc, Tc, d)
    for kw in (dict(reciprocal=True), dict(reciprocal=True, normal_mode=1, normal_cos=COS60)):
        ki, kd, _, cc = _check_contract(ctx, cpu, Pc, Qc, Tc, d, kw, Np, Nq, forward=fwd)
        n = int(cc[3])
        assert n > 1000 and cc[0] - n > 1000
        # point
        gs = ctx.sums(Tc)
        cs, _ = RH.robust_sums(Pc, Qc, Tc, ki, kd, "point", "trimmed", len(Q), d, trim_fraction=1.0)
        assert gs[0] == n == cs[0]
        _close(gs, cs, JH.sums_abs(Pc, Qc, Tc, ki, kd, "point"))
        assert np.array_equal(ctx.rejection_counts(), cc)                       # a sums call reports the same counts
        # plane
        gs = ctx.plane_sums(Tc)
        cs = PH.plane_sums(Pc, Qc, Tc, ki, kd, Np)
        assert gs[0] == n == cs[0] and gs[2] == cs[2]
        _close(gs, cs, JH.sums_abs(Pc, Qc, Tc, ki, kd, "plane", Np))
        # generalized
        gs = ctx.gicp_sums(Tc, 1e-3)
        cs, cabs = GH.gicp_sums(Pc, Qc, Tc, ki, kd, Np, Nq, 1e-3)
        assert gs[0] == gs[2] == n == cs[0]
        _close(gs, cs, cabs)
        # coloured
        gs = ctx.color_sums(Tc, 0.968)
        cs, cabs = CH.color_sums(Pc, Qc, Tc, ki, kd, Np, G, Ip, Iq, 0.968)
        assert gs[0] == n == cs[0] and gs[2] == cs[2]
        _close(gs, cs, cabs)
        assert np.array_equal(ctx.rejection_counts(), cc)
        # robust: the selection runs over the survivors
        for rk in ROBUST_CASES:
            for metric in ("point", "plane"):
                gs, gi = ctx.robust_sums(Tc, metric, **rk)
                cs, ii = RH.robust_sums(Pc, Qc, Tc, ki, kd, metric, n_q=len(Q), d=d, Nc=Np, **rk)
                assert np.array_equal(gi[[0, 1, 2, 4, 6, 7]], ii[[0, 1, 2, 4, 6, 7]]), (kw, metric, rk, gi, ii)
                assert gi[3] == ii[3] and gi[5] == gs[0] and gi[0] <= n
                if metric == "plane":
                    assert gs[2] == cs[2]
                loss = rk["loss"]
                extra = {k: v for k, v in rk.items() if k != "loss"}
                _close(gs, cs, JH.sums_abs(Pc, Qc, Tc, ki, kd, metric, Np, loss=loss, n_q=len(Q), d=d, **extra))
    ctx.close()


def test_a_filter_that_rejects_nothing_gives_the_fused_kernels_bits(icp, bumpy):
    """3: oriented mode with cos = -1 and reciprocity off rejects nothing: sums and plane_sums under rejection (search,
    k_reject, weighted sums with every weight 1) are bit-identical to the fused k_match / k_match_plane with rejection off."""
    P, Q, T_gt = bumpy
    d = 4 * 0.004
    rng = np.random.default_rng(12)
    ctx = icp.ICP(0)
    ctx.set_target(P, d); ctx.set_source(Q)
    ctx.estimate_normals(d, MIN_NB)
    ctx.set_source_normals(rng.normal(size=Q.shape).astype(np.float32))
    c = ctx.frame()
    for ang, sh in ((0.0, 0.0), (0.7, -0.003)):
        Tc = H.to_centred(RH.motion(ang, sh) @ T_gt, c).astype(np.float32)
        ctx.set_rejection()
        s_off, p_off = ctx.sums(Tc), ctx.plane_sums(Tc)
        ctx.set_rejection(oriented=True, normal_cos=-1.0)
        s_on, p_on = ctx.sums(Tc), ctx.plane_sums(Tc)
        cc = ctx.rejection_counts()
        assert s_on.tobytes() == s_off.tobytes() and p_on.tobytes() == p_off.tobytes()
        assert cc[0] == cc[3] == int(s_off[0]) > 1000 and cc[1] == cc[2] == 0
    T0 = RH.motion(1.0, 0.002) @ T_gt
    ctx.set_rejection()
    a = [ctx.refine(T0, max_iterations=5, metric=m) for m in ("point", "plane")]
    ctx.set_rejection(oriented=True, normal_cos=-1.0)
    b = [ctx.refine(T0, max_iterations=5, metric=m) for m in ("point", "plane")]
    for (Ta, ra), (Tb, rb) in zip(a, b):
        assert np.array_equal(Ta, Tb) and bytes(ra) == bytes(rb)
    ctx.close()


def test_ties_duplicates_and_the_bound_on_a_dyadic_lattice(icp):
    """4: coordinates on a 2^-10 lattice, P symmetric about 0 (the frame is exactly 0), d = 2^-6, identity T: a target
    equidistant from two source points keeps the lower index only; of a duplicated source point the lower index only; a source
    point exactly at d is matched and kept.  Then T = 2 I (not rigid, exact on the lattice): p~ = 2 p' lies more than one
    cell outside the source grid for the outer targets.  Everything against numpy_brute in both directions."""
    u = np.float32(1.0 / 1024)
    d = 16 * u
    rng = np.random.default_rng(7)
    A = rng.integers(-512, 512, size=(600, 3)).astype(np.float32)
    made = np.array([[100, 0, 2000], [200, 0, 2000], [300, 0, 2000]], np.float32)
    half = np.concatenate([made, A])
    P = (np.concatenate([half, -half]) * u).astype(np.float32)
    Qs = np.array([[108, 0, 2000], [92, 0, 2000],           # 0, 1: both nearest to target 0, which is equidistant from them
                   [200, 4, 2000], [200, 4, 2000],          # 2, 3: one point twice
                   [316, 0, 2000],                          # 4: exactly at d from target 2
                   [317, 0, 2000]], np.float32)             # 5: one lattice step beyond d
    Q = (np.concatenate([Qs, A[:300] + rng.integers(-6, 7, size=(300, 3)), A[:100] + rng.integers(-6, 7, size=(100, 3))]) * u).astype(np.float32)
    ctx = icp.ICP(0)
    ctx.set_target(P, float(d)); ctx.set_source(Q)
    assert not ctx.frame().any()
    ctx.set_rejection(reciprocal=True)
    I = np.eye(4, dtype=np.float32)
    gi, gd, gw = ctx.rejection(I)
    bi, bd, bw, bc = JH.restate(H.numpy_brute, P, Q, I, float(d), reciprocal=True)
    assert np.array_equal(gi, bi) and gd.tobytes() == bd.tobytes() and np.array_equal(gw, bw)
    assert np.array_equal(ctx.rejection_counts(), bc)
    assert gw[:6].tolist() == [0, 3, 0, 3, 0, 1] and gi[:6].tolist() == [0, -1, 1, -1, 2, -1]
    assert gd[4] == d * d and gd[0] == np.float32(64) * u * u
    assert bc[3] > 100 and bc[2] > 10
    # the reverse search by itself, for every target
    rb = JH.reverse_search(H.numpy_brute, P, Q, I, float(d), np.arange(len(P)))
    assert rb[0] == 0 and rb[1] == 2 and rb[2] == 4
    ctx.close()
    # T = 2 I on sources at half the targets' coordinates
    T2 = np.diag([2, 2, 2, 1]).astype(np.float32)
    Q2 = (P[rng.choice(len(P), 500, replace=False)] * np.float32(0.5)).astype(np.float32)
    ctx = icp.ICP(0)
    ctx.set_target(P, float(d)); ctx.set_source(Q2)
    ctx.set_rejection(reciprocal=True)
    gi, gd, gw = ctx.rejection(T2)
    bi, bd, bw, bc = JH.restate(H.numpy_brute, P, Q2, T2, float(d), reciprocal=True)
    assert np.array_equal(gi, bi) and gd.tobytes() == bd.tobytes() and np.array_equal(gw, bw)
    assert np.array_equal(ctx.rejection_counts(), bc) and bc[0] == 500
    pt = RH.apply_f32(JH.reverse_map(T2), P[H.numpy_brute(P, Q2, T2, float(d))[0]])
    outside = np.any((pt > Q2.max(0) + 4 * d) | (pt < Q2.min(0) - 4 * d), axis=1)
    assert outside.sum() > 100 and np.all(gw[outside] == 3)
    ctx.close()


@pytest.fixture(scope="module")
def first_hit(cpu, bumpy):
    """The first source point of the bumpy pair with a correspondence at the edge test's transform (CPU restatement)."""
    P, Q, T_gt = bumpy
    c = P.astype(np.float64).mean(0).astype(np.float32)
    idx, _, _ = cpu.pass_((P - c).astype(np.float32), (Q - c).astype(np.float32), H.to_centred(RH.motion(0.3, 0.002) @ T_gt, c).astype(np.float32),
                          4 * 0.004)
    return int(np.flatnonzero(idx >= 0)[0])


@pytest.mark.parametrize("n_q", [1, 63, 64, 65, 257, 524_289])
def test_rejection_at_edge_sizes(icp, cpu, bumpy, first_hit, n_q):
    """5: one lane, a ragged wave, exactly one wave, one lane more, a ragged second workgroup; and 524 289 source points:
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
    ctx.set_source_normals(H.raw_normals(rng, n_q))
    ctx.estimate_normals(d, MIN_NB)
    Np, Nq = ctx.target_normals(), ctx.source_normals()
    c = ctx.frame()
    Pc, Qc = (P - c).astype(np.float32), (Qn - c).astype(np.float32)
    Tc = H.to_centred(RH.motion(0.3, 0.002) @ T_gt, c).astype(np.float32)
    fwd = JH.cpu_search(cpu)(Pc, Qc, Tc, d)
    for kw in (dict(reciprocal=True), dict(reciprocal=True, normal_mode=1, normal_cos=COS60)):
        ki, kd, _, cc = _check_contract(ctx, cpu, Pc, Qc, Tc, d, kw, Np, Nq, forward=fwd)
        print("edge size %d, %s: counts %s" % (n_q, kw, cc.tolist()))
        assert cc[0] >= 1 and (n_q < 1000 or (cc[3] > 1000 and cc[2] > 1000))
        gs = ctx.gicp_sums(Tc, 1e-3)
        cs, cabs = GH.gicp_sums(Pc, Qc, Tc, ki, kd, Np, Nq, 1e-3)
        assert gs[0] == cc[3]
        _close(gs, cs, cabs)
    T, r = ctx.refine(T_gt, max_iterations=2)
    assert np.all(np.isfinite(T)) and r.history_n[0] <= fwd[0].size
    ctx.close()


def test_degenerate_source_grids(icp, cpu, bumpy):
    """5, continued: a source inside one cell of its grid, a needle-shaped source (a line of cells), and a source whose box
    is disjoint from the target's: every count zero and refine is TOO_FEW."""
    P, Q, T_gt = bumpy
    d = 4 * 0.004
    ctx = icp.ICP(0)
    ctx.set_target(P, d)
    c = ctx.frame()
    Pc = (P - c).astype(np.float32)
    Tc = H.to_centred(T_gt, c).astype(np.float32)
    fi, _ = JH.cpu_search(cpu)(Pc, (Q - c).astype(np.float32), Tc, d)
    q0 = Q[np.flatnonzero(fi >= 0)[500]].astype(np.float64)            # a source point well inside the overlap
    rng = np.random.default_rng(15)
    cell = q0 + rng.uniform(-0.4 * d, 0.4 * d, size=(40, 3))           # a box of 0.8 d: one cell of edge 1.02 d
    t = np.linspace(-10 * d, 10 * d, 400)
    needle = q0 + np.column_stack([t, rng.uniform(-0.3 * d, 0.3 * d, 400), rng.uniform(-0.3 * d, 0.3 * d, 400)])
    for name, Qn, dims in (("one cell", cell, (1, 1, 1)), ("needle", needle, (20, 1, 1))):
        Qn = Qn.astype(np.float32)
        ctx.set_source(Qn)
        Qc = (Qn - c).astype(np.float32)
        assert tuple(int(v) for v in np.floor((Qc.max(0).astype(np.float64) - Qc.min(0)) / (1.02 * float(np.float32(d)))) + 1) == dims
        _, _, _, cc = _check_contract(ctx, cpu, Pc, Qc, Tc, d, dict(reciprocal=True))
        print("%s: %d source points, counts %s" % (name, len(Qn), cc.tolist()))
        assert cc[0] >= 30 and cc[3] >= 10 and cc[2] >= 10
    far = (Q + np.float32(1000.0)).astype(np.float32)
    ctx.set_source(far[:5000])
    ctx.set_rejection(reciprocal=True)
    gi, gd, gw = ctx.rejection(Tc)
    assert np.all(gi == -1) and not gd.any() and np.all(gw == 1) and not ctx.rejection_counts().any()
    T, r = ctx.refine(T_gt)
    assert r.status == icp.TOO_FEW and r.iterations == 0 and r.n_corr == 0 and np.max(np.abs(T - T_gt)) <= 1e-12
    ctx.close()


def test_rejection_is_deterministic_and_torch_agrees(icp, bumpy):
    """6: two calls give identical bits; numpy and GPU torch inputs give identical bits; order_source on and off see the same
    surviving pairs."""
    import torch
    P, Q, T_gt = bumpy
    d = 4 * 0.004
    rng = np.random.default_rng(3)
    Nq = rng.normal(size=Q.shape).astype(np.float32)
    T0 = RH.motion(1.0, 0.002) @ T_gt
    ctx = icp.ICP(0)
    ctx.set_target(P, d); ctx.set_source(Q)
    ctx.estimate_normals(d, MIN_NB); ctx.set_source_normals(Nq)
    ctx.set_rejection(reciprocal=True, normal_angle=60)
    Tc = H.to_centred(T0, ctx.frame()).astype(np.float32)
    a, b = ctx.rejection(Tc), ctx.rejection(Tc)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    s1, s2 = ctx.gicp_sums(Tc), ctx.gicp_sums(Tc)
    assert s1.tobytes() == s2.tobytes()
    T1, r1 = ctx.refine(T0, max_iterations=6)
    T2, r2 = ctx.refine(T0, max_iterations=6)
    assert np.array_equal(T1, T2) and bytes(r1) == bytes(r2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, ctx.rejection(Tc)))     # a refine leaves the stage call alone
    dev = torch.device("cuda:0")
    ctx2 = icp.ICP(0)
    ctx2.set_target(torch.from_numpy(P).to(dev), d); ctx2.set_source(torch.from_numpy(Q).to(dev))
    ctx2.estimate_normals(d, MIN_NB); ctx2.set_source_normals(torch.from_numpy(Nq).to(dev))
    ctx2.set_rejection(reciprocal=True, normal_angle=60)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, ctx2.rejection(Tc)))
    assert ctx2.gicp_sums(Tc).tobytes() == s1.tobytes()
    T3, r3 = ctx2.refine(T0, max_iterations=6)
    assert np.array_equal(T3, T1) and bytes(r3) == bytes(r1)
    # order_source: another lane order, the same pairs
    kept = int(np.count_nonzero(a[2] == 0))
    for metric in ("point", "gicp"):
        Ta, ra = ctx.refine(T0, max_iterations=1, order_source=True, metric=metric)
        Tb, rb = ctx.refine(T0, max_iterations=1, order_source=False, metric=metric)
        assert ra.history_n[0] == rb.history_n[0] == kept and ra.n_corr == rb.n_corr
        assert np.isclose(ra.history_rmse[0], rb.history_rmse[0], rtol=1e-12) and np.max(np.abs(Ta - Tb)) <= 1e-9
    ctx.close(); ctx2.close()


def test_refine_trajectory_under_reciprocity_equals_the_cpu_loop(icp, cpu, bumpy):
    """7: point and generalized metrics with reciprocity on, eight iterations from 1.5 degrees off the generator's pose,
    against the CPU loop on the restatement under the existing trajectory tests' rule: |dT| <= 1e-5, iterations within one,
    the same status, the first history entries to 1e-9; and the survivors' count of every iteration exactly."""
    from super4pcs_amd import normals
    P, Q, T_gt = bumpy
    d = 4 * 0.004
    T0 = RH.motion(1.5, 0.004) @ T_gt
    ctx = icp.ICP(0)
    ctx.set_target(P, d); ctx.set_source(Q)
    ctx.estimate_normals(d)
    ctx.set_source_normals(normals.estimate_normals(Q, k=16))
    ctx.set_rejection(reciprocal=True)
    c = ctx.frame()
    Pc, Qc = (P - c).astype(np.float32), (Q - c).astype(np.float32)
    for metric in ("point", "gicp"):
        T, r = ctx.refine(T0, metric=metric, max_iterations=8)
        if metric == "point":
            Tc, its, status, hist, hist_n = JH.cpu_refine_reject(cpu, icp.solve, Pc, Qc, c, T0, d, max_iterations=8, reciprocal=True)
        else:
            Tc, its, status, hist, hist_n = JH.cpu_refine_gicp_reject(cpu, icp.solve_plane, Pc, Qc, ctx.target_normals(), ctx.source_normals(),
                                                                      c, T0, d, max_iterations=8, reciprocal=True)
        print("%s trajectory under reciprocity: gpu %d its (%s) rmse %.6g n %s; cpu %d its (%s) |dT| %.2g"
              % (metric, r.iterations, icp.STATUS_NAMES[r.status], r.rmse, list(r.history_n[:r.history_len]), its, icp.STATUS_NAMES[status],
                 np.max(np.abs(T - Tc))))
        assert np.max(np.abs(T - Tc)) <= 1e-5
        assert abs(r.iterations - its) <= 1 and r.status == status
        k = min(r.history_len, len(hist), 3)
        assert np.allclose(list(r.history_rmse[:k]), hist[:k], rtol=1e-9)
        assert list(r.history_n[:k]) == hist_n[:k] and 1000 < r.n_corr < 0.6 * len(Q)
        assert r.fitness == r.n_corr / len(Q)
    ctx.close()


def test_state_and_argument_errors(icp, cpu, bumpy):
    """8: -7 for a normal test without source normals or without target normals, at the first pass; -1 for a bad cosine, mode
    or flag; set_source after set_rejection rebuilds the source grid, and the results on the new source are the contract."""
    P, Q, T_gt = bumpy
    P, Q = P[:40_000], Q[:20_000]
    d = 4 * 0.004
    rng = np.random.default_rng(6)
    ctx = icp.ICP(0)
    ctx.set_target(P, d); ctx.set_source(Q)
    c = ctx.frame()
    Pc = (P - c).astype(np.float32)
    Tc = H.to_centred(T_gt, c).astype(np.float32)

    def code(fn):
        with pytest.raises(icp.ICPError) as e:
            fn()
        return e.value.code

    ctx.set_rejection(normal_angle=60)                                 # accepted: the state is checked at the first pass
    calls = (lambda: ctx.sums(Tc), lambda: ctx.rejection(Tc), lambda: ctx.refine(T_gt), lambda: ctx.refine(T_gt, loss="huber"),
             lambda: ctx.robust_sums(Tc, "point", "huber"))
    assert all(code(f) == -7 for f in calls)                           # neither
    ctx.set_source_normals(rng.normal(size=Q.shape).astype(np.float32))
    assert all(code(f) == -7 for f in calls)                           # no target normals
    ctx.estimate_normals(d)
    for f in calls:
        f()
    ctx.set_target(P, d)                                               # drops the target normals
    assert all(code(f) == -7 for f in calls)
    ctx.estimate_normals(d)
    ctx.set_source(Q)                                                  # drops the source normals
    assert all(code(f) == -7 for f in calls)
    ctx.set_rejection()                                                # off: nothing is needed
    ctx.sums(Tc); ctx.refine(T_gt, max_iterations=1)
    idx, d2, why = ctx.rejection(Tc)                                   # off: the one-way search
    gi, gd = ctx.correspondences(Tc)
    assert np.array_equal(idx, gi) and np.array_equal(d2, gd) and np.array_equal(why, (gi < 0).astype(np.int32))
    for kw in (dict(normal_cos=1.5), dict(normal_cos=-0.1), dict(normal_cos=float("nan")), dict(normal_cos=-1.5, oriented=True),
               dict(normal_cos=1.0000001, oriented=True)):
        assert code(lambda: ctx.set_rejection(**kw)) == -1, kw
    for rec, mode in ((2, 0), (-1, 0), (0, 3), (0, -1)):
        r = icp.Reject()
        r.reciprocal, r.normal_mode = rec, mode
        assert ctx.L.s4p_icp_set_rejection(ctx.h, ctypes.byref(r)) == -1
    with pytest.raises(ValueError):
        ctx.set_rejection(normal_angle=60, normal_cos=0.5)
    # a failed set_rejection leaves the state as it was (off)
    assert np.array_equal(ctx.rejection(Tc)[2], (gi < 0).astype(np.int32))
    # set_source after set_rejection: the grid follows the new source
    ctx.set_rejection(reciprocal=True)
    for Qn in (Q, Q[5000:17_001], Q[::-1].copy()):
        ctx.set_source(Qn)
        _, _, _, cc = _check_contract(ctx, cpu, Pc, (Qn - c).astype(np.float32), Tc, d, dict(reciprocal=True))
        assert cc[3] > 1000 and cc[2] > 1000
    # and a new target (another frame, another d) drops it too
    ctx.set_target(P[:30_000], 2 * d)
    c2 = ctx.frame()
    Tc2 = H.to_centred(T_gt, c2).astype(np.float32)
    _, _, _, cc = _check_contract(ctx, cpu, (P[:30_000] - c2).astype(np.float32), (Qn - c2).astype(np.float32), Tc2, 2 * d,
                                  dict(reciprocal=True))
    assert cc[3] > 1000 and cc[2] > 1000
    ctx.close()


def test_facade_cli_and_binding_agree_on_the_hippo(icp, tmp_path, s4p_lib_built):
    """9: the hippo fixture through MatchSuper4PCS + RefineICP with reciprocal and normal_angle_deg = 60
    (tests/icp_facade_app), through `Super4PCS ... --icp 30 --icp-reciprocal --icp-normal-angle 60 -m`, and through icp.refine
    from the same Super4PCS result."""
    from super4pcs_amd import build as B
    g = np.load(os.path.join(ROOT, "tests", "golden", "hippo_config1.npz"))
    Ps, Qu = g["Ps"].astype(np.float32), g["Qu"].astype(np.float32)
    delta, overlap, n_s = 0.01, 0.7, 200
    exe = apps.build_app(tmp_path, "icp_facade_app", apps.ICP_FACADE_LIBS)

    def app(metric, angle):
        rows, stats = apps.run_icp_app(exe, Ps, Qu, delta, overlap, n_s, "--metric", metric, "--reciprocal", "--normal-angle-deg", angle)
        return rows, int(stats[6])

    rows, n_app = app("point", 60)
    M, Mf = rows["registered"].astype(np.float64), rows["registered"]
    Qm = apps.move_f32(Mf, Qu)
    dT, r = icp.refine(Ps, Qm, np.eye(4), max_distance=np.float32(4.0 * delta), reciprocal=True, normal_angle=60)
    dT0, r0 = icp.refine(Ps, Qm, np.eye(4), max_distance=np.float32(4.0 * delta))
    want = icp.compose(dT, M).astype(np.float32)
    print("hippo under rejection: facade == icp.py max diff %.2g, %d iterations (%s), rmse %.4g, n_corr %d (one-way %d)"
          % (np.max(np.abs(rows["refined"] - want)), r.iterations, icp.STATUS_NAMES[r.status], r.rmse, r.n_corr, r0.n_corr))
    assert np.max(np.abs(rows["refined"] - want)) <= 1e-6 and n_app == r.n_corr
    assert 3 <= r.n_corr < r0.n_corr and np.max(np.abs(rows["refined"] - Mf)) > 0
    # the other metrics take the options too
    for metric in ("plane", "gicp"):
        rows_m, n_m = app(metric, 60)
        assert np.array_equal(rows_m["registered"], Mf)
        dTm, rm = icp.refine(Ps, Qm, np.eye(4), max_distance=np.float32(4.0 * delta), metric=metric, reciprocal=True, normal_angle=60)
        assert np.max(np.abs(rows_m["refined"] - icp.compose(dTm, M).astype(np.float32))) <= 1e-6 and n_m == rm.n_corr
    # command line
    cli = B.build_cli()
    apps.write_obj(tmp_path / "P.obj", Ps); apps.write_obj(tmp_path / "Q.obj", Qu)
    got, _ = apps.run_cli(cli, tmp_path / "P.obj", tmp_path / "Q.obj", delta, overlap, n_s,
                          ["--icp", "30", "--icp-reciprocal", "--icp-normal-angle", "60"])
    assert np.max(np.abs(got - want)) <= 2e-6


def test_multiscale_forwards_the_rejection(icp):
    """10: refine_multiscale(..., reciprocal=True) equals the hand-run levels, bit for bit."""
    from super4pcs_amd import multiscale, voxel
    from tests import multiscale_helpers as MH
    case = MH.small_pair()
    P, Q, T0 = case["P"], case["Q"], case["T0"]
    voxels, its, d_fine = (0.15, 0.06, 0), (6, 6, 6), 0.05
    for kw in (dict(reciprocal=True), dict(reciprocal=True, normal_angle=60, metric="plane")):
        T, levels = multiscale.refine_multiscale(P, Q, T0=T0, voxel_sizes=voxels, max_distance=d_fine, max_iterations=its, **kw)
        Tn, plain = multiscale.refine_multiscale(P, Q, T0=T0, voxel_sizes=voxels, max_distance=d_fine, max_iterations=its,
                                                 metric=kw.get("metric", "point"))
        Tc = T0
        for l, (v, it) in enumerate(zip(voxels, its)):
            Pl = voxel.voxel_downsample(P, v)[0] if v > 0 else P
            Ql = voxel.voxel_downsample(Q, v)[0] if v > 0 else Q
            Tc, r = icp.refine(Pl, Ql, T0=Tc, max_distance=max(d_fine, 3.0 * v), max_iterations=it, **kw)
            assert bytes(r) == bytes(levels[l]), (kw, l, r.as_dict(), levels[l].as_dict())
        assert np.array_equal(T, Tc)
        assert 0 < levels[-1].n_corr < plain[-1].n_corr
