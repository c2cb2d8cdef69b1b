"""Symmetric ICP on the MI355X (include/s4p_icp_symm.h): the symmetric sums against the numpy restatement
(tests/icp_symm_helpers.py), edge sizes, the sign rule, zero normals, rejection, determinism, the trajectory against the CPU
loop, an exact pose, a planar target, state and argument errors, the facade / command line / Python binding agreeing, and the
multi-scale chain."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import apps
from tests import icp_helpers as H
from tests import icp_plane_helpers as PH
from tests import icp_symm_helpers as SH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
MIN_NB = 6
DELTA = 0.004
D_BUMPY = 4 * DELTA


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
    return D.bumpy_pair(20_000, overlap=0.5, delta=DELTA, seed=11)


@pytest.fixture(scope="module")
def lidar():
    from super4pcs_amd import datasets as D
    return D.lidar_pair_scaled(0.02, delta=0.05)




def _frames(ctx, P, Q, T_caller):
    c = ctx.frame()
    return (P - c).astype(np.float32), (Q - c).astype(np.float32), H.to_centred(T_caller, c).astype(np.float32)


def _assert_sums(gs, cs, cabs, what):
    assert gs[0] == cs[0] and gs[2] == cs[2], (what, gs[:3], cs[:3])
    err = np.abs(gs - cs)
    worst = float(np.max(err / np.maximum(cabs, 1e-300)))
    print("symmetric sums, %s: n %d, with a term %d: max |gpu - cpu| / sum|term| %.3g" % (what, int(gs[0]), int(gs[2]), worst))
    assert np.all(err <= 1e-10 * cabs), (what, gs, cs)


def _check_symm_sums(ctx, cpu, P, Q, Np, Nq, T_caller, d, what=""):
    """Correspondences bit for bit, [0] and [2] exactly, every other entry within 1e-10 of its sum of |term|."""
    Pc, Qc, Tc = _frames(ctx, P, Q, T_caller)
    gi, gd = ctx.correspondences(Tc)
    ci, cd, _ = cpu.pass_(Pc, Qc, Tc, d)
    assert np.array_equal(gi, ci) and np.array_equal(gd, cd)
    gs = ctx.symmetric_sums(Tc)
    cs, cabs = SH.symm_sums(Pc, Qc, Tc, ci, cd, Np, Nq)
    assert gs[0] == np.count_nonzero(ci >= 0)
    _assert_sums(gs, cs, cabs, "n_Q %d %s" % (len(Q), what))
    return int(cs[0]), int(cs[2])


def test_symm_sums_are_the_contract(icp, cpu, bumpy, lidar):
    """Caller source normals (some zero, not unit length, one NaN); caller target normals, then estimated ones; three
    transforms around the generator's pose for each."""
    rng = np.random.default_rng(4)
    for name, (P, Q, T_gt), d in (("bumpy", bumpy, D_BUMPY), ("lidar", lidar, 4 * 0.05)):
        assert name != "bumpy" or (len(P) <= 20_000 and len(Q) <= 20_000)
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
            n, nt = _check_symm_sums(ctx, cpu, P, Q, Np, Nq, H.motion(ang, sh) @ T_gt, d, name + ", caller normals")
            assert n > 1000 and 0 < n - nt < n               # some pairs have two zero normals, most have a term
        ctx.estimate_normals(d, MIN_NB)
        Ne = ctx.target_normals()
        assert np.array_equal(ctx.source_normals(), Nq)              # untouched by the target's normals
        for ang, sh in ((0.0, 0.0), (0.5, -0.004), (2.0, -0.02)):
            n, nt = _check_symm_sums(ctx, cpu, P, Q, Ne, Nq, H.motion(ang, sh) @ T_gt, d, name + ", estimated target normals")
            assert n > 1000 and nt > 1000
        ctx.close()


@pytest.fixture(scope="module")
def first_hit(cpu, bumpy):
    """The first source point of the bumpy pair with a correspondence at the edge test's transform (CPU restatement)."""
    P, Q, T_gt = bumpy
    c = P.astype(np.float64).mean(0).astype(np.float32)
    idx, _, _ = cpu.pass_((P - c).astype(np.float32), (Q - c).astype(np.float32), H.to_centred(H.motion(0.3, 0.002) @ T_gt, c).astype(np.float32),
                          D_BUMPY)
    return int(np.flatnonzero(idx >= 0)[0])


@pytest.mark.parametrize("n_q", [1, 63, 64, 65, 257, 524_289])
def test_symm_sums_at_edge_sizes(icp, cpu, bumpy, first_hit, n_q):
    """One lane, a ragged wave, exactly one wave, one lane more, a ragged second workgroup; and 524 289 source points: one
    more than the 2048 x 256 lanes of a full launch, so the grid-stride loop runs a second, ragged round."""
    P, Q, T_gt = bumpy
    d = D_BUMPY
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
    ctx.estimate_normals(d, MIN_NB)
    Np = ctx.target_normals()
    n, _ = _check_symm_sums(ctx, cpu, P, Qn, Np, Nq, H.motion(0.3, 0.002) @ T_gt, d, "edge size")
    assert n >= (1 if n_q < 1000 else 1000)
    T, r = ctx.refine(T_gt, metric="symmetric", max_iterations=2)
    assert np.all(np.isfinite(T)) and r.history_n[0] >= 1
    ctx.close()


def test_symm_sums_ignore_the_sign_of_either_normal(icp, cpu, bumpy):
    """Negating any subset of the source normals, of the target normals, or of both returns identical bits for all 31 sums:
    every negation is exact and (-a)(-b) = ab exactly.  A wrong or missing alignment of the two normals changes them."""
    P, Q, T_gt = bumpy
    d = D_BUMPY
    rng = np.random.default_rng(21)
    ctx = icp.ICP(0)
    ctx.set_target(P, d); ctx.set_source(Q)
    Rp, Rq = H.raw_normals(rng, len(P)), H.raw_normals(rng, len(Q))
    Rp[5, 0] = Rq[5, 0] = 0.5                                         # a NaN has no negation to compare
    ctx.set_target_normals(Rp); ctx.set_source_normals(Rq)
    Np, Nq = ctx.target_normals(), ctx.source_normals()               # as stored: some zero, the rest of unit length
    Pc, Qc, Tc = _frames(ctx, P, Q, H.motion(0.4, 0.003) @ T_gt)
    ci, cd, _ = cpu.pass_(Pc, Qc, Tc, d)
    assert SH.dot_is_decided(Pc, Qc, Tc, ci, Np, Nq)                   # the precondition: no pair with dot == 0 and two normals
    _, _, _, dot, _, _ = SH.pair_terms(Pc, Qc, Tc, ci, Np, Nq)
    assert np.count_nonzero(dot < 0) > 1000 and np.count_nonzero(dot > 0) > 1000
    s0 = ctx.symmetric_sums(Tc)
    fp = np.where(rng.random(len(P)) < 0.5, -1.0, 1.0).astype(np.float32)[:, None]
    fq = np.where(rng.random(len(Q)) < 0.5, -1.0, 1.0).astype(np.float32)[:, None]
    one_p, one_q = np.ones_like(fp), np.ones_like(fq)
    for what, a, b in (("source subset", one_p, fq), ("target subset", fp, one_q), ("both subsets", fp, fq),
                       ("all of both", -one_p, -one_q), ("all source", one_p, -one_q)):
        ctx.set_target_normals(Rp * a); ctx.set_source_normals(Rq * b)
        # normalising commutes with negation: what is stored is the first upload's, negated bit for bit
        assert np.array_equal(ctx.target_normals(), Np * a) and np.array_equal(ctx.source_normals(), Nq * b)
        s = ctx.symmetric_sums(Tc)
        assert s.tobytes() == s0.tobytes(), (what, s - s0)
    ctx.close()


def test_symm_zero_normals(icp, cpu, bumpy):
    """A pair with a zero target normal and a nonzero source normal carries a term; a pair with both zero counts in [0] and
    [1] only; a cloud where every pair is of the second kind ends DEGENERATE."""
    P, Q, T_gt = bumpy
    d = D_BUMPY
    rng = np.random.default_rng(22)
    raw_q = rng.normal(size=Q.shape).astype(np.float32)
    raw_q[::3] = 0
    ctx = icp.ICP(0)
    ctx.set_target(P, d); ctx.set_source(Q)
    ctx.set_target_normals(np.zeros_like(P)); ctx.set_source_normals(raw_q)
    Nq = ctx.source_normals()                                        # as stored
    assert np.array_equal(Nq, PH.normalise(raw_q)) and not Nq[::3].any() and Nq[1::3].any(1).all()
    Pc, Qc, Tc = _frames(ctx, P, Q, T_gt)
    ci, cd, _ = cpu.pass_(Pc, Qc, Tc, d)
    hit = ci >= 0
    s = ctx.symmetric_sums(Tc)
    assert s[0] == hit.sum() and s[2] == np.count_nonzero(hit & Nq.any(1)) and 0 < s[2] < s[0]
    cs, cabs = SH.symm_sums(Pc, Qc, Tc, ci, cd, np.zeros_like(P), Nq)
    _assert_sums(s, cs, cabs, "zero target normals")
    # every normal zero: counted, no term, no step
    ctx.set_source_normals(np.zeros_like(Q))
    s = ctx.symmetric_sums(Tc)
    assert s[0] == hit.sum() and abs(s[1] - cs[1]) <= 1e-10 * cabs[1] and not s[2:].any()
    T, r = ctx.refine(T_gt, metric="symmetric")
    assert r.status == icp.DEGENERATE and r.iterations == 0 and np.max(np.abs(T - T_gt)) <= 1e-12 and r.n_corr == hit.sum()
    ctx.close()


def test_symm_sums_under_rejection(icp, cpu, bumpy):
    """With reciprocal=True and with normal_angle=60 (up to sign) the sums equal the restatement on the pairs ICP.rejection
    keeps; with rejection off again the sums return to the earlier bits."""
    from super4pcs_amd import normals
    P, Q, T_gt = bumpy
    d = D_BUMPY
    ctx = icp.ICP(0)
    ctx.set_target(P, d); ctx.set_source(Q)
    ctx.estimate_normals(d, MIN_NB)
    ctx.set_source_normals(normals.estimate_normals(Q, k=16))
    Np, Nq = ctx.target_normals(), ctx.source_normals()
    Pc, Qc, Tc = _frames(ctx, P, Q, H.motion(0.5, 0.003) @ T_gt)
    s_off = ctx.symmetric_sums(Tc)
    for kw in (dict(reciprocal=True), dict(normal_angle=60), dict(reciprocal=True, normal_angle=60)):
        ctx.set_rejection(**kw)
        ki, kd, why = ctx.rejection(Tc)
        counts = ctx.rejection_counts()
        assert counts[3] == np.count_nonzero(ki >= 0) > 1000 and counts[0] - counts[3] > 0, (kw, counts)
        gs = ctx.symmetric_sums(Tc)
        assert np.array_equal(ctx.rejection_counts(), counts)
        cs, cabs = SH.symm_sums(Pc, Qc, Tc, ki, kd, Np, Nq)
        assert gs[0] == counts[3] < s_off[0]
        _assert_sums(gs, cs, cabs, "rejection %s" % (kw,))
        T, r = ctx.refine(H.motion(0.5, 0.003) @ T_gt, metric="symmetric", max_iterations=3)
        assert np.all(np.isfinite(T)) and r.n_corr > 0
    ctx.set_rejection()
    assert ctx.symmetric_sums(Tc).tobytes() == s_off.tobytes()
    ctx.close()


def _exact_pose_setup(icp, bumpy, n_q=8000):
    """Q: a subset of P moved rigidly; normals of P estimated once, Q's the same normals moved with it."""
    P = bumpy[0]
    rng = np.random.default_rng(5)
    pick = np.sort(rng.choice(len(P), n_q, replace=False))
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


def test_symm_is_deterministic_and_torch_agrees(icp, bumpy):
    """Two calls and a second context give identical sums, T and Result bytes; numpy and torch device inputs too;
    order_source on and off see the same correspondences."""
    import torch
    P, Q, Np, Nq, T_true, d = _exact_pose_setup(icp, bumpy)
    T0 = H.motion(1.0, 0.002) @ T_true
    ctx = icp.ICP(0)
    ctx.set_target(P, d); ctx.set_source(Q)
    ctx.set_target_normals(Np); ctx.set_source_normals(Nq * 2.5)
    Tc = H.to_centred(T0, ctx.frame()).astype(np.float32)
    s1, s2 = ctx.symmetric_sums(Tc), ctx.symmetric_sums(Tc)
    assert s1.tobytes() == s2.tobytes()
    T1, r1 = ctx.refine(T0, metric="symmetric")
    T2, r2 = ctx.refine(T0, metric="symmetric")
    assert np.array_equal(T1, T2) and bytes(r1) == bytes(r2)
    assert ctx.symmetric_sums(Tc).tobytes() == s1.tobytes()          # the refine's source order leaves the stage call alone
    dev = torch.device("cuda:0")
    ctx2 = icp.ICP(0)
    ctx2.set_target(torch.from_numpy(P).to(dev), d); ctx2.set_source(torch.from_numpy(Q).to(dev))
    ctx2.set_target_normals(torch.from_numpy(Np).to(dev)); ctx2.set_source_normals(torch.from_numpy(Nq * 2.5).to(dev))
    assert np.array_equal(ctx2.source_normals(), ctx.source_normals())
    assert ctx2.symmetric_sums(Tc).tobytes() == s1.tobytes()
    T3, r3 = ctx2.refine(T0, metric="symmetric")
    assert np.array_equal(T3, T1) and bytes(r3) == bytes(r1)
    # order_source: another summation order, the same pairs
    Ta, ra = ctx.refine(T0, metric="symmetric", max_iterations=1, order_source=True)
    Tb, rb = ctx.refine(T0, metric="symmetric", max_iterations=1, order_source=False)
    assert ra.history_n[0] == rb.history_n[0] == int(s1[0]) and ra.n_corr == rb.n_corr
    assert np.isclose(ra.history_rmse[0], rb.history_rmse[0], rtol=1e-12) and np.max(np.abs(Ta - Tb)) <= 1e-9
    ctx.close(); ctx2.close()


@pytest.fixture(scope="module")
def trajectory_case(icp, bumpy):
    """The bumpy pair with estimated target normals and k-nearest-neighbour source normals, as the library stores them."""
    from super4pcs_amd import normals
    P, Q, T_gt = bumpy
    ctx = icp.ICP(0)
    ctx.set_target(P, D_BUMPY)
    ctx.set_source(Q)
    ctx.estimate_normals(D_BUMPY)
    ctx.set_source_normals(normals.estimate_normals(Q, k=16))
    c = ctx.frame()
    yield ctx, c, (P - c).astype(np.float32), (Q - c).astype(np.float32), ctx.target_normals(), ctx.source_normals()
    ctx.close()


def _trajectory(icp, cpu, case, T0, T_gt, what):
    ctx, c, Pc, Qc, Np, Nq = case
    T, r = ctx.refine(T0, metric="symmetric")
    Tc, its, status, hist = SH.cpu_refine_symm(cpu, icp.solve_symmetric, Pc, Qc, Np, Nq, c, T0, D_BUMPY)
    print("symmetric trajectory, %s: gpu %d its (%s) rmse %.6g; cpu %d its (%s) |dT| %.2g; rot err %.4g -> %.4g deg"
          % (what, r.iterations, icp.STATUS_NAMES[r.status], r.rmse, its, icp.STATUS_NAMES[status], np.max(np.abs(T - Tc)),
             H.rot_err_deg(T0, T_gt), H.rot_err_deg(T, T_gt)))
    assert r.iterations == its and r.status == status
    assert np.max(np.abs(T - Tc)) <= 1e-5
    k = min(r.history_len, len(hist))
    assert k == len(hist) and np.allclose(list(r.history_rmse[:k]), hist[:k], rtol=1e-9, atol=0)
    return T, r


def test_symm_refine_trajectory_equals_the_cpu_loop(icp, cpu, bumpy, trajectory_case):
    """The CPU restatement of the symmetric sums plus s4p_icp_solve_symmetric, from 1.5 degrees off the generator's pose:
    same iterations and status, |T - T_cpu| <= 1e-5, the rmse history within rtol 1e-9."""
    T_gt = bumpy[2]
    _trajectory(icp, cpu, trajectory_case, H.motion(1.5, 0.004) @ T_gt, T_gt, "1.5 degrees")


@pytest.fixture(scope="module")
def knn_normals_case(icp, bumpy):
    """The bumpy pair with the 16-nearest-neighbour normals of both clouds (super4pcs_amd.normals), the target's uploaded as
    caller normals, as the library stores them."""
    from super4pcs_amd import normals
    P, Q, T_gt = bumpy
    ctx = icp.ICP(0)
    ctx.set_target(P, D_BUMPY)
    ctx.set_source(Q)
    ctx.set_target_normals(normals.estimate_normals(P, k=16))
    ctx.set_source_normals(normals.estimate_normals(Q, k=16))
    c = ctx.frame()
    yield ctx, c, (P - c).astype(np.float32), (Q - c).astype(np.float32), ctx.target_normals(), ctx.source_normals()
    ctx.close()


# Starts (degrees off the generator's pose) tried in this order on the CPU; the first at which the restated plane loop needs
# at least twice the restated symmetric loop's iterations is the one the device runs.  With 16-neighbour normals on the
# noisy target the restated plane loop often does not meet the stop rule within 30 iterations (its rmse keeps moving by
# more than 1e-6 of itself) where the symmetric loop meets it in 13 to 19; which starts those are depends on the noise, so
# the list is long and the choice is made when the test runs.
SLOW_PLANE_STARTS = (1.0, 1.5, 2.5, 4.0, 12.0, 0.5, 2.0, 3.0, 5.0, 6.0, 8.0, 10.0)


def test_symm_refine_trajectory_where_the_plane_loop_needs_twice_the_iterations(icp, cpu, bumpy, knn_normals_case):
    """A start chosen on the CPU: the restated point-to-plane loop (same pairs, same target normals, s4p_icp_solve_plane)
    needs at least twice the restated symmetric loop's iterations from it.  The device's symmetric refine from that start
    equals the CPU loop: same iterations and status, |T - T_cpu| <= 1e-5, the rmse history within rtol 1e-9.  The device's
    plane result from the same start is printed, not asserted.

    The pair is the bumpy pair with the 16-nearest-neighbour normals of both clouds.  With target normals estimated within
    d = 4 delta instead (the case of the test above) no start between 2 and 12 degrees qualifies: there the restated plane
    loop stops after 4 to 10 iterations and the symmetric one after 14 to 27 ("Symmetric ICP")."""
    ctx, c, Pc, Qc, Np, Nq = knn_normals_case
    T_gt = bumpy[2]
    chosen = None
    for ang in SLOW_PLANE_STARTS:
        T0 = H.motion(ang, 0.004) @ T_gt
        _, its_s, st_s, _ = SH.cpu_refine_symm(cpu, icp.solve_symmetric, Pc, Qc, Np, Nq, c, T0, D_BUMPY)
        _, its_p, st_p, _ = PH.cpu_refine_plane(cpu, icp.solve_plane, Pc, Qc, Np, c, T0, D_BUMPY)
        print("start %g degrees: cpu symmetric %d its (%s), cpu plane %d its (%s)"
              % (ang, its_s, icp.STATUS_NAMES[st_s], its_p, icp.STATUS_NAMES[st_p]))
        if its_s >= 1 and its_p >= 2 * its_s:
            chosen = (ang, T0)
            break
    assert chosen is not None, "no start of %s at which the plane loop needs twice the symmetric loop's iterations" % (SLOW_PLANE_STARTS,)
    ang, T0 = chosen
    T, r = _trajectory(icp, cpu, knn_normals_case, T0, T_gt, "%g degrees" % ang)
    Tp, rp = ctx.refine(T0, metric="plane")
    print("from %g degrees on the device: symmetric %d its (%s), rot err %.4g deg; plane %d its (%s), rot err %.4g deg"
          % (ang, r.iterations, icp.STATUS_NAMES[r.status], H.rot_err_deg(T, T_gt), rp.iterations, icp.STATUS_NAMES[rp.status],
             H.rot_err_deg(Tp, T_gt)))


def test_symm_refine_reaches_an_exact_pose(icp, bumpy):
    """A rigidly moved subset of P with the same normals on both clouds, from 1 degree off: back to 1e-5, fitness 1."""
    P, Q, Np, Nq, T_true, d = _exact_pose_setup(icp, bumpy)
    T0 = H.motion(1.0, 0.002) @ T_true
    ctx = icp.ICP(0)
    ctx.set_target(P, d); ctx.set_source(Q)
    ctx.set_target_normals(Np); ctx.set_source_normals(Nq)
    T, r = ctx.refine(T0, max_iterations=64, rel_tol=0.0, metric="symmetric")
    print("symmetric exact pose: |T0 - T_true| %.2g -> |T - T_true| %.2g, %d iterations (%s), rmse %.3g, fitness %.6f"
          % (np.max(np.abs(T0 - T_true)), np.max(np.abs(T - T_true)), r.iterations, icp.STATUS_NAMES[r.status], r.rmse, r.fitness))
    assert np.max(np.abs(T - T_true)) <= 1e-5 and r.fitness == 1.0
    ctx.close()


def test_symm_planar_target_is_degenerate(icp, cpu):
    """z = 0 with every normal along z on both clouds: in-plane motion carries no term, the first solve is DEGENERATE on the
    device and on the CPU loop alike, and T stays T0."""
    rng = np.random.default_rng(8)
    P = np.column_stack([rng.uniform(-1, 1, (20_000, 2)), np.zeros(20_000)]).astype(np.float32)
    Q = P[rng.choice(len(P), 8_000, replace=False)] + np.array([0, 0, 0.01], np.float32)
    T0 = H.motion(0.5, np.array([0.01, -0.02, 0.0]), axis=(0, 0, 1))
    up = np.array([0, 0, 1], np.float32)
    Np, Nq = np.tile(up, (len(P), 1)), np.tile(up, (len(Q), 1))
    ctx = icp.ICP(0)
    ctx.set_target(P, 0.08); ctx.set_source(Q)
    ctx.set_target_normals(Np); ctx.set_source_normals(Nq)
    Pc, Qc, Tc = _frames(ctx, P, Q, T0)
    gs = ctx.symmetric_sums(Tc)
    ci, cd, _ = cpu.pass_(Pc, Qc, Tc, 0.08)
    cs, cabs = SH.symm_sums(Pc, Qc, Tc, ci, cd, Np, Nq)
    assert np.all(np.isfinite(gs)) and gs[0] == cs[0] > 5_000
    for s in (gs, cs):
        with pytest.raises(icp.ICPError) as e:
            icp.solve_symmetric(s)
        assert e.value.code == icp.ERR_DEGENERATE
    T, r = ctx.refine(T0, metric="symmetric")
    Tcpu, its, status, hist = SH.cpu_refine_symm(cpu, icp.solve_symmetric, Pc, Qc, Np, Nq, ctx.frame(), T0, 0.08)
    assert r.status == status == icp.DEGENERATE and r.iterations == its == 0
    assert np.max(np.abs(T - T0)) <= 1e-12 and np.max(np.abs(Tcpu - T0)) <= 1e-12
    ctx.close()


def test_symm_state_and_argument_errors(icp, bumpy):
    """-7 without target or source normals; set_source invalidates the source normals; the C ABI refuses an id past point
    and plane in s4p_icp_refine_robust, s4p_icp_robust_sums and the batch calls with -1, as before."""
    P, Q, T_gt = bumpy
    P, Q = P[:10_000], Q[:3_000]
    d = D_BUMPY
    rng = np.random.default_rng(6)
    Nq = rng.normal(size=Q.shape).astype(np.float32)
    ctx = icp.ICP(0)
    ctx.set_target(P, d)
    ctx.set_source(Q)

    def code(fn):
        with pytest.raises(icp.ICPError) as e:
            fn()
        return e.value.code

    I4 = np.eye(4)
    assert code(lambda: ctx.symmetric_sums(I4)) == -7               # neither
    ctx.set_source_normals(Nq)
    assert code(lambda: ctx.symmetric_sums(I4)) == -7               # no target normals
    assert code(lambda: ctx.refine(T_gt, metric="symmetric")) == -7
    ctx.estimate_normals(d)
    ctx.symmetric_sums(I4)
    ctx.set_source(Q)                                               # invalidates the source normals
    assert code(lambda: ctx.symmetric_sums(I4)) == -7
    assert code(lambda: ctx.refine(T_gt, metric="symmetric")) == -7
    with pytest.raises(icp.ICPError, match="source normals first"):
        ctx.symmetric_sums(I4)
    ctx.set_source_normals(Nq)
    ctx.set_target(P, d)                                            # invalidates the target normals, keeps the source's
    assert code(lambda: ctx.symmetric_sums(I4)) == -7
    with pytest.raises(icp.ICPError, match="target normals first"):
        ctx.refine(T_gt, metric="symmetric")
    ctx.estimate_normals(d)
    with pytest.raises(ValueError):
        ctx.refine(T_gt, metric="symmetric", loss="huber")
    # the C ABI: metric ids are 0 (point) and 1 (plane); the library's own number for this metric is refused like any other
    L = ctx.L
    dp, fp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float)
    rob = icp.robust_params("huber")
    prm = icp.Params(); L.s4p_icp_default_params(ctypes.byref(prm))
    T16 = np.ascontiguousarray(T_gt, np.float64).reshape(16).copy()
    Tf = np.eye(4, dtype=np.float32).reshape(16)
    res = icp.Result(); out = np.zeros(64, np.float64); info = np.zeros(8, np.float64)
    bp = icp.BatchParams(); L.s4p_icp_default_params(ctypes.byref(bp.icp))
    order = np.zeros(1, np.int32)
    for metric_id in (4, 2, 5):
        assert L.s4p_icp_refine_robust(ctx.h, ctypes.byref(prm), metric_id, ctypes.byref(rob), T16.ctypes.data_as(dp), ctypes.byref(res),
                                       info.ctypes.data_as(dp)) == -1
        assert L.s4p_icp_robust_sums(ctx.h, Tf.ctypes.data_as(fp), metric_id, ctypes.byref(rob), out.ctypes.data_as(dp),
                                     info.ctypes.data_as(dp)) == -1
        assert L.s4p_icp_sums_batch(ctx.h, metric_id, 1, Tf.ctypes.data_as(fp), out.ctypes.data_as(dp)) == -1
        bp.metric = metric_id
        assert L.s4p_icp_refine_batch(ctx.h, ctypes.byref(bp), 1, T16.ctypes.data_as(dp), ctypes.byref(res),
                                      order.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == -1
    assert np.array_equal(T16.reshape(4, 4), T_gt)
    ctx.close()


def test_facade_cli_and_binding_agree_on_the_hippo(icp, tmp_path, s4p_lib_built):
    """The hippo fixture through MatchSuper4PCS + RefineICP(Symmetric) (tests/icp_facade_app), through
    `Super4PCS ... --icp 10 --icp-metric symmetric -m`, and through icp.refine from the same Super4PCS result."""
    from super4pcs_amd import build as B
    g = np.load(os.path.join(ROOT, "tests", "golden", "hippo_config1.npz"))
    Ps, Qu = g["Ps"].astype(np.float32), g["Qu"].astype(np.float32)
    delta, overlap, n_s = 0.01, 0.7, 200
    exe = apps.build_app(tmp_path, "icp_facade_app", apps.ICP_FACADE_LIBS)
    rows, _ = apps.run_icp_app(exe, Ps, Qu, delta, overlap, n_s, "--metric", "symmetric", "--max-iterations", 10)
    M, Mf = rows["registered"].astype(np.float64), rows["registered"]
    Qm = apps.move_f32(Mf, Qu)
    dT, r = icp.refine(Ps, Qm, np.eye(4), max_distance=np.float32(4.0 * delta), metric="symmetric", max_iterations=10)
    want = icp.compose(dT, M).astype(np.float32)
    print("hippo symmetric: facade == icp.py max diff %.2g, %d iterations (%s), rmse %.4g"
          % (np.max(np.abs(rows["refined"] - want)), r.iterations, icp.STATUS_NAMES[r.status], r.rmse))
    assert np.max(np.abs(rows["refined"] - want)) <= 1e-6
    assert np.max(np.abs(rows["refined"] - Mf)) > 0
    # command line
    cli = B.build_cli()
    apps.write_obj(tmp_path / "P.obj", Ps); apps.write_obj(tmp_path / "Q.obj", Qu)
    args = ["--icp", "10", "--icp-metric", "symmetric"]
    got, _ = apps.run_cli(cli, tmp_path / "P.obj", tmp_path / "Q.obj", delta, overlap, n_s, args)
    assert np.max(np.abs(got - want)) <= 1e-6
    rc = subprocess.run([cli, "-i", str(tmp_path / "P.obj"), str(tmp_path / "Q.obj"), "-o", str(overlap), "-d", str(delta), "-t", "1000",
                         "-n", str(n_s)] + args + ["-m", str(tmp_path / "mat.txt"), "--icp-loss", "huber"],
                        capture_output=True, text=True, timeout=60)
    assert rc.returncode == 1 and "Usage:" in rc.stderr


def test_refine_multiscale_symmetric_is_the_chain_of_downsample_and_refine(icp):
    """refine_multiscale(metric="symmetric") equals its own sequence of voxel_downsample + icp.refine calls, with given normals
    (voxel means, renormalised per level) and with normals left to icp.refine's rule."""
    from super4pcs_amd import multiscale, voxel
    from tests import multiscale_helpers as MH
    case = MH.small_pair()
    P, Q, T0 = case["P"], case["Q"], case["T0"]
    voxels, d_fine, iterations = (0.15, 0.06, 0), 0.05, (12, 10, 8)
    for given in (dict(target_normals=case["Np"], source_normals=case["Nq"]), dict()):
        T, levels = multiscale.refine_multiscale(P, Q, T0=T0, voxel_sizes=voxels, max_distance=d_fine, max_iterations=iterations,
                                                 metric="symmetric", **given)
        assert len(levels) == 3
        Tc = T0
        for l, (v, it) in enumerate(zip(voxels, iterations)):
            d = max(d_fine, 3.0 * v)
            if v > 0:
                Pl, _, Npl, _, _ = voxel.voxel_downsample(P, v, normals=given.get("target_normals"))
                Ql, _, Nql, _, _ = voxel.voxel_downsample(Q, v, normals=given.get("source_normals"))
                assert 20 < len(Pl) < len(P) and 20 < len(Ql) < len(Q)
            else:
                Pl, Ql, Npl, Nql = P, Q, given.get("target_normals"), given.get("source_normals")
            Tc, r = icp.refine(Pl, Ql, T0=Tc, max_distance=d, metric="symmetric", target_normals=Npl, source_normals=Nql, max_iterations=it)
            assert bytes(r) == bytes(levels[l]), (l, r.as_dict(), levels[l].as_dict())
            assert r.n_corr > 0
        assert np.array_equal(T, Tc)
        print("multi-scale symmetric (%s normals): pose error %.4g -> %.4g, iterations %s"
              % ("given" if given else "estimated", MH.pose_error(T0, case["T_gt"], Q), MH.pose_error(T, case["T_gt"], Q),
                 [r.iterations for r in levels]))
