"""The generalized, coloured, rejection and batch kernels of the ICP library on the MI355X in the regimes their own modules did
not enter (inputs in tests/icp_edge_cases.py, their regimes, input conditions and floors asserted on the
host in tests/test_icp_edge_metrics_host.py): k_color_gradient on one-cell, flat, needle and enlarged grids, on tiny targets,
on duplicates, far from the origin and past one trip of its grid-stride loop; the sums and the pair filters where every match
is a 1000-way tie, where one target serves 300 sources, in cell -1 and cell n and on a lattice of float steps; the batch
kernels with 64 poses, a compacted active list and the far end of the slab.

Every comparison is one the existing modules make, by their own checkers: _check_gradients and _check_color_sums
(test_gpu_icp_color.py), _check_gicp_sums (test_gpu_icp_gicp.py), _check_contract and _close (test_gpu_icp_reject.py),
_assert_same_bytes (test_gpu_icp_batch.py), and the trajectory rules of those modules.  No tolerance is new."""
import numpy as np
import pytest

from tests import icp_color_helpers as CH
from tests import icp_edge_cases as E
from tests import icp_gicp_helpers as GH
from tests import icp_helpers as H
from tests import icp_plane_helpers as PH
from tests import icp_reject_helpers as JH
from tests import icp_robust_helpers as RH
from tests.golden.make_icp_parity_golden import _motion
from tests.test_gpu_icp_batch import _assert_same_bytes, _singles
from tests.test_gpu_icp_color import _check_color_sums, _check_gradients
from tests.test_gpu_icp_edges import MemoCPU
from tests.test_gpu_icp_gicp import _check_gicp_sums
from tests.test_gpu_icp_reject import _check_contract, _close

pytestmark = pytest.mark.gpu
F = np.float32
MIN_NB = 6
LAMBDAS = (0.0, 0.968, 1.0)
EPSILONS = (1e-3, 1.0)


@pytest.fixture(scope="module")
def icp(s4p_lib_built):
    from super4pcs_amd import build as B
    B.build_icp()
    B.build_normals()
    from super4pcs_amd import icp as I
    return I


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return MemoCPU(H.build_cpu(tmp_path_factory.mktemp("icp_cpu")))


# ---------------------------------------------------------------------------------------------------------------------
# a. gradients at every target point

@pytest.mark.parametrize("name", sorted(E.GRADIENT_CASES))
def test_gradients_at_every_target_point(icp, name):
    """r = d, min_neighbours = 6; caller normals and, where section 15 does not list the case as SPARSE, estimated ones.  The
    zero pattern and every component within 2^-23 of the point's largest (_check_gradients), the host module's floor on the
    nonzero count, and two calls with the same bytes."""
    case = E.GRADIENT_CASES[name]()
    Ip = E.intensity(case)
    ctx = icp.ICP(0)
    ctx.set_target(case.P, case.d)
    ctx.set_target_intensity(Ip)
    setups = list(E.gradient_normals(case)) + ([("estimated", None)] if name not in E.SPARSE else [])
    for label, raw in setups:
        if raw is None:
            ctx.estimate_normals(case.d, MIN_NB)
        else:
            ctx.set_target_normals(raw)
            assert np.array_equal(ctx.target_normals(), PH.normalise(raw))
        Np = ctx.target_normals()
        ctx.estimate_color_gradients(case.d, MIN_NB)
        G, zero = _check_gradients(ctx, case.P, Np, Ip, case.d, MIN_NB, "%s, %s normals" % (name, label))
        assert E.gradient_floor(name, len(case.P))(int((~zero).sum())), (name, label, (~zero).sum())
        ctx.estimate_color_gradients(case.d, MIN_NB)
        assert ctx.target_color_gradients().tobytes() == G.tobytes()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# b. past one trip

@pytest.fixture(scope="module")
def full(icp):
    """The 600 k target of full_launch_pair with estimated normals, a texture and gradients within d / 2: every target-side
    kernel takes a second trip (600 000 > 2048 x 256)."""
    case = E.full_launch_pair()
    assert E.launch(len(case.P)) == (E.K_MAX_BLOCKS, 1, 2)
    ctx = icp.ICP(0)
    ctx.set_target(case.P, case.d)
    ctx.estimate_normals(case.d, MIN_NB)
    Ip = E.intensity(case)
    ctx.set_target_intensity(Ip)
    ctx.estimate_color_gradients(case.d / 2, MIN_NB)
    yield case, ctx, Ip
    ctx.close()


def test_gradients_past_one_trip(icp, cpu, full):
    """A sorted sample of the 600 k target (3000 random points, 2000 that a lane computes on its second trip, the 2000 places
    around the one where the second trip begins and the 500 where it ends) by _check_gradients' rule on the rows the
    restatement computes with which=; then the coloured sums at n_Q = 524 288 and 524 289 with those gradients, and the
    generalized sums once: the gathers of intensity and normals loop here as well."""
    case, ctx, Ip = full
    pick, pos = E.gradient_sample(case.P, case.d)
    lanes = E.K_MAX_BLOCKS * E.K_BLOCK
    late = pos[pick] >= lanes + 1000
    assert late.sum() >= 2000
    Np = ctx.target_normals()
    G, zw = _check_gradients(ctx, case.P, Np, Ip, case.d / 2, MIN_NB, "full_launch, %d on a second trip" % late.sum(), which=pick)
    assert (~zw).sum() > 0.5 * len(pick) and (~zw[late]).sum() > 0.5 * late.sum()
    ctx.estimate_color_gradients(case.d / 2, MIN_NB)
    assert ctx.target_color_gradients().tobytes() == G.tobytes()
    Qm = case.Q.astype(np.float64) @ case.T0[:3, :3].T + case.T0[:3, 3]
    Iq_all = E.intensity(case, Qm)
    for n_q in E.FULL_LAUNCH_N:
        Q, Iq = case.Q[:n_q], Iq_all[:n_q]
        ctx.set_source(Q)
        ctx.set_source_intensity(Iq)
        n, nt = _check_color_sums(ctx, cpu, case.P, Q, Np, G, Ip, Iq, case.T0, case.d, lams=(0.0, 0.968))
        assert n > 100_000 and 0.8 * n < nt <= n
    raw_q = E.source_normals(n_q, 8)
    ctx.set_source_normals(raw_q)
    assert _check_gicp_sums(ctx, cpu, case.P, Q, Np, PH.normalise(raw_q), case.T0, case.d, eps_list=(1e-3,)) > 100_000


# ---------------------------------------------------------------------------------------------------------------------
# c. sums and pair filters on the geometric cases

@pytest.mark.parametrize("name", E.SUMS_CASES)
def test_sums_and_rejection_on_the_geometric_cases(icp, cpu, name):
    """Per case, at the base pose and one motion: the coloured sums at lambda 0, 0.968 and 1 and the generalized sums at
    epsilon 1e-3 and 1 (source normals some zero, one NaN); the rejection contract for reciprocity and for reciprocity with the
    60 degree normal test, the counts that make the case bite, and every sums call on the kept pairs."""
    case = (E.DENSE.get(name) or E.SMALL[name])()
    inp = E.sums_inputs(case)
    Ip, Iq = inp["Ip"], inp["Iq"]
    ctx = icp.ICP(0)
    ctx.set_target(case.P, case.d)
    ctx.set_source(case.Q)
    ctx.set_target_normals(inp["raw_p"])
    ctx.set_source_normals(inp["raw_q"])
    Np, Nq = ctx.target_normals(), ctx.source_normals()
    assert np.array_equal(Np, PH.normalise(inp["raw_p"])) and np.array_equal(Nq, PH.normalise(inp["raw_q"]))
    ctx.set_target_intensity(Ip)
    ctx.set_source_intensity(Iq)
    ctx.estimate_color_gradients(case.d, MIN_NB)
    G = ctx.target_color_gradients()                                   # compared with the restatement in test a
    c = ctx.frame()
    Pc, Qc = (case.P - c).astype(F), (case.Q - c).astype(F)
    pl = E.plan(case.P, case.d, c)
    for T in inp["poses"]:
        n, nt = _check_color_sums(ctx, cpu, case.P, case.Q, Np, G, Ip, Iq, T, case.d, lams=LAMBDAS)
        assert 1 <= n and (name not in E.HAS_MISSES or n < len(case.Q))
        assert _check_gicp_sums(ctx, cpu, case.P, case.Q, Np, Nq, T, case.d, eps_list=EPSILONS) == n
        Tc = H.to_centred(T, c).astype(F)
        fwd = JH.cpu_search(cpu)(Pc, Qc, Tc, case.d)
        for kw in E.REJECTIONS:
            ki, kd, why, cc = _check_contract(ctx, cpu, Pc, Qc, Tc, case.d, kw, Np, Nq, forward=fwd)
            print("%s %s: matched %d, by normals %d, by reciprocity %d, kept %d" % (name, kw, cc[0], cc[1], cc[2], cc[3]))
            gi, gd, gw = ctx.rejection(Tc)
            E.check_reject_counts(name, kw, pl, Qc, Tc, gi, gw, ctx.rejection_counts())
            assert cc[0] == n and cc[3] >= (0 if kw.get("normal_mode") else 1)
            kept = int(cc[3])
            gs = ctx.sums(Tc)                                          # k_wsum<false> on the kept pairs
            cs, _ = RH.robust_sums(Pc, Qc, Tc, ki, kd, "point", "trimmed", len(Qc), case.d, trim_fraction=1.0)
            assert gs[0] == kept == cs[0]
            _close(gs, cs, JH.sums_abs(Pc, Qc, Tc, ki, kd, "point"))
            gs = ctx.plane_sums(Tc)                                    # k_wsum<true>
            cs = PH.plane_sums(Pc, Qc, Tc, ki, kd, Np)
            assert gs[0] == kept == cs[0] and gs[2] == cs[2]
            _close(gs, cs, JH.sums_abs(Pc, Qc, Tc, ki, kd, "plane", Np))
            gs = ctx.gicp_sums(Tc, 1e-3)
            cs, cabs = GH.gicp_sums(Pc, Qc, Tc, ki, kd, Np, Nq, 1e-3)
            assert gs[0] == gs[2] == kept == cs[0]
            _close(gs, cs, cabs)
            gs = ctx.color_sums(Tc, 0.968)
            cs, cabs = CH.color_sums(Pc, Qc, Tc, ki, kd, Np, G, Ip, Iq, 0.968)
            assert gs[0] == kept == cs[0] and gs[2] == cs[2]
            _close(gs, cs, cabs)
            assert np.array_equal(ctx.rejection_counts(), cc)
        ctx.set_rejection()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# d. trajectories

@pytest.mark.parametrize("name", ["far", "box_faces"])
def test_color_and_gicp_refines_on_edge_cases_equal_the_cpu_loops(icp, cpu, name):
    """Eight iterations from half a degree off, estimated target normals, gradients within d / 2, k-nearest-neighbour source
    normals: the transform within 1e-5 of the CPU loop's, iterations within one, the first history entries to 1e-9 and, for
    the generalized metric, the same status -- the rules of test_gpu_icp_color.py and test_gpu_icp_gicp.py."""
    from super4pcs_amd import normals
    case = E.SMALL[name]()
    inp = E.sums_inputs(case)
    Ip, Iq = inp["Ip"], inp["Iq"]
    ctx = icp.ICP(0)
    ctx.set_target(case.P, case.d)
    ctx.set_source(case.Q)
    ctx.estimate_normals(case.d, MIN_NB)
    ctx.set_source_normals(normals.estimate_normals(case.Q, k=16))
    ctx.set_target_intensity(Ip)
    ctx.set_source_intensity(Iq)
    ctx.estimate_color_gradients(case.d / 2, MIN_NB)
    c = ctx.frame()
    Pc, Qc = (case.P - c).astype(F), (case.Q - c).astype(F)
    T0 = E.pose(case, RH.motion(0.5, 0.003))
    Np, Nq, G = ctx.target_normals(), ctx.source_normals(), ctx.target_color_gradients()
    for metric in ("color", "gicp"):
        T, r = ctx.refine(T0, metric=metric, max_iterations=8)
        if metric == "color":
            Tc, its, status, hist = CH.cpu_refine_color(cpu, icp.solve_plane, Pc, Qc, Np, G, Ip, Iq, c, T0, case.d, max_iterations=8)
        else:
            Tc, its, status, hist = GH.cpu_refine_gicp(cpu, icp.solve_plane, Pc, Qc, Np, Nq, c, T0, case.d, max_iterations=8)
        print("%s %s: gpu %d its (%s) rmse %.6g n %d; cpu %d its (%s) |dT| %.2g" % (
            name, metric, r.iterations, icp.STATUS_NAMES[r.status], r.rmse, r.n_corr, its, icp.STATUS_NAMES[status], np.max(np.abs(T - Tc))))
        assert np.max(np.abs(T - Tc)) <= 1e-5
        assert abs(r.iterations - its) <= 1 and r.iterations >= 2
        if metric == "gicp":
            assert r.status == status
        k = min(r.history_len, len(hist), 3)
        assert k == 3 and np.allclose(list(r.history_rmse[:k]), hist[:k], rtol=1e-9)
        assert 0 < r.n_corr < len(case.Q)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# e. batch

LOST_EVERY, LOST_AT = 9, 4                       # poses 4, 13, ..., 58 have no correspondence


def _starts64(case):
    """64 distinct starts: growing small motions, every ninth start carried 10 units away (no correspondence), so the
    active list is compacted after the first pass and rows and poses differ from then on."""
    out = []
    for b in range(64):
        M = _motion(0.15 * b, [0.0004 * b, -0.0002 * b, 0.0001 * (b % 5)])
        if b % LOST_EVERY == LOST_AT:
            M = M.copy(); M[:3, 3] += [10.0, 0.0, 0.0]
        out.append(E.pose(case, M))
    return np.stack(out)


@pytest.mark.parametrize("metric", ["point", "plane"])
@pytest.mark.parametrize("name", ["ragged_257", "box_faces"])
def test_refine_batch_of_64_equals_the_single_refines(icp, name, metric):
    case = E.SMALL[name]()
    ctx = icp.ICP(0)
    ctx.set_target(case.P, case.d)
    ctx.set_source(case.Q)
    ctx.estimate_normals(case.d)
    T0s = _starts64(case)
    assert len({T.tobytes() for T in T0s}) == 64
    Ts, res, order = ctx.refine_batch(T0s, order_source=False, metric=metric)
    Tw, rw = _singles(ctx, T0s, order_source=False, metric=metric)
    _assert_same_bytes(Ts, res, Tw, rw)
    its = [r.iterations for r in res]
    lost = [b for b in range(64) if b % LOST_EVERY == LOST_AT]
    print(name, metric, "iterations", its)
    assert all(res[b].status == icp.TOO_FEW and res[b].iterations == 0 and res[b].n_corr == 0 for b in lost)
    assert all(res[b].iterations > 0 for b in range(64) if b not in lost) and res[63].iterations > 0
    # the list is compacted after the first pass, and for the point metric (which converges at different counts) again later
    assert len(set(its)) >= (3 if metric == "point" else 2)
    assert np.array_equal(order, icp.rank_batch(res)) and sorted(order[-len(lost):]) == lost
    ctx.close()


@pytest.mark.parametrize("metric", ["point", "plane"])
def test_batch_of_64_past_the_full_launch(icp, full, metric):
    """n_Q = 524 289: 64 poses times 2048 slab rows (pose 63 writes and sums the far end of the slab), lanes on two trips; then
    a refine of three poses, two iterations, against the singles."""
    case, ctx, _ = full
    Q = case.Q[:E.FULL_LAUNCH_N[1]]
    assert E.launch(len(Q)) == (E.K_MAX_BLOCKS, 1, 2)
    ctx.set_source(Q)
    c = ctx.frame()
    Ms = [_motion(0.02 * b, [0.0002 * b, -0.0001 * b, 0.0]) for b in range(64)]
    Ts = np.stack([H.to_centred(E.pose(case, M), c).astype(F) for M in Ms])
    got = ctx.sums_batch(Ts, metric)
    want = np.stack([ctx.sums(T) if metric == "point" else ctx.plane_sums(T) for T in Ts])
    assert got.shape == (64, 31 if metric == "plane" else 17) and np.all(want[:, 0] > 10_000)
    assert np.array_equal(got, want)
    assert len({row.tobytes() for row in got}) == 64
    T0s = np.stack([E.pose(case, M) for M in (Ms[0], Ms[40], Ms[63])])
    Tb, res, _ = ctx.refine_batch(T0s, order_source=False, metric=metric, max_iterations=2)
    Tw, rw = _singles(ctx, T0s, order_source=False, metric=metric, max_iterations=2)
    _assert_same_bytes(Tb, res, Tw, rw)
    assert all(r.iterations == 2 and r.n_corr > 10_000 for r in res)
