"""Batched multi-start ICP (include/s4p_icp_batch.h) on the device: sums_batch against the single sums calls bit for bit at
the launch's edge shapes, refine_batch against the single refines byte for byte through every stop of the state machine and
every compaction of the active list, the ordered-source variant, the ranking, the refusals, the interfaces and the
multi-scale entry.  Cases from tests/icp_edge_cases.py; the single calls are the reference throughout."""
import ctypes as C

import numpy as np
import pytest

from tests import icp_edge_cases as E
from tests import icp_helpers as H
from tests import multiscale_helpers as MH
from tests.golden.make_icp_parity_golden import _motion

pytestmark = pytest.mark.gpu
F = np.float32

# The largest entrywise |T_ordered - T_unordered| the refine cases below show on the MI355X, times
# 100.  The effect is the order of the double sums fed back through a float-rounded T: below a float step of an entry.
ORDER_T_OBSERVED = 9.7145e-17
ORDER_T_BOUND = 100 * ORDER_T_OBSERVED


@pytest.fixture(scope="module")
def icp(s4p_lib_built):
    from super4pcs_amd import build as B
    B.build_icp()
    from super4pcs_amd import icp as I
    return I


def _ctx(icp, case, Q=None, normals=None):
    ctx = icp.ICP(0)
    ctx.set_target(case.P, case.d)
    ctx.set_source(case.Q if Q is None else Q)
    if normals is None:
        ctx.estimate_normals(case.d)
    else:
        ctx.set_target_normals(normals)
    return ctx


@pytest.fixture(scope="module")
def box(icp):
    case = E.box_faces()
    ctx = _ctx(icp, case)
    yield case, ctx
    ctx.close()


def _centred(ctx, case, motions):
    c = ctx.frame()
    return np.stack([H.to_centred(E.pose(case, M), c).astype(F) for M in motions])


def _motions(B):
    """B distinct small motions, the first the identity."""
    return [_motion(0.25 * b, [0.001 * b, -0.0005 * b, 0.0003 * (b % 5)]) for b in range(B)]


def _single_sums(ctx, Ts, metric):
    return np.stack([ctx.sums(T) if metric == "point" else ctx.plane_sums(T) for T in Ts])


def _bytes(r):
    return bytes(r)


# ---------------------------------------------------------------------------------------------------------------------
# sums

@pytest.mark.parametrize("B", [1, 2, 7, 64])
@pytest.mark.parametrize("metric", ["point", "plane"])
def test_sums_batch_rows_are_the_single_sums(box, metric, B):
    """box_faces: n_Q = 15 000, 59 workgroups, a partial last block and a partial last wave."""
    case, ctx = box
    assert E.launch(len(case.Q))[0] == 59 and len(case.Q) % 256 and len(case.Q) % 64
    Ts = _centred(ctx, case, _motions(B))
    got = ctx.sums_batch(Ts, metric)
    want = _single_sums(ctx, Ts, metric)
    assert got.shape == (B, 31 if metric == "plane" else 17) and want[0, 0] > 1000
    assert np.array_equal(got, want)
    if B > 1:
        assert not np.array_equal(got[0], got[1])


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_sums_batch_on_ragged_sources(icp, n):
    case = E.ragged(n)
    ctx = _ctx(icp, case)
    try:
        Ts = _centred(ctx, case, _motions(3))
        for metric in ("point", "plane"):
            got = ctx.sums_batch(Ts, metric)
            assert np.array_equal(got, _single_sums(ctx, Ts, metric)), metric
            assert got[0, 0] == n
    finally:
        ctx.close()


def test_sums_batch_past_the_full_launch(icp):
    """524 289 source points: the first size whose lanes take two trips (kMaxBlocks x kBlock + 1)."""
    case = E.full_launch_pair()
    Q = case.Q[:E.FULL_LAUNCH_N[1]]
    assert E.launch(len(Q)) == (E.K_MAX_BLOCKS, 1, 2)
    ctx = _ctx(icp, case, Q)
    try:
        Ts = _centred(ctx, case, [_motion(0.3, 0.002), _motion(0.0, 0.0)])
        for metric in ("point", "plane"):
            got = ctx.sums_batch(Ts, metric)
            assert np.array_equal(got, _single_sums(ctx, Ts, metric)), metric
            assert got[0, 0] > 100_000
    finally:
        ctx.close()


def test_sums_batch_far_from_the_origin_and_outside_the_grid(icp):
    """The far case (coordinates of 1e4, equal distances the rule), one pose of it with every image outside the grid."""
    case = E.far()
    ctx = _ctx(icp, case)
    try:
        away = np.eye(4); away[:3, 3] = [50.0, 0.0, 0.0]
        Ts = _centred(ctx, case, [np.eye(4), away, _motion(0.5, 0.001)])
        for metric in ("point", "plane"):
            got = ctx.sums_batch(Ts, metric)
            assert np.array_equal(got, _single_sums(ctx, Ts, metric)), metric
            assert got[0, 0] > 10_000 and got[2, 0] > 1000 and not got[1].any()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# refine

def _starts(case):
    """The true pose (converges at once), 2 degrees, 10 degrees, a pose without any correspondence in the middle, one more
    good start after it: the active list loses its front, its middle and its end at different iterations."""
    lost = np.eye(4); lost[:3, 3] = [10.0, 0.0, 0.0]
    return np.stack([E.pose(case, M) for M in (np.eye(4), _motion(2.0, 0.004), _motion(10.0, 0.01), lost, _motion(1.0, -0.003))])


def _singles(ctx, T0s, **kw):
    out = [ctx.refine(T0, **kw) for T0 in T0s]
    return np.stack([T for T, _ in out]), [r for _, r in out]


def _assert_same_bytes(Ts, res, Tw, rw):
    for b in range(len(Tw)):
        assert np.array_equal(Ts[b], Tw[b]), (b, Ts[b] - Tw[b])
        assert _bytes(res[b]) == _bytes(rw[b]), (b, res[b].as_dict(), rw[b].as_dict())


@pytest.mark.parametrize("metric", ["point", "plane"])
def test_refine_batch_unordered_equals_the_single_refines(box, icp, metric):
    case, ctx = box
    T0s = _starts(case)
    Ts, res, order = ctx.refine_batch(T0s, order_source=False, metric=metric)
    Tw, rw = _singles(ctx, T0s, order_source=False, metric=metric)
    its = [r.iterations for r in res]
    print(metric, "iterations", its, "status", [r.status for r in res], "n_corr", [r.n_corr for r in res])
    _assert_same_bytes(Ts, res, Tw, rw)
    assert res[3].status == icp.TOO_FEW and res[3].iterations == 0 and res[3].n_corr == 0 and res[3].history_len == 1
    assert np.array_equal(Ts[3], T0s[3])
    # the poses leave the active list at different iterations: the lost one (in the middle) first, and for the point metric
    # the true pose (the front) and the last one (the end) before the 2 degree and the 10 degree starts
    assert len(set(its)) >= 3 and min(its[b] for b in (0, 1, 2, 4)) > 0
    if metric == "point":
        assert res[0].status == icp.CONVERGED and its[0] < its[1] < its[2] and its[4] < its[2]
    assert np.array_equal(order, icp.rank_batch(res)) and order[-1] == 3


@pytest.mark.parametrize("metric", ["point", "plane"])
def test_refine_batch_with_a_pose_that_runs_out_of_iterations(box, icp, metric):
    case, ctx = box
    T0s = _starts(case)
    full = [r.iterations for r in ctx.refine_batch(T0s, order_source=False, metric=metric)[1]]
    cap = max(full) - 1                                   # the slowest pose is cut short, a faster one still converges
    assert cap > min(i for i in full if i > 0)
    Ts, res, _ = ctx.refine_batch(T0s, order_source=False, metric=metric, max_iterations=cap)
    Tw, rw = _singles(ctx, T0s, order_source=False, metric=metric, max_iterations=cap)
    _assert_same_bytes(Ts, res, Tw, rw)
    st = [r.status for r in res]
    assert icp.MAX_ITERATIONS in st and icp.CONVERGED in st and st[3] == icp.TOO_FEW
    assert max(r.iterations for r in res) == cap
    # zero iterations: the final pass alone
    Ts, res, _ = ctx.refine_batch(T0s, order_source=False, metric=metric, max_iterations=0)
    Tw, rw = _singles(ctx, T0s, order_source=False, metric=metric, max_iterations=0)
    _assert_same_bytes(Ts, res, Tw, rw)


def test_refine_batch_plane_degenerate_on_a_flat_target(icp):
    case = E.flat()
    ctx = _ctx(icp, case, normals=np.tile(np.array([0, 0, 1], F), (len(case.P), 1)))
    try:
        T0s = np.stack([E.pose(case, M) for M in (np.eye(4), _motion(0.2, 0.001), _motion(0.0, [0.002, 0.0, 0.0]))])
        for order_source in (False, True):
            Ts, res, _ = ctx.refine_batch(T0s, metric="plane", order_source=order_source)
            Tw, rw = _singles(ctx, T0s, metric="plane", order_source=False)
            assert all(r.status == icp.DEGENERATE and r.iterations == 0 for r in res)
            assert all(r.status == icp.DEGENERATE for r in rw)
            assert np.array_equal(Ts, Tw)                     # no solve was applied: the start, through the centred frame and back
            assert np.max(np.abs(Ts - T0s)) < 1e-12
            if not order_source:
                _assert_same_bytes(Ts, res, Tw, rw)
    finally:
        ctx.close()


@pytest.mark.parametrize("metric", ["point", "plane"])
def test_refine_batch_ordered_source(box, icp, metric):
    """Pose 0 is the single ordered call bit for bit; the others differ from their unordered results by the order of the
    double sums only: same status, iterations and final count, T within ORDER_T_BOUND."""
    case, ctx = box
    T0s = _starts(case)
    To, ro, _ = ctx.refine_batch(T0s, order_source=True, metric=metric)
    T1, r1 = ctx.refine(T0s[0], order_source=True, metric=metric)
    assert np.array_equal(To[0], T1) and _bytes(ro[0]) == _bytes(r1)
    Tu, ru, _ = ctx.refine_batch(T0s, order_source=False, metric=metric)
    worst = float(np.max(np.abs(To - Tu)))
    ulp = float(np.max(np.spacing(np.abs(Tu).astype(F))))
    print("ordered vs unordered, %s: max |dT| = %.3e (float step of the largest entry %.3e, bound %.3e)" % (metric, worst, ulp, ORDER_T_BOUND))
    for b in range(len(T0s)):
        assert (ro[b].status, ro[b].iterations, ro[b].n_corr) == (ru[b].status, ru[b].iterations, ru[b].n_corr), b
    assert worst <= ORDER_T_BOUND


# ---------------------------------------------------------------------------------------------------------------------
# ranking, refusals, interfaces

def test_order_prefers_the_pose_the_full_clouds_prefer(box, icp):
    case, ctx = box
    T0s = np.stack([E.pose(case, _motion(40.0, 0.0)), E.pose(case, _motion(2.0, 0.004))])
    Ts, res, order = ctx.refine_batch(T0s)
    print("n_corr", [r.n_corr for r in res], "rmse", [r.rmse for r in res])
    assert np.array_equal(order, icp.rank_batch(res)) and list(order) == [1, 0]
    assert res[1].n_corr > res[0].n_corr
    T, r, i = icp.refine_best(case.P, case.Q, T0s, max_distance=case.d)
    assert i == 1 and np.array_equal(T, Ts[1]) and _bytes(r) == _bytes(res[1])


def test_refusals(box, icp):
    case, ctx = box
    T0s = _starts(case)
    L = icp.load_library()
    ctx.set_rejection(reciprocal=True)
    try:
        for call in (lambda: ctx.refine_batch(T0s), lambda: ctx.sums_batch(T0s.astype(F))):
            with pytest.raises(icp.ICPError) as e:
                call()
            assert e.value.code == -7 and "rejection" in str(e.value)
    finally:
        ctx.set_rejection()
    bare = icp.ICP(0)
    try:
        with pytest.raises(icp.ICPError) as e:
            bare.refine_batch(T0s)
        assert e.value.code == -7
        bare.set_target(case.P, case.d)
        bare.set_source(case.Q)
        with pytest.raises(icp.ICPError) as e:
            bare.refine_batch(T0s, metric="plane")
        assert e.value.code == -7 and "normals" in str(e.value)
        assert len(bare.refine_batch(T0s[:2], max_iterations=1)[1]) == 2
    finally:
        bare.close()
    with pytest.raises(ValueError):
        ctx.refine_batch(T0s, metric="gicp")
    with pytest.raises(ValueError):
        ctx.refine_batch(np.tile(np.eye(4), (65, 1, 1)))
    # the C entry points themselves
    T = np.tile(np.eye(4), (65, 1, 1)).astype(np.float64)
    res = (icp.Result * 65)()
    dp = C.POINTER(C.c_double)
    p = icp.BatchParams()
    L.s4p_icp_default_params(C.byref(p.icp))
    for B, metric in ((65, 0), (0, 0), (2, 2), (2, -1)):
        p.metric = metric
        assert L.s4p_icp_refine_batch(ctx.h, C.byref(p), B, T.ctypes.data_as(dp), res, None) == -1, (B, metric)
    p.metric = 0
    assert L.s4p_icp_refine_batch(ctx.h, C.byref(p), 2, None, res, None) == -1
    assert L.s4p_icp_refine_batch(ctx.h, C.byref(p), 2, T.ctypes.data_as(dp), None, None) == -1
    out = np.empty((65, 31))
    T32 = T.astype(F)
    fp = C.POINTER(C.c_float)
    assert L.s4p_icp_sums_batch(ctx.h, 0, 65, T32.ctypes.data_as(fp), out.ctypes.data_as(dp)) == -1
    assert L.s4p_icp_sums_batch(ctx.h, 3, 2, T32.ctypes.data_as(fp), out.ctypes.data_as(dp)) == -1
    assert L.s4p_icp_sums_batch(ctx.h, 0, 2, None, out.ctypes.data_as(dp)) == -1


def test_numpy_and_device_inputs_and_repeated_calls_give_the_same_bits(box, icp):
    import torch
    case, ctx = box
    T0s = _starts(case)
    a = ctx.refine_batch(T0s, metric="plane")
    b = ctx.refine_batch(T0s, metric="plane")
    dev = icp.ICP(0)
    try:
        dev.set_target(torch.from_numpy(case.P).cuda(), case.d)
        dev.set_source(torch.from_numpy(case.Q).cuda())
        dev.estimate_normals(case.d)
        c = dev.refine_batch(T0s, metric="plane")
        Tc = _centred(ctx, case, _motions(4))
        assert np.array_equal(dev.sums_batch(Tc), ctx.sums_batch(Tc))
    finally:
        dev.close()
    for other in (b, c):
        assert np.array_equal(a[0], other[0]) and np.array_equal(a[2], other[2])
        assert [_bytes(r) for r in a[1]] == [_bytes(r) for r in other[1]]
    T1 = icp.refine_best(case.P, case.Q, T0s, max_distance=case.d)
    T2 = icp.refine_best(torch.from_numpy(case.P).cuda(), torch.from_numpy(case.Q).cuda(), T0s, max_distance=case.d)
    assert np.array_equal(T1[0], T2[0]) and _bytes(T1[1]) == _bytes(T2[1]) and T1[2] == T2[2]


def test_multiscale_from_several_starts_ends_where_the_good_start_ends(icp):
    from super4pcs_amd import multiscale
    case = MH.small_pair()
    P, Q, good = case["P"], case["Q"], case["T0"]
    bad = case["T_gt"] @ MH.rot_about((0.3, -0.5, 0.8), 40.0, Q.astype(np.float64).mean(0))
    kw = dict(voxel_sizes=(0.15, 0), max_distance=0.05, max_iterations=20, order_source=False)
    T, levels = multiscale.refine_multiscale(P, Q, starts=[bad, good], **kw)
    Tw, lw = multiscale.refine_multiscale(P, Q, T0=good, **kw)
    assert np.array_equal(T, Tw) and [_bytes(r) for r in levels] == [_bytes(r) for r in lw]
    Tb, _ = multiscale.refine_multiscale(P, Q, T0=bad, **kw)
    assert not np.array_equal(Tb, T)                              # the bad start alone ends elsewhere: the batch chose
    for bad_kw in (dict(loss="huber"), dict(metric="gicp"), dict(metric="color"), dict(reciprocal=True), dict(T0=good)):
        with pytest.raises(ValueError):
            multiscale.refine_multiscale(P, Q, starts=[bad, good], **{**kw, **bad_kw})
