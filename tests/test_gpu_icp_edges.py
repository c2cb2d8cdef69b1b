"""The ICP library (libsuper4pcs_icp.so) on the MI355X in the regimes its contract tests did not enter (DESIGN.md section 15;
inputs in tests/icp_edge_cases.py, their regimes asserted on the host in tests/test_icp_edges_host.py): one-cell and flat and
enlarged grids, ragged and tiny sources, queries outside the target's box, clouds far from the origin, launches whose
lanes take two and three trips with a full 2048-row slab, and residual keys crafted bit for bit for the radix select.

Every comparison is one the existing modules make, by their own checkers: _check_pass (test_gpu_icp.py), _check_plane_sums
(test_gpu_icp_plane.py) and _check (test_gpu_icp_robust.py).  Estimated normals are compared bit for bit with a literal
restatement of k_normals (tests/icp_plane_cpu/icp_normals_literal.cpp: the same terms in the same order, the same Jacobi) and,
as an independent reference, by test_gpu_icp_plane.py's rule against numpy's eigh."""
import contextlib
import hashlib

import numpy as np
import pytest

from tests import icp_edge_cases as E
from tests import icp_helpers as H
from tests import icp_plane_helpers as PH
from tests import icp_robust_helpers as RH
from tests.test_gpu_icp import _check_pass
from tests.test_gpu_icp_plane import MIN_NB, _check_plane_sums
from tests.test_gpu_icp_robust import _check

pytestmark = pytest.mark.gpu
F = np.float32
MOTIONS = ((0.0, 0.0), (0.3, 0.002), (-0.5, -0.003))
ROBUST = (dict(loss="trimmed", trim_fraction=0.7), dict(loss="trimmed", trim_fraction=0.3), dict(loss="huber"), dict(loss="tukey"))


def _digest(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.shape, a.dtype)).encode())
        h.update(a.tobytes())
    return h.digest()


class MemoCPU:
    """The CPU restatement with its passes remembered, keyed on a digest of the clouds (the checkers each ask for the pass of
    the transform they are given: the large cases pay 3.5 s per million source points for one).  Inside recording(), the n
    of every pass is kept in order."""

    def __init__(self, cpu):
        self.cpu, self.pair, self.memo, self.ns = cpu, None, {}, None

    def pass_(self, Pc, Qc, T, d, want_idx=True, threads=0):
        pair = _digest(Pc, Qc)
        if pair != self.pair:
            self.pair, self.memo = pair, {}                                               # one pair's passes at a time
        key = (np.asarray(T, F).tobytes(), float(d), want_idx)
        if key not in self.memo:
            self.memo[key] = self.cpu.pass_(Pc, Qc, T, d, want_idx=want_idx, threads=threads)
        if self.ns is not None:
            self.ns.append(int(self.memo[key][2][0]))
        return self.memo[key]

    @contextlib.contextmanager
    def recording(self):
        self.ns = ns = []
        try:
            yield ns
        finally:
            self.ns = None

    def brute(self, *a):
        return self.cpu.brute(*a)


@pytest.fixture(scope="module")
def icp(s4p_lib_built):
    from super4pcs_amd import build as B
    B.build_icp()
    from super4pcs_amd import icp as I
    return I


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return MemoCPU(H.build_cpu(tmp_path_factory.mktemp("icp_cpu")))


@pytest.fixture(scope="module")
def pcpu(tmp_path_factory):
    return PH.build_plane_cpu(tmp_path_factory.mktemp("icp_plane_cpu"))


@pytest.fixture(scope="module")
def literal(tmp_path_factory):
    return PH.build_normals_literal(tmp_path_factory.mktemp("icp_normals_literal"))


def _context(icp, case, Q=None):
    ctx = icp.ICP(0)
    ctx.set_target(case.P, case.d)
    ctx.set_source(case.Q if Q is None else Q)
    return ctx


def _check_frame(ctx, P):
    """Within one float step of the float64 mean: the library's double sums differ from numpy's only in their order, so the
    float result can differ only where the mean sits on a rounding tie."""
    c = ctx.frame()
    want = E.frame(P)
    assert np.all((c == want) | (c == np.nextafter(want, F(np.inf))) | (c == np.nextafter(want, F(-np.inf)))), (c, want)
    return c


def _caller_normals(P, seed):
    raw = np.random.default_rng(seed).normal(size=P.shape).astype(F) * 3
    raw[::11] = 0
    return raw


# Cases where almost no target point has min_neighbours points within d (the radius cannot exceed max_distance), so that
# test_gpu_icp_plane.py's floor on separated normals cannot hold: the one-point target, the 50 k points of a unit cube at
# d = 0.004, the needle's 30 points per unit volume at d = 0.05 and the flat cloud's 1.6 neighbours at d = 0.01.  Their zero
# normals, and the few nonzero ones, are still compared bit for bit.
SPARSE = ("one_target", "enlarged", "needle", "flat")


def _check_estimated_normals(ctx, pcpu, literal, P, d, name, sample=None):
    """On a sample (every point when None): the bits of the literal restatement of k_normals, and test_gpu_icp_plane.py's
    _check_normals against numpy's eigh, floor on the separated count included except for the SPARSE cases.  Returns
    (normals, number of nonzero normals in the sample)."""
    r = d
    c = ctx.frame()
    Pc = (P - c).astype(F)
    ctx.estimate_normals(r, MIN_NB)
    G = ctx.target_normals()
    L, dims, h = literal(Pc, d, r, MIN_NB, which=sample, threads=16)
    Gs = G if sample is None else G[sample]
    diff = np.flatnonzero((Gs.view(np.uint32) != L.view(np.uint32)).any(1))
    assert len(diff) == 0, (name, len(diff), diff[:5], Gs[diff[:3]], L[diff[:3]])
    k, c6 = pcpu.cov(Pc, r, threads=16)
    s = np.arange(len(P)) if sample is None else sample
    N, w = PH.normals_from_cov(k[s], c6[s], MIN_NB)
    zero_g, zero_c = ~G[s].any(1), ~N.any(1)
    assert np.array_equal(zero_g, zero_c) and np.array_equal(zero_c, k[s] < MIN_NB)
    sep = (w[:, 1] >= 4 * w[:, 0]) & ~zero_c
    if name not in SPARSE:
        assert sep.sum() > 0.1 * len(s), (name, sep.sum())
    if name not in SPARSE or sep.any():
        dots = np.abs((G[s][sep].astype(np.float64) * N[sep].astype(np.float64)).sum(1))
        assert dots.min() >= 1 - 1e-6, dots.min()
    nz = G.any(1)
    assert np.all(np.abs(np.linalg.norm(G[nz].astype(np.float64), axis=1) - 1) < 1e-6)
    ctx.estimate_normals(r, MIN_NB)
    assert np.array_equal(ctx.target_normals(), G)                 # two calls, identical bits
    print("normals %s: n %d, grid %s, checked %d bit for bit, separated %d, zero %d" % (name, len(P), dims.tolist(), len(s), sep.sum(),
                                                                                     zero_c.sum()))
    return G, int(np.count_nonzero(~zero_c))


def _robust_everywhere(ctx, cpu, case, Q, N, T_caller):
    Tc = H.to_centred(T_caller, ctx.frame()).astype(F)
    for kw in ROBUST:
        for metric in ("point", "plane"):
            _check(ctx, cpu, case.P, Q, N, Tc, case.d, metric, kw)


@pytest.mark.parametrize("name", sorted(E.SMALL))
def test_small_cases_are_the_contract(icp, cpu, pcpu, literal, name):
    """Per case: idx and d2 bit for bit against the CPU restatement (and numpy where small) and the 17 sums, at the base pose
    and two motions; the plane sums with caller and with estimated normals; the robust sums for four losses and both metrics;
    the estimated normals at every target point."""
    case = E.SMALL[name]()
    ctx = _context(icp, case)
    c = _check_frame(ctx, case.P)
    Pc, Qc = (case.P - c).astype(F), (case.Q - c).astype(F)
    for k, (ang, sh) in enumerate(MOTIONS):
        T = E.pose(case, RH.motion(ang, sh))
        n = _check_pass(ctx, cpu, case.P, case.Q, T, case.d)
        if k == 0:
            assert n >= 1 and (name not in E.HAS_MISSES or n < len(case.Q)), (name, n)
        if len(Pc) * len(Qc) <= 4e7:
            Tc = H.to_centred(T, c).astype(F)
            gi, gd = ctx.correspondences(Tc)
            ni, nd = H.numpy_brute(Pc, Qc, Tc, case.d)
            assert np.array_equal(gi, ni) and np.array_equal(gd, nd)
        print("%s motion %d: matched %d of %d" % (name, k, n, len(case.Q)))
    raw = _caller_normals(case.P, 4)
    ctx.set_target_normals(raw)
    Nu = PH.normalise(raw)
    assert np.array_equal(ctx.target_normals(), Nu)
    for ang, sh in MOTIONS[:2]:
        T = E.pose(case, RH.motion(ang, sh))
        _check_plane_sums(ctx, cpu, case.P, case.Q, Nu, T, case.d)
        _robust_everywhere(ctx, cpu, case, case.Q, Nu, T)
    Ne, _ = _check_estimated_normals(ctx, pcpu, literal, case.P, case.d, name)
    for ang, sh in MOTIONS[:2]:
        T = E.pose(case, RH.motion(ang, sh))
        _check_plane_sums(ctx, cpu, case.P, case.Q, Ne, T, case.d)
        _robust_everywhere(ctx, cpu, case, case.Q, Ne, T)
    ctx.close()


def _large_case(icp, cpu, pcpu, literal, case, n_qs, twice=False):
    ctx = icp.ICP(0)
    ctx.set_target(case.P, case.d)
    _check_frame(ctx, case.P)
    assert E.launch(len(case.P))[2] >= 2                                  # the target's kernels loop as well
    rng = np.random.default_rng(9)
    sample = np.sort(rng.choice(len(case.P), 3000, replace=False))
    raw = _caller_normals(case.P, 5)
    Nu = PH.normalise(raw)
    Ne = None
    for n_q in n_qs:
        Q = case.Q[:n_q]
        assert E.launch(n_q)[0] == E.K_MAX_BLOCKS
        ctx.set_source(Q)
        for k, (ang, sh) in enumerate(MOTIONS):
            n = _check_pass(ctx, cpu, case.P, Q, RH.motion(ang, sh) @ case.T0, case.d)
            assert 1000 < n < n_q
            print("%s n_Q %d motion %d: matched %d" % (case.name, n_q, k, n))
        if n_q > E.K_MAX_BLOCKS * E.K_BLOCK:                               # the later trips see matched sources
            c = ctx.frame()
            ci, _, _ = cpu.pass_((case.P - c).astype(F), (Q - c).astype(F), H.to_centred(case.T0, c).astype(F), case.d)
            assert np.any(ci[E.K_MAX_BLOCKS * E.K_BLOCK:] >= 0)
        ctx.set_target_normals(raw)
        assert _check_plane_sums(ctx, cpu, case.P, Q, Nu, case.T0, case.d) > 1000
        _robust_everywhere(ctx, cpu, case, Q, Nu, case.T0)
        if Ne is None:
            Ne, nonzero = _check_estimated_normals(ctx, pcpu, literal, case.P, case.d, case.name, sample)
            assert nonzero > 2900
        else:
            ctx.estimate_normals(case.d, MIN_NB)
            assert np.array_equal(ctx.target_normals(), Ne)
        assert _check_plane_sums(ctx, cpu, case.P, Q, Ne, case.T0, case.d) > 1000
        Tc = H.to_centred(case.T0, ctx.frame()).astype(F)
        for kw in (ROBUST[0], ROBUST[3]):
            _check(ctx, cpu, case.P, Q, Ne, Tc, case.d, "plane", kw)
        if twice:                                                         # determinism across multi-trip lanes
            a = (ctx.correspondences(Tc), ctx.sums(Tc), ctx.plane_sums(Tc), ctx.robust_sums(Tc, "plane", "tukey"),
                 ctx.robust_sums(Tc, "point", "trimmed", trim_fraction=0.4))
            b = (ctx.correspondences(Tc), ctx.sums(Tc), ctx.plane_sums(Tc), ctx.robust_sums(Tc, "plane", "tukey"),
                 ctx.robust_sums(Tc, "point", "trimmed", trim_fraction=0.4))
            flat = lambda t: [np.asarray(x).tobytes() for part in t for x in (part if isinstance(part, tuple) else (part,))]
            assert flat(a) == flat(b)
    ctx.close()


def test_full_launch_sizes_are_the_contract(icp, cpu, pcpu, literal):
    """n_Q = 524 288 (2048 workgroups, one trip per lane) and 524 289 (lane 0 takes a second trip) on a 600 k target."""
    _large_case(icp, cpu, pcpu, literal, E.full_launch_pair(), E.FULL_LAUNCH_N)


def test_long_launch_is_the_contract_and_deterministic(icp, cpu, pcpu, literal):
    """1.3 M points per cloud: two to three trips per lane with a ragged last trip, 2048 slab rows; two calls, identical bytes."""
    case = E.long_launch()
    _large_case(icp, cpu, pcpu, literal, case, (len(case.Q),), twice=True)


def test_frame_of_identical_points_is_exact(icp):
    """n equal points: every partial sum k v is exact in double and (n v) / n = v, so the frame is v itself; n = 600 001 takes
    k_stats through a second trip."""
    v = np.array([0.3, -1.7, 2.9], F)
    for n in (1, 1000, 600_001):
        ctx = icp.ICP(0)
        ctx.set_target(np.tile(v, (n, 1)), 0.1)
        assert np.array_equal(ctx.frame(), v), n
        ctx.set_source(v[None] + np.array([[0.05, 0, 0], [0.5, 0, 0]], F))
        gi, gd = ctx.correspondences(np.eye(4, dtype=F))
        dx = F(F(v[0] + F(0.05)) - v[0])
        assert gi.tolist() == [0, -1] and gd[0] == dx * dx and gd[1] == 0
        ctx.close()


@pytest.mark.parametrize("name", ["box_faces", "far"])
def test_refine_on_edge_cases_equals_the_cpu_loop(icp, cpu, name):
    """The existing trajectory rules on sources that start outside the target's box (k_source_keys sorts them last) and on
    clouds far from the origin: the first three history_n and history_rmse (rtol 1e-9) are the CPU loop's, the transform is
    within 1e-5 of it, n_corr is the CPU pass's n at the returned float transform; order_source=False agrees."""
    case = E.SMALL[name]()
    ctx = _context(icp, case)
    c = ctx.frame()
    Pc, Qc = (case.P - c).astype(F), (case.Q - c).astype(F)
    T0 = E.pose(case, RH.motion(0.5, 0.003))
    T, r = ctx.refine(T0)
    with cpu.recording() as hist_n:
        Tc, its, status, hist = H.cpu_refine(cpu, icp.solve, Pc, Qc, c, T0, case.d, threads=16)
    k = min(r.history_len, len(hist), 3)
    print("%s refine: gpu %d its (%s) rmse %.6g n %d; cpu %d its (%s) |dT| %.2g; history_n %s" % (
        name, r.iterations, icp.STATUS_NAMES[r.status], r.rmse, r.n_corr, its, icp.STATUS_NAMES[status], np.max(np.abs(T - Tc)),
        list(r.history_n[:k])))
    assert k == 3
    assert abs(r.iterations - its) <= 1 and r.status == status
    assert list(r.history_n[:k]) == hist_n[:k]
    assert np.allclose(list(r.history_rmse[:k]), hist[:k], rtol=1e-9, atol=0)
    assert np.max(np.abs(T - Tc)) <= 1e-5
    _, _, s = cpu.pass_(Pc, Qc, H.to_centred(T, c).astype(F), case.d, want_idx=False, threads=16)
    assert r.n_corr == s[0] and 0 < r.n_corr < len(case.Q)
    Tu, ru = ctx.refine(T0, order_source=False)
    assert list(ru.history_n[:k]) == hist_n[:k]
    assert np.max(np.abs(Tu - T)) <= 1e-5
    ctx.close()


@pytest.mark.parametrize("metric", ["point", "plane"])
def test_selection_on_crafted_keys(icp, cpu, metric):
    """The radix select on keys chosen bit for bit (tests/icp_edge_cases.py: crafted_multisets): info[:3] = [M, k, bits of
    np.partition's k-th], info[4] the count of keys not above it (ties at the threshold kept; plus, for the plane metric, the
    matches without a key), and for Tukey the contract's s = max(1.4826 sqrt(u_k), 1e-6 d) at the median."""
    I = np.eye(4, dtype=F)
    for ms in E.crafted_multisets(metric):
        ctx = icp.ICP(0)
        ctx.set_target(ms.P, E.KEY_D)
        ctx.set_source(ms.Q)
        ctx.set_target_normals(ms.N)
        assert np.array_equal(ctx.frame(), np.zeros(3, F))
        M, n_q = len(ms.keys), len(ms.Q)
        free = E.N_UNKEYED if metric == "plane" else 0
        for k in ms.ks:
            assert 1 <= k <= M < n_q
            xi = E.trim_for(k, n_q)
            thr, count = E.expected_selection(ms.keys, k)
            s, info = ctx.robust_sums(I, metric, "trimmed", trim_fraction=xi)
            print("%s %s k %d: info %s, want thr %#x count %d" % (metric, ms.name, k, info[:5].tolist(), thr, count))
            assert info[:5].tolist() == [M, k, thr, 0.0, count + free], (ms.name, k)
            assert s[0] == count + free
            _check(ctx, cpu, ms.P, ms.Q, ms.N, I, E.KEY_D, metric, dict(loss="trimmed", trim_fraction=xi))
        km = (M + 1) // 2
        thr, _ = E.expected_selection(ms.keys, km)
        s, info = ctx.robust_sums(I, metric, "tukey")
        assert info[:3].tolist() == [M, km, thr] and info[3] == E.median_scale(thr, E.KEY_D), (ms.name, info)
        _check(ctx, cpu, ms.P, ms.Q, ms.N, I, E.KEY_D, metric, dict(loss="tukey"))
        _check(ctx, cpu, ms.P, ms.Q, ms.N, I, E.KEY_D, metric, dict(loss="huber"))
        ctx.close()


def test_trim_fraction_products(icp):
    """k = ceil(trim_fraction * n_Q) on the double product: whole products and ones a rounding step above a whole number, for
    both metrics."""
    import math
    I = np.eye(4, dtype=F)
    for metric in ("point", "plane"):
        for xi, n_q in E.TRIM_PRODUCTS:
            ms = E.trim_product_case(n_q, metric)
            assert len(ms.Q) == n_q
            free = E.TRIM_N_UNKEYED if metric == "plane" else 0
            ctx = icp.ICP(0)
            ctx.set_target(ms.P, E.KEY_D)
            ctx.set_source(ms.Q)
            ctx.set_target_normals(ms.N)
            k = math.ceil(xi * n_q)
            assert 1 <= k <= len(ms.keys) < n_q
            thr, count = E.expected_selection(ms.keys, k)
            s, info = ctx.robust_sums(I, metric, "trimmed", trim_fraction=xi)
            assert info[:5].tolist() == [len(ms.keys), k, thr, 0.0, count + free] and count == k, (metric, xi, n_q, info)
            ctx.close()
