"""libsuper4pcs_normals.so on the MI355X on the clouds of tests/grid_regime_cases.py: degenerate shapes (one point many times,
lines, planes, a diagonal, a slab), clusters and an outlier far apart, clouds far from the origin, duplicated clouds, the edge
of the spacing estimate, and scales from 2^-38 to 3e38.  They reach the branches of set_cloud's planner, of the neighbour
walk and of the clustering grid that a unit cube near the origin never does: grids of one cell and of 800 000, cells that hold
the whole cloud, rings over empty cells, clamped query cells, d2 = +inf.  Every entry point equals its restatement bit for
bit (tests/test_grid_regimes_host.py shows that the restatements agree among themselves on the same cases), and each case's
grid is asserted to be in the regime the case is named for.  Below the documented limits (a planned cell edge under 2^-43, an
eps whose float square is subnormal) the library refuses; before that check existed, the same clouds came back with status OK
and wrong lists (DESIGN.md section "Grid regimes")."""
import time

import numpy as np
import pytest

from tests import cluster_helpers as CH
from tests import grid_regime_cases as G
from tests import knn_helpers as KH
from tests import normals_helpers as NH
from tests import normals_suite as S
from tests import orient_helpers as OH

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def clu():
    return S.normals_module("cluster")


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return NH.build_cpu(tmp_path_factory.mktemp("regimes_normals_cpu"))


@pytest.fixture(scope="module")
def cluster_cpu(tmp_path_factory):
    return CH.build_cpu(tmp_path_factory.mktemp("regimes_cluster_cpu"))


@pytest.fixture(scope="module")
def context(clu):
    """context(name): the case's own context, made at its first use and shared by the tests of the case."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = clu.Cluster(0)
            made[name].set_cloud(G.CASES[name]()[0])
        return made[name]
    yield get
    for ctx in made.values():
        ctx.close()


def _same_lists(got, want, what):
    gi, gd, gc = (np.asarray(a) for a in got)
    wi, wd, wc = want
    assert gi.dtype == np.int32 and gd.dtype == np.float32 and gc.dtype == np.int32 and gi.shape == wi.shape and gd.shape == wd.shape
    bad = np.flatnonzero((gi != wi).any(1) | (KH.bits(gd) != KH.bits(wd)).any(1) | (gc != wc))
    assert len(bad) == 0, (what, len(bad), bad[:5], gi[bad[:2]], wi[bad[:2]], gd[bad[:2]], wd[bad[:2]], gc[bad[:2]], wc[bad[:2]])
    # the padding, stated on the device's own output: -1 and +inf from cnt on
    pad = np.arange(gi.shape[1])[None, :] >= gc[:, None]
    assert (gi[pad] == -1).all() and np.isposinf(gd[pad]).all() and (gi[~pad] >= 0).all()


@pytest.mark.parametrize("name", G.ACCEPTED)
def test_the_grid_is_in_the_regime_of_the_case(context, name):
    g = context(name).grid()
    print("%s: n %d cell %.6g spacing %.6g dims %s cells %d nonempty %d max_per_cell %d" % (
        name, len(G.CASES[name]()[0]), g["cell"], g["spacing"], g["dims"], g["cells"], g["nonempty"], g["max_per_cell"]))
    assert G.CASES[name].regime(g), g
    assert g["cell"] >= G.MIN_CELL


@pytest.mark.parametrize("name", G.ACCEPTED)
def test_lists_equal_the_brute_force(context, name):
    X, radius, _, _ = G.CASES[name]()
    ctx = context(name)
    n = len(X)
    for k in G.KS:
        for bounded in (False, True):
            for ex in (False, True):
                want = G.reference_lists(name, k, bounded, ex)
                t0 = time.perf_counter()
                got = ctx.search(k, radius if bounded else None, exclude_self=ex)
                dt = time.perf_counter() - t0
                if name == "two_clusters_1d":
                    print("two_clusters_1d (separation %g): search k %d %s exclude_self %d: %.1f ms" % (
                        G.SEPARATION_1D, k, "radius" if bounded else "unbounded", ex, 1e3 * dt))
                assert got[0].shape == (n, k) and got[2].shape == (n,)
                _same_lists(got, want, (name, k, bounded, ex))


@pytest.mark.parametrize("name", G.ACCEPTED)
def test_queries_in_and_far_outside_the_box_equal_the_brute_force(context, name):
    X, radius, _, _ = G.CASES[name]()
    ctx = context(name)
    Q, own = G.queries(X)
    assert len(Q) == 36
    for k in G.KS:
        for r in (None, radius):
            with np.errstate(over="ignore"):
                want = KH.numpy_lists(X, k, r, queries=Q)
            got = ctx.search_at(Q, k, r)
            _same_lists(got, want, (name, k, r))
            assert got[2][-1] == 0 and (got[0][-1] == -1).all() and np.isposinf(got[1][-1]).all()      # the non-finite query
            self_form = ctx.search(k, r, exclude_self=False)
            _same_lists(tuple(v[:8] for v in got), tuple(v[own] for v in self_form), (name, "self", k, r))


@pytest.mark.parametrize("name", G.ACCEPTED)
def test_normals_equal_the_restatement_bit_for_bit(context, cpu, name):
    X, radius, _, _ = G.CASES[name]()
    ctx = context(name)
    for k in (3, 16, 32):
        for r in (None, radius):
            got = ctx.estimate(k, r)
            want = cpu.normals(X, k, r, threads=16)
            bad = np.flatnonzero((NH.bits(got) != NH.bits(want)).any(1))
            assert len(bad) == 0, (name, k, r, len(bad), bad[:5], got[bad[:3]], want[bad[:3]])
            if name in G.PLANES:                          # the constant coordinate's e is exactly 0: the normal is the axis itself
                axis = np.zeros(3, np.float32)
                axis[G.PLANES[name]] = 1
                cnt = G.reference_lists(name, k, r is not None, False)[2]
                assert (got[cnt >= 3] == axis).all() and (got[cnt < 3] == 0).all() and (r is not None or (cnt >= 3).all())
            if name == "identical":
                assert (got == 0).all() and not np.signbit(got).any()


@pytest.mark.parametrize("name", G.ACCEPTED)
def test_outlier_filters_equal_the_references(context, name):
    X, radius, _, _ = G.CASES[name]()
    ctx = context(name)
    n = len(X)
    keep, stats, md = ctx.statistical_outliers(8, 1.0)
    _, d2, cnt = G.reference_lists(name, 8, False, True)
    assert (cnt == min(8, n - 1)).all()
    with np.errstate(invalid="ignore"):
        m_ref = KH.mean_dist(d2, cnt)
        assert np.array_equal(md, m_ref), (name, np.flatnonzero(md != m_ref)[:5])                     # exactly
        if np.isfinite(m_ref).all():
            KH.check_sor(n, 8, 1.0, md, stats, keep, m_ref, name)
        else:                                             # scale_3e38: m = +inf, so mu = +inf and sigma = t = NaN, and no m <= t
            print(name, stats)
            assert name == "scale_3e38" and np.isposinf(m_ref).all()
            assert stats["mean"] == np.inf and np.isnan(stats["stddev"]) and np.isnan(stats["threshold"])
            assert stats["n"] == n and stats["kept"] == 0 and not keep.any()
    # the radius filter: at least 2 other points within the radius, from the distance matrix and from the short lists
    got = ctx.radius_outliers(radius, 2)
    want = G.numpy_density(X, radius) - 1 >= 2
    assert got.dtype == bool and np.array_equal(got, want), (name, np.flatnonzero(got != want)[:5])
    cnt32 = G.reference_lists(name, 32, True, True)[2]
    assert np.array_equal(got[cnt32 < 32], cnt32[cnt32 < 32] >= 2) and got[cnt32 == 32].all()
    print("%s: statistical kept %d of %d, radius kept %d" % (name, keep.sum(), n, got.sum()))


@pytest.mark.parametrize("name", G.ACCEPTED)
def test_orientation_equals_the_restatement(context, name):
    X, radius, _, _ = G.CASES[name]()
    ctx = context(name)
    N = OH.random_normals(len(X), 7 + len(X))
    for bounded in (False, True):
        idx = G.reference_lists(name, 8, bounded, True)[0]
        for vp in (None, G.viewpoint(X)):
            with np.errstate(over="ignore", invalid="ignore"):
                info = OH.same(ctx, X, N, idx, 8, radius if bounded else None, vp, (name, bounded, vp))
            assert info["components"] >= (2 if name in G.TWO_CLUSTERS else 1)


def _same_clusters(ctx, cluster_cpu, X, eps, min_points, what):
    label, kind, stats = ctx.dbscan(eps, min_points)
    want_l, want_k, want_s = cluster_cpu.dbscan(X, eps, min_points)
    assert label.dtype == np.int32 and kind.dtype == np.uint8
    print(what, "eps %g min_points %d" % (eps, min_points), stats)
    assert np.array_equal(kind, want_k), (what, "kind", np.flatnonzero(kind != want_k)[:8])
    assert np.array_equal(label, want_l), (what, "label", np.flatnonzero(label != want_l)[:8])
    assert stats == want_s, (what, stats, want_s)
    count = ctx.density(eps)
    assert count.dtype == np.int32 and np.array_equal(count, cluster_cpu.density(X, eps)), what
    assert np.array_equal(count, G.numpy_density(X, eps)) and np.array_equal(count >= min_points, kind == CH.CORE), what
    return stats, count


@pytest.mark.parametrize("name", G.ACCEPTED)
def test_clustering_equals_the_restatement(context, cluster_cpu, name):
    X, _, eps, mp = G.CASES[name]()
    ctx = context(name)
    _same_clusters(ctx, cluster_cpu, X, eps, mp, name)
    if name in G.TWO_CLUSTERS:                           # eps = 2000: one cell, one cluster, every point core
        stats, count = _same_clusters(ctx, cluster_cpu, X, np.float32(2000.0), mp, name)
        assert stats == {"core": len(X), "border": 0, "noise": 0, "clusters": 1} and (count == len(X)).all()


def _flat(out):
    if isinstance(out, (tuple, list)):
        return [_flat(v) for v in out]
    if isinstance(out, dict):
        return {key: _flat(v) for key, v in sorted(out.items())}
    if isinstance(out, np.ndarray):
        return (out.dtype.str, out.shape, np.ascontiguousarray(out).tobytes())
    return out


def _four_calls(ctx, name):
    X, _, eps, _ = G.CASES[name]()
    N = OH.random_normals(len(X), 3)
    return _flat([ctx.grid(), ctx.search(8), ctx.estimate(16), ctx.density(eps), ctx.orient(N, 8, return_info=True)])


def test_one_context_across_cases_equals_fresh_contexts(clu):
    """The arena only grows, and the cell ranges are allocated anew between a grid of one cell and one of 800 000."""
    one = clu.Cluster(0)
    cells = []
    for name in G.ONE_CONTEXT_ORDER:
        one.set_cloud(G.CASES[name]()[0])
        got = _four_calls(one, name)
        fresh = clu.Cluster(0)
        fresh.set_cloud(G.CASES[name]()[0])
        want = _four_calls(fresh, name)
        fresh.close()
        for what, a, b in zip(("grid", "search", "estimate", "density", "orient"), got, want):
            assert a == b, (name, what)
        cells.append(one.grid()["cells"])
    one.close()
    print("cells along the sequence:", cells)
    assert min(cells) == 1 and max(cells) >= 2 ** 19


@pytest.mark.parametrize("kind", ["numpy", "torch"])
@pytest.mark.parametrize("name", G.REFUSED)
def test_a_cloud_below_the_scale_limit_is_refused_and_the_context_stays_usable(clu, name, kind):
    """Before set_cloud checked the planned cell edge, scale_below came back with status OK and lists that differed from
    the brute force (DESIGN.md section "Grid regimes" has the counts)."""
    X = G.CASES[name]()[0]
    line = G.CASES["line_x"]()[0]
    ctx = clu.Cluster(0)
    ctx.set_cloud(line)
    if kind == "torch":
        import torch
        X = S.to_device(np.array(X))
    with pytest.raises(clu.NormalsError) as e:
        ctx.set_cloud(X)
    assert e.value.code == -1 and "too small for float distances" in str(e.value) and "rescale the cloud" in str(e.value)
    with pytest.raises(clu.NormalsError) as e:            # the cloud before it is gone: no stale grid answers
        ctx.search(8)
    assert e.value.code == -7 and "set_cloud first" in str(e.value)
    ctx.set_cloud(line)
    _same_lists(ctx.search(8, exclude_self=True), G.reference_lists("line_x", 8, False, True), (name, kind, "after"))
    ctx.close()


def test_an_eps_with_a_subnormal_square_is_refused_and_a_normal_one_is_exact(clu, cluster_cpu):
    X = np.random.default_rng(1).uniform(size=(100, 3)).astype(np.float32)
    ctx = clu.Cluster(0)
    ctx.set_cloud(X)
    assert np.float32(1e-23) * np.float32(1e-23) == 0 and 0 < np.float32(1e-20) * np.float32(1e-20) < G.FLT_MIN
    for eps in (1e-23, 1e-20):                            # a zero and a subnormal square
        for call in (lambda: ctx.dbscan(eps, 4), lambda: ctx.density(eps)):
            with pytest.raises(clu.NormalsError) as e:
                call()
            assert e.value.code == -1 and "normal square in float" in str(e.value)
    assert np.float32(2e-19) * np.float32(2e-19) >= G.FLT_MIN
    stats, count = _same_clusters(ctx, cluster_cpu, X, np.float32(2e-19), 1, "eps 2e-19")
    assert stats["clusters"] == 100 and (count == 1).all()
    ctx.close()
