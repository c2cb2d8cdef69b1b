"""The references of the grid-regime cases (tests/grid_regime_cases.py) carry every case on their own, so that a mismatch on
the MI355X (tests/test_gpu_grid_regimes.py) is the device's: the numpy brute force and the tests/normals_cpu brute force give
the same lists on every case, tests/cluster_cpu's density equals a numpy count, and every case holds what its name claims (the
lists that cross the gap, the short lists, the ties, the +inf entries, the duplicates, the subnormal distances).  The refusal
texts and the documented limits are checked against the library's source and headers.  No GPU."""
import os
import re

import numpy as np
import pytest

from tests import cluster_helpers as CH
from tests import grid_regime_cases as G
from tests import knn_helpers as KH
from tests import normals_helpers as NH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return NH.build_cpu(tmp_path_factory.mktemp("regimes_normals_cpu"))


@pytest.fixture(scope="module")
def cluster_cpu(tmp_path_factory):
    return CH.build_cpu(tmp_path_factory.mktemp("regimes_cluster_cpu"))


def test_the_case_list():
    assert len(G.CASES) == 27 and set(G.REFUSED) < set(G.CASES) and set(G.ONE_CONTEXT_ORDER) < set(G.ACCEPTED)
    for name, fn in G.CASES.items():
        X, radius, eps, mp = fn()
        assert X.dtype == np.float32 and len(X) <= (4000 if name == "dup20" else 600) and radius > 0 and eps > 0 and mp >= 1
        assert fn() is fn() and not X.flags.writeable                       # computed once, left unchanged
        assert (fn.regime is None) == (name in G.REFUSED)               # a refused cloud has no grid
        with np.errstate(over="ignore"):
            assert name == "scale_below" or (np.isfinite(eps * eps) and eps * eps >= G.FLT_MIN)      # an eps the library accepts


@pytest.mark.parametrize("name", list(G.CASES))
def test_two_brute_forces_give_the_same_lists(cpu, name):
    X, radius, _, _ = G.CASES[name]()
    for bounded in (False, True):
        r = radius if bounded else None
        for k in G.KS:
            for ex in (False, True):
                wi, wd, wc = G.reference_lists(name, k, bounded, ex)
                with np.errstate(over="ignore", invalid="ignore"):
                    gi, gd, gc = KH.cpu_lists(cpu, X, k, r, exclude_self=ex)
                assert np.array_equal(gi, wi) and np.array_equal(KH.bits(gd), KH.bits(wd)) and np.array_equal(gc, wc), (name, k, r, ex)
                assert (wc == (wi >= 0).sum(1)).all() and np.isposinf(wd[wi < 0]).all()
        if len(X) <= 600:                                 # and the unsliced numpy form, once
            with np.errstate(over="ignore", invalid="ignore"):
                a = KH.numpy_lists(X, 8, r, exclude_self=True)
            b = G.reference_lists(name, 8, bounded, True)
            assert np.array_equal(a[0], b[0]) and np.array_equal(KH.bits(a[1]), KH.bits(b[1])) and np.array_equal(a[2], b[2])


_numpy_density = G.numpy_density


# scale_below is left out: its eps has a subnormal square, which the library refuses and at which the restatement's own
# cell grid loses neighbours in just the way the library's did
@pytest.mark.parametrize("name", [n for n in G.CASES if n != "scale_below"])
def test_cluster_restatement_equals_numpy(cluster_cpu, name):
    X, _, eps, mp = G.CASES[name]()
    epss = [eps] + ([np.float32(2000.0)] if name in G.TWO_CLUSTERS else [])
    for e in epss:
        count = cluster_cpu.density(X, e)
        assert np.array_equal(count, _numpy_density(X, e)), (name, e)
        label, kind, stats = cluster_cpu.dbscan(X, e, mp)
        assert np.array_equal(kind == CH.CORE, count >= mp)
        if len(X) <= 600:
            with np.errstate(over="ignore"):
                nl, nk, ns, nc = CH.numpy_dbscan(X, e, mp)
            assert np.array_equal(label, nl) and np.array_equal(kind, nk) and stats == ns and np.array_equal(count, nc), (name, e)
        print(name, float(e), mp, stats, "density", count.min(), count.max())
    if name in G.TWO_CLUSTERS:                           # eps = 2000: one cell, one cluster, every point core
        assert stats == {"core": len(X), "border": 0, "noise": 0, "clusters": 1} and (count == len(X)).all()


def _side(X):
    return X[:, 0] > 0.5 * G.SEPARATION_1D


def test_two_clusters_1d_lists_cross_the_gap_unbounded_and_are_short_with_the_radius():
    X, radius, _, _ = G.CASES["two_clusters_1d"]()
    far = _side(X)
    assert far.sum() == 20 and (~far).sum() == 20
    for ex in (False, True):
        idx, d2, cnt = G.reference_lists("two_clusters_1d", 32, False, ex)
        assert (cnt == 32).all() and (far[idx] != far[:, None]).any(1).all()      # 20 points a side: every list crosses
        assert (d2[:, -1] > 0.9 * G.SEPARATION_1D ** 2).all()
        idx, d2, cnt = G.reference_lists("two_clusters_1d", 32, True, ex)
        assert (cnt == 20 - ex).all() and (far[np.where(idx < 0, np.arange(40)[:, None], idx)] == far[:, None]).all()
    idx, _, cnt = G.reference_lists("two_clusters_1d", 8, False, True)
    assert (cnt == 8).all() and (far[idx] == far[:, None]).all()                  # k = 8 stays on its side


def test_two_clusters_2d_lists():
    X, radius, _, _ = G.CASES["two_clusters_2d"]()
    far = X[:, 0] > 500
    idx, _, cnt = G.reference_lists("two_clusters_2d", 32, False, True)
    assert far.sum() == 200 and (cnt == 32).all() and (far[idx] == far[:, None]).all()
    cnt = G.reference_lists("two_clusters_2d", 32, True, True)[2]
    assert (cnt < 32).all() and cnt.max() > 3


def test_offset_1e6_is_quantised_to_sixteenths_with_ties_and_duplicates():
    X = G.CASES["offset_1e6"]()[0]
    assert np.array_equal(X * 16, np.round(X * 16)) and X.min() >= 1e6
    dup = len(X) - len(np.unique(X, axis=0))
    idx, d2, cnt = G.reference_lists("offset_1e6", 8, False, True)
    ties = (d2[:, 1:] == d2[:, :-1])
    print("offset_1e6: %d duplicates, %d rows with a tie in the 8-list, %d zero distances" % (dup, ties.any(1).sum(), (d2 == 0).sum()))
    assert dup >= 10 and ties.any(1).mean() > 0.9 and (d2 == 0).sum() >= 2 * dup
    assert (idx[:, 1:][ties] > idx[:, :-1][ties]).all()                           # ties go to the smaller index
    for name, step in (("offset_neg3e4", 512), ("straddle", None)):
        Y = G.CASES[name]()[0]
        assert len(np.unique(Y, axis=0)) == len(Y)
        if step:
            assert np.array_equal(Y * step, np.round(Y * step)) and Y.max() < -2.9e4
        else:
            assert (Y.min(0) < 0).all() and (Y.max(0) > 0).all()


def test_dup20_lists_start_with_the_duplicates():
    X = G.CASES["dup20"]()[0]
    assert len(X) == 4000 and len(np.unique(X, axis=0)) == 200
    idx, d2, cnt = G.reference_lists("dup20", 32, False, True)
    assert (d2[:, :19] == 0).all() and (d2[:, 19] > 0).all() and (np.diff(idx[:, :19], axis=1) > 0).all()
    assert (G.reference_lists("dup20", 32, True, True)[2] < 32).any()


def test_degenerate_shapes_are_what_they_claim():
    X = G.CASES["identical"]()[0]
    assert len(X) == 257 and len(np.unique(X, axis=0)) == 1
    idx, d2, cnt = G.reference_lists("identical", 32, False, True)
    assert (d2 == 0).all() and (cnt == 32).all() and np.array_equal(idx[5], [0, 1, 2, 3, 4] + list(range(6, 33)))
    for a, name in enumerate(("line_x", "line_y", "line_z")):
        Y = G.CASES[name]()[0]
        e = Y.max(0) - Y.min(0)
        assert len(Y) == 257 and e[a] > 0.9 and (np.delete(e, a) == 0).all() and (np.delete(Y[0], a) != 0).all()
    for name, a in G.PLANES.items():
        Y = G.CASES[name]()[0]
        e = Y.max(0) - Y.min(0)
        assert len(Y) == 600 and e[a] == 0 and (np.delete(e, a) > 0.9).all() and Y[0, a] != 0
    D = G.CASES["diagonal"]()[0]
    assert len(D) == 257 and (D[:, 0] == D[:, 1]).all() and (D[:, 1] == D[:, 2]).all()
    e = np.ptp(G.CASES["slab"]()[0].astype(np.float64), axis=0)
    assert 0.9 < e[0] <= 1 and 0.9e-6 < e[1] <= 1e-6 and 0.9e-12 < e[2] <= 1e-12
    F = G.CASES["far_outlier"]()[0]
    assert len(F) == 501 and (np.abs(F).max(1) > 1).sum() == 1
    assert [len(G.CASES["plan_k_edge_%d" % n]()[0]) for n in (15, 16, 17)] == [15, 16, 17]
    for name in ("line_x", "plane_z", "diagonal", "slab", "far_outlier", "straddle"):      # the radius leaves lists short
        cnt = G.reference_lists(name, 32, True, True)[2]
        assert (cnt < 32).any() and cnt.max() >= 3, name


def test_overflowing_scales_hold_real_indices_at_plus_infinity_in_index_order():
    """At 3e19 most pairs overflow, but the 32 nearest of 400 points do not; at 3e38 every distance but 0 does, and the lists
    are the point itself and then the smallest indices, all real, at +inf."""
    for name in G.OVERFLOW:
        X = G.CASES[name]()[0]
        with np.errstate(over="ignore"):
            share = np.isposinf(CH.d2_matrix(X)).mean()
        idx, d2, cnt = G.reference_lists(name, 32, False, False)
        inf = np.isposinf(d2)
        print("%s: %.0f %% of the pairs and %.0f %% of the entries of the 32-lists are +inf" % (name, 100 * share, 100 * inf.mean()))
        assert share > 0.5 and (cnt == 32).all() and (idx >= 0).all(), name
        both = inf[:, 1:] & inf[:, :-1]
        assert (idx[:, 1:][both] > idx[:, :-1][both]).all() and not (inf[:, :-1] & ~inf[:, 1:]).any()
        if name == "scale_3e38":
            assert np.array_equal(idx[:, 0], np.arange(len(X))) and (d2[:, 0] == 0).all() and inf[:, 1:].all()
            assert np.array_equal(idx[40, 1:], np.arange(31)) and np.array_equal(idx[3, 1:], [0, 1, 2] + list(range(4, 32)))
            assert np.array_equal(G.reference33(name, True), G.reference33(name, False))      # fl(r * r) is +inf: unbounded
        else:
            assert not inf.any() and (G.reference_lists(name, 32, True, False)[2] < 32).any()
    for name in ("scale_1e-9", "scale_1e15", "scale_1e18", "scale_limit"):
        assert np.isfinite(G.reference_lists(name, 32, False, True)[1]).all()


def test_small_scales_sit_on_both_sides_of_the_limit():
    """scale_below exists because its neighbour distances are subnormal in float; scale_limit's are normal by far."""
    d2 = G.reference_lists("scale_below", 8, False, True)[1]
    assert (d2[:, 7] < G.FLT_MIN).all() and (d2[:, 7] >= 0).all()
    d2 = G.reference_lists("scale_limit", 8, False, True)[1]
    assert (d2[:, 0] >= 2.0 ** 20 * G.FLT_MIN).all()
    d2 = G.reference_lists("scale_1e-15", 8, False, True)[1]
    assert (d2[:, 0] >= G.FLT_MIN).all()                  # normal distances, yet a cell edge below the limit: refused as well
    # the cell of these cubes is at most L / 32 with L the diagonal of the bounds (plan_spacing's cap)
    for name in G.REFUSED:
        X = G.CASES[name]()[0].astype(np.float64)
        assert np.linalg.norm(X.max(0) - X.min(0)) / 32 < G.MIN_CELL
    X = G.CASES["scale_limit"]()[0].astype(np.float64)
    assert G.MIN_CELL <= np.linalg.norm(X.max(0) - X.min(0)) / 32 < 2 * G.MIN_CELL


def _text(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return re.sub(r"\s*\n\s*\*?\s*", " ", f.read())


def test_refusal_texts_and_documented_limits():
    """The messages the GPU refusal tests look for are the library's, and the headers state both limits."""
    src = _text("super4pcs_amd", "normals_src", "s4p_normals.hip")
    assert "spacing is too small for float distances" in src and "rescale the cloud" in src and G.MIN_CELL == 2.0 ** -43
    assert "finite and normal square in float" in _text("super4pcs_amd", "normals_src", "s4p_cluster.inc")
    for header, words in (("s4p_normals.h", ("Limits", "below 2^-43", "rescale")), ("s4p_knn.h", ("Limits", "below 2^-43")),
                          ("s4p_cluster.h", ("Limits", "FLT_MIN = 2^-126", "set_cloud"))):
        text = _text("include", header)
        assert all(w in text for w in words), header
