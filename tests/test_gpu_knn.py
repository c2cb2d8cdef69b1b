"""Neighbour lists on the MI355X (include/s4p_knn.h): idx, the bits of d2, the padding and cnt equal the numpy brute force on
tiny clouds (n from 1 to 257, with duplicates, k up to 32 > n - 1, with and without a radius and the own index) and the CPU
restatement on sampled queries of real clouds and of one multi-trip size; search_at with queries on and off the surface,
outside the grid and non-finite; determinism, numpy against torch; bad arguments."""
import numpy as np
import pytest

from tests import knn_helpers as KH
from tests import normals_helpers as NH
from tests import normals_suite as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def knn():
    return S.normals_module("knn")


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return NH.build_cpu(tmp_path_factory.mktemp("knn_cpu"))


def _same(got, want, rows=None, what=None):
    gi, gd, gc = (np.asarray(a) if rows is None else np.asarray(a)[rows] for a in got)
    wi, wd, wc = want
    assert gi.dtype == np.int32 and gd.dtype == np.float32 and gc.dtype == np.int32
    bad = np.flatnonzero((gi != wi).any(1) | (KH.bits(gd) != KH.bits(wd)).any(1) | (gc != wc))
    assert len(bad) == 0, (what, bad[:5], gi[bad[:2]], wi[bad[:2]], gd[bad[:2]], wd[bad[:2]], gc[bad[:2]], wc[bad[:2]])


@pytest.mark.parametrize("n", KH.TINY_N)
@pytest.mark.parametrize("dup", [False, True])
def test_tiny_shapes_equal_numpy(knn, n, dup):
    X = KH.tiny_cloud(n, dup)
    ctx = knn.Knn(0)
    ctx.set_cloud(X)
    short = 0
    for k in (1, 2, 8, 31, 32):
        for r in (None, KH.tiny_radius(n)):
            for ex in (False, True):
                want = KH.numpy_lists(X, k, r, exclude_self=ex)
                got = ctx.search(k, r, exclude_self=ex)
                assert got[0].shape == (n, k) and got[1].shape == (n, k) and got[2].shape == (n,)
                _same(got, want, what=(n, dup, k, r, ex))
                # the padding, stated on the device's own output: -1 and +inf from cnt on
                pad = np.arange(k)[None, :] >= got[2][:, None]
                assert (got[0][pad] == -1).all() and np.isposinf(got[1][pad]).all() and (got[0][~pad] >= 0).all()
                short += int(r is not None and k == 8 and (want[2] < min(k, n - ex)).any())
    assert short == 2 or n < 8                           # the radius leaves lists short
    ctx.close()


def _real_clouds():
    from super4pcs_amd import datasets as D
    rng = np.random.default_rng(3)
    dup = D.bumpy_pair(6000, overlap=0.5, delta=0.004, seed=12)[0]
    dup = np.concatenate([dup, dup[rng.integers(0, len(dup), 2000)], dup[:500]]).astype(np.float32)
    return {"dup": dup, "lidar": D.lidar_pair_scaled(0.004, delta=0.05)[0]}


@pytest.fixture(scope="module")
def real(knn):
    out = {}
    for name, X in _real_clouds().items():
        ctx = knn.Knn(0)
        ctx.set_cloud(X)
        out[name] = (X, ctx)
    yield out
    for _, ctx in out.values():
        ctx.close()


@pytest.mark.parametrize("name", ["dup", "lidar"])
def test_real_shapes_equal_the_restatement_bit_for_bit(knn, cpu, real, name):
    X, ctx = real[name]
    assert len(X) == (8500 if name == "dup" else 20000)
    rng = np.random.default_rng(7)
    sample = np.sort(rng.choice(len(X), size=3000, replace=False))
    radius = np.float32(0.6 * ctx.grid()["spacing"])
    for k in (1, 16, 32):
        for r in (None, radius):
            # one brute-force pass gives both forms: the k + 1 list holds the k list and the list without the own index
            idx1, _ = cpu.knn(X, k + 1, r, queries=X[sample], threads=16)
            for ex in (False, True):
                fn = lambda X_, k_, r_, queries: (idx1[:, :k_].copy(), (idx1[:, :k_] >= 0).sum(1).astype(np.int32))      # noqa: E731
                want = KH.lists(fn, X, k, r, X[sample], ex, own=sample)
                _same(ctx.search(k, r, exclude_self=ex), want, rows=sample, what=(name, k, r, ex))
                if not ex:
                    ic, cc = cpu.knn(X, k, r, queries=X[sample], threads=16)
                    assert np.array_equal(want[0], ic) and np.array_equal(want[2], cc)
    _, cnt = cpu.knn(X, 32, radius, queries=X[sample[:500]], threads=16)
    assert cnt.min() < 32                                # the radius really bounds


def test_search_at_equals_numpy_and_the_self_form(knn, real):
    X, ctx = real["dup"]
    rng = np.random.default_rng(8)
    lo, hi = X.min(0), X.max(0)
    Q = np.concatenate([X[rng.integers(0, len(X), 150)] + rng.normal(scale=0.003, size=(150, 3)),      # on the surface
                        rng.uniform(lo, hi, size=(60, 3)),                                               # off it
                        rng.uniform(lo - 2 * (hi - lo), hi + 2 * (hi - lo), size=(60, 3)),               # outside the grid's box
                        np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan]])]).astype(np.float32)
    for k in (1, 8, 32):
        for r in (None, np.float32(0.02)):
            want = KH.numpy_lists(X, k, r, queries=Q)
            got = ctx.search_at(Q, k, r)
            _same(got, want, what=(k, r))
            assert (got[2][-4:] == 0).all() and (got[0][-4:] == -1).all() and np.isposinf(got[1][-4:]).all()
    pick = rng.integers(0, len(X), 1000)
    for k, r in ((16, None), (32, np.float32(0.01))):
        a = ctx.search_at(X[pick], k, r)
        b = ctx.search(k, r, exclude_self=False)
        _same(a, tuple(v[pick] for v in b), what=("self", k, r))
    i, d, c = ctx.search_at(np.zeros((0, 3), np.float32), 4)
    assert i.shape == (0, 4) and d.shape == (0, 4) and c.shape == (0,)


def test_one_multi_trip_size_equals_the_restatement(knn, cpu):
    """524 289 points: above 2048 x 256, a lane of the grid-stride kernel takes a second and a third trip.  The sample holds
    the last 256 indices (the ragged last trip)."""
    from super4pcs_amd import datasets as D
    n = 524_289
    X = D.bumpy_pair(n, overlap=0.5, delta=0.004, seed=11)[0]
    assert len(X) == n > 2048 * 256
    ctx = knn.Knn(0)
    ctx.set_cloud(X)
    rng = np.random.default_rng(7)
    sample = np.unique(np.concatenate([rng.choice(n - 256, size=3000 - 256, replace=False), np.arange(n - 256, n)]))
    assert len(sample) == 3000
    k = 32
    idx1, _ = cpu.knn(X, k + 1, None, queries=X[sample], threads=16)
    fn = lambda X_, k_, r_, queries: (idx1[:, :k_].copy(), (idx1[:, :k_] >= 0).sum(1).astype(np.int32))      # noqa: E731
    for ex in (False, True):
        want = KH.lists(fn, X, k, None, X[sample], ex, own=sample)
        _same(ctx.search(k, None, exclude_self=ex), want, rows=sample, what=(n, ex))
    ctx.close()


def test_two_calls_and_numpy_torch_agree(knn, real):
    import torch
    X, ctx = real["lidar"]
    a = ctx.search(16, None, exclude_self=True)
    b = ctx.search(16, None, exclude_self=True)
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.uint32) if u.dtype == np.float32 else u, v.view(np.uint32) if v.dtype == np.float32 else v)
    Xt = S.to_device(X)
    t = knn.knn(Xt, 16, exclude_self=True)
    assert all(v.is_cuda for v in t) and t[0].dtype == torch.int32 and t[1].dtype == torch.float32 and t[2].dtype == torch.int32
    assert tuple(t[0].shape) == (len(X), 16)
    _same(tuple(S.to_host(v) for v in t), a, what="torch self")
    _same(knn.knn(X, 16, exclude_self=True), a, what="one-shot")
    Q = X[:777] + np.float32(0.01)
    qn = knn.knn(X, 8, radius=0.5, queries=Q)
    qt = knn.knn(Xt, 8, radius=0.5, queries=S.to_device(Q))
    assert all(v.is_cuda for v in qt)
    _same(tuple(S.to_host(v) for v in qt), qn, what="torch queries")


def test_bad_arguments(knn):
    import ctypes as C
    X = np.random.default_rng(1).uniform(size=(100, 3)).astype(np.float32)
    ctx = knn.Knn(0)
    for call in (lambda: ctx.search(4), lambda: ctx.search_at(X[:5], 4), lambda: ctx.statistical_outliers(4), lambda: ctx.radius_outliers(0.1, 2)):
        with pytest.raises(knn.NormalsError) as e:                      # before set_cloud
            call()
        assert e.value.code == -7 and "set_cloud first" in str(e.value)
    ctx.set_cloud(X)
    bad = [lambda: ctx.search(0), lambda: ctx.search(33), lambda: ctx.search(4, radius=float("nan")),
           lambda: ctx.search_at(X[:5], 0), lambda: ctx.search_at(X[:5], 33), lambda: ctx.search_at(X[:5], 4, radius=float("nan")),
           lambda: ctx.statistical_outliers(0), lambda: ctx.statistical_outliers(33), lambda: ctx.statistical_outliers(8, -0.5),
           lambda: ctx.statistical_outliers(8, float("nan")), lambda: ctx.statistical_outliers(8, float("inf")),
           lambda: ctx.radius_outliers(float("nan"), 4), lambda: ctx.radius_outliers(0.0, 4), lambda: ctx.radius_outliers(-1.0, 4),
           lambda: ctx.radius_outliers(float("inf"), 4), lambda: ctx.radius_outliers(0.1, 0), lambda: ctx.radius_outliers(0.1, 33)]
    for i, call in enumerate(bad):
        with pytest.raises(knn.NormalsError) as e:
            call()
        assert e.value.code == -1 and len(str(e.value)) > 30, i
    # null outputs with m > 0, straight through the C ABI
    L, h = ctx.L, ctx.h
    idx = np.empty((100, 4), np.int32); d2 = np.empty((100, 4), np.float32); keep = np.empty(100, np.uint8)
    cols = [np.ascontiguousarray(X[:5, a]) for a in range(3)]
    q = [c.ctypes.data for c in cols]
    for rc in (L.s4p_knn_search(h, 4, -1.0, 0, None, d2.ctypes.data, None), L.s4p_knn_search(h, 4, -1.0, 0, idx.ctypes.data, None, None),
               L.s4p_knn_search_at(h, q[0], q[1], q[2], 5, 4, -1.0, None, d2.ctypes.data, None),
               L.s4p_knn_search_at(h, None, q[1], q[2], 5, 4, -1.0, idx.ctypes.data, d2.ctypes.data, None),
               L.s4p_knn_search_at(h, q[0], q[1], q[2], -1, 4, -1.0, idx.ctypes.data, d2.ctypes.data, None),
               L.s4p_knn_search(h, 4, -1.0, 2, idx.ctypes.data, d2.ctypes.data, None),
               L.s4p_outliers_statistical(h, 4, 2.0, None, None, None), L.s4p_outliers_radius(h, 0.1, 2, None)):
        assert rc == -1 and len(L.s4p_normals_last_error(h)) > 10
    # m == 0 needs no pointers; cnt, mean_dist and stats may be null
    assert L.s4p_knn_search_at(h, None, None, None, 0, 4, -1.0, None, None, None) == 0
    assert L.s4p_knn_search(h, 4, -1.0, 0, idx.ctypes.data, d2.ctypes.data, None) == 0
    assert L.s4p_outliers_statistical(h, 4, 2.0, None, keep.ctypes.data, None) == 0
    st = knn.OutlierStats()
    assert L.s4p_outliers_statistical(h, 4, 2.0, None, keep.ctypes.data, C.byref(st)) == 0 and st.n == 100 and st.kept == int(keep.sum())
    ctx.close()
