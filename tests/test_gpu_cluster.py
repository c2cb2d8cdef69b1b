"""Density clustering on the MI355X (include/s4p_cluster.h): label, kind, stats and density equal the restatement
(tests/cluster_cpu through tests/cluster_helpers.py) exactly on tiny clouds (n from 1 to 257, with duplicates, three
min_points), on the border tie, on a chain of diameter 4095, on a lattice where d2 == r2 many times, on the cloud with a dense
fragment (through Python, the facade and the command line), on the lidar cloud and on one multi-trip size whose pairs sit at
the float boundary of eps; determinism, numpy against torch, density against the core flag and against the neighbour lists,
every refusal, and the context's other calls after a cluster call."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import apps
from tests import cluster_helpers as CH
from tests import knn_helpers as KH
from tests import normals_helpers as NH
from tests import normals_suite as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def clu():
    return S.normals_module("cluster")


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return CH.build_cpu(tmp_path_factory.mktemp("cluster_cpu"))


def _same(ctx, cpu, X, eps, min_points, what):
    """One dbscan call and one density call equal the restatement.  Returns (label, kind, stats)."""
    label, kind, stats = ctx.dbscan(eps, min_points)
    want_l, want_k, want_s = cpu.dbscan(X, eps, min_points)
    assert label.dtype == np.int32 and kind.dtype == np.uint8
    print(what, stats)
    bad = np.flatnonzero(kind != want_k)
    assert len(bad) == 0, (what, "kind", len(bad), bad[:8], kind[bad[:8]], want_k[bad[:8]])
    bad = np.flatnonzero(label != want_l)
    assert len(bad) == 0, (what, "label", len(bad), bad[:8], label[bad[:8]], want_l[bad[:8]])
    assert stats == want_s, (what, stats, want_s)
    count = ctx.density(eps)
    assert count.dtype == np.int32 and np.array_equal(count, cpu.density(X, eps)), what
    assert np.array_equal(count >= min_points, kind == CH.CORE), what
    return label, kind, stats


@pytest.mark.parametrize("n", CH.TINY_N)
@pytest.mark.parametrize("dup", [False, True])
def test_tiny_clouds_equal_the_restatement(clu, cpu, n, dup):
    X = KH.tiny_cloud(n, dup)
    ctx = clu.Cluster(0)
    ctx.set_cloud(X)
    for mp in CH.TINY_MIN_POINTS:
        label, kind, stats = _same(ctx, cpu, X, CH.tiny_eps(n), mp, (n, dup, mp))
        if mp == 1:
            assert stats["noise"] == 0 and stats["border"] == 0 and (label >= 0).all()
    if n == 1:
        assert ctx.dbscan(CH.tiny_eps(n), 2)[2] == {"core": 0, "border": 0, "noise": 1, "clusters": 0}
    ctx.close()


@pytest.mark.parametrize("seed", range(6))
def test_border_tie_goes_to_the_smallest_index(clu, cpu, seed):
    X, i = CH.border_tie(seed)
    ctx = clu.Cluster(0)
    ctx.set_cloud(X)
    label, kind, stats = _same(ctx, cpu, X, 1.0, 10, ("border tie", seed))
    assert CH.sizes(label) == [13, 12] and kind[i] == CH.BORDER
    assert float(X[label == label[i], 0].min()) == (-1.0 if seed in CH.BORDER_TIE_LEFT else 1.0)
    ctx.close()


def test_chain_of_diameter_4095(clu, cpu):
    X = CH.chain()
    ctx = clu.Cluster(0)
    ctx.set_cloud(X)
    label, kind, stats = _same(ctx, cpu, X, 1.0, 3, "chain 3")
    assert stats == {"core": 4094, "border": 2, "noise": 0, "clusters": 1} and (label == 0).all()
    label, kind, stats = _same(ctx, cpu, X, np.nextafter(np.float32(1), np.float32(0)), 1, "chain below 1")
    assert stats["clusters"] == 4096 and np.array_equal(label, np.arange(4096))
    label, kind, stats = _same(ctx, cpu, X, 1.0, 4, "chain 4")
    assert stats == {"core": 0, "border": 0, "noise": 4096, "clusters": 0} and (label == -1).all()
    ctx.close()


def test_lattice_of_ties(clu, cpu):
    X = CH.lattice_of_ties()
    ctx = clu.Cluster(0)
    ctx.set_cloud(X)
    kinds = set()
    for mp in (1, 4, 10, 30):
        kinds |= set(_same(ctx, cpu, X, 0.25, mp, ("lattice", mp))[1].tolist())
    assert kinds == {0, 1, 2}
    ctx.close()


def test_fragment_goes_through_python_the_facade_and_the_command_line(clu, cpu, s4p_lib_built, tmp_path):
    """The cloud the statistical filter cannot clean: the surface, a dense blob away from it and 60 planted points.  At
    (0.03, 4) there are two clusters; keeping the largest removes the blob and the planted points, 209 in all, through
    keep_clusters, KeepLargestClusters (normals and colours move with their points) and --cluster-eps."""
    X, planted = CH.fragment_cloud()
    F = CH.FRAGMENT
    ctx = clu.Cluster(0)
    ctx.set_cloud(X)
    label, kind, stats = _same(ctx, cpu, X, F["eps"], F["min_points"], "fragment")
    ctx.close()
    assert stats == F["stats"] and CH.sizes(label) == F["sizes"]
    kept, mask, lab = clu.keep_clusters(X, F["eps"], F["min_points"], keep=1)
    assert np.array_equal(lab, label) and int((~mask).sum()) == F["removed"] and np.array_equal(kept, X[label == 0])
    both = clu.keep_clusters(X, F["eps"], F["min_points"], keep=2)[1]
    assert np.array_equal(both, label >= 0)
    assert np.array_equal(clu.keep_clusters(X, F["eps"], F["min_points"], keep=2, min_size=150)[1], mask)
    # the facade
    heads, (got_label, got_mask), rest = S.run_points_app(S.build_facade_app(tmp_path), ["cluster", F["eps"], F["min_points"], "1", "1"], X)
    n = len(X)
    assert heads[0] == "clusters 2" and np.array_equal(got_label, label)
    assert heads[1:] == ["removed %d" % F["removed"]] and len(got_mask) == n and np.array_equal(got_mask != 0, mask)
    rest = rest.astype(np.float32)
    assert np.array_equal(NH.bits(rest[:, :3]), NH.bits(X[mask])) and (rest[:, 3] == 1).all()
    assert np.array_equal(rest[:, 4].astype(np.int64), np.flatnonzero(mask))
    # the command line: both inputs filtered, -r holds the kept points of the second
    apps.write_obj(tmp_path / "P.obj", X); apps.write_obj(tmp_path / "Q.obj", X)
    cli = S.cli()
    M, out = apps.run_cli(cli, tmp_path / "P.obj", tmp_path / "Q.obj", 0.01, 0.6, 200,
                          ["--cluster-eps", F["eps"], "--cluster-min-points", F["min_points"], "-r", tmp_path / "R.obj"])
    assert "removed %d of input1, %d of input2" % (F["removed"], F["removed"]) in out, out
    head, body = (tmp_path / "R.ply").read_bytes().split(b"end_header\n", 1)          # a point set is written as a binary PLY
    assert b"element vertex %d\n" % (n - F["removed"]) in head and len(body) == 12 * (n - F["removed"]) and np.isfinite(M).all()
    # a cloud left with no cluster is refused with the flag's name
    r = subprocess.run([cli, "-i", str(tmp_path / "P.obj"), str(tmp_path / "Q.obj"), "--cluster-eps", "1e-6", "--cluster-min-points", "4", "-m",
                        str(tmp_path / "none.txt")], capture_output=True, text=True, timeout=apps.TIMEOUT)
    assert r.returncode == 254 and "--cluster-eps: no cluster" in r.stdout + r.stderr and not (tmp_path / "none.txt").exists()


@pytest.mark.parametrize("eps,mp", sorted(CH.LIDAR))
def test_lidar_cloud_equals_the_restatement(clu, cpu, eps, mp):
    X = CH.lidar_cloud()
    ctx = clu.Cluster(0)
    ctx.set_cloud(X)
    label, kind, stats = _same(ctx, cpu, X, eps, mp, ("lidar", eps, mp))
    want = CH.LIDAR[eps, mp]
    assert stats == want["stats"] and (want["largest"] is None or CH.sizes(label)[0] == want["largest"])
    ctx.close()


def test_one_multi_trip_size_at_the_float_boundary(clu, cpu):
    """524 289 points: above 2048 x 256, a lane of every grid-stride kernel takes a second and a third trip.  Several pairs
    sit within 4e-8 (relative) of eps, so the bits of d2 decide.  Two calls, numpy and torch give the same bits."""
    import torch
    X = CH.large_cloud()
    G = CH.LARGE
    assert len(X) == 524_289 > 2048 * 256
    ctx = clu.Cluster(0)
    ctx.set_cloud(X)
    label, kind, stats = _same(ctx, cpu, X, G["eps"], G["min_points"], "large")
    assert stats == G["stats"] and CH.sizes(label) == G["sizes"]
    l2, k2, s2 = ctx.dbscan(G["eps"], G["min_points"])
    assert np.array_equal(label, l2) and np.array_equal(kind, k2) and s2 == stats
    ctx.close()
    t = clu.Cluster(0)
    t.set_cloud(S.to_device(X))
    lt, kt, st = t.dbscan(G["eps"], G["min_points"])
    ct = t.density(G["eps"])
    assert lt.is_cuda and kt.is_cuda and ct.is_cuda and lt.dtype == torch.int32 and kt.dtype == torch.uint8 and ct.dtype == torch.int32
    assert np.array_equal(S.to_host(lt), label) and np.array_equal(S.to_host(kt), kind) and st == stats
    assert np.array_equal(S.to_host(ct) >= G["min_points"], kind == CH.CORE)
    t.close()


def test_numpy_and_torch_give_the_same_bits_and_two_calls_too(clu):
    X = KH.tiny_cloud(257, True)
    eps = CH.tiny_eps(257)
    a = clu.cluster_dbscan(X, eps, 2)
    b = clu.cluster_dbscan(X, eps, 2)
    t = clu.cluster_dbscan(S.to_device(X), eps, 2)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert t[0].is_cuda and np.array_equal(S.to_host(t[0]), a[0]) and np.array_equal(S.to_host(t[1]), a[1]) and t[2] == a[2]
    kept, mask, lab = clu.keep_clusters(S.to_device(X), eps, 2, keep=3)
    kn, mn, ln = clu.keep_clusters(X, eps, 2, keep=3)
    assert kept.is_cuda and mask.is_cuda and np.array_equal(S.to_host(kept), kn) and np.array_equal(S.to_host(mask), mn)
    assert 0 < mn.sum() < len(X) and np.array_equal(np.isin(ln, clu.largest_labels(ln, 3)), mn)


def test_density_equals_the_short_neighbour_lists(clu):
    """Where a radius search with k = 32 comes out short, its count of other points plus the point itself is the density."""
    X = CH.lidar_cloud()
    ctx = clu.Cluster(0)
    ctx.set_cloud(X)
    for r in (0.3, 0.5):
        cnt = ctx.search(32, radius=r, exclude_self=True)[2]
        den = ctx.density(r)
        short = cnt < 32
        assert 0.2 < short.mean() and np.array_equal(den[short], cnt[short] + 1) and (den[~short] >= 33).all()
    ctx.close()


def test_other_calls_on_the_context_are_unchanged_after_a_cluster_call(clu):
    X = CH.fragment_cloud()[0]
    ctx = clu.Cluster(0)
    ctx.set_cloud(X)
    g0 = ctx.grid()
    n0 = ctx.estimate(16)
    i0, d0, c0 = ctx.search(8, exclude_self=True)
    keep0 = ctx.statistical_outliers(16, 2.0)[0]
    ctx.dbscan(0.03, 4)
    ctx.density(0.2)
    assert ctx.grid() == g0
    assert np.array_equal(NH.bits(ctx.estimate(16)), NH.bits(n0))
    i1, d1, c1 = ctx.search(8, exclude_self=True)
    assert np.array_equal(i1, i0) and np.array_equal(NH.bits(d1), NH.bits(d0)) and np.array_equal(c1, c0)
    assert np.array_equal(ctx.statistical_outliers(16, 2.0)[0], keep0)
    ctx.close()


def test_refusals(clu):
    X = np.random.default_rng(1).uniform(size=(100, 3)).astype(np.float32)
    ctx = clu.Cluster(0)
    L, h = clu.load_library(), ctx.h
    lab = np.full(100, 7, np.int32)
    cnt = np.full(100, 7, np.int32)
    for rc in (L.s4p_cluster_dbscan(h, 0.1, 4, lab.ctypes.data, None, None), L.s4p_cluster_dbscan_device(h, 0.1, 4, lab.ctypes.data, None, None),
               L.s4p_cluster_density(h, 0.1, cnt.ctypes.data), L.s4p_cluster_density_device(h, 0.1, cnt.ctypes.data)):
        assert rc == -7 and b"set_cloud first" in L.s4p_normals_last_error(h)                       # before set_cloud
    ctx.set_cloud(X)
    nan, inf = float("nan"), float("inf")
    bad = [lambda: ctx.dbscan(nan, 4), lambda: ctx.dbscan(inf, 4), lambda: ctx.dbscan(0.0, 4), lambda: ctx.dbscan(-0.1, 4),
           lambda: ctx.dbscan(1e20, 4), lambda: ctx.dbscan(0.1, 0), lambda: ctx.dbscan(0.1, -5),
           lambda: ctx.density(nan), lambda: ctx.density(inf), lambda: ctx.density(0.0), lambda: ctx.density(-1.0), lambda: ctx.density(1e20)]
    for i, call in enumerate(bad):
        with pytest.raises(clu.NormalsError) as e:
            call()
        assert e.value.code == -1 and len(str(e.value)) > 40, i
    for rc in (L.s4p_cluster_dbscan(h, 0.1, 4, None, None, None), L.s4p_cluster_dbscan_device(h, 0.1, 4, None, None, None),
               L.s4p_cluster_density(h, 0.1, None), L.s4p_cluster_density_device(h, 0.1, None)):
        assert rc == -1 and len(L.s4p_normals_last_error(h)) > 20
    assert L.s4p_cluster_dbscan(None, 0.1, 4, lab.ctypes.data, None, None) == -1 and L.s4p_cluster_density(None, 0.1, cnt.ctypes.data) == -1
    assert (lab == 7).all() and (cnt == 7).all()
    # the optional outputs may be null
    assert L.s4p_cluster_dbscan(h, 0.1, 4, lab.ctypes.data, None, None) == 0
    assert np.array_equal(lab, ctx.dbscan(0.1, 4)[0])
    ctx.close()
