"""Density clustering (include/s4p_cluster.h, libsuper4pcs_normals.so) on the host: the header's declarations against the
binding and the exports, the new kernels in the library's namespace, the loud failure without a device, the restatement
(tests/cluster_cpu) against a full-matrix numpy brute force on the tiny shapes of the GPU tests and against
sklearn.cluster.DBSCAN on the real clouds, the reference figures of the planted and the lidar clouds, the border rule's two
outcomes, the command line's new flags and the facade header with and without Eigen."""
import ctypes

import numpy as np
import pytest

from tests import cluster_helpers as CH
from tests import knn_helpers as KH
from tests import normals_suite as S


@pytest.fixture(scope="module")
def clu():
    return S.normals_module("cluster")


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return CH.build_cpu(tmp_path_factory.mktemp("cluster_cpu"))


def test_header_declarations_equal_the_binding_and_the_exports(clu):
    from super4pcs_amd import normals
    txt, decl, _ = S.check_header("s4p_cluster.h", "s4p_cluster_", clu.SYMBOLS, clu.load_library(),
                                  closed_prefixes="s4p_(?:normals|knn|outliers|voxel|orient)_")
    assert len(decl) == 4
    assert ctypes.sizeof(clu.ClusterStats) == 32
    assert (clu.NOISE, clu.BORDER, clu.CORE) == (0, 1, 2) and "S4P_CLUSTER_ERR_INTERNAL (-8)" in txt and normals.ERR_NAMES[-8] == "INTERNAL"


def test_new_kernels_live_in_the_library_namespace(clu):
    S.check_kernels_in_namespace(("k_cluster_walk<0>", "k_cluster_walk<1>", "k_cluster_link", "k_cluster_flatten", "k_cluster_label"),
                                 stray=r"(?<!s4p_nrm::)(?<!__device_stub__)\bk_cluster_\w+")


@pytest.mark.skipif(S.gpu_visible(), reason="checks the failure without a device")
def test_calls_fail_loudly_without_a_device(clu):
    X = np.zeros((10, 3), np.float32)
    S.check_no_device(clu.NormalsError, (lambda: clu.cluster_dbscan(X, 0.1), lambda: clu.keep_clusters(X, 0.1), lambda: clu.Cluster(0)))


def test_largest_labels_break_size_ties_by_the_smaller_label(clu):
    lab = np.array([2, 2, 0, 0, -1, 1, 1, 1, 3, -1], np.int32)
    assert clu.largest_labels(lab) == [1] and clu.largest_labels(lab, keep=2) == [1, 0] and clu.largest_labels(lab, keep=9) == [1, 0, 2, 3]
    assert clu.largest_labels(lab, keep=9, min_size=2) == [1, 0, 2] and clu.largest_labels(lab, keep=2, min_size=4) == []
    assert clu.largest_labels(np.full(5, -1, np.int32)) == []
    with pytest.raises(ValueError):
        clu.largest_labels(lab, keep=0)


@pytest.mark.parametrize("n", CH.TINY_N)
@pytest.mark.parametrize("dup", [False, True])
def test_restatement_equals_the_numpy_brute_force_on_the_tiny_shapes(cpu, n, dup):
    X = KH.tiny_cloud(n, dup)
    eps = CH.tiny_eps(n)
    seen = set()
    for mp in CH.TINY_MIN_POINTS:
        label, kind, stats, count = CH.numpy_dbscan(X, eps, mp)
        l2, k2, s2 = cpu.dbscan(X, eps, mp)
        assert np.array_equal(label, l2) and np.array_equal(kind, k2) and stats == s2, (n, dup, mp)
        assert np.array_equal(count, cpu.density(X, eps))
        seen |= set(kind.tolist())
        if mp == 1:
            assert stats["noise"] == 0 and stats["border"] == 0
    if n == 1:
        assert CH.numpy_dbscan(X, eps, 2)[2] == {"core": 0, "border": 0, "noise": 1, "clusters": 0}
    if n >= 33 or (n >= 8 and not dup):                      # the three kinds together (n = 8, 9 with duplicates: no border)
        assert seen == {CH.NOISE, CH.BORDER, CH.CORE}, (n, dup, seen)


def test_border_point_takes_the_smallest_index_among_its_nearest_cores(cpu):
    """The point at x = 1 is border (count 9) at d2 = 1 from eight cores, four of each cluster: the smallest index decides,
    and both outcomes occur over the six permutations."""
    sides = {}
    for s in range(6):
        X, i = CH.border_tie(s)
        label, kind, stats, count = CH.numpy_dbscan(X, 1.0, 10)
        l2, k2, s2 = cpu.dbscan(X, 1.0, 10)
        assert np.array_equal(label, l2) and np.array_equal(kind, k2) and stats == s2
        assert CH.sizes(label) == [13, 12] and kind[i] == CH.BORDER and count[i] == 9 and stats == {"core": 24, "border": 1, "noise": 0, "clusters": 2}
        near = np.flatnonzero((CH.d2_matrix(X)[i] == 1) & (kind == CH.CORE))
        assert len(near) == 8 and label[i] == label[near.min()] and len(set(label[near].tolist())) == 2
        sides[s] = float(X[label == label[i], 0].min())
    assert [s for s in range(6) if sides[s] == -1.0] == list(CH.BORDER_TIE_LEFT) and [s for s in range(6) if sides[s] == 1.0] == [1, 2, 3]


def test_chain_and_lattice_of_ties(cpu):
    X = CH.chain()
    label, kind, stats = cpu.dbscan(X, 1.0, 3)
    assert stats == {"core": 4094, "border": 2, "noise": 0, "clusters": 1} and (label == 0).all()
    assert sorted(X[kind == CH.BORDER, 0].tolist()) == [0.0, 4095.0]
    label, kind, stats = cpu.dbscan(X, np.nextafter(np.float32(1), np.float32(0)), 1)
    assert stats == {"core": 4096, "border": 0, "noise": 0, "clusters": 4096} and np.array_equal(label, np.arange(4096))
    assert cpu.dbscan(X, 1.0, 4)[2] == {"core": 0, "border": 0, "noise": 4096, "clusters": 0}
    P = CH.lattice_of_ties()
    assert len(P) == 400
    kinds = set()
    for mp in (1, 4, 10, 30):
        label, kind, stats, count = CH.numpy_dbscan(P, 0.25, mp)
        l2, k2, s2 = cpu.dbscan(P, 0.25, mp)
        assert np.array_equal(label, l2) and np.array_equal(kind, k2) and stats == s2, mp
        kinds |= set(kind.tolist())
    assert kinds == {0, 1, 2}
    assert (CH.d2_matrix(P) == np.float32(0.0625)).sum() > 400          # d2 == r2 exactly, many times


def test_reference_figures_of_the_fragment_and_the_lidar_clouds(cpu, clu):
    X, planted = CH.fragment_cloud()
    F = CH.FRAGMENT
    assert len(X) == F["n"] and planted.sum() == 60
    label, kind, stats = cpu.dbscan(X, F["eps"], F["min_points"])
    assert stats == F["stats"] and CH.sizes(label) == F["sizes"]
    keep = np.isin(label, clu.largest_labels(label, 1))
    assert int((~keep).sum()) == F["removed"] and keep[planted].sum() == 1          # 6001: the surface and one planted point on it
    blob = np.linalg.norm(X - np.array([1.2, 0, 0], np.float32), axis=1) < 0.15
    assert (blob & ~planted).sum() == 150 and not keep[blob].any()         # the fragment goes with the planted points
    L = CH.lidar_cloud()
    assert len(L) == 20000
    for (eps, mp), want in CH.LIDAR.items():
        label, kind, stats = cpu.dbscan(L, eps, mp)
        assert stats == want["stats"], (eps, mp, stats)
        assert want["largest"] is None or CH.sizes(label)[0] == want["largest"]


@pytest.mark.parametrize("name,eps,mp", [("fragment", 0.03, 4), ("lidar", 0.5, 10), ("lidar", 0.3, 5)])
def test_restatement_equals_sklearn_where_no_pair_lies_at_the_boundary(cpu, name, eps, mp):
    """Core set, core labels and noise set equal sklearn.cluster.DBSCAN's: its numbering is also by the smallest core index.
    Border labels may differ (sklearn's depend on its visiting order).  No pair lies within 1e-6 (relative) of eps."""
    sk = pytest.importorskip("sklearn.cluster")
    X = CH.fragment_cloud()[0] if name == "fragment" else CH.lidar_cloud()
    gap = CH.boundary_gap(X, eps)
    print("%s eps %g: smallest relative gap to eps %.2e" % (name, eps, gap))
    assert gap > 1e-6
    label, kind, stats = cpu.dbscan(X, eps, mp)
    m = sk.DBSCAN(eps=float(np.float32(eps)), min_samples=mp).fit(X.astype(np.float64))
    core = np.zeros(len(X), bool)
    core[m.core_sample_indices_] = True
    assert np.array_equal(core, kind == CH.CORE)
    assert np.array_equal(m.labels_[core], label[core])
    assert np.array_equal(m.labels_ == -1, kind == CH.NOISE)


def test_cli_cluster_flags(tmp_path):
    S.check_cli_flags(
        tmp_path,
        bad=(["--cluster-min-points", "4"], ["--cluster-keep", "2"],                                  # both need --cluster-eps
             ["--cluster-eps", "0"], ["--cluster-eps", "-0.1"], ["--cluster-eps", "nan"], ["--cluster-eps", "inf"],
             ["--cluster-eps", "1e20"], ["--cluster-eps", "1e-50"], ["--cluster-eps", "0.1x"], ["--cluster-eps", ""], ["--cluster-eps"],
             ["--cluster-eps", "0.1", "--cluster-min-points", "0"], ["--cluster-eps", "0.1", "--cluster-min-points", "-3"],
             ["--cluster-eps", "0.1", "--cluster-min-points", "4.5"], ["--cluster-eps", "0.1", "--cluster-min-points", "x"],
             ["--cluster-eps", "0.1", "--cluster-min-points", ""], ["--cluster-eps", "0.1", "--cluster-min-points"],
             ["--cluster-eps", "0.1", "--cluster-min-points", "3000000000"],
             ["--cluster-eps", "0.1", "--cluster-keep", "0"], ["--cluster-eps", "0.1", "--cluster-keep", "1.5"],
             ["--cluster-eps", "0.1", "--cluster-keep", ""], ["--cluster-eps", "0.1", "--cluster-keep"]),
        good=(["--cluster-eps", "0.03"], ["--cluster-min-points", "4", "--cluster-eps", "3e-2"],
              ["--cluster-eps", "0.5", "--cluster-min-points", "1", "--cluster-keep", "3"],
              ["--remove-outliers", "16", "--voxel-size", "0.01", "--cluster-eps", "0.03", "--estimate-normals", "16", "--icp", "10"]),
        usage_word="--cluster-eps e", usage_order=("--orient-normals k", "--cluster-eps e"))


def test_cli_refuses_an_input_with_faces(tmp_path):
    S.check_cli_refuses_faces(tmp_path, ["--cluster-eps", "0.1"])


@pytest.mark.skipif(S.gpu_visible(), reason="checks the failure without a device")
def test_cli_valid_command_fails_with_the_device_error_without_a_gpu(tmp_path):
    S.check_cli_no_device(tmp_path, ["--cluster-eps", "0.2", "--cluster-min-points", "4"], "ClusterDBSCAN (MI355X)")


@pytest.mark.parametrize("eigen", [False, True])
def test_facade_header_compiles_with_and_without_eigen(clu, tmp_path, eigen):
    S.check_facade_header(tmp_path, "cluster.h", eigen, "cluster", np.random.default_rng(2).uniform(size=(20, 3)),
                          no_device_args=["0.2", "4", "1", "1"], no_device_text=("ClusterDBSCAN (MI355X)", "no HIP device"),
                          bad_args=(["0", "4", "1", "1"], ["-1", "4", "1", "1"], ["nan", "4", "1", "1"], ["inf", "4", "1", "1"], ["1e20", "4", "1", "1"],
                                    ["0.2", "0", "1", "1"], ["0.2", "4", "0", "1"], ["0.2", "4", "1", "0"]),
                          bad_text="ClusterDBSCAN:")
