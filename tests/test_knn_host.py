"""Neighbour lists and outlier removal (include/s4p_knn.h, libsuper4pcs_normals.so) on the host: the header's declarations
against the binding and the exports, s4p_normals.h and its symbol list untouched, the new kernels in the library's
namespace, the loud failure without a device, the restatement's lists against the numpy brute force on the tiny shapes of
the GPU tests, the reference statistics, the command line's new flags and the facade header with and without Eigen."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from tests import knn_helpers as KH
from tests import normals_helpers as NH
from tests import normals_suite as S


@pytest.fixture(scope="module")
def knn():
    return S.normals_module("knn")


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return NH.build_cpu(tmp_path_factory.mktemp("knn_cpu"))


def test_header_declarations_equal_the_binding_and_the_exports(knn):
    # the new functions carry their own prefixes
    _, decl, _ = S.check_header("s4p_knn.h", "s4p_(?:knn|outliers)_", knn.SYMBOLS, knn.load_library(), closed_prefixes="s4p_normals_")
    assert len(decl) == 8
    assert ctypes.sizeof(knn.OutlierStats) == 40


def test_the_normals_header_and_its_symbol_list_are_unchanged(knn):
    from super4pcs_amd import normals
    assert S.declared("s4p_normals.h", "s4p_normals_") == sorted(normals.SYMBOLS) and len(normals.SYMBOLS) == 10
    digest = hashlib.sha256(open(os.path.join(S.INCLUDE, "s4p_normals.h"), "rb").read()).hexdigest()
    # the header as of the scale limit in its Limits paragraph: a comment grew, no declaration changed
    assert digest == "f5f72bed94da6af3e2c3cfa3c129249e091cc62eff74a555a0d401bb0a9d2f22", digest
    assert not [s for s in knn.SYMBOLS if s.startswith("s4p_normals_")]


def test_new_kernels_live_in_the_library_namespace(knn):
    S.check_kernels_in_namespace(["k_knn_search<%d, %d>" % (k, mode) for k in (8, 16, 32) for mode in (0, 1, 2)] +
                                 ["k_knn_normals<%d>" % k for k in (8, 16, 32)] + ["k_sor_rows<0>", "k_sor_rows<1>", "k_sor_reduce", "k_sor_mask"])


@pytest.mark.skipif(S.gpu_visible(), reason="checks the failure without a device")
def test_create_fails_loudly_without_a_device(knn):
    X = np.zeros((10, 3), np.float32)
    S.check_no_device(knn.NormalsError, (lambda: knn.Knn(0), lambda: knn.knn(X, 4), lambda: knn.remove_statistical_outliers(X),
                                         lambda: knn.remove_radius_outliers(X, 0.1, 2)))


@pytest.mark.parametrize("n", KH.TINY_N)
@pytest.mark.parametrize("dup", [False, True])
def test_restatement_lists_equal_numpy_on_the_tiny_shapes(cpu, n, dup):
    X = KH.tiny_cloud(n, dup)
    for k in (1, 2, 8, 31, 32):
        for r in (None, KH.tiny_radius(n)):
            for ex in (False, True):
                ic, dc, cc = KH.cpu_lists(cpu, X, k, r, exclude_self=ex)
                inp, dn, cn = KH.numpy_lists(X, k, r, exclude_self=ex)
                assert np.array_equal(ic, inp) and np.array_equal(cc, cn) and np.array_equal(KH.bits(dc), KH.bits(dn)), (n, dup, k, r, ex)
                if r is None:
                    assert (cn == min(k, n - 1 if ex else n)).all()
                if not ex:
                    assert (dn[:, 0] == 0).all() and (inp[:, 0] <= np.arange(n)).all()      # itself, or a duplicate of smaller index
                else:
                    assert not (inp == np.arange(n)[:, None]).any()


def test_lists_without_self_keep_duplicates():
    X = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 0, 0]], np.float32)
    idx, d2, cnt = KH.numpy_lists(X, 2, exclude_self=True)
    assert idx.tolist() == [[2, 3], [0, 2], [0, 3], [0, 2]] and d2[0].tolist() == [0, 0] and cnt.tolist() == [2, 2, 2, 2]
    m = KH.mean_dist(d2, cnt)
    assert m.tolist() == [0.0, 1.0, 0.0, 0.0]
    mu, sigma, t = KH.sor_reference(m, 2.0)
    assert mu == 0.25 and sigma == 0.5 and t == 1.25
    assert KH.sor_reference(np.zeros(1), 2.0) == (0.0, 0.0, 0.0)


def test_planted_points_are_outliers_of_the_reference(cpu):
    """The reference statistics on the small bumpy cloud of the GPU test, k = 16: every original point is kept, at least 51
    of the 60 planted points are removed, and no m_j lies within 1e-9 (relative) of the threshold."""
    from super4pcs_amd import datasets as D
    X, planted = KH.plant(D.bumpy_pair(6000, overlap=0.5, delta=0.004, seed=12)[0], 60)
    assert len(X) == 6060 and planted.sum() == 60
    _, d2, cnt = KH.cpu_lists(cpu, X, 16, exclude_self=True)
    m = KH.mean_dist(d2, cnt)
    mu, sigma, t = KH.sor_reference(m, 2.0)
    keep = m <= t
    gap = np.min(np.abs(m - t)) / t
    print("bumpy + 60, k 16: mu %.6g sigma %.6g t %.6g, gap %.3g, planted removed %d" % (mu, sigma, t, gap, (~keep[planted]).sum()))
    assert gap > 1e-9 and keep[~planted].all() and (~keep[planted]).sum() >= 51


def test_cli_remove_outliers_flags(tmp_path):
    S.check_cli_flags(
        tmp_path,
        bad=(["--remove-outliers", "0"], ["--remove-outliers", "33"], ["--remove-outliers", "1.5"], ["--remove-outliers", "x"],
             ["--remove-outliers", ""], ["--remove-outliers-std", "2.0"], ["--remove-outliers", "16", "--remove-outliers-std", "-1"],
             ["--remove-outliers", "16", "--remove-outliers-std", "nan"], ["--remove-outliers", "16", "--remove-outliers-std", "2x"]),
        good=(["--remove-outliers", "1"], ["--remove-outliers", "32", "--remove-outliers-std", "0"],
              ["--remove-outliers-std", "1.5", "--remove-outliers", "16"],
              ["--remove-outliers", "16", "--estimate-normals", "16", "--icp", "5", "--icp-metric", "gicp"]),
        usage_word="--remove-outliers")


def test_cli_refuses_an_input_with_faces(tmp_path):
    S.check_cli_refuses_faces(tmp_path, ["--remove-outliers", "16"])


@pytest.mark.skipif(S.gpu_visible(), reason="checks the failure without a device")
def test_cli_valid_command_fails_with_the_device_error_without_a_gpu(tmp_path):
    S.check_cli_no_device(tmp_path, ["--remove-outliers", "16"], "RemoveOutliers (MI355X)")


@pytest.mark.parametrize("eigen", [False, True])
def test_facade_header_compiles_with_and_without_eigen(knn, tmp_path, eigen):
    S.check_facade_header(tmp_path, "outliers.h", eigen, "outliers", np.random.default_rng(2).uniform(size=(20, 3)),
                          no_device_args=["stat", "8", "2.0"], no_device_text=("no HIP device",),
                          bad_args=(["stat", "0", "2.0"], ["stat", "33", "2.0"], ["stat", "8", "-1"], ["radius", "-1", "4"], ["radius", "0.1", "33"]),
                          bad_text="RemoveOutliers:")
