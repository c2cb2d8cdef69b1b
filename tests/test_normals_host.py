"""Normal estimation (include/s4p_normals.h, libsuper4pcs_normals.so) on the host: exports and binding, the library's
namespace, the loud failure without a device, the CPU restatement's neighbour sets against a numpy lexsort brute force and
its normals against numpy eigh, the command line's new flags and the facade header."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import normals_helpers as NH
from tests import normals_suite as S


@pytest.fixture(scope="module")
def nrm():
    return S.normals_module("normals")


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return NH.build_cpu(tmp_path_factory.mktemp("normals_cpu"))


def test_header_declarations_equal_the_binding_and_the_exports(nrm):
    S.check_header("s4p_normals.h", "s4p_normals_", nrm.SYMBOLS, nrm.load_library(), restype=None)   # create returns the handle, last_error a string


def test_kernels_live_in_their_own_namespace(nrm):
    dyn = subprocess.run(["nm", "-D", "--defined-only", nrm.LIB_PATH], capture_output=True, text=True).stdout
    assert "_ZN3s4p" not in dyn
    out = S.check_kernels_in_namespace(("k_knn_normals<8>", "k_knn_normals<32>"))
    assert "s4p_icp::" not in out
    for k in ("k_normals", "k_match", "k_final", "k_match_plane", "k_final_plane", "k_stats"):
        assert not re.search(r"\b%s\b" % k, out), k
    # only the HIP runtime (and the C / C++ runtimes) are linked
    needed = subprocess.run(["readelf", "-d", nrm.LIB_PATH], capture_output=True, text=True).stdout
    assert "super4pcs" not in needed


@pytest.mark.skipif(S.gpu_visible(), reason="checks the failure without a device")
def test_create_fails_loudly_without_a_device(nrm):
    S.check_no_device(nrm.NormalsError, (lambda: nrm.Normals(0), lambda: nrm.estimate_normals(np.zeros((10, 3), np.float32))))


def _cloud_with_ties(rng, n):
    """A small lattice-like cloud: integer coordinates (many exactly equal distances), duplicated points."""
    P = rng.integers(0, 6, size=(n, 3)).astype(np.float32) * np.float32(0.25)
    P[n // 3:n // 3 + n // 10] = P[:n // 10]
    return P


@pytest.mark.parametrize("k,radius", [(3, None), (8, None), (16, 0.6), (32, None), (32, 0.3)])
def test_restatement_neighbour_sets_equal_numpy_lexsort(cpu, k, radius):
    rng = np.random.default_rng(k)
    P = _cloud_with_ties(rng, 400)
    idx, cnt = cpu.knn(P, k, radius)
    ib, cb = NH.numpy_knn(P, k, radius)
    assert np.array_equal(cnt, cb) and np.array_equal(idx, ib)
    # the first neighbour is at d2 = 0: the point itself or a duplicate of smaller index
    assert np.array_equal(P[idx[:, 0]], P) and np.all(idx[:, 0] <= np.arange(len(P)))
    # separate queries, some off the cloud
    Q = np.concatenate([P[:50] + np.float32(0.125), rng.uniform(-1, 2, size=(30, 3)).astype(np.float32)])
    idx, cnt = cpu.knn(P, k, radius, queries=Q)
    ib, cb = NH.numpy_knn(P, k, radius, queries=Q)
    assert np.array_equal(cnt, cb) and np.array_equal(idx, ib)


def test_restatement_normals_agree_with_numpy_eigh(cpu):
    rng = np.random.default_rng(5)
    n = 3000
    xy = rng.uniform(-1, 1, size=(n, 2))
    z = 0.1 * np.sin(2 * xy[:, 0]) + 0.05 * np.cos(3 * xy[:, 1]) + rng.normal(scale=0.003, size=n)
    P = np.column_stack([xy, z]).astype(np.float32)
    for k, radius in ((8, None), (16, None), (32, 0.2)):
        N = cpu.normals(P, k, radius)
        idx, cnt = cpu.knn(P, k, radius)
        P64 = P.astype(np.float64)
        checked = 0
        for i in range(0, n, 7):
            nb = idx[i, :cnt[i]]
            if len(nb) < 3:
                assert not N[i].any()
                continue
            e = P64[nb] - P64[i]
            m = e.mean(0)
            Cm = e.T @ e / len(e) - np.outer(m, m)
            w, V = np.linalg.eigh(Cm)
            if not w[1] >= 4 * max(w[0], 1e-30):
                continue                                      # well-conditioned neighbourhoods only
            v = V[:, 0]
            v = v * (1 if v[np.argmax(np.abs(v))] > 0 else -1)
            assert np.max(np.abs(N[i].astype(np.float64) - v)) <= 1e-6, (i, N[i], v)
            checked += 1
        assert checked > 200
        assert np.all(np.abs(np.linalg.norm(N[N.any(1)].astype(np.float64), axis=1) - 1) < 1e-6)


def test_restatement_zero_normals(cpu):
    P = np.array([[0, 0, 0], [1, 0, 0], [5, 5, 5], [5, 5, 5], [5, 5, 5]], np.float32)
    N = cpu.normals(P, 3, 1.5)
    assert not N.any()                               # fewer than 3 within r, or all coincident (trace 0)
    N = cpu.normals(P, 3)
    assert not N[2:].any()


def test_cli_estimate_normals_flags(tmp_path):
    S.check_cli_flags(
        tmp_path,
        bad=(["--estimate-normals", "2"], ["--estimate-normals", "33"], ["--estimate-normals", "16.5"], ["--estimate-normals", "x"],
             ["--estimate-normals", ""], ["--estimate-normals", "16", "--estimate-normals-radius", "0"],
             ["--estimate-normals", "16", "--estimate-normals-radius", "-1"],
             ["--estimate-normals", "16", "--estimate-normals-radius", "nan"],
             ["--estimate-normals", "16", "--estimate-normals-radius", "0.1x"], ["--estimate-normals-radius", "0.1"]),
        good=(["--estimate-normals", "3"], ["--estimate-normals", "32", "--estimate-normals-radius", "0.05"],
              ["--estimate-normals-radius", "0.05", "--estimate-normals", "16"]),
        usage_word="--estimate-normals")


@pytest.mark.skipif(S.gpu_visible(), reason="checks the failure without a device")
def test_cli_valid_command_fails_with_the_device_error_without_a_gpu(tmp_path):
    S.check_cli_no_device(tmp_path, ["--estimate-normals", "16", "-a", "20"], "EstimateNormals (MI355X)")


def test_facade_header_compiles_in_a_small_app(nrm, tmp_path):
    assert os.path.exists(S.build_facade_app(tmp_path))
