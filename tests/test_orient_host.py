"""Normal orientation (include/s4p_normals_orient.h, libsuper4pcs_normals.so) on the host: the header's declarations against
the binding and the exports, the new kernels in the library's namespace, the loud failure without a device, the restatement
(tests/orient_helpers.py) on a lattice where every decision is a tie-break, on the clouds of the issue's prototype (100 %
outward) and on two separate clusters, the simple call's expression, the command line's new flags and the facade header with
and without Eigen."""
import ctypes

import numpy as np
import pytest

from tests import normals_helpers as NH
from tests import normals_suite as S
from tests import orient_helpers as OH


@pytest.fixture(scope="module")
def nrm():
    return S.normals_module("normals")


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return NH.build_cpu(tmp_path_factory.mktemp("orient_cpu"))


def test_header_declarations_equal_the_binding_and_the_exports(nrm):
    txt, decl, _ = S.check_header("s4p_normals_orient.h", "s4p_orient_", nrm.ORIENT_SYMBOLS, nrm.load_orient(),
                                  closed_prefixes="s4p_(?:normals|knn|outliers|voxel)_")
    assert len(decl) == 4
    assert ctypes.sizeof(nrm.OrientStats) == 32
    assert (nrm.ORIENT_OUTWARD, nrm.ORIENT_VIEWPOINT) == (0, 1) and "S4P_ORIENT_ERR_INTERNAL (-8)" in txt and nrm.ERR_NAMES[-8] == "INTERNAL"


def test_new_kernels_live_in_the_library_namespace(nrm):
    S.check_kernels_in_namespace(("k_orient_edges", "k_orient_min<0>", "k_orient_min<1>", "k_orient_hook", "k_orient_jump", "k_orient_anchor",
                                  "k_orient_anchor_flip", "k_orient_apply", "k_orient_towards"),
                                 stray=r"(?<!s4p_nrm::)(?<!__device_stub__)\bk_orient_\w+")


@pytest.mark.skipif(S.gpu_visible(), reason="checks the failure without a device")
def test_calls_fail_loudly_without_a_device(nrm):
    X = np.zeros((10, 3), np.float32)
    S.check_no_device(nrm.NormalsError, (lambda: nrm.orient_normals(X, X), lambda: nrm.estimate_normals(X, orient="outward")))
    with pytest.raises(ValueError):
        nrm.estimate_normals(X, queries=X, orient="outward")
    with pytest.raises(ValueError):
        nrm.estimate_normals(X, orient="inward")


def test_weights_are_symmetric_and_clamped():
    rng = np.random.default_rng(3)
    A = rng.normal(size=(500, 3)).astype(np.float32); B = rng.normal(size=(500, 3)).astype(np.float32)
    assert np.array_equal(OH.bits(OH.dot(A, B)), OH.bits(OH.dot(B, A)))
    N = np.array([[0, 0, 1], [0, 0, -1], [0, 0, 2], [1, 0, 0], [0, 0, 0], [np.nan, 0, 1], [3e38, 3e38, 0], [3e38, -3e38, 0]], np.float32)
    assert OH.usable(N).tolist() == [True, True, True, True, False, False, True, True]
    idx = np.array([[1, 2, 3], [0, 4, 5], [0, 1, 3], [0, -1, -1], [0, 1, 2], [0, 1, 2], [7, 0, -1], [6, -1, -1]], np.int32)
    lo, hi, w, f = OH.edges(N, idx)
    got = {(int(a), int(b)): (float(x), bool(y)) for a, b, x, y in zip(lo, hi, w, f)}
    # |d| = 2 clamps to 0, orthogonal normals weigh 1, an overflow to NaN (inf - inf) weighs 0 without a flip
    assert got == {(0, 1): (0.0, True), (0, 2): (0.0, False), (0, 3): (1.0, False), (1, 2): (0.0, True), (2, 3): (1.0, False),
                   (0, 6): (1.0, False), (6, 7): (0.0, False)}


def test_lattice_of_ties_gets_one_sign():
    """16 x 16 planar lattice, normals +-z of random sign: every weight is 0, so the tree is decided by the index
    tie-breaks alone; one component, one sign, and the anchor (farthest from the centre, smallest index: a corner) keeps
    its own."""
    X, N = OH.lattice(16)
    assert 0.3 < (N[:, 2] > 0).mean() < 0.7
    idx = OH.numpy_lists(X, 8, exclude_self=True)[0]
    lo, hi, w, f = OH.edges(N, idx)
    assert not w.any() and f.any() and not f.all()
    flip, comp, ncomp = OH.reference(X, N, idx)
    out = OH.apply(N, flip)
    assert ncomp == 1 and (comp == 0).all()                      # the four corners tie in d2: the smallest index anchors
    assert len(np.unique(out[:, 2])) == 1 and out[0, 2] == N[0, 2]
    # towards a viewpoint above the plane every normal ends as +z
    flip, comp, ncomp = OH.reference(X, N, idx, viewpoint=(0.9, 0.9, 5.0))
    assert ncomp == 1 and (OH.apply(N, flip)[:, 2] == 1).all()


def test_restatement_orients_the_prototype_clouds_outward(cpu):
    """PCA normals from the 16 nearest points (the point included), graph k = 8: the sphere and the noisy bumpy cloud come out
    100 % outward (n . x > 0), from about half and two thirds before."""
    from super4pcs_amd import datasets as D
    for name, X, before in (("sphere", D.sphere_cloud(3000, 3), 0.48), ("bumpy", D.bumpy_pair(6000, noise_sigma=0.001, seed=12)[0], 0.64)):
        N = OH.pca_normals(X, cpu.knn(X, 16, threads=16)[0])
        idx = OH.cpu_lists(cpu, X, 8, exclude_self=True)[0]
        out0 = ((N * X).sum(1) > 0).mean()
        flip, comp, ncomp = OH.reference(X, N, idx)
        out1 = ((OH.apply(N, flip) * X).sum(1) > 0).mean()
        print("%s: n %d, outward %.4f -> %.4f, components %d" % (name, len(X), out0, out1, ncomp))
        assert abs(out0 - before) < 0.03 and out1 == 1.0 and ncomp == 1


def test_two_clusters_are_anchored_separately():
    X, N, C = OH.two_clusters()
    idx = OH.numpy_lists(X, 8, exclude_self=True)[0]
    radial = X.astype(np.float64) - C
    for vp in (None, (0.0, 0.0, 0.0)):
        flip, comp, ncomp = OH.reference(X, N, idx, vp)
        out = OH.apply(N, flip).astype(np.float64)
        assert ncomp == 2 and len(np.unique(comp)) == 2
        assert ((C[comp, 0] < 0) == (C[:, 0] < 0)).all()         # every anchor lies in its points' own cluster
        assert ((out * radial).sum(1) > 0).all()                 # both spheres outward: the nearest point of each faces the origin
    assert 0.3 < ((N * radial).sum(1) > 0).mean() < 0.7


def test_towards_is_one_expression():
    X = np.array([[1, 0, 0], [1, 0, 0], [1, 0, 0], [0, 2, 0], [0, 2, 0], [0, 0, 1]], np.float32)
    N = np.array([[0, 1, 0], [1, 0, 0], [-1, 0, 0], [0, 0, 0], [0, np.inf, 0], [0, np.nan, 1]], np.float32)
    out, flip = OH.towards(X, N, (0, 0, 0))
    assert flip.tolist() == [False, True, False, False, False, False]      # n . g = 0 stays; no normal and non-finite stay
    assert np.array_equal(OH.bits(out[[0, 2, 3, 4, 5]]), OH.bits(N[[0, 2, 3, 4, 5]])) and out[1].tolist() == [-1, 0, 0]


def test_cli_orient_flags(tmp_path):
    S.check_cli_flags(
        tmp_path,
        bad=(["--orient-normals", "8"],                                                      # needs --estimate-normals
             ["--estimate-normals", "16", "--orient-viewpoint", "0,0,0"],                    # needs --orient-normals
             ["--orient-viewpoint", "0,0,0"],
             ["--estimate-normals", "16", "--orient-normals", "0"], ["--estimate-normals", "16", "--orient-normals", "33"],
             ["--estimate-normals", "16", "--orient-normals", "8.5"], ["--estimate-normals", "16", "--orient-normals", "x"],
             ["--estimate-normals", "16", "--orient-normals", ""], ["--estimate-normals", "16", "--orient-normals"],
             ["--estimate-normals", "16", "--orient-normals", "8", "--orient-viewpoint", "0,0"],
             ["--estimate-normals", "16", "--orient-normals", "8", "--orient-viewpoint", "0,0,0,0"],
             ["--estimate-normals", "16", "--orient-normals", "8", "--orient-viewpoint", "0,0,nan"],
             ["--estimate-normals", "16", "--orient-normals", "8", "--orient-viewpoint", "0,inf,0"],
             ["--estimate-normals", "16", "--orient-normals", "8", "--orient-viewpoint", "0 0 0"],
             ["--estimate-normals", "16", "--orient-normals", "8", "--orient-viewpoint", "1e39,0,0"],
             ["--estimate-normals", "16", "--orient-normals", "8", "--orient-viewpoint", ""]),
        good=(["--estimate-normals", "16", "--orient-normals", "1"], ["--orient-normals", "32", "--estimate-normals", "3"],
              ["--orient-viewpoint", "0,-1.5,2e3", "--orient-normals", "8", "--estimate-normals", "16"],
              ["--estimate-normals", "16", "--orient-normals", "8", "--icp", "10", "--icp-normal-angle", "60"]),
        usage_word="--orient-normals k", usage_order=("--icp-starts K", "--orient-normals k"))


@pytest.mark.skipif(S.gpu_visible(), reason="checks the failure without a device")
def test_cli_valid_command_fails_with_the_device_error_without_a_gpu(tmp_path):
    S.check_cli_no_device(tmp_path, ["--estimate-normals", "16", "--orient-normals", "8"])


@pytest.mark.parametrize("eigen", [False, True])
def test_facade_header_compiles_with_and_without_eigen(nrm, tmp_path, eigen):
    S.check_facade_header(tmp_path, "normals.h", eigen, "orient", np.random.default_rng(2).uniform(0.1, 1, size=(20, 6)),
                          no_device_args=["8", "-1"], no_device_text=("OrientNormals (MI355X)", "no HIP device"),
                          bad_args=(["0", "-1"], ["33", "-1"], ["8", "nan"], ["8", "-1", "0", "nan", "0"], ["8", "-1", "inf", "0", "0"]),
                          bad_text="OrientNormals:")
