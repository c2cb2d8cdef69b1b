"""Plane segmentation (include/s4p_plane.h, libsuper4pcs_normals.so) on the host: the header's declarations against the
binding and the exports, the new kernels in the library's namespace, the pinned struct sizes, the loud failure without a
device, the restatement (tests/plane_cpu) against the numpy float64 statement on tiny clouds and on the lidar cloud with every
residual away from the bound, the planted ground of the lidar cloud, the peeling rule on the restatement, the command line's
new flags and the facade header with and without Eigen."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import normals_suite as S
from tests import plane_helpers as PH


@pytest.fixture(scope="module")
def pln():
    return S.normals_module("plane")


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return PH.build_cpu(tmp_path_factory.mktemp("plane_cpu"))


def test_header_declarations_equal_the_binding_and_the_exports(pln):
    from super4pcs_amd import cluster, knn, voxel
    txt, decl, exported = S.check_header("s4p_plane.h", "s4p_plane_", pln.SYMBOLS, pln.load_library(),
                                         closed_prefixes="s4p_(?:normals|knn|outliers|voxel|orient|cluster)_")
    assert len(decl) == 2
    # nothing new under the older prefixes: the exports are the ones their bindings list
    older = set(re.findall(r"\b(s4p_(?:normals|knn|outliers|voxel|cluster)_\w+)", exported))
    known = set(knn.SYMBOLS) | set(voxel.SYMBOLS) | set(cluster.SYMBOLS)
    assert {s for s in older if not s.startswith("s4p_normals_")} <= known, older - known
    assert (pln.MAX_TRIALS, pln.MAX_REFINE, pln.SUM_BLOCK) == (1 << 20, 16, PH.SUM_BLOCK)
    for name, value in (("S4P_PLANE_MAX_TRIALS", "(1 << 20)"), ("S4P_PLANE_MAX_REFINE", "16"), ("S4P_PLANE_SUM_BLOCK", "128")):
        assert "#define %s %s" % (name, value) in txt


def test_struct_sizes_are_pinned(pln, tmp_path):
    assert ctypes.sizeof(pln.PlaneOptions) == 24 and ctypes.sizeof(pln.PlaneResult) == 56
    assert pln.PlaneOptions.seed.offset == 8 and pln.PlaneOptions.refine.offset == 16
    assert (pln.PlaneResult.centre.offset, pln.PlaneResult.d_centred.offset, pln.PlaneResult.inliers.offset, pln.PlaneResult.trial.offset) == (16, 28, 32, 48)
    probe = tmp_path / "sizes.c"
    probe.write_text('#include <stddef.h>\n#include "s4p_plane.h"\n_Static_assert(sizeof(s4p_plane_options) == 24, "options");\n'
                     '_Static_assert(sizeof(s4p_plane_result) == 56, "result");\n_Static_assert(offsetof(s4p_plane_result, trial) == 48, "trial");\n')
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I" + S.INCLUDE, str(probe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_new_kernels_live_in_the_library_namespace(pln):
    S.check_kernels_in_namespace(("k_plane_candidates", "k_plane_count", "k_plane_argmax", "k_plane_mask", "k_plane_moments", "k_plane_refit"),
                                 stray=r"(?<!s4p_nrm::)(?<!__device_stub__)\bk_plane_\w+")


@pytest.mark.skipif(S.gpu_visible(), reason="checks the failure without a device")
def test_calls_fail_loudly_without_a_device(pln):
    X = np.zeros((10, 3), np.float32)
    S.check_no_device(pln.NormalsError, (lambda: pln.segment_plane(X, 0.1), lambda: pln.segment_planes(X, 0.1), lambda: pln.remove_planes(X, 0.1),
                                         lambda: pln.Plane(0)))


def test_splitmix_statement_equals_the_published_stream():
    """The first outputs of splitmix64 from state 0 and from state 1234567 (the reference values of its author's C code)."""
    assert [PH.splitmix_element(0, k) for k in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert [PH.splitmix_element(1234567, k) for k in range(2)] == [6457827717110365317, 3203168211198807973]


# (n, seed) pairs of the tiny clouds.  For each the smallest relative distance of a residual from the inlier bound, over the
# winning plane, every refit plane and every point, is above 1e-5 (asserted below), so float64 and fmaf count the same points.
TINY_CASES = [(3, 0), (4, 1), (63, 0), (64, 0), (65, 1), (255, 0), (256, 1), (257, 0), (4095, 0), (4096, 0), (4097, 1)]


@pytest.mark.parametrize("n,seed", TINY_CASES)
@pytest.mark.parametrize("refine", [0, 1, 3])
def test_restatement_equals_the_numpy_statement_on_the_tiny_clouds(cpu, n, seed, refine):
    X = PH.tiny_cloud(n)
    ex = None
    if n == 257:                                               # one case with an exclude mask
        ex = (np.random.default_rng(5).uniform(size=n) < 0.3).astype(np.uint8)
    a = cpu.segment(X, PH.TINY_DISTANCE, 64, seed, refine, ex, all_counts=True)
    b = PH.numpy_segment(X, PH.TINY_DISTANCE, 64, seed, refine, ex)
    gap = PH.residual_gap(X, PH.TINY_DISTANCE, b[2]["planes"], ex)
    print("n %d seed %d refine %d: smallest relative gap to the bound %.2e, trial %d, inliers %d" % (n, seed, refine, gap, b[2]["trial"], b[2]["inliers"]))
    assert gap > 1e-5
    assert PH.same(a, b), (a[0], b[0], a[2]["trial"], b[2]["trial"])
    assert np.array_equal(a[2]["valid"], b[2]["valid"]) and a[2]["counts"][a[2]["trial"]] == b[2]["counts"][b[2]["trial"]]
    assert a[2]["trial"] >= 0 and len(b[2]["planes"]) >= 1 and (ex is None or not a[1][ex != 0].any())


def test_restatement_equals_the_numpy_statement_on_degenerate_clouds(cpu):
    for X, valid in ((PH.identical_cloud(), False), (PH.collinear_cloud(), False), (PH.duplicates_cloud(distinct=4), True)):
        a = cpu.segment(X, 0.01, 256, 0, 1, all_counts=True)
        b = PH.numpy_segment(X, 0.01, 256, 0, 1)
        assert PH.same(a, b) and np.array_equal(a[2]["valid"], b[2]["valid"])
        if valid:
            assert 0 < a[2]["valid_trials"] < 128 and PH.residual_gap(X, 0.01, b[2]["planes"]) > 1e-5
        else:
            assert a[2]["trial"] == -1 and a[2]["valid_trials"] == 0 and not a[1].any() and not a[0].any()
    X = PH.tiny_cloud(64)
    ex = np.ones(64, np.uint8)
    ex[[3, 40]] = 0
    a = cpu.segment(X, 0.05, 64, 0, 1, ex)
    assert PH.same(a, PH.numpy_segment(X, 0.05, 64, 0, 1, ex)) and a[2]["alive"] == 2 and a[2]["trial"] == -1


def test_planted_ground_of_the_lidar_cloud(cpu):
    """distance 0.15, 1024 trials, one refit, seed 0: the two statements agree (no residual within 1e-5 of the bound), and the
    ground is found: |n_z| > 0.999, at least 99 % of the inliers have |z| < 0.15, at least 99 % of the points with |z| < 0.1
    are inliers."""
    X = PH.lidar_cloud()
    assert len(X) == 20000
    a = cpu.segment(X, all_counts=True, **PH.LIDAR)
    b = PH.numpy_segment(X, **PH.LIDAR)
    gap = PH.residual_gap(X, PH.LIDAR["distance"], b[2]["planes"])
    print("lidar: smallest relative gap to the bound %.2e, plane %s, inliers %d, trial %d" % (gap, a[0], a[2]["inliers"], a[2]["trial"]))
    assert gap > 1e-5 and len(b[2]["planes"]) == 2
    assert PH.same(a, b) and np.array_equal(a[2]["valid"], b[2]["valid"]) and a[2]["counts"][a[2]["trial"]] == b[2]["counts"][b[2]["trial"]]
    plane, mask, info = a
    z = X[:, 2]
    assert abs(plane[2]) > 0.999
    assert (np.abs(z[mask != 0]) < 0.15).mean() >= 0.99
    assert mask[np.abs(z) < 0.1].mean() >= 0.99
    assert info["inliers"] == int(mask.sum()) and 11300 < info["inliers"] < 11500 and info["alive"] == 20000
    # a second plane on the rest is far smaller: the first is unambiguous
    second = cpu.segment(X, 0.15, 1024, 1, 1, mask)
    assert second[2]["inliers"] < 1000 and not (second[1] & mask).any()


def test_peeling_stops_at_the_first_small_plane_and_labels_in_order(pln, cpu):
    X = PH.box_corner()

    def seg(p, ex):
        return cpu.segment(X, 0.01, 512, 3 + p, 1, ex)
    planes, labels = pln.peel_planes(seg, len(X), max_planes=4, min_inliers=800)
    sizes = np.bincount(labels[labels >= 0]).tolist()
    assert len(planes) == 3 and planes.shape == (3, 4) and sizes == sorted(sizes, reverse=True) and labels.dtype == np.int32
    assert [int(np.argmax(np.abs(p[:3]))) for p in planes] == [2, 0, 1]                    # z = 0, x = 0, y = 0
    for p in range(3):                                                                     # plane p never takes a point of an earlier plane
        _, mask, info = seg(p, (labels >= 0) & (labels < p))
        assert np.array_equal(mask != 0, labels == p) and info["inliers"] == sizes[p]
    assert seg(3, labels >= 0)[2]["inliers"] < 800                                         # the fourth is what stopped the loop
    p2, l2 = pln.peel_planes(seg, len(X), max_planes=2, min_inliers=800)
    assert np.array_equal(p2, planes[:2]) and np.array_equal(l2, np.where(labels == 2, -1, labels))
    p1, l1 = pln.peel_planes(seg, len(X), max_planes=4, min_inliers=2500)                  # the second face is too small: one plane
    assert len(p1) == 1 and np.array_equal(l1, np.where(labels == 0, 0, -1))
    p0, l0 = pln.peel_planes(seg, len(X), max_planes=4, min_inliers=10 ** 6)
    assert p0.shape == (0, 4) and (l0 == -1).all()
    with pytest.raises(ValueError):
        pln.peel_planes(seg, len(X), max_planes=0)


def test_cli_remove_plane_flags(tmp_path):
    S.check_cli_flags(
        tmp_path,
        bad=(["--remove-plane-trials", "64"], ["--remove-plane-count", "2"],                                  # both need --remove-plane
             ["--remove-plane", "-0.1"], ["--remove-plane", "nan"], ["--remove-plane", "inf"], ["--remove-plane", "1e39"],
             ["--remove-plane", "0.1x"], ["--remove-plane", ""], ["--remove-plane"],
             ["--remove-plane", "0.1", "--remove-plane-trials", "0"], ["--remove-plane", "0.1", "--remove-plane-trials", "-3"],
             ["--remove-plane", "0.1", "--remove-plane-trials", "4.5"], ["--remove-plane", "0.1", "--remove-plane-trials", "x"],
             ["--remove-plane", "0.1", "--remove-plane-trials", ""], ["--remove-plane", "0.1", "--remove-plane-trials"],
             ["--remove-plane", "0.1", "--remove-plane-trials", "1048577"],
             ["--remove-plane", "0.1", "--remove-plane-count", "0"], ["--remove-plane", "0.1", "--remove-plane-count", "1.5"],
             ["--remove-plane", "0.1", "--remove-plane-count", ""], ["--remove-plane", "0.1", "--remove-plane-count"],
             ["--remove-plane", "0.1", "--remove-plane-count", "3000000000"]),
        good=(["--remove-plane", "0.15"], ["--remove-plane-trials", "1048576", "--remove-plane", "1.5e-1"], ["--remove-plane", "0"],
              ["--remove-plane", "0.5", "--remove-plane-trials", "1", "--remove-plane-count", "3"],
              ["--remove-outliers", "16", "--voxel-size", "0.01", "--remove-plane", "0.15", "--cluster-eps", "0.03", "--estimate-normals", "16"]),
        usage_word="--remove-plane d", usage_order=("--cluster-eps e", "--remove-plane d"))
    src = open(os.path.join(S.ROOT, "demos", "Super4PCS", "super4pcs_cli.cc")).read()
    assert "[--remove-plane d] [--remove-plane-trials T] [--remove-plane-count K]" in src.split("#include")[0]


def test_cli_refuses_an_input_with_faces(tmp_path):
    S.check_cli_refuses_faces(tmp_path, ["--remove-plane", "0.1"])


@pytest.mark.skipif(S.gpu_visible(), reason="checks the failure without a device")
def test_cli_valid_command_fails_with_the_device_error_without_a_gpu(tmp_path):
    S.check_cli_no_device(tmp_path, ["--remove-plane", "0.2", "--remove-plane-trials", "64"], "RemovePlanes (MI355X)")


@pytest.mark.parametrize("eigen", [False, True])
def test_facade_header_compiles_with_and_without_eigen(pln, tmp_path, eigen):
    exe, path = S.check_facade_header(
        tmp_path, "plane.h", eigen, "plane", np.random.default_rng(2).uniform(size=(20, 3)),
        no_device_args=["0.2", "64", "1", "1"], no_device_text=("SegmentPlane (MI355X)", "no HIP device"),
        bad_args=(["-1", "64", "1", "1"], ["nan", "64", "1", "1"], ["inf", "64", "1", "1"], ["1e39", "64", "1", "1"], ["0.2", "0", "1", "1"],
                  ["0.2", "1048577", "1", "1"], ["0.2", "64", "-1", "1"], ["0.2", "64", "17", "1"]),
        bad_text="SegmentPlane:")
    r = subprocess.run([exe, "plane", path, "0.2", "64", "1", "0"], capture_output=True, text=True)
    assert r.returncode == 1 and "count must be at least 1" in r.stderr
