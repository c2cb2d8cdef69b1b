"""Radius normals (include/s4p_shape.h, libsuper4pcs_normals.so) on the host: the header's declarations against the binding
and the exports, the new kernel in the library's namespace, the loud failure without a device in Python, the facade program
and the command line, the two new flags, the facade header with and without Eigen, the restatement (tests/shape_cpu) against
the numpy statement with Python-integer moments on tiny and degenerate clouds, the restatement's grid against its brute
force, the asserted bound on the quantised offsets, and the planted answer: on the project's own noisy cloud a radius of 0.02
recovers the surface's normal where 32 neighbours do not."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import apps
from tests import normals_helpers as NH
from tests import normals_suite as S
from tests import shape_helpers as SH

APP = "shape_app"


@pytest.fixture(scope="module")
def shp():
    return S.normals_module("shape")


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return SH.build_cpu(tmp_path_factory.mktemp("shape_cpu"))


def test_header_declarations_equal_the_binding_and_the_exports(shp):
    from super4pcs_amd import cluster, knn, normals, plane, voxel
    txt, decl, exported = S.check_header("s4p_shape.h", "s4p_shape_", shp.SYMBOLS, shp.load_library(),
                                         closed_prefixes="s4p_(?:normals|knn|outliers|voxel|orient|cluster|plane)_")
    assert len(decl) == 4
    # nothing new under the older prefixes: the exports are the ones their bindings list
    older = set(re.findall(r"\b(s4p_(?:normals|knn|outliers|voxel|cluster|plane)_\w+)", exported))
    known = set(knn.SYMBOLS) | set(voxel.SYMBOLS) | set(cluster.SYMBOLS) | set(plane.SYMBOLS)
    assert {s for s in older if not s.startswith("s4p_normals_")} <= known, older - known
    assert sorted(s for s in older if s.startswith("s4p_normals_")) == sorted(normals.SYMBOLS)
    assert issubclass(shp.Shape, plane.Plane)


def test_new_kernel_lives_in_the_library_namespace(shp):
    S.check_kernels_in_namespace(("k_shape_walk",), stray=r"(?<!s4p_nrm::)(?<!__device_stub__)\bk_shape_\w+")


@pytest.mark.skipif(S.gpu_visible(), reason="checks the failure without a device")
def test_calls_fail_loudly_without_a_device(shp):
    X = np.zeros((10, 3), np.float32)
    S.check_no_device(shp.NormalsError, (lambda: shp.estimate_normals_radius(X, 0.1), lambda: shp.estimate_normals_radius(X, 0.1, queries=X),
                                         lambda: shp.estimate_normals_radius(X, 0.1, orient="outward"), lambda: shp.Shape(0)))


def test_python_argument_rules_and_surface_variation(shp):
    X = np.zeros((10, 3), np.float32)
    with pytest.raises(ValueError):
        shp.estimate_normals_radius(X, 0.1, queries=X, orient="outward")
    with pytest.raises(ValueError):
        shp.estimate_normals_radius(X, 0.1, orient="inward")
    eig = np.array([[2, 1, 1], [1, 1, 0], [0, 0, 0], [1, 0.5, -0.25], [1e-30, 0, 0], [0.5, 0, -0.5]], np.float32)
    got = shp.surface_variation(eig)
    assert got.dtype == np.float32 and np.array_equal(NH.bits(got), NH.bits(SH.surface_variation(eig)))
    assert np.array_equal(got, np.array([0.25, 0, 0, -0.2, 0, 0], np.float32))          # a sum that is not > 0 gives 0; nothing is clamped


def test_cli_estimate_normals_within_flags(tmp_path):
    within = ["--estimate-normals-within", "0.02"]
    S.check_cli_flags(
        tmp_path,
        bad=(["--estimate-normals-min", "5"],                                                            # needs --estimate-normals-within
             ["--estimate-normals", "16", "--estimate-normals-min", "5"],
             within + ["--estimate-normals", "16"], ["--estimate-normals", "16"] + within,                # k or a radius, not both
             within + ["--estimate-normals-radius", "0.1"],                                              # that radius trims k neighbours
             ["--estimate-normals-within", "0"], ["--estimate-normals-within", "-0.1"], ["--estimate-normals-within", "nan"],
             ["--estimate-normals-within", "inf"], ["--estimate-normals-within", "1e39"], ["--estimate-normals-within", "1.9e19"],
             ["--estimate-normals-within", "1e-46"], ["--estimate-normals-within", "0.1x"], ["--estimate-normals-within", ""],
             ["--estimate-normals-within"],
             within + ["--estimate-normals-min", "0"], within + ["--estimate-normals-min", "-2"], within + ["--estimate-normals-min", "2.5"],
             within + ["--estimate-normals-min", "x"], within + ["--estimate-normals-min", ""], within + ["--estimate-normals-min"],
             within + ["--estimate-normals-min", "3000000000"],
             ["--orient-normals", "8"], within + ["--orient-viewpoint", "0,0,0"]),
        good=(within, ["--estimate-normals-within", "2e-2", "--estimate-normals-min", "1"], ["--estimate-normals-min", "2147483647"] + within,
              within + ["--orient-normals", "8"], ["--orient-viewpoint", "0,0,1", "--orient-normals", "8"] + within,
              ["--remove-outliers", "16", "--voxel-size", "0.01", "--remove-plane", "0.15", "--cluster-eps", "0.03"] + within +
              ["-a", "20", "--icp", "10", "--icp-metric", "symmetric"]),
        usage_word="--estimate-normals-within r", usage_order=("--remove-plane d", "--estimate-normals-within r"))
    src = open(os.path.join(S.ROOT, "demos", "Super4PCS", "super4pcs_cli.cc")).read()
    assert "[--estimate-normals-within r] [--estimate-normals-min m]" in src.split("#include")[0]


@pytest.mark.skipif(S.gpu_visible(), reason="checks the failure without a device")
def test_cli_valid_command_fails_with_the_device_error_without_a_gpu(tmp_path):
    S.check_cli_no_device(tmp_path, ["--estimate-normals-within", "0.2", "--estimate-normals-min", "5", "-a", "20"], "EstimateNormalsRadius (MI355X)")


@pytest.mark.parametrize("eigen", [False, True])
def test_facade_header_compiles_with_and_without_eigen(shp, tmp_path, eigen):
    extra = S.check_header_alone(tmp_path, "shape.h", eigen)
    exe = apps.build_app(tmp_path, APP, S.NORMALS_LIBS, ["-Werror"] + extra)
    path = str(tmp_path / "P.txt")
    apps.write_xyz(path, np.random.default_rng(2).uniform(size=(20, 3)))
    if not S.gpu_visible():
        for tail in ([], ["plain"]):
            r = subprocess.run([exe, "shape", path, "0.3", "3"] + tail, capture_output=True, text=True)
            assert r.returncode == 1 and "EstimateNormalsRadius (MI355X)" in r.stderr and "no HIP device" in r.stderr, r.stderr
    for bad in (["0", "3"], ["-1", "3"], ["nan", "3"], ["inf", "3"], ["1e39", "3"], ["1.9e19", "3"], ["1e-46", "3"], ["0.3", "0"], ["0.3", "-4"]):
        r = subprocess.run([exe, "shape", path] + bad, capture_output=True, text=True)
        assert r.returncode == 1 and "EstimateNormalsRadius:" in r.stderr, (bad, r.stderr)
    assert subprocess.run([exe, "shape", str(tmp_path / "none.txt"), "0.3", "3"]).returncode == 2
    assert subprocess.run([exe, "other", path, "0.3", "3"]).returncode == 2


def _both(cpu, X, radius, min_neighbours=3, queries=None):
    """The restatement with its grid, the restatement by brute force and the numpy statement agree in normals, eigenvalues,
    counts and the nine moments.  Returns the restatement's (normals, eig, count, moments)."""
    a = cpu.estimate(X, radius, min_neighbours, queries, moments=True)
    b = cpu.estimate(X, radius, min_neighbours, queries, moments=True, brute=True)
    c = SH.numpy_estimate(X, radius, min_neighbours, queries, want_moments=True)
    assert SH.same(a, b) and np.array_equal(a[3], b[3])
    assert np.array_equal(a[3], c[3]), np.flatnonzero((a[3] != c[3]).any(1))[:5]
    assert SH.same(a, c), SH.differing(a, c)
    return a


@pytest.mark.parametrize("n", [n for n in SH.SIZES if n <= 257])
def test_restatement_equals_the_numpy_statement_on_the_tiny_clouds(cpu, n):
    X = SH.cube_cloud(n)
    N, E, cnt, mom = _both(cpu, X, SH.cube_radius(n))
    Nb, Eb, cb, _ = _both(cpu, X, SH.BEYOND)
    assert (cb == n).all() and (cnt >= 1).all() and np.array_equal(mom[:, 0], cnt)
    for nrm, eig, c in ((N, E, cnt), (Nb, Eb, cb)):
        has = nrm.any(1)
        assert not has[c < 3].any() and not eig[~has].any()
        ln = np.linalg.norm(nrm[has].astype(np.float64), axis=1)
        assert np.all(np.abs(ln - 1) < 1e-6) and np.all(np.abs(nrm[has]).max(1) == nrm[has].max(1))      # unit, the largest component positive
        assert np.all(eig[:, 0] >= eig[:, 1]) and np.all(eig[:, 1] >= eig[:, 2])
    if n >= 63:
        assert 10 < np.median(cnt) < 40 and Nb.any(1).all()
    # beyond the extent every row sees the whole cloud: the eigenvalues are the cloud's own for every row, up to the rounding of
    # another centre (the offsets are taken from the query)
    if n >= 4:
        assert np.allclose(Eb, Eb[0], rtol=1e-4, atol=1e-7)


def test_restatement_equals_the_numpy_statement_above_one_block(cpu):
    X = SH.cube_cloud(4097)
    r = SH.cube_radius(4097)
    N, E, cnt, _ = _both(cpu, X, r, queries=X[::16])
    full = cpu.estimate(X, r)
    assert SH.same(tuple(a[::16] for a in full), (N, E, cnt)) and 12 < np.median(cnt) < 30
    _both(cpu, X, SH.BEYOND, queries=X[:8])


def test_restatement_equals_the_numpy_statement_on_degenerate_and_extreme_clouds(cpu):
    # identical points: the covariance is zero; collinear: rank one, a normal exists (any direction across the line the Jacobi
    # lands on) and two eigenvalues are zero or a residue; coplanar: the normal is the plane's
    N, E, cnt, _ = _both(cpu, SH.identical_cloud(), 0.5)
    assert (cnt == 100).all() and not N.any() and not E.any()
    N, E, cnt, _ = _both(cpu, SH.collinear_cloud(), 0.3)
    line = np.array([1, 2, -3]) / np.sqrt(14.0)
    assert N.any(1).sum() > 90 and np.abs(N[N.any(1)].astype(np.float64) @ line).max() < 1e-6 and np.abs(E[:, 1:]).max() < 1e-12 * E[:, 0].max()
    N, E, cnt, _ = _both(cpu, SH.coplanar_cloud(), 0.2)
    assert N.any(1).all() and np.array_equal(N, np.tile(np.array([0, 0, 1], np.float32), (len(N), 1))) and np.abs(E[:, 2]).max() == 0
    # the lattice: at r = 1 the six axis neighbours lie on the bound and count, at the float below they do not
    L = SH.lattice_cloud()
    inner = ((L > 0) & (L < 7)).all(1)
    assert (_both(cpu, L, 1.0)[2][inner] == 7).all() and (_both(cpu, L, SH.below(1.0))[2] == 1).all()
    # E changes at a power of two: 0.25 has s = 20, the float below it s = 21
    X = SH.cube_cloud(257)
    assert SH.scale_exponent(0.25) == 20 and SH.scale_exponent(SH.below(0.25)) == 21
    a, b = _both(cpu, X, 0.25), _both(cpu, X, SH.below(0.25))
    assert np.array_equal(a[2], b[2]) and not np.array_equal(a[3], b[3])              # the same sets, offsets at twice the resolution
    # each offset moves by at most half a step, r 2^-19, so an entry of C by at most 4 r (r 2^-19) + 2 (r 2^-19)^2 and an eigenvalue by at
    # most three times that (Weyl, a 3 x 3 matrix): below r^2 2^-15; a normal may turn freely where two eigenvalues nearly coincide
    assert np.abs(a[1].astype(np.float64) - b[1]).max() < 0.25 ** 2 * 2.0 ** -15
    # a cloud translated by 1e4 and a cloud scaled by 2^40 and 2^-40: the same integers, eigenvalues x 2^80 and 2^-80 exactly
    _both(cpu, (X + np.float32(1.0e4)).astype(np.float32), 0.25)
    Z = SH.scale_cloud()
    base = _both(cpu, Z, 1.2)
    for e in (40, -40):
        f = np.float32(2.0 ** e)
        got = _both(cpu, Z * f, np.float32(1.2) * f)
        assert np.array_equal(got[3], base[3]) and np.array_equal(NH.bits(got[0]), NH.bits(base[0]))
        assert np.array_equal(NH.bits(got[1]), NH.bits(base[1] * f * f))
    # two far clusters at a tiny radius
    F = SH.two_far_clusters()
    N, E, cnt, _ = _both(cpu, F, 3.0e-4)
    assert 3 < np.median(cnt) < 100 and cnt.max() <= 300


def test_min_neighbours_and_queries_off_the_cloud(cpu):
    X = SH.cube_cloud(257)
    r = SH.cube_radius(257)
    base = _both(cpu, X, r)
    i = int(np.argmax(base[2]))                              # a row with many neighbours: at, below and above its count
    c = int(base[2][i])
    assert c >= 4
    for mn, has in ((c - 1, True), (c, True), (c + 1, False), (1, True), (2, True)):
        got = _both(cpu, X, r, mn)
        assert np.array_equal(got[2], base[2]) and got[0][i].any() == has and got[1][i].any() == has
        keep = base[2] >= max(3, mn)
        assert np.array_equal(NH.bits(got[0][keep]), NH.bits(base[0][keep])) and not got[0][~keep].any() and not got[1][~keep].any()
    h = 1.001 * float(r)
    Qs = np.concatenate([X[:5], X[:3] + np.float32(0.01),
                         np.array([[-0.5 * h, 0.5, 0.5], [1 + 0.9 * h, 0.5, 0.5], [0.5, -1.5 * h, 0.5], [0.5, 0.5, 1 + 2.5 * h],     # around the bounds
                                   [50, 50, 50], [-3e38, 0, 0], [1e30, -1e30, 1e30],                                              # far away
                                   [np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf]], np.float32)]).astype(np.float32)
    N, E, cnt, _ = _both(cpu, X, r, queries=Qs)
    assert np.array_equal(cnt[:5], base[2][:5]) and np.array_equal(NH.bits(N[:5]), NH.bits(base[0][:5]))
    assert (cnt[-6:] == 0).all() and not N[-6:].any() and not E[-6:].any()
    empty = cpu.estimate(X, r, queries=np.zeros((0, 3), np.float32))
    assert empty[0].shape == (0, 3) and empty[2].shape == (0,)


def test_quantised_offsets_stay_within_the_bound(cpu):
    """|u| <= 2^19 + 1 over every accepted neighbour the module's calls met (the restatement keeps the largest), and the
    bound is nearly reached: at the float below a power of two a neighbour at distance r has u = 2^19."""
    r = SH.below(1.0)
    X = np.array([[0, 0, 0], [r, 0, 0], [0, -r, 0], [0, 0, r], [1, 0, 0], [0.5, 0.5, 0.5]], np.float32)
    N, E, cnt, mom = cpu.estimate(X, r, moments=True)
    assert cnt[0] == 5 and SH.numpy_moments(X, r, X[0])[3] == 1 << 19
    assert cpu.umax >= 1 << 19
    for radius in (SH.below(0.5), 0.5, 3.0e-4, 2.0 ** -60, SH.below(2.0 ** 60)):
        f = np.float32(radius) / np.float32(0.5)
        cpu.estimate((SH.cube_cloud(257) * f).astype(np.float32), radius)
    assert cpu.umax <= SH.U_BOUND, cpu.umax


def test_planted_answer_a_radius_recovers_the_normal_that_32_neighbours_lose(cpu, tmp_path_factory):
    """Q of bumpy_pair(300000) with its default noise 0.004, 3000 seeded queries: the median angle to the noise-free surface's
    normal is below 5 degrees at r = 0.02 and above 20 degrees with the 32 nearest neighbours."""
    Q, qs, truth = SH.planted()
    P = SH.PLANTED
    assert len(Q) == P["n"] and len(qs) == P["queries"]
    N, E, cnt = cpu.estimate(Q, P["radius"], queries=qs)
    ang = SH.angles_deg(N, truth)
    knn = NH.build_cpu(tmp_path_factory.mktemp("normals_cpu")).normals(Q, P["knn"], queries=qs, threads=16)
    ang32 = SH.angles_deg(knn, truth)
    print("radius %.3f: median %.2f deg, p90 %.2f, neighbours median %d max %d; k = %d: median %.2f deg, p90 %.2f"
          % (P["radius"], np.median(ang), np.percentile(ang, 90), np.median(cnt), cnt.max(), P["knn"], np.median(ang32), np.percentile(ang32, 90)))
    assert N.any(1).all() and knn.any(1).all()
    assert np.median(ang) < P["below_deg"]
    assert np.median(ang32) > P["above_deg"]
    # the surface variation of a noisy sheet 0.004 thick in a ball of 0.02 is small but not zero
    sv = SH.surface_variation(E)
    assert 0.01 < np.median(sv) < 0.2 and (sv >= 0).all() and (sv <= 1 / 3 + 1e-6).all()
