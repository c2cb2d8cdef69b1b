"""FPFH descriptors and the feature matcher (include/s4p_feature.h, libsuper4pcs_normals.so) on the host: the header's
declarations against the binding and the exports, the new kernels in the library's namespace, the loud failure without a
device in Python and in the facade program, the facade header with and without Eigen, the restatement (tests/feature_cpu)
against the numpy statement with Python-integer histograms on tiny clouds, the lattice, the plane's known answer and invalid
input, the boundary table against math.atan2, the matcher's restatement against Python integers, the quality of the
restatement's matches on the project's registration pair, and poses_from_matches."""
import math
import re
import subprocess

import numpy as np
import pytest

from tests import apps
from tests import feature_helpers as FH
from tests import normals_suite as S
from tests import shape_helpers as SH

APP = "feature_app"


@pytest.fixture(scope="module")
def ft():
    return S.normals_module("features")


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return FH.build_cpu(tmp_path_factory.mktemp("feature_cpu"))


@pytest.fixture(scope="module")
def pair(cpu, tmp_path_factory):
    """bumpy_pair(3000, noise_sigma=0.001), normals within 0.04 oriented outward, the restatement's descriptors at r = 0.08
    and its mutual matches."""
    P, Q, T = FH.pair_clouds()
    Pn, Qn = FH.pair_normals(SH.build_cpu(tmp_path_factory.mktemp("shape_cpu")))
    Fp, Fq = cpu.fpfh(P, Pn, FH.PAIR["radius"])[0], cpu.fpfh(Q, Qn, FH.PAIR["radius"])[0]
    return dict(P=P, Q=Q, T=T, Fp=Fp, Fq=Fq, M=FH.pairs_of(cpu.match(Fp, Fq, True)[0]))


def test_header_declarations_equal_the_binding_and_the_exports(ft):
    from super4pcs_amd import cluster, knn, normals, plane, shape, voxel
    txt, decl, exported = S.check_header("s4p_feature.h", "s4p_feature_", ft.SYMBOLS, ft.load_library(),
                                         closed_prefixes="s4p_(?:normals|knn|outliers|voxel|orient|cluster|plane|shape)_")
    assert len(decl) == 4
    # nothing new under the older prefixes: the exports are the ones their bindings list
    older = set(re.findall(r"\b(s4p_(?:normals|knn|outliers|voxel|cluster|plane|shape)_\w+)", exported))
    known = set(knn.SYMBOLS) | set(voxel.SYMBOLS) | set(cluster.SYMBOLS) | set(plane.SYMBOLS) | set(shape.SYMBOLS)
    assert {s for s in older if not s.startswith("s4p_normals_")} <= known, older - known
    assert sorted(s for s in older if s.startswith("s4p_normals_")) == sorted(normals.SYMBOLS)
    assert issubclass(ft.Features, shape.Shape)
    assert "#define S4P_FEATURE_BINS 33" in txt and "#define S4P_FEATURE_MAX 4096" in txt and ft.BINS == 33 and ft.MAX_VALUE == 4096


def test_new_kernels_live_in_the_library_namespace(ft):
    S.check_kernels_in_namespace(("k_feature_normals", "k_feature_spfh", "k_feature_fpfh", "k_feature_rows", "k_feature_match", "k_feature_pick"),
                                 stray=r"(?<!s4p_nrm::)(?<!__device_stub__)\bk_feature_\w+")


@pytest.mark.skipif(S.gpu_visible(), reason="checks the failure without a device")
def test_calls_fail_loudly_without_a_device(ft):
    X = np.zeros((10, 3), np.float32)
    F = np.zeros((10, 33), np.uint16)
    S.check_no_device(ft.NormalsError, (lambda: ft.compute_fpfh(X, 0.1), lambda: ft.compute_fpfh(X, 0.1, normals=X), lambda: ft.match_features(F, F),
                                        lambda: ft.Features(0)))


def test_python_argument_rules(ft):
    X = np.zeros((10, 3), np.float32)
    with pytest.raises(ValueError):
        ft.compute_fpfh(X, 0.1, orient="inward")
    with pytest.raises(ValueError):
        ft.compute_fpfh(X, 0.1, normals=X, normal_radius=0.05)
    for kw in (dict(max_distance=0), dict(max_distance=0.1, trials=0), dict(max_distance=0.1, starts=0)):
        with pytest.raises(ValueError):
            ft.poses_from_matches(X, X, np.zeros((5, 2), np.int32), **kw)
    assert ft.poses_from_matches(X, X, np.zeros((2, 2), np.int32), 0.1).shape == (0, 4, 4)
    assert "orient" in ft.compute_fpfh.__doc__ and "WARNING" in ft.compute_fpfh.__doc__ and "refine_best" in ft.poses_from_matches.__doc__


@pytest.mark.parametrize("eigen", [False, True])
def test_facade_header_compiles_with_and_without_eigen(ft, tmp_path, eigen):
    extra = S.check_header_alone(tmp_path, "features.h", eigen)
    exe = apps.build_app(tmp_path, APP, S.NORMALS_LIBS, ["-Werror"] + extra)
    path = str(tmp_path / "P.txt")
    rng = np.random.default_rng(2)
    apps.write_xyz(path, np.concatenate([rng.uniform(size=(20, 3)), FH.random_normals(20)], 1))
    if not S.gpu_visible():
        for args in (["fpfh", path, "0.3"], ["match", path, path, "0.3", "1"]):
            r = subprocess.run([exe] + args, capture_output=True, text=True)
            assert r.returncode == 1 and "ComputeFPFH (MI355X)" in r.stderr and "no HIP device" in r.stderr, r.stderr
    for bad in ("0", "-1", "nan", "inf", "1e39", "1.9e19", "1e-46"):
        r = subprocess.run([exe, "fpfh", path, bad], capture_output=True, text=True)
        assert r.returncode == 1 and "ComputeFPFH:" in r.stderr, (bad, r.stderr)
    assert subprocess.run([exe, "fpfh", str(tmp_path / "none.txt"), "0.3"]).returncode == 2
    assert subprocess.run([exe, "match", path, str(tmp_path / "none.txt"), "0.3", "1"]).returncode == 2
    assert subprocess.run([exe, "other", path, "0.3"]).returncode == 2 and subprocess.run([exe, "fpfh", path]).returncode == 2


def _all_three(cpu, X, N, radius):
    """The restatement with its grid, the restatement by brute force and the numpy statement agree in descriptors, counts and
    SPFH rows.  Returns the restatement's (F, count, S)."""
    a = cpu.fpfh(X, N, radius, spfh=True)
    b = cpu.fpfh(X, N, radius, spfh=True, brute=True)
    c = FH.numpy_fpfh(X, N, radius, want_spfh=True)
    assert FH.same(a, b) and np.array_equal(a[2], b[2])
    assert np.array_equal(a[2], c[2]), np.flatnonzero((a[2] != c[2]).any(1))[:5]
    assert FH.same(a, c), FH.differing(a, c)
    assert a[0].max(initial=0) <= 4096 and a[2].max(initial=0) <= 1 << 15
    return a


def test_boundary_table_equals_the_cosines_and_sines_and_atan2():
    """The header's literals are fl(cos beta_k), fl(sin beta_k); on a dense fan of directions at three magnitudes the bin
    equals floor((atan2(y, x) + pi) / (2 pi / 11)) everywhere except within 1e-6 rad of a boundary."""
    mine, header = FH.theta_bounds(), FH.header_bounds()
    assert all(a[0] == b[0] and a[1] == b[1] for a, b in zip(mine, header))
    th = np.linspace(-math.pi, math.pi, 400001)[:-1]
    total = excluded = 0
    for scale in (1.0, 1.0e-3, 3.0e4):
        x = (np.cos(th) * scale).astype(np.float32); y = (np.sin(th) * scale).astype(np.float32)
        ang = np.arctan2(y.astype(np.float64), x.astype(np.float64))
        t = (ang + math.pi) / (2 * math.pi / 11)
        near = np.abs(t - np.rint(t)) * (2 * math.pi / 11) < 1.0e-6
        want = np.minimum(10, np.floor(t)).astype(np.int64)
        got = FH.bin_theta(x, y, header)
        assert np.array_equal(got[~near], want[~near]), int((got[~near] != want[~near]).sum())
        assert set(got) == set(range(11))
        total += len(th); excluded += int(near.sum())
    print("directions %d, excluded within 1e-6 rad of a boundary: %d" % (total, excluded))
    assert excluded < 0.001 * total
    # the axes and the plane's pair
    assert list(FH.bin_theta([1, 0, -1, 0, -1], [0, 1, 0, -1, -0.0], header)) == [5, 8, 10, 2, 10]


@pytest.mark.parametrize("n", [n for n in FH.SIZES if n <= 257])
def test_restatement_equals_the_numpy_statement_on_the_tiny_clouds(cpu, n):
    X = FH.cube_cloud(n)
    N = FH.random_normals(n)
    F, cnt, Srows = _all_three(cpu, X, N, FH.cube_radius(n))
    Fb, cb, _ = _all_three(cpu, X, N, SH.BEYOND)
    if n >= 63:
        assert 8 < np.median(cnt) < 40 and Fb.any(1).all()
        for tab, top in ((F, 4096), (Srows, 1 << 15)):
            sums = tab.reshape(n, 3, 11).astype(np.int64).sum(2)
            assert ((sums == 0) | ((sums > top - 11) & (sums <= top))).all()          # eleven floors lose less than eleven
        assert set(np.flatnonzero(Fb.any(0))) == set(range(33))                       # random normals meet every bin


def test_restatement_equals_the_numpy_statement_on_lattices_and_the_planes_known_answer(cpu):
    L = FH.lattice_cloud()
    N = FH.random_normals(len(L), 3)
    inner = ((L > 0) & (L < 7)).all(1)
    assert (_all_three(cpu, L, N, 1.0)[1][inner] == 6).all()                          # d2 = fl(r^2) sits on the rim and counts
    F, cnt, _ = _all_three(cpu, L, N, FH.below(1.0))
    assert not F.any() and not cnt.any()
    assert (_all_three(cpu, L, N, 1.5)[1][inner] == 18).all()
    # a plane with one normal: alpha = 0, phi = 0, theta = 0 for every pair
    P, Np = FH.plane_lattice()
    F, cnt, Srows = _all_three(cpu, P, Np, 2.5)
    want = np.zeros(33, np.uint16); want[[5, 16, 27]] = 4096
    interior = ((P[:, :2] >= 3) & (P[:, :2] <= 8)).all(1)
    assert interior.sum() == 36 and (cnt[interior] == 20).all() and np.array_equal(F[interior], np.tile(want, (36, 1)))
    assert np.array_equal(F, np.tile(want, (len(P), 1)))                              # and every other row, whose neighbours are fewer
    assert np.array_equal(Srows, np.tile((want.astype(np.int64) * 8).astype(np.uint16), (len(P), 1)))


def test_restatement_equals_the_numpy_statement_on_invalid_and_degenerate_input(cpu):
    X = FH.cube_cloud(257)
    N, bad = FH.mixed_normals(257)
    F, cnt, _ = _all_three(cpu, X, N, 0.3)
    assert not F[bad].any() and not cnt[bad].any() and F[np.setdiff1d(np.arange(257), bad)].any(1).all()
    Xn = X.copy()
    Xn[3, 0] = np.nan; Xn[100, 2] = np.inf; Xn[200] = -np.inf
    F, cnt, _ = _all_three(cpu, Xn, N, 0.3)
    assert not F[[3, 100, 200]].any() and not cnt[[3, 100, 200]].any()
    F, cnt, _ = _all_three(cpu, SH.identical_cloud(), FH.random_normals(100, 4), 0.5)
    assert not F.any() and not cnt.any()
    S3 = np.array([[0, 0, 0], [0, 0, 0.5], [0.25, 0, 0]], np.float32)
    N3 = np.tile(np.array([[0, 0, 1]], np.float32), (3, 1))
    assert list(_all_three(cpu, S3, N3, 1.0)[1]) == [1, 1, 2]                         # the stacked pair is skipped
    F, cnt, _ = _all_three(cpu, S3[:2], N3[:2], 1.0)
    assert not F.any() and not cnt.any()
    # a neighbour at exactly r / 32, nearer ones and one just beyond: the weights of the numpy statement are asserted in [64, 2^16]
    rng = np.random.default_rng(17)
    W = np.concatenate([np.array([[0, 0, 0], [1 / 32, 0, 0], [0, -1 / 64, 0], [0, 0, 1 / 1024], [0, 1 / 32, 1 / 1024]], np.float32),
                        rng.uniform(-0.6, 0.6, (60, 3)).astype(np.float32)])
    _all_three(cpu, W, FH.random_normals(len(W), 6), 1.0)
    B = FH.ball_cloud()
    assert _all_three(cpu, B, FH.random_normals(len(B), 7), 0.8)[1].min() > 256
    # translated to 1e4 and scaled by 2^-40: every feature is a ratio of lengths
    _all_three(cpu, (X + np.float32(1.0e4)).astype(np.float32), FH.random_normals(257), 0.25)
    Z, Nz = FH.scale_cloud(), FH.random_normals(300, 9)
    f = np.float32(2.0 ** -40)
    assert FH.same(_all_three(cpu, Z * f, Nz, np.float32(1.2) * f), _all_three(cpu, Z, Nz, 1.2))


def test_matcher_restatement_equals_python_integers(cpu):
    for m, n in ((1, 1), (3, 7), (40, 65), (65, 40)):
        fa, fb = FH.random_tables(m, n)
        for mutual in (True, False):
            got, want = cpu.match(fa, fb, mutual), FH.numpy_match(fa, fb, mutual)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (m, n, mutual)
    fa, fb = FH.random_tables(30, 50, zero_rows=False)
    fb[40] = fb[3] = fa[10]; fa[20] = 0; fb[0] = 0
    idx, dist = cpu.match(fa, fb, False)
    assert idx[10] == 3 and dist[10] == 0 and idx[20] == -1 and dist[20] == -1 and not (idx == 0).any()
    assert np.array_equal(idx, FH.numpy_match(fa, fb, False)[0])
    for other in (np.zeros((5, 33), np.uint16), np.zeros((0, 33), np.uint16)):
        assert (cpu.match(fa, other)[0] == -1).all() and (cpu.match(other, fa)[0] == -1).all()
    fa[2, 5] = 4097
    assert cpu.match(fa, fb) is None and cpu.match(fb, fa) is None


def test_quality_of_the_matches_on_the_registration_pair(pair):
    """bumpy_pair(3000, noise_sigma=0.001), r = 0.08: the share of mutual matches that lie within r of each other under the
    generator's pose is at least 3 x the mean share of the same matches with B's indices permuted (20 seeds), and there are
    at least 100 matches.  The restatement gives 490 matches and 14.3 % against 2.1 % (the largest of the 20: 2.9 %)."""
    P, Q, T, M = pair["P"], pair["Q"], pair["T"], pair["M"]
    r = FH.PAIR["radius"]
    Qm = Q.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    share = float((np.linalg.norm(P[M[:, 0]] - Qm[M[:, 1]], axis=1) <= r).mean())
    perm = [float((np.linalg.norm(P[M[:, 0]] - Qm[M[np.random.default_rng(s).permutation(len(M)), 1]], axis=1) <= r).mean()) for s in range(20)]
    print("mutual matches %d, within r %.1f %%, permuted mean %.1f %% max %.1f %%" % (len(M), 100 * share, 100 * np.mean(perm), 100 * max(perm)))
    assert len(M) >= 100
    assert share >= 3 * np.mean(perm)
    assert np.array_equal(M[:, 0], np.sort(M[:, 0])) and len(set(M[:, 1])) == len(M)            # ascending a; mutual: no b twice


def _rigid(seed):
    rng = np.random.default_rng(seed)
    A = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    if np.linalg.det(A) < 0:
        A[:, 0] = -A[:, 0]
    T = np.eye(4)
    T[:3, :3] = A; T[:3, 3] = rng.uniform(-1, 1, 3)
    return T


def test_poses_from_matches_recovers_planted_poses(ft):
    rng = np.random.default_rng(5)
    T = _rigid(6)
    P = rng.uniform(-1, 1, (200, 3))
    Q = (P - T[:3, 3]) @ T[:3, :3]                                # T Q = P
    M = np.stack([np.arange(200), np.arange(200)], 1)
    T0 = ft.poses_from_matches(P, Q, M, 0.05)
    assert T0.shape == (16, 4, 4) and T0.dtype == np.float64 and np.abs(T0[0] - T).max() < 1e-9
    assert np.array_equal(T0, ft.poses_from_matches(P, Q, M, 0.05)) and ft.poses_from_matches(P, Q, M, 0.05, starts=3).shape == (3, 4, 4)
    # 30 % planted, 70 % random partners
    M2 = M.copy()
    wrong = rng.permutation(200)[:140]
    M2[wrong, 1] = rng.integers(0, 200, 140)
    T0 = ft.poses_from_matches(P, Q, M2, 0.05, seed=1)
    assert len(T0) >= 1 and FH.rotation_angle_deg(T0[0], T) < 1.0 and np.abs(T0[0][:3, 3] - T[:3, 3]).max() < 0.05
    # nothing but short edges: no candidate
    assert ft.poses_from_matches(P * 1e-3, Q * 1e-3, M, 0.05).shape == (0, 4, 4)


def test_poses_from_matches_on_the_registration_pair(ft, pair):
    """At least one of the first 16 candidates is within 10 degrees of the generator's rotation (the restatement's matches
    give 3.5 and 6.3 degrees first)."""
    T0 = ft.poses_from_matches(pair["P"], pair["Q"], pair["M"], FH.PAIR["max_distance"])
    ang = [FH.rotation_angle_deg(t, pair["T"]) for t in T0]
    print("angles to the generator's rotation:", " ".join("%.1f" % a for a in ang))
    assert 1 <= len(T0) <= 16 and min(ang) < 10.0
