"""FPFH descriptors and the feature matcher on the MI355X (include/s4p_feature.h): descriptor rows and counts equal the
restatement (tests/feature_cpu through tests/feature_helpers.py) bit for bit: at the edges of the wave and the workgroup; on
524 289 points; with both ring choices of the grid; with distances on the rim; on duplicates, a pair stacked along its normals,
invalid normals, saturated weights, a ball where every point pairs with every other, a cloud at 1e4 and one scaled by 2^-40;
with a null count; twice and in both forms; every refusal; the context's other calls before and after.  The matcher equals its
restatement over ragged row and column tiles, on ties, rows of zeros, the largest distance, a refused value, m = 0, and on the
real descriptors of the registration pair; the facade program equals the Python path."""
import subprocess

import numpy as np
import pytest

from tests import apps
from tests import feature_helpers as FH
from tests import normals_helpers as NH
from tests import normals_suite as S
from tests import shape_helpers as SH

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ft():
    return S.normals_module("features")


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return FH.build_cpu(tmp_path_factory.mktemp("feature_cpu"))


@pytest.fixture(scope="module")
def pair(cpu, tmp_path_factory):
    """The registration pair of the host test: clouds, outward normals, the restatement's descriptors and mutual matches."""
    P, Q, T = FH.pair_clouds()
    Pn, Qn = FH.pair_normals(SH.build_cpu(tmp_path_factory.mktemp("shape_cpu")))
    Fp, Fq = cpu.fpfh(P, Pn, FH.PAIR["radius"]), cpu.fpfh(Q, Qn, FH.PAIR["radius"])
    return dict(P=P, Q=Q, Pn=Pn, Qn=Qn, Fp=Fp, Fq=Fq, match=cpu.match(Fp[0], Fq[0], True))


def _same(ctx, cpu, X, N, what, radius):
    """One fpfh call equals the restatement.  Returns the call's (F, count)."""
    got = ctx.fpfh(N, radius)
    want = cpu.fpfh(X, N, radius)
    assert got[0].dtype == np.uint16 and got[0].shape == (len(X), 33) and got[1].dtype == np.int32 and got[1].shape == (len(X),)
    print(what, "rows", len(X), "count median", np.median(got[1]), "max", got[1].max(), "rows of zeros", int((~got[0].any(1)).sum()))
    assert FH.same(got, want), (what, FH.differing(got, want))
    assert got[0].max(initial=0) <= 4096
    return got


def _ctx(ft, X):
    ctx = ft.Features(0)
    ctx.set_cloud(X)
    return ctx


@pytest.mark.parametrize("n", FH.SIZES)
def test_sizes_at_the_edges_equal_the_restatement(ft, cpu, n):
    X = FH.cube_cloud(n)
    N = FH.random_normals(n)
    ctx = _ctx(ft, X)
    F, cnt = _same(ctx, cpu, X, N, (n, "20"), FH.cube_radius(n))
    Fb, cb = _same(ctx, cpu, X, N, (n, "beyond"), SH.BEYOND)
    if n >= 63:
        assert 8 < np.median(cnt) < 40 and cb.min() >= n - n // 10 - 2 and Fb.any(1).all()
        sums = F.reshape(n, 3, 11).sum(2)
        assert ((sums == 0) | ((sums > 4096 - 11) & (sums <= 4096))).all()        # eleven floors lose less than eleven
    ctx.close()


def test_one_large_size_numpy_and_torch(ft, cpu):
    """524 289 points: above 2048 x 256 a lane takes a second and a third trip; the grid of edge r does not fit the cell cap."""
    import torch
    X = FH.large_cloud()
    N = FH.radial_normals(X, (0, 0, 0))
    assert len(X) == 524_289
    ctx = _ctx(ft, X)
    F, cnt = _same(ctx, cpu, X, N, "large", FH.LARGE_RADIUS)
    assert 8 <= np.median(cnt) <= 16 and F.any(1).mean() > 0.999
    ctx.close()
    t = _ctx(ft, S.to_device(X))
    Ft, ct = t.fpfh(S.to_device(N), FH.LARGE_RADIUS)
    assert Ft.is_cuda and Ft.dtype == torch.uint16 and ct.dtype == torch.int32 and FH.same((Ft, ct), (F, cnt))
    t.close()


def test_both_ring_choices_of_the_grid(ft, cpu):
    """Two clusters 1e-3 wide and 4 apart.  At r = 2 the grid of edge r / 2 has a few cells (two rings); at 3e-4 and 2e-3 neither
    that grid nor the one of edge r fits the cell cap: one ring on an enlarged grid."""
    X = SH.two_far_clusters()
    N = FH.random_normals(len(X), 1)
    ctx = _ctx(ft, X)
    assert 3 < np.median(_same(ctx, cpu, X, N, "far clusters", 3.0e-4)[1]) < 100
    _same(ctx, cpu, X, N, "far clusters, one ball", 2.0e-3)
    assert (_same(ctx, cpu, X, N, "two rings", 2.0)[1] >= 290).all()
    ctx.close()
    X = FH.cube_cloud(4097)
    ctx = _ctx(ft, X)
    _same(ctx, cpu, X, FH.random_normals(4097, 2), "two rings, 4097", 0.125)
    _same(ctx, cpu, X, FH.random_normals(4097, 2), "one ring, 4097", 0.015)
    ctx.close()


def test_lattice_distances_on_the_rim(ft, cpu):
    L = FH.lattice_cloud()
    N = FH.random_normals(len(L), 3)
    inner = ((L > 0) & (L < 7)).all(1)
    ctx = _ctx(ft, L)
    assert (_same(ctx, cpu, L, N, "lattice 1", 1.0)[1][inner] == 6).all()
    F, cnt = _same(ctx, cpu, L, N, "lattice below 1", FH.below(1.0))
    assert not cnt.any() and not F.any()
    ctx.close()


def test_duplicates_stacked_pairs_and_invalid_normals(ft, cpu):
    X = SH.identical_cloud()
    ctx = _ctx(ft, X)
    F, cnt = _same(ctx, cpu, X, FH.random_normals(len(X), 4), "identical", 0.5)
    assert not F.any() and not cnt.any()
    # two points stacked along their common normal: v = d x n = 0, the pair is skipped; the third point pairs with both
    X = np.array([[0, 0, 0], [0, 0, 0.5], [0.25, 0, 0]], np.float32)
    N = np.tile(np.array([[0, 0, 1]], np.float32), (3, 1))
    ctx.set_cloud(X)
    F, cnt = _same(ctx, cpu, X, N, "stacked", 1.0)
    assert list(cnt) == [1, 1, 2] and F.any(1).all()
    ctx.set_cloud(X[:2])
    F, cnt = _same(ctx, cpu, X[:2], N[:2], "stacked alone", 1.0)
    assert not cnt.any() and not F.any()
    # zero, NaN, infinite, underflowing, overflowing and far-from-unit normals in a cloud
    X = FH.cube_cloud(257)
    N, bad = FH.mixed_normals(257)
    ctx.set_cloud(X)
    F, cnt = _same(ctx, cpu, X, N, "mixed normals", 0.3)
    assert not F[bad].any() and not cnt[bad].any() and np.median(cnt) > 10
    # a point that is not finite never reaches the call: set_cloud refuses the cloud
    Xn = X.copy(); Xn[5, 1] = np.nan
    with pytest.raises(ft.NormalsError) as e:
        ctx.set_cloud(Xn)
    assert e.value.code == -1
    ctx.close()


def test_weight_saturation_and_a_ball_inside_one_radius(ft, cpu):
    """A neighbour at exactly r / 32 (64 r^2 / d2 = 65536 on the nose), nearer ones and farther ones; then 300 points that all
    pair with each other, so that every counter passes 256."""
    rng = np.random.default_rng(17)
    X = np.concatenate([np.array([[0, 0, 0], [1 / 32, 0, 0], [0, -1 / 64, 0], [0, 0, 1 / 1024], [0, 1 / 32, 1 / 1024]], np.float32),
                        rng.uniform(-0.6, 0.6, (60, 3)).astype(np.float32)])
    N = FH.random_normals(len(X), 6)
    ctx = _ctx(ft, X)
    _, cnt = _same(ctx, cpu, X, N, "saturation", 1.0)
    d2 = ((X[1:5] - X[0]) ** 2).sum(1)
    q = np.minimum(np.float32(64) * (np.float32(1) / d2), np.float32(65536))
    assert list(q.astype(np.int64)) == [65536, 65536, 65536, 65472] and cnt[0] >= 4
    B = FH.ball_cloud()
    ctx.set_cloud(B)
    _, cnt = _same(ctx, cpu, B, FH.random_normals(len(B), 7), "ball", 0.8)
    assert cnt.min() > 256 and cnt.max() == 299
    ctx.close()


def test_translated_and_scaled_clouds(ft, cpu):
    X = (FH.cube_cloud(4097) + np.float32(1.0e4)).astype(np.float32)
    ctx = _ctx(ft, X)
    _same(ctx, cpu, X, FH.random_normals(4097, 8), "at 1e4", 0.125)
    Z = FH.scale_cloud()
    N = FH.random_normals(len(Z), 9)
    ctx.set_cloud(Z)
    base = _same(ctx, cpu, Z, N, "scale 1", 1.2)
    assert 20 < np.median(base[1]) < 60
    f = np.float32(2.0 ** -40)
    ctx.set_cloud(Z * f)
    assert FH.same(_same(ctx, cpu, Z * f, N, "scale 2^-40", np.float32(1.2) * f), base)      # every feature is a ratio
    ctx.close()


def test_null_count_both_forms_and_two_calls(ft, cpu):
    import torch
    X = FH.cube_cloud(4097, seed=1)
    N = FH.random_normals(4097, 10)
    r = float(FH.cube_radius(4097))
    want = cpu.fpfh(X, N, r)
    ctx = _ctx(ft, X)
    L = ft.load_library()
    F = np.full((4097, 33), 7, np.uint16)
    assert L.s4p_feature_fpfh(ctx.h, N.ctypes.data, r, F.ctypes.data, None) == 0 and np.array_equal(F, want[0])
    a, b = ctx.fpfh(N, r), ctx.fpfh(N, r)
    assert FH.same(a, want) and FH.same(a, b) and not FH.same(a, ctx.fpfh(N, 1.5 * r))
    ctx.close()
    t = _ctx(ft, S.to_device(X))
    d = t.fpfh(S.to_device(N), r)
    assert d[0].is_cuda and d[0].dtype == torch.uint16 and FH.same(d, want)
    Fd = torch.full((4097, 33), 7, dtype=torch.uint16, device="cuda")
    nd = S.to_device(N)
    torch.cuda.synchronize()
    assert L.s4p_feature_fpfh_device(t.h, nd.data_ptr(), r, Fd.data_ptr(), None) == 0 and np.array_equal(Fd.cpu().numpy(), want[0])
    t.close()


def test_compute_fpfh_orients_by_default(ft):
    """Without normals: Shape.estimate(radius / 2), Normals.orient outward and fpfh on one context; orient=None skips the
    orientation, and the descriptors differ."""
    P = FH.pair_clouds()[0]
    r = FH.PAIR["radius"]
    ctx = _ctx(ft, P)
    N = ctx.estimate(r / 2)[0]
    want = ctx.fpfh(ctx.orient(N, 8), r)
    raw = ctx.fpfh(N, r)
    ctx.close()
    assert FH.same(ft.compute_fpfh(P, r), want) and FH.same(ft.compute_fpfh(P, r, normal_radius=r / 2, orient="outward"), want)
    assert FH.same(ft.compute_fpfh(P, r, orient=None), raw) and not FH.same(raw, want)
    assert FH.same(ft.compute_fpfh(P, r, normals=N), raw)
    with pytest.raises(ValueError):
        ft.compute_fpfh(P, r, orient="inward")
    with pytest.raises(ValueError):
        ft.compute_fpfh(P, r, normals=N, normal_radius=0.1)


def test_other_calls_on_the_context_are_unchanged_after_a_feature_call(ft):
    from super4pcs_amd import normals
    from tests import cluster_helpers as CH
    X = CH.lidar_cloud()
    ctx = _ctx(ft, X)
    g0 = ctx.grid()
    n0 = normals.Normals.estimate(ctx, 16)
    i0, d0, c0 = ctx.search(8, exclude_self=True)
    s0 = ctx.estimate(0.5)
    first = ctx.fpfh(FH.radial_normals(X), 0.5)
    fa, fb = FH.random_tables(300, 500)
    ctx.match(fa, fb)
    ctx.fpfh(FH.random_normals(len(X), 11), 0.3)
    assert ctx.grid() == g0
    assert np.array_equal(NH.bits(normals.Normals.estimate(ctx, 16)), NH.bits(n0))
    i1, d1, c1 = ctx.search(8, exclude_self=True)
    assert np.array_equal(i1, i0) and np.array_equal(NH.bits(d1), NH.bits(d0)) and np.array_equal(c1, c0)
    assert SH.same(ctx.estimate(0.5), s0)
    assert FH.same(ctx.fpfh(FH.radial_normals(X), 0.5), first)
    ctx.close()


def test_refusals(ft):
    X = np.random.default_rng(1).uniform(size=(100, 3)).astype(np.float32)
    N = FH.random_normals(100, 12)
    ctx = ft.Features(0)
    L, h = ft.load_library(), ctx.h
    F = np.full((100, 33), 7, np.uint16); cnt = np.full(100, 7, np.int32)
    for fn in (L.s4p_feature_fpfh, L.s4p_feature_fpfh_device):
        assert fn(h, N.ctypes.data, 0.1, F.ctypes.data, cnt.ctypes.data) == -7 and b"set_cloud first" in L.s4p_normals_last_error(h)
    ctx.set_cloud(X)
    for i, r in enumerate((float("nan"), float("inf"), 0.0, -0.1, 1e-20, 1e20)):
        with pytest.raises(ft.NormalsError) as e:
            ctx.fpfh(N, r)
        assert e.value.code == -1 and len(str(e.value)) > 30, i
    for fn in (L.s4p_feature_fpfh, L.s4p_feature_fpfh_device):
        assert fn(h, None, 0.1, F.ctypes.data, cnt.ctypes.data) == -1 and b"null normals" in L.s4p_normals_last_error(h)
        assert fn(h, N.ctypes.data, 0.1, None, cnt.ctypes.data) == -1 and b"null fpfh" in L.s4p_normals_last_error(h)
        assert fn(None, N.ctypes.data, 0.1, F.ctypes.data, cnt.ctypes.data) == -1
    assert (F == 7).all() and (cnt == 7).all()
    with pytest.raises(ValueError):
        ctx.fpfh(N[:50], 0.1)
    # the limits themselves are allowed
    assert not ctx.fpfh(N, 1.1e-19)[1].any() and (ctx.fpfh(N, 1.8e19)[1] >= 98).all()
    # the matcher: on a context with and without a cloud
    fa, fb = FH.random_tables(20, 30)
    idx = np.full(20, 7, np.int32); dist = np.full(20, 7, np.int32)
    fresh = ft.Features(0)
    for hh in (h, fresh.h):
        for fn in (L.s4p_feature_match, L.s4p_feature_match_device):
            for m, n in ((-1, 30), (2 ** 31 - 1, 30), (20, -1), (20, 2 ** 31 - 1), (2 ** 40, 30)):
                assert fn(hh, fa.ctypes.data, m, fb.ctypes.data, n, 1, idx.ctypes.data, dist.ctypes.data) == -1 and b"m and n must" in L.s4p_normals_last_error(hh)
            assert fn(hh, None, 20, fb.ctypes.data, 30, 1, idx.ctypes.data, dist.ctypes.data) == -1 and b"null" in L.s4p_normals_last_error(hh)
            assert fn(hh, fa.ctypes.data, 20, None, 30, 1, idx.ctypes.data, dist.ctypes.data) == -1
            assert fn(hh, fa.ctypes.data, 20, fb.ctypes.data, 30, 1, None, dist.ctypes.data) == -1
            assert fn(None, fa.ctypes.data, 20, fb.ctypes.data, 30, 1, idx.ctypes.data, dist.ctypes.data) == -1
            assert fn(hh, None, 0, None, 0, 1, None, None) == 0 and fn(hh, None, 0, fb.ctypes.data, 30, 0, None, None) == 0      # m = 0: nothing touched
    assert (idx == 7).all() and (dist == 7).all()
    # a value of 4097 in either table, anywhere: refused before anything is written
    for which, row, col in ((0, 0, 0), (0, 19, 32), (1, 29, 32), (1, 7, 15)):
        ta, tb = fa.copy(), fb.copy()
        (ta, tb)[which][row, col] = 4097
        with pytest.raises(ft.NormalsError) as e:
            fresh.match(ta, tb)
        assert e.value.code == -1 and "4096" in str(e.value)
        assert L.s4p_feature_match(fresh.h, ta.ctypes.data, 20, tb.ctypes.data, 30, 1, idx.ctypes.data, dist.ctypes.data) == -1
        (ta, tb)[which][row, col] = 4096
        fresh.match(ta, tb)
    assert (idx == 7).all() and (dist == 7).all()
    with pytest.raises(ValueError):
        fresh.match(fa.astype(np.int16), fb)
    with pytest.raises(ValueError):
        fresh.match(fa[:, :32], fb)
    fresh.close()
    ctx.close()


def _match_same(ctx, cpu, fa, fb, what):
    for mutual in (True, False):
        want = cpu.match(fa, fb, mutual)
        got = ctx.match(fa, fb, mutual)
        assert got[0].dtype == np.int32 and got[1].dtype == np.int32
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (what, mutual, int((got[0] != want[0]).sum()))
    return got


@pytest.mark.parametrize("m", [1, 63, 64, 65, 257, 1025])
def test_matcher_over_ragged_row_and_column_tiles(ft, cpu, m):
    import torch
    ctx = ft.Features(0)
    for n in (1, 64, 65, 1025, 4097):
        fa, fb = FH.random_tables(m, n)
        idx, dist = _match_same(ctx, cpu, fa, fb, (m, n))
        assert (idx >= 0).sum() >= m - 1
    want = cpu.match(fa, fb, True)
    ti, td = ctx.match(torch.from_numpy(fa).cuda(), torch.from_numpy(fb).cuda(), True)
    assert ti.is_cuda and ti.dtype == torch.int32 and np.array_equal(ti.cpu().numpy(), want[0]) and np.array_equal(td.cpu().numpy(), want[1])
    ctx.close()


def test_matcher_ties_rows_of_zeros_and_a_null_dist(ft, cpu):
    ctx = ft.Features(0)
    L = ft.load_library()
    fa, fb = FH.random_tables(100, 300, seed=1, zero_rows=False)
    fb[200] = fb[3] = fa[10]; fb[250] = fb[100] = fb[50] = fa[11]            # identical rows of B: the smallest index wins
    fa[20] = 0; fa[99] = 0; fb[0] = 0; fb[299] = 0; fb[64] = 0
    idx, dist = _match_same(ctx, cpu, fa, fb, "ties")
    assert idx[10] == 3 and idx[11] == 50 and dist[10] == 0 and idx[20] == -1 and dist[20] == -1 and idx[99] == -1
    assert not np.isin(idx, [0, 64, 299]).any()
    want = FH.numpy_match(fa[:24], fb[:70], True)
    assert np.array_equal(ctx.match(fa[:24], fb[:70], True)[0], want[0])
    # A's identical rows: mutual keeps the smallest index of A
    fa[30] = fa[31] = fb[151]
    idx, _ = _match_same(ctx, cpu, fa, fb, "ties in A")
    assert ctx.match(fa, fb, True)[0][30] == 151 and ctx.match(fa, fb, True)[0][31] == -1 and idx[31] == 151
    # B entirely zero, B empty, A entirely zero
    for other in (np.zeros((40, 33), np.uint16), np.zeros((0, 33), np.uint16)):
        idx, dist = _match_same(ctx, cpu, fa, other, "zero B")
        assert (idx == -1).all() and (dist == -1).all()
    idx, dist = _match_same(ctx, cpu, np.zeros((40, 33), np.uint16), fb, "zero A")
    assert (idx == -1).all() and (dist == -1).all()
    # dist null
    want = cpu.match(fa, fb, True)
    idx = np.full(100, 7, np.int32)
    assert L.s4p_feature_match(ctx.h, fa.ctypes.data, 100, fb.ctypes.data, 300, 1, idx.ctypes.data, None) == 0 and np.array_equal(idx, want[0])
    ctx.close()


def test_matcher_largest_distances_do_not_wrap(ft, cpu):
    """Rows of 4096 e_k against a row of zeros but one, in another bin: D = 4096^2 + 1 needs more than 16 and 24 bits; rows of
    4096 everywhere against it: 32 * 4096^2 + 4095^2, the largest D between usable rows, needs 30."""
    eye = (np.eye(33, dtype=np.uint16) * 4096).astype(np.uint16)
    last = np.zeros((2, 33), np.uint16)
    last[:, 32] = 1                                              # two identical rows: index 0 wins
    full = np.full((3, 33), 4096, np.uint16)
    ctx = ft.Features(0)
    idx, dist = _match_same(ctx, cpu, eye[:32], last, "e_k")
    assert (dist == 4096 ** 2 + 1).all() and (idx == 0).all()
    idx, dist = _match_same(ctx, cpu, full, last, "full")
    assert (dist == 32 * 4096 ** 2 + 4095 ** 2).all() and (idx == 0).all()
    A, B = np.concatenate([eye, full]), np.concatenate([last, full, eye])
    idx, dist = _match_same(ctx, cpu, A, B, "mixed")
    want = FH.numpy_match(A, B, False)
    assert np.array_equal(idx, want[0]) and np.array_equal(dist, want[1])
    ctx.close()


def test_real_descriptors_of_the_pair_and_their_matches(ft, cpu, pair):
    ctx = _ctx(ft, pair["P"])
    Fp = ctx.fpfh(pair["Pn"], FH.PAIR["radius"])
    ctx.set_cloud(pair["Q"])
    Fq = ctx.fpfh(pair["Qn"], FH.PAIR["radius"])
    assert FH.same(Fp, pair["Fp"]), FH.differing(Fp, pair["Fp"])
    assert FH.same(Fq, pair["Fq"]), FH.differing(Fq, pair["Fq"])
    idx, dist = ctx.match(Fp[0], Fq[0], True)
    assert np.array_equal(idx, pair["match"][0]) and np.array_equal(dist, pair["match"][1])
    M = ft.match_features(Fp[0], Fq[0])
    assert M.dtype == np.int32 and np.array_equal(M, FH.pairs_of(pair["match"][0])) and len(M) >= 100
    import torch
    Mt = ft.match_features(torch.from_numpy(Fp[0]).cuda(), torch.from_numpy(Fq[0]).cuda())
    assert Mt.is_cuda and np.array_equal(Mt.cpu().numpy(), M)
    ctx.close()


def test_the_facade_program_equals_the_python_path(ft, cpu, pair, tmp_path):
    exe = apps.build_app(tmp_path, "feature_app", S.NORMALS_LIBS, ["-Werror"])
    r = FH.PAIR["radius"]
    P, Q = pair["P"][:1500], pair["Q"][:1500]
    Pn, Qn = NH.point3d_normalise(pair["Pn"][:1500]), NH.point3d_normalise(pair["Qn"][:1500])
    Pn[7] = 0                                                    # a point without a normal: a row of zeros
    ctx = _ctx(ft, P)
    Fp = ctx.fpfh(Pn, r)[0]
    ctx.set_cloud(Q)
    Fq = ctx.fpfh(Qn, r)[0]
    ctx.close()
    assert np.array_equal(Fp, cpu.fpfh(P, Pn, r)[0]) and not Fp[7].any()
    apps.write_xyz(tmp_path / "P.xyzn", np.concatenate([P, Pn], 1)); apps.write_xyz(tmp_path / "Q.xyzn", np.concatenate([Q, Qn], 1))
    out = subprocess.run([exe, "fpfh", str(tmp_path / "P.xyzn"), repr(r)], capture_output=True, text=True, timeout=apps.TIMEOUT)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0] == "none %d" % int((~Fp.any(1)).sum())
    assert np.array_equal(np.array([[int(v) for v in ln.split()] for ln in lines[1:]], np.uint16), Fp)
    for mutual in (1, 0):
        out = subprocess.run([exe, "match", str(tmp_path / "P.xyzn"), str(tmp_path / "Q.xyzn"), repr(r), str(mutual)], capture_output=True, text=True,
                             timeout=apps.TIMEOUT)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        want = ft.match_features(Fp, Fq, bool(mutual))
        assert lines[0] == "matches %d" % len(want) and len(want) > 20
        assert np.array_equal(np.array([[int(v) for v in ln.split()] for ln in lines[1:]], np.int32).reshape(-1, 2), want)
