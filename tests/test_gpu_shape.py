"""Radius normals on the MI355X (include/s4p_shape.h): normal, eigenvalues and count equal the restatement (tests/shape_cpu
through tests/shape_helpers.py) bit for bit: at the edges of the wave and the workgroup with about 20 neighbours and with a
radius beyond the extent, where 20 000 neighbours push the moment sums past 2^32; on a lattice with distances on the bound; at
a power-of-two radius and the float below it; on identical, collinear and coplanar points; on a cloud at 1e4 and on clouds
scaled by 2^40 and 2^-40; on two far clusters whose grid is enlarged; over min_neighbours; at query positions on, around and
far from the cloud; on 524 289 points with numpy and torch; on the 3000 planted queries; with null outputs; twice and in both
forms; every refusal; the context's other calls before and after; the facade program and the command line."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import apps
from tests import helpers as H
from tests import normals_helpers as NH
from tests import normals_suite as S
from tests import shape_helpers as SH

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shp():
    return S.normals_module("shape")


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return SH.build_cpu(tmp_path_factory.mktemp("shape_cpu"))


def _same(ctx, cpu, X, what, radius, min_neighbours=3, queries=None):
    """One estimate call equals the restatement.  Returns the call's (normals, eig, count)."""
    got = ctx.estimate(radius, min_neighbours, queries)
    want = cpu.estimate(X, radius, min_neighbours, queries)
    rows = len(X) if queries is None else len(queries)
    assert got[0].dtype == np.float32 and got[0].shape == (rows, 3) and got[1].dtype == np.float32 and got[1].shape == (rows, 3)
    assert got[2].dtype == np.int32 and got[2].shape == (rows,)
    print(what, "rows", rows, "count median", np.median(got[2]) if rows else None, "max", got[2].max() if rows else None,
          "without a normal", int((~got[0].any(1)).sum()))
    assert SH.same(got, want), (what, SH.differing(got, want))
    return got


@pytest.mark.parametrize("n", SH.SIZES)
def test_sizes_at_the_edges_equal_the_restatement(shp, cpu, n):
    """n at the wave, at 256 and around it and above 4096, with about 20 neighbours and with the whole cloud in every ball."""
    X = SH.cube_cloud(n)
    ctx = shp.Shape(0)
    ctx.set_cloud(X)
    N, E, cnt = _same(ctx, cpu, X, (n, "20"), SH.cube_radius(n))
    Nb, Eb, cb = _same(ctx, cpu, X, (n, "beyond"), SH.BEYOND)
    assert (cb == n).all() and (cnt >= 1).all() and not N[cnt < 3].any() and not E[cnt < 3].any()
    if n >= 63:
        assert 10 < np.median(cnt) < 40 and Nb.any(1).all()
    ctx.close()


def test_moment_sums_pass_two_to_the_32(shp, cpu):
    X = SH.moment_cloud()
    ctx = shp.Shape(0)
    ctx.set_cloud(X)
    N, E, cnt = _same(ctx, cpu, X, "20000 beyond", SH.BEYOND)
    mom = cpu.estimate(X, SH.BEYOND, queries=X[:4], moments=True)[3]
    assert (cnt == len(X)).all() and len(X) == 20000 and mom[:, 4].min() > 1 << 32 and N.any(1).all()
    ctx.close()


def test_lattice_distances_on_the_bound_count(shp, cpu):
    L = SH.lattice_cloud()
    inner = ((L > 0) & (L < 7)).all(1)
    ctx = shp.Shape(0)
    ctx.set_cloud(L)
    assert (_same(ctx, cpu, L, "lattice 1", 1.0)[2][inner] == 7).all()
    N, E, cnt = _same(ctx, cpu, L, "lattice below 1", SH.below(1.0))
    assert (cnt == 1).all() and not N.any() and not E.any()
    ctx.close()


def test_radius_at_a_power_of_two_and_the_float_below(shp, cpu):
    X = SH.cube_cloud(4097)
    ctx = shp.Shape(0)
    ctx.set_cloud(X)
    assert SH.scale_exponent(0.125) == 21 and SH.scale_exponent(SH.below(0.125)) == 22
    a = _same(ctx, cpu, X, "2^-3", 0.125)
    b = _same(ctx, cpu, X, "below 2^-3", SH.below(0.125))
    assert np.array_equal(a[2], b[2]) and not np.array_equal(NH.bits(a[1]), NH.bits(b[1]))
    # each offset moves by at most half a step, r 2^-19, so an entry of C by at most 4 r (r 2^-19) + 2 (r 2^-19)^2 and an eigenvalue by at
    # most three times that (Weyl, a 3 x 3 matrix): below r^2 2^-15; a normal may turn freely where two eigenvalues nearly coincide
    assert np.abs(a[1].astype(np.float64) - b[1]).max() < 0.125 ** 2 * 2.0 ** -15
    # the largest quantised offset: a neighbour at distance r, r the float below 1
    r = SH.below(1.0)
    T = np.array([[0, 0, 0], [r, 0, 0], [0, -r, 0], [0, 0, r], [1, 0, 0], [0.5, 0.5, 0.5]], np.float32)
    ctx.set_cloud(T)
    assert _same(ctx, cpu, T, "u = 2^19", r)[2][0] == 5
    ctx.close()


def test_identical_collinear_and_coplanar_points(shp, cpu):
    ctx = shp.Shape(0)
    X = SH.identical_cloud()
    ctx.set_cloud(X)
    N, E, cnt = _same(ctx, cpu, X, "identical", 0.5)
    assert (cnt == 100).all() and not N.any() and not E.any()
    X = SH.collinear_cloud()
    ctx.set_cloud(X)
    N, E, cnt = _same(ctx, cpu, X, "collinear", 0.3)
    assert N.any(1).all() and np.abs(N.astype(np.float64) @ (np.array([1, 2, -3]) / np.sqrt(14.0))).max() < 1e-6
    X = SH.coplanar_cloud()
    ctx.set_cloud(X)
    N, E, cnt = _same(ctx, cpu, X, "coplanar", 0.2)
    assert np.array_equal(N, np.tile(np.array([0, 0, 1], np.float32), (len(X), 1))) and np.abs(E[:, 2]).max() == 0
    ctx.close()


def test_translated_and_scaled_clouds(shp, cpu):
    ctx = shp.Shape(0)
    X = (SH.cube_cloud(4097) + np.float32(1.0e4)).astype(np.float32)
    ctx.set_cloud(X)
    _same(ctx, cpu, X, "at 1e4", 0.125)
    Z = SH.scale_cloud()
    ctx.set_cloud(Z)
    base = _same(ctx, cpu, Z, "scale 1", 1.2)
    assert 20 < np.median(base[2]) < 60
    for e in (40, -40):
        f = np.float32(2.0 ** e)
        ctx.set_cloud(Z * f)
        got = _same(ctx, cpu, Z * f, "scale 2^%d" % e, np.float32(1.2) * f)
        assert np.array_equal(got[2], base[2]) and np.array_equal(NH.bits(got[0]), NH.bits(base[0]))
        assert np.array_equal(NH.bits(got[1]), NH.bits(base[1] * f * f))                  # the eigenvalues scale by exactly 2^80 and 2^-80
    ctx.close()


def test_two_far_clusters_at_a_tiny_radius(shp, cpu):
    """The grid of edge r would have (4 / 3e-4)^3 cells: it is enlarged until it fits, and a block of 27 cells then holds a
    whole cluster."""
    F = SH.two_far_clusters()
    ctx = shp.Shape(0)
    ctx.set_cloud(F)
    N, E, cnt = _same(ctx, cpu, F, "far clusters", 3.0e-4)
    assert 3 < np.median(cnt) < 100 and cnt.max() < 300
    _same(ctx, cpu, F, "far clusters, one ball", 2.0e-3)
    ctx.close()


def test_min_neighbours_at_below_and_above_a_rows_count(shp, cpu):
    X = SH.cube_cloud(257)
    r = SH.cube_radius(257)
    ctx = shp.Shape(0)
    ctx.set_cloud(X)
    base = _same(ctx, cpu, X, "min 3", r)
    i = int(np.argmax(base[2]))
    c = int(base[2][i])
    assert c >= 4
    for mn, has in ((c - 1, True), (c, True), (c + 1, False), (1, True), (2, True), (2 ** 31 - 1, False)):
        got = _same(ctx, cpu, X, ("min", mn), r, mn)
        assert np.array_equal(got[2], base[2]) and got[0][i].any() == has and got[1][i].any() == has
    ctx.close()


def test_queries_on_around_and_far_from_the_cloud(shp, cpu):
    X = SH.cube_cloud(4097)
    r = SH.cube_radius(4097)
    h = 1.0001 * float(r)
    ctx = shp.Shape(0)
    ctx.set_cloud(X)
    own = ctx.estimate(r)
    around = [[-0.5 * h, 0.5, 0.5], [1 + 0.5 * h, 0.5, 0.5], [0.5, -1.5 * h, 0.5], [0.5, 0.5, 1 + 1.5 * h], [0.5, 1 + 2.5 * h, 0.5],
              [-0.9 * h, -0.9 * h, -0.9 * h], [1 + 0.3 * h, 1 + 0.3 * h, 1 + 0.3 * h]]
    far = [[50, 50, 50], [-3e38, 0, 0], [1e30, -1e30, 1e30], [np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf]]
    Qs = np.concatenate([X[:300], X[:50] + np.float32(0.01), np.array(around + far, np.float32)]).astype(np.float32)
    N, E, cnt = _same(ctx, cpu, X, "queries", r, queries=Qs)
    assert SH.same((N[:300], E[:300], cnt[:300]), tuple(a[:300] for a in own))         # a query on a cloud point is that point's row
    assert (cnt[-len(far):] == 0).all() and not N[-len(far):].any() and not E[-len(far):].any()
    assert cnt[350:350 + len(around)].max() > 0                                            # positions outside the bounds still have neighbours
    _same(ctx, cpu, X, "queries beyond", SH.BEYOND, queries=Qs)
    empty = ctx.estimate(r, queries=np.zeros((0, 3), np.float32))
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3) and empty[2].shape == (0,)
    ctx.close()


def test_one_large_size_numpy_and_torch(shp, cpu):
    """524 289 points: above 2048 x 256 a lane takes a second and a third trip."""
    import torch
    X = SH.large_cloud()
    assert len(X) == 524_289
    ctx = shp.Shape(0)
    ctx.set_cloud(X)
    N, E, cnt = _same(ctx, cpu, X, "large", SH.LARGE_RADIUS)
    assert 10 < np.median(cnt) < 30 and N.any(1).mean() > 0.999
    ctx.close()
    t = shp.Shape(0)
    t.set_cloud(S.to_device(X))
    Nt, Et, ct = t.estimate(SH.LARGE_RADIUS)
    assert Nt.is_cuda and Nt.dtype == torch.float32 and ct.dtype == torch.int32 and SH.same((Nt, Et, ct), (N, E, cnt))
    q = S.to_device(X[::64].copy())
    Nq, Eq, cq = t.estimate(SH.LARGE_RADIUS, queries=q)
    assert Nq.is_cuda and SH.same((Nq, Eq, cq), (N[::64], E[::64], cnt[::64]))
    t.close()


def test_planted_queries_equal_the_restatement_and_recover_the_normal(shp, cpu):
    Q, qs, truth = SH.planted()
    P = SH.PLANTED
    ctx = shp.Shape(0)
    ctx.set_cloud(Q)
    N, E, cnt = _same(ctx, cpu, Q, "planted", P["radius"], queries=qs)
    ang = SH.angles_deg(N, truth)
    print("median angle %.2f deg, p90 %.2f; neighbours median %d, max %d" % (np.median(ang), np.percentile(ang, 90), np.median(cnt), cnt.max()))
    assert np.median(ang) < P["below_deg"] and 300 < np.median(cnt) < 800
    sv = shp.surface_variation(E)
    assert np.array_equal(NH.bits(sv), NH.bits(SH.surface_variation(E))) and 0.01 < np.median(sv) < 0.2
    ctx.close()


def test_null_eig_and_null_count(shp, cpu):
    X = SH.cube_cloud(257)
    r = float(SH.cube_radius(257))
    want = cpu.estimate(X, r)
    ctx = shp.Shape(0)
    ctx.set_cloud(X)
    L, h = shp.load_library(), ctx.h
    q = S.cols(X)
    for eig_on, count_on in ((False, False), (True, False), (False, True)):
        for at in (False, True):
            N = np.full((257, 3), 7, np.float32); E = np.full((257, 3), 7, np.float32); cnt = np.full(257, 7, np.int32)
            pe, pc = (E.ctypes.data if eig_on else None), (cnt.ctypes.data if count_on else None)
            rc = L.s4p_shape_estimate_at(h, *S.xyzn(q), r, 3, N.ctypes.data, pe, pc) if at else L.s4p_shape_estimate(h, r, 3, N.ctypes.data, pe, pc)
            assert rc == 0 and np.array_equal(NH.bits(N), NH.bits(want[0]))
            assert np.array_equal(NH.bits(E), NH.bits(want[1])) if eig_on else (E == 7).all()
            assert np.array_equal(cnt, want[2]) if count_on else (cnt == 7).all()
    ctx.close()


def test_two_calls_and_both_forms_give_the_same_bits(shp):
    import torch
    X = SH.cube_cloud(4097, seed=1)
    r = SH.cube_radius(4097)
    a = shp.estimate_normals_radius(X, r)
    b = shp.estimate_normals_radius(X, r)
    t = shp.estimate_normals_radius(S.to_device(X), r)
    assert SH.same(a, b) and t[0].is_cuda and t[2].dtype == torch.int32 and SH.same(a, t) and a[0].any(1).mean() > 0.9
    assert not SH.same(a, shp.estimate_normals_radius(X, 1.5 * r))
    qa = shp.estimate_normals_radius(X, r, queries=X[::7])
    qt = shp.estimate_normals_radius(S.to_device(X), r, queries=S.to_device(X[::7].copy()))
    qm = shp.estimate_normals_radius(S.to_device(X), r, queries=X[::7])                       # a device cloud, host queries: host rows
    assert SH.same(qa, tuple(v[::7] for v in a)) and qt[0].is_cuda and SH.same(qa, qt) and isinstance(qm[0], np.ndarray) and SH.same(qa, qm)
    # orient: the same lines, one sign per surface, through the existing orientation on the same context
    ctx = shp.Shape(0)
    ctx.set_cloud(X)
    want = ctx.orient(a[0], 8)
    ctx.close()
    o = shp.estimate_normals_radius(X, r, orient="outward")
    assert np.array_equal(NH.bits(o[0]), NH.bits(want)) and np.array_equal(NH.bits(np.abs(o[0])), NH.bits(np.abs(a[0]))) and SH.same((a[0],) + o[1:], a)
    ot = shp.estimate_normals_radius(S.to_device(X), r, orient="outward")
    assert ot[0].is_cuda and SH.same(o, ot)


def test_other_calls_on_the_context_are_unchanged_after_a_shape_call(shp):
    """Shape.estimate is the radius call; the k-nearest-neighbour estimate of the same context is normals.Normals.estimate."""
    from super4pcs_amd import normals
    from tests import cluster_helpers as CH
    X = CH.lidar_cloud()
    ctx = shp.Shape(0)
    ctx.set_cloud(X)
    g0 = ctx.grid()
    n0 = normals.Normals.estimate(ctx, 16)
    i0, d0, c0 = ctx.search(8, exclude_self=True)
    l0, k0, s0 = ctx.dbscan(0.5, 10)
    p0 = ctx.segment(0.15)
    first = ctx.estimate(0.5)
    ctx.estimate(0.3, 5, queries=X[:1000] + np.float32(0.05))
    ctx.estimate(5.0, queries=X[:10])
    assert ctx.grid() == g0
    assert np.array_equal(NH.bits(normals.Normals.estimate(ctx, 16)), NH.bits(n0))
    i1, d1, c1 = ctx.search(8, exclude_self=True)
    assert np.array_equal(i1, i0) and np.array_equal(NH.bits(d1), NH.bits(d0)) and np.array_equal(c1, c0)
    l1, k1, s1 = ctx.dbscan(0.5, 10)
    assert np.array_equal(l1, l0) and np.array_equal(k1, k0) and s1 == s0
    p1 = ctx.segment(0.15)
    assert np.array_equal(NH.bits(p1[0]), NH.bits(p0[0])) and np.array_equal(p1[1], p0[1])
    assert SH.same(ctx.estimate(0.5), first)
    ctx.close()


def test_refusals(shp):
    X = np.random.default_rng(1).uniform(size=(100, 3)).astype(np.float32)
    ctx = shp.Shape(0)
    L, h = shp.load_library(), ctx.h
    N = np.full((100, 3), 7, np.float32); E = np.full((100, 3), 7, np.float32); cnt = np.full(100, 7, np.int32)
    q = S.cols(X)
    out = (N.ctypes.data, E.ctypes.data, cnt.ctypes.data)
    for fn in (L.s4p_shape_estimate, L.s4p_shape_estimate_device):
        assert fn(h, 0.1, 3, *out) == -7 and b"set_cloud first" in L.s4p_normals_last_error(h)
    for fn in (L.s4p_shape_estimate_at, L.s4p_shape_estimate_at_device):
        assert fn(h, *S.xyzn(q), 0.1, 3, *out) == -7 and b"set_cloud first" in L.s4p_normals_last_error(h)
    ctx.set_cloud(X)
    nan, inf = float("nan"), float("inf")
    bad = [lambda: ctx.estimate(nan), lambda: ctx.estimate(inf), lambda: ctx.estimate(0.0), lambda: ctx.estimate(-0.1), lambda: ctx.estimate(1e-20),
           lambda: ctx.estimate(1e20), lambda: ctx.estimate(0.1, 0), lambda: ctx.estimate(0.1, -3), lambda: ctx.estimate(nan, queries=X),
           lambda: ctx.estimate(1e20, queries=X), lambda: ctx.estimate(0.1, 0, queries=X)]
    for i, call in enumerate(bad):
        with pytest.raises(shp.NormalsError) as e:
            call()
        assert e.value.code == -1 and len(str(e.value)) > 30, i
    for fn in (L.s4p_shape_estimate, L.s4p_shape_estimate_device):
        assert fn(h, 0.1, 3, None, E.ctypes.data, cnt.ctypes.data) == -1 and b"null normal" in L.s4p_normals_last_error(h)
        assert fn(None, 0.1, 3, *out) == -1
    for fn in (L.s4p_shape_estimate_at, L.s4p_shape_estimate_at_device):
        assert fn(h, *S.xyzn(q), 0.1, 3, None, E.ctypes.data, cnt.ctypes.data) == -1 and b"null normal" in L.s4p_normals_last_error(h)
        for k in range(3):
            args = S.xyzn(q)
            args[k] = None
            assert fn(h, *args, 0.1, 3, *out) == -1 and b"null query" in L.s4p_normals_last_error(h)
        for m in (-1, 2 ** 31 - 1, 2 ** 40):
            assert fn(h, *S.xyzn(q)[:3], m, 0.1, 3, *out) == -1 and b"m must be" in L.s4p_normals_last_error(h)
        assert fn(None, *S.xyzn(q), 0.1, 3, *out) == -1
        assert fn(h, None, None, None, 0, 0.1, 3, *out) == 0                        # m = 0: nothing to do, nothing touched
    assert (N == 7).all() and (E == 7).all() and (cnt == 7).all()
    # the limits themselves are allowed: the smallest and the largest radius with a normal, finite square
    assert (ctx.estimate(1.1e-19)[2] == 1).all() and (ctx.estimate(1.8e19)[2] == 100).all() and (ctx.estimate(0.1, 2 ** 31 - 1)[2] >= 1).all()
    ctx.close()


def test_the_facade_program_and_the_command_line_equal_the_python_path(shp, cpu, s4p_lib_built, tmp_path):
    from super4pcs_amd import capi
    delta, overlap, n_s, r = 0.01, 0.6, 200, 0.05
    P, Q, _ = H.small_pair(8000, delta=delta, seed=33)
    want = [cpu.estimate(Z, r, 5) for Z in (P, Q)]
    got = [shp.estimate_normals_radius(Z, r, 5) for Z in (P, Q)]
    assert SH.same(got[0], want[0]) and SH.same(got[1], want[1])
    none = [int((~w[0].any(1)).sum()) for w in want]
    print("neighbours median %d / %d, without a normal %d / %d" % (np.median(want[0][2]), np.median(want[1][2]), none[0], none[1]))
    assert np.median(want[0][2]) > 32
    # the facade: normals as Point3D::set_normal renormalises them, curvature in float
    exe = apps.build_app(tmp_path, "shape_app", S.NORMALS_LIBS, ["-Werror"])
    heads, _, rows = S.run_points_app(exe, ["shape", r, 5], P)
    assert heads == ["none %d" % none[0]] and rows.shape == (len(P), 4)
    rows = rows.astype(np.float32)
    assert np.array_equal(NH.bits(rows[:, :3]), NH.bits(NH.point3d_normalise(want[0][0])))
    assert np.array_equal(NH.bits(rows[:, 3]), NH.bits(shp.surface_variation(want[0][1])))
    heads, _, plain = S.run_points_app(exe, ["shape", r, 5, "plain"], P)
    assert heads == ["none %d" % none[0]] and np.array_equal(plain.astype(np.float32), rows[:, :3])
    # the command line: -a filters on the radius normals; the matrix and the registered cloud are the Python path's
    apps.write_obj(tmp_path / "P.obj", P); apps.write_obj(tmp_path / "Q.obj", Q)
    flags = ["-a", "20", "--estimate-normals-within", r, "--estimate-normals-min", "5"]
    M, out = apps.run_cli(S.cli(), tmp_path / "P.obj", tmp_path / "Q.obj", delta, overlap, n_s, flags + ["-r", tmp_path / "reg.obj"])
    Pn, Qn = NH.point3d_normalise(want[0][0]), NH.point3d_normalise(want[1][0])
    gm = capi.Matcher(capi.make_options(delta, overlap, n_s, max_normal_difference=20.0))
    _, Mp, gQ = gm.compute_transformation(P, Q, Pn, None, Qn, None)
    print("cli:\n%s\npython:\n%s" % (M, Mp))
    assert np.max(np.abs(M - np.asarray(Mp, np.float64))) <= 1e-5
    assert "Estimated normals within radius 0.05, min neighbours 5: %d points of input1 without a normal, %d of input2" % (none[0], none[1]) in out, out
    head, body = (tmp_path / "reg.ply").read_bytes().split(b"end_header\n", 1)
    assert b"element vertex %d\n" % len(Q) in head and np.array_equal(np.frombuffer(body, "<f4").reshape(-1, 3), gQ)
    # --orient-normals follows the new flag as it follows --estimate-normals; the two estimators together are a usage error
    M2, out2 = apps.run_cli(S.cli(), tmp_path / "P.obj", tmp_path / "Q.obj", delta, overlap, n_s, flags + ["--orient-normals", "8"])
    assert "Oriented normals: k 8" in out2 and np.isfinite(M2).all()
    bad = subprocess.run([S.cli(), "-i", str(tmp_path / "P.obj"), str(tmp_path / "Q.obj"), "--estimate-normals", "16"] + [str(f) for f in flags],
                         capture_output=True, text=True)
    assert bad.returncode == 1 and "Usage:" in bad.stderr
