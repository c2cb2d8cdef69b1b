"""Normal orientation on the MI355X (include/s4p_normals_orient.h): the flip mask, the component ids, the counts and every
output bit against the restatement (tests/orient_helpers.py: Kruskal and a tree walk) on tiny clouds (n from 1 to 257, with
duplicates and zero normals, k up to 32 > n - 1, both modes, with and without a radius), on lattices where every decision is a
tie-break, on two clusters and on the real clouds of the neighbour-list tests; one multi-trip size for determinism and the
outward property; the semantic result on the sphere and the bumpy cloud; the simple call; non-finite normals; the effect on
ICP's oriented normal-angle filter; refusals; the facade and the command line."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import apps
from tests import helpers as H
from tests import knn_helpers as KH
from tests import normals_helpers as NH
from tests import normals_suite as S
from tests import orient_helpers as OH

pytestmark = pytest.mark.gpu
VIEW = (0.3, -0.2, 2.0)


@pytest.fixture(scope="module")
def nrm():
    return S.normals_module("normals")


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return NH.build_cpu(tmp_path_factory.mktemp("orient_cpu"))


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 257])
@pytest.mark.parametrize("dup", [False, True])
def test_tiny_clouds_equal_the_restatement(nrm, n, dup):
    """k = 1 gives a forest of many small trees with many mutual picks; k = 32 exceeds n - 1; the radius isolates points."""
    X = KH.tiny_cloud(n, dup)
    N = OH.random_normals(n, 7 + n)
    ctx = nrm.Normals(0)
    ctx.set_cloud(X)
    many, alone = 0, 0
    for k in (1, 2, 8, 32):
        for r in (None, KH.tiny_radius(n)):
            idx, _, cnt = OH.numpy_lists(X, k, r, exclude_self=True)
            for vp in (None, VIEW):
                info = OH.same(ctx, X, N, idx, k, r, vp, (n, dup, k, r, vp))
                many += int(k == 1 and info["components"] > 4)
                alone += int(r is not None and (cnt == 0).any())
    assert n < 64 or (many >= 2 and alone >= 2)
    ctx.close()


@pytest.mark.parametrize("m", [16, 64])
def test_lattice_of_ties_equals_the_restatement_with_one_sign(nrm, cpu, m):
    X, N = OH.lattice(m)
    ctx = nrm.Normals(0)
    ctx.set_cloud(X)
    idx = OH.cpu_lists(cpu, X, 8, exclude_self=True)[0]
    info = OH.same(ctx, X, N, idx, 8, None, None, ("lattice", m))
    out = ctx.orient(N, 8)
    assert info["components"] == 1 and len(np.unique(out[:, 2])) == 1 and 0.3 < info["flipped_count"] / len(X) < 0.7
    print("lattice %d: rounds %d, max jumps %d" % (m, info["rounds"], info["max_jumps"]))
    ctx.close()


def test_two_clusters_are_anchored_separately(nrm):
    X, N, Cn = OH.two_clusters()
    ctx = nrm.Normals(0)
    ctx.set_cloud(X)
    idx = OH.numpy_lists(X, 8, exclude_self=True)[0]
    radial = X.astype(np.float64) - Cn
    for vp in (None, (0.0, 0.0, 0.0)):
        info = OH.same(ctx, X, N, idx, 8, None, vp, ("clusters", vp))
        assert info["components"] == 2
        out = ctx.orient(N, 8, viewpoint=vp).astype(np.float64)
        assert ((out * radial).sum(1) > 0).all()                 # a viewpoint between them makes both face it: both outward
    ctx.close()


def _real_clouds():
    from super4pcs_amd import datasets as D
    rng = np.random.default_rng(3)
    dup = D.bumpy_pair(6000, overlap=0.5, delta=0.004, seed=12)[0]
    dup = np.concatenate([dup, dup[rng.integers(0, len(dup), 2000)], dup[:500]]).astype(np.float32)
    return {"dup": dup, "lidar": D.lidar_pair_scaled(0.004, delta=0.05)[0]}


@pytest.mark.parametrize("name", ["dup", "lidar"])
def test_real_clouds_equal_the_restatement_bit_for_bit(nrm, cpu, name):
    X = _real_clouds()[name]
    assert len(X) == (8500 if name == "dup" else 20000)
    ctx = nrm.Normals(0)
    ctx.set_cloud(X)
    N = ctx.estimate(16)
    idx16 = OH.cpu_lists(cpu, X, 16, exclude_self=True)[0]
    for k, vp in ((8, None), (16, None), (8, VIEW)):
        info = OH.same(ctx, X, N, np.ascontiguousarray(idx16[:, :k]), k, None, vp, (name, k, vp))
        print("%s k %d: vertices %d components %d flipped %d rounds %d max jumps %d"
              % (name, k, info["vertices"], info["components"], info["flipped_count"], info["rounds"], info["max_jumps"]))
        assert info["rounds"] >= 2
    ctx.close()


def test_one_multi_trip_size_is_deterministic_and_outward(nrm):
    """524 289 points on a sphere: above 2048 x 256, a lane of every grid-stride kernel takes a second and a third trip.  Two
    calls, the host and the device form, numpy and torch give the same bits, and every normal ends pointing outward."""
    import torch
    from super4pcs_amd import datasets as D
    n = 524_289
    X = D.sphere_cloud(n, 3)
    assert len(X) == n > 2048 * 256
    ctx = nrm.Normals(0)
    ctx.set_cloud(X)
    N = ctx.estimate(16)
    a, info = ctx.orient(N, 8, return_info=True)
    b = ctx.orient(N, 8)
    t = ctx.orient(S.to_device(N), 8)
    assert t.is_cuda and np.array_equal(OH.bits(a), OH.bits(b)) and np.array_equal(OH.bits(a), OH.bits(S.to_host(t)))
    Xt = S.to_device(X)
    u = nrm.estimate_normals(Xt, k=16, orient="outward")
    assert u.is_cuda and np.array_equal(OH.bits(a), OH.bits(S.to_host(u)))
    assert info["vertices"] == n and info["components"] == 1 and info["rounds"] >= 2
    assert ((a.astype(np.float64) * X).sum(1) > 0).all()
    assert np.array_equal(np.abs(a), np.abs(N)) and np.array_equal(info["flipped"], (a != N).any(1))
    print("sphere %d: rounds %d, max jumps %d, flipped %d" % (n, info["rounds"], info["max_jumps"], info["flipped_count"]))
    ctx.close()


def test_sphere_and_bumpy_cloud_come_out_outward(nrm):
    """The feature itself: the estimates point out of the surface on about half (sphere) and two thirds (bumpy) of the points,
    and on all of them after orient; through the context, the one-shot function and estimate_normals(orient=)."""
    from super4pcs_amd import datasets as D
    for name, X in (("sphere", D.sphere_cloud(3000, 3)), ("bumpy", D.bumpy_pair(6000, noise_sigma=0.001, seed=12)[0])):
        N = nrm.estimate_normals(X, k=16)
        before = ((N * X).sum(1) > 0).mean()
        O = nrm.orient_normals(X, N, k=8)
        after = ((O * X).sum(1) > 0).mean()
        print("%s: outward %.4f -> %.4f" % (name, before, after))
        assert before < 0.7 and after == 1.0
        assert np.array_equal(OH.bits(nrm.estimate_normals(X, k=16, orient="outward")), OH.bits(O))
        assert np.array_equal(OH.bits(nrm.estimate_normals(X, k=16, orient=None)), OH.bits(N))      # the default is untouched
        V = nrm.orient_normals(X, N, k=8, viewpoint=(0, 0, 0))      # from inside a closed surface everything faces inward
        assert ((V * X).sum(1) < 0).all()
        W = nrm.estimate_normals(X, k=16, orient=(0, 0, 0))
        assert np.array_equal(OH.bits(W), OH.bits(V))


def test_orient_towards_equals_the_numpy_expression(nrm):
    rng = np.random.default_rng(6)
    X = np.concatenate([np.array([[1, 0, 0], [1, 0, 0], [1, 0, 0], [0, 2, 0], [0, 2, 0], [0, 0, 1]], np.float32),
                        rng.uniform(-1, 1, size=(3000, 3)).astype(np.float32)])
    N = np.concatenate([np.array([[0, 1, 0], [1, 0, 0], [-1, 0, 0], [0, 0, 0], [0, np.inf, 0], [0, np.nan, 1]], np.float32),
                        OH.random_normals(3000, 9)])
    ctx = nrm.Normals(0)
    ctx.set_cloud(X)
    for vp in ((0, 0, 0), VIEW, (5.0, 5.0, -7.0)):
        want, flip = OH.towards(X, N, vp)
        got = ctx.orient_towards(N, vp)
        assert np.array_equal(OH.bits(got), OH.bits(want)), vp
        assert 0.2 < flip.mean() < 0.8
        t = ctx.orient_towards(S.to_device(N), vp)
        assert t.is_cuda and np.array_equal(OH.bits(S.to_host(t)), OH.bits(want))
    want, flip = OH.towards(X, N, (0, 0, 0))
    assert flip[:6].tolist() == [False, True, False, False, False, False]      # n . g = 0, no normal, non-finite: untouched
    fl = np.full(len(X), 7, np.uint8)
    buf = N.copy()
    v = (C.c_float * 3)(0, 0, 0)
    assert nrm.load_orient().s4p_orient_towards(ctx.h, buf.ctypes.data, v, fl.ctypes.data) == 0
    assert np.array_equal(fl.astype(bool), flip) and np.array_equal(OH.bits(buf), OH.bits(want))
    ctx.close()


def test_non_finite_normals_count_as_zero_normals(nrm):
    """A normal with a NaN or an infinite component is no vertex: it keeps its bits, takes no part in the graph, and gets
    component -1, exactly as (0, 0, 0) does."""
    X = KH.tiny_cloud(257, False)
    N = OH.random_normals(257, 11)
    N[5] = (np.nan, 0, 1); N[40] = (0, np.inf, 0); N[41] = (-np.inf, np.nan, 0); N[200] = (0, -0.0, 0)
    Z = N.copy()
    Z[[5, 40, 41, 200]] = 0
    ctx = nrm.Normals(0)
    ctx.set_cloud(X)
    for k in (2, 8):
        idx = OH.numpy_lists(X, k, exclude_self=True)[0]
        info = OH.same(ctx, X, N, idx, k, None, None, ("nonfinite", k))
        assert (info["component"][[5, 40, 41, 200]] == -1).all() and not info["flipped"][[5, 40, 41, 200]].any()
        zi = ctx.orient(Z, k, return_info=True)[1]
        assert np.array_equal(zi["flipped"], info["flipped"]) and np.array_equal(zi["component"], info["component"])
    ctx.close()


def test_oriented_normals_make_the_oriented_pair_filter_usable(nrm):
    """bumpy_pair(6000, noise 0.001, seed 12) at the generator's pose, normal_angle = 60: with oriented normals of both
    clouds the oriented filter keeps exactly the pairs the unoriented one keeps; with the raw estimates it keeps strictly
    fewer (DESIGN.md section 26 records the counts)."""
    from super4pcs_amd import build as B, datasets as D
    B.build()
    B.build_icp()
    from super4pcs_amd import icp
    from tests import icp_helpers as IH
    P, Q, T = D.bumpy_pair(6000, noise_sigma=0.001, seed=12)
    d = 4 * 0.004
    Np, Nq = nrm.estimate_normals(P, k=16), nrm.estimate_normals(Q, k=16)
    Op, Oq = nrm.orient_normals(P, Np, k=8), nrm.orient_normals(Q, Nq, k=8)
    ctx = icp.ICP(0)
    ctx.set_target(P, d); ctx.set_source(Q)
    Tc = IH.to_centred(T, ctx.frame()).astype(np.float32)
    kept = {}
    for name, (a, b) in (("oriented", (Op, Oq)), ("raw", (Np, Nq))):
        ctx.set_target_normals(a); ctx.set_source_normals(b)
        for mode in (False, True):
            ctx.set_rejection(normal_angle=60, oriented=mode)
            kept[name, mode] = ctx.rejection(Tc)[2] == 0
    n = {key: int(v.sum()) for key, v in kept.items()}
    print("kept pairs at 60 degrees:", n)
    assert n["oriented", False] == n["raw", False] > 1000                # a sign does not matter to the unoriented filter
    assert np.array_equal(kept["oriented", True], kept["oriented", False])
    assert n["raw", True] < n["raw", False]
    ctx.close()


def test_refusals(nrm):
    X = np.random.default_rng(1).uniform(size=(100, 3)).astype(np.float32)
    N = OH.random_normals(100, 2)
    ctx = nrm.Normals(0)
    L, h = nrm.load_orient(), ctx.h
    v = (C.c_float * 3)(0, 0, 0)
    buf = N.copy()
    for rc in (L.s4p_orient_consistent(h, 8, -1.0, 0, None, buf.ctypes.data, None, None, None), L.s4p_orient_towards(h, buf.ctypes.data, v, None),
               L.s4p_orient_consistent_device(h, 8, -1.0, 0, None, buf.ctypes.data, None, None, None),
               L.s4p_orient_towards_device(h, buf.ctypes.data, v, None)):
        assert rc == -7 and b"set_cloud first" in L.s4p_normals_last_error(h)                       # before set_cloud
    ctx.set_cloud(X)
    nan, inf = float("nan"), float("inf")
    bad = [lambda: ctx.orient(N, 0), lambda: ctx.orient(N, 33), lambda: ctx.orient(N, -1), lambda: ctx.orient(N, 8, radius=nan),
           lambda: ctx.orient(N, 8, radius=inf), lambda: ctx.orient(N, 8, viewpoint=(0, nan, 0)), lambda: ctx.orient(N, 8, viewpoint=(inf, 0, 0)),
           lambda: ctx.orient_towards(N, (0, 0, nan)), lambda: ctx.orient_towards(N, (-inf, 0, 0))]
    for i, call in enumerate(bad):
        with pytest.raises(nrm.NormalsError) as e:
            call()
        assert e.value.code == -1 and len(str(e.value)) > 40, i
    for rc in (L.s4p_orient_consistent(h, 8, -1.0, 0, None, None, None, None, None),                # null normals
               L.s4p_orient_consistent(h, 8, -1.0, 1, None, buf.ctypes.data, None, None, None),     # viewpoint mode without one
               L.s4p_orient_consistent(h, 8, -1.0, 2, v, buf.ctypes.data, None, None, None),        # no such mode
               L.s4p_orient_towards(h, None, v, None), L.s4p_orient_towards(h, buf.ctypes.data, None, None),
               L.s4p_orient_consistent_device(h, 8, -1.0, 0, None, None, None, None, None), L.s4p_orient_towards_device(h, None, v, None)):
        assert rc == -1 and len(L.s4p_normals_last_error(h)) > 20
    assert L.s4p_orient_consistent(None, 8, -1.0, 0, None, buf.ctypes.data, None, None, None) == -1
    assert np.array_equal(buf, N)
    # the optional outputs may be null, and the outward mode needs no viewpoint
    assert L.s4p_orient_consistent(h, 8, -1.0, 0, None, buf.ctypes.data, None, None, None) == 0
    assert np.array_equal(OH.bits(buf), OH.bits(ctx.orient(N, 8)))
    with pytest.raises(ValueError):
        ctx.orient(N[:50], 8)
    ctx.close()


def test_facade_and_command_line(nrm, s4p_lib_built, tmp_path):
    """The facade program's orient: OrientNormals on points whose normals went through Point3D::set_normal equals the Python
    result on the same normals (a flipped point is renormalised once more, the others are untouched).  The command line with
    --estimate-normals 16 --orient-normals 8 --icp 10 --icp-normal-angle 60 registers; the two `needs` rules are usage errors."""
    X = KH.tiny_cloud(257, True)
    N0 = OH.random_normals(257, 13)
    Nin = NH.point3d_normalise(N0)                                # what the app's points hold: set_normal renormalises
    exe = S.build_facade_app(tmp_path)
    for extra, vp in (([], None), (list(VIEW), VIEW)):
        heads, _, got = S.run_points_app(exe, ["orient", "8", "-1"] + extra, np.concatenate([X, N0], 1))
        got = got.astype(np.float32)
        O = nrm.orient_normals(X, Nin, k=8, viewpoint=vp)
        flip = (OH.bits(O) != OH.bits(Nin)).any(1)
        want = Nin.copy()
        want[flip] = NH.point3d_normalise(O)[flip]
        assert heads == ["flipped %d" % flip.sum()] and flip.sum() > 20 and np.array_equal(OH.bits(got), OH.bits(want)), vp
    delta, overlap, n_s = 0.01, 0.6, 200
    P, Q, _ = H.small_pair(8000, delta=delta, seed=33)
    apps.write_obj(tmp_path / "P.obj", P); apps.write_obj(tmp_path / "Q.obj", Q)
    cli = S.cli()
    M, out = apps.run_cli(cli, tmp_path / "P.obj", tmp_path / "Q.obj", delta, overlap, n_s,
                          ["--estimate-normals", "16", "--orient-normals", "8", "--icp", "10", "--icp-normal-angle", "60"])
    assert "Oriented normals: k 8, outward" in out and "ICP:" in out and np.isfinite(M).all() and abs(np.linalg.det(M[:3, :3]) - 1) < 1e-3
    base = [cli, "-i", str(tmp_path / "P.obj"), str(tmp_path / "Q.obj")]
    for bad in (["--orient-normals", "8"], ["--estimate-normals", "16", "--orient-viewpoint", "0,0,0"]):
        r = subprocess.run(base + bad, capture_output=True, text=True)
        assert r.returncode == 1 and "Usage:" in r.stderr, (bad, r.returncode)
