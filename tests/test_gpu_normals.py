"""Normal estimation on the MI355X (include/s4p_normals.h): bit-exact against the CPU restatement (tests/normals_cpu) for
k in {3, 8, 16, 32} with and without a radius on a bumpy cloud, a small lidar scene and a cloud with duplicated points, at
524 289 and 1.3 M points (k in {3, 16, 32}: grid-stride lanes take a second and third trip), and through
estimate_at; determinism and numpy / torch agreement; planes, spheres and the zero-normal cases; registration
parity of the -a filter with estimated normals; the command line's --estimate-normals."""
import os
import subprocess

import numpy as np
import pytest

from tests import apps
from tests import helpers as H
from tests import normals_helpers as NH
from tests import normals_suite as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
KS = (3, 8, 16, 32)


@pytest.fixture(scope="module")
def nrm():
    return S.normals_module("normals")


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return NH.build_cpu(tmp_path_factory.mktemp("normals_cpu"))


def _clouds():
    from super4pcs_amd import datasets as D
    bumpy = D.bumpy_pair(100_000, overlap=0.5, delta=0.004, seed=11)[0]
    lidar = D.lidar_pair_scaled(0.004, delta=0.05)[0]
    rng = np.random.default_rng(3)
    dup = D.bumpy_pair(6000, overlap=0.5, delta=0.004, seed=12)[0]
    dup = np.concatenate([dup, dup[rng.integers(0, len(dup), 2000)], dup[:500]]).astype(np.float32)
    return {"bumpy": bumpy, "lidar": lidar, "dup": dup}


@pytest.fixture(scope="module")
def clouds():
    return _clouds()


@pytest.fixture(scope="module")
def contexts(nrm, clouds):
    out = {}
    for name, X in clouds.items():
        ctx = nrm.Normals(0)
        ctx.set_cloud(X)
        out[name] = ctx
    yield out
    for ctx in out.values():
        ctx.close()


@pytest.mark.parametrize("name", ["bumpy", "lidar", "dup"])
def test_normals_equal_the_restatement_bit_for_bit(nrm, cpu, clouds, contexts, name):
    X = clouds[name]
    ctx = contexts[name]
    g = ctx.grid()
    rng = np.random.default_rng(7)
    sample = np.sort(rng.choice(len(X), size=min(len(X), 3000), replace=False))
    radius = np.float32(0.6 * g["spacing"])              # small enough that some points have fewer than k neighbours
    print("%s: n %d, grid %s" % (name, len(X), g))
    for k in KS:
        for r in (None, radius):
            G = ctx.estimate(k, r)
            C = cpu.normals(X, k, r, queries=X[sample], threads=16)
            diff = np.flatnonzero((NH.bits(G[sample]) != NH.bits(C)).any(1))
            assert len(diff) == 0, (name, k, r, diff[:5], G[sample][diff[:3]], C[diff[:3]])
            zero = ~C.any(1)
            assert zero.mean() < 0.5 and (r is not None or k > 3 or zero.mean() < 0.5)
    # the hybrid radius really bounds: with it, some points lose neighbours at k = 32
    _, cnt = cpu.knn(X, 32, radius, queries=X[sample[:500]], threads=16)
    assert cnt.min() < 32


@pytest.mark.parametrize("n", [524_289, 1_300_000])
def test_normals_at_multi_trip_sizes_equal_the_restatement_bit_for_bit(nrm, cpu, n):
    """Clouds above 2048 x 256 points, where a lane of every grid-stride kernel takes a second and a third trip: the first such
    size and 1.3 M.  The sample always holds the last 256 indices (the ragged last trip)."""
    from super4pcs_amd import datasets as D
    X = D.bumpy_pair(n, overlap=0.5, delta=0.004, seed=11)[0]
    assert len(X) == n > 2048 * 256
    ctx = nrm.Normals(0)
    ctx.set_cloud(X)
    g = ctx.grid()
    rng = np.random.default_rng(7)
    sample = np.unique(np.concatenate([rng.choice(n - 256, size=3000 - 256, replace=False), np.arange(n - 256, n)]))
    assert len(sample) == 3000
    radius = np.float32(0.6 * g["spacing"])
    print("bumpy %d: grid %s" % (n, g))
    for k in (3, 16, 32):
        for r in (None, radius):
            G = ctx.estimate(k, r)
            C = cpu.normals(X, k, r, queries=X[sample], threads=16)
            diff = np.flatnonzero((NH.bits(G[sample]) != NH.bits(C)).any(1))
            assert len(diff) == 0, (n, k, r, diff[:5], G[sample][diff[:3]], C[diff[:3]])
            zero = ~C.any(1)
            assert zero.mean() < 0.5
    ctx.close()


def test_estimate_at_equals_the_restatement(nrm, cpu, clouds, contexts):
    X = clouds["bumpy"]
    ctx = contexts["bumpy"]
    rng = np.random.default_rng(8)
    Q = np.concatenate([X[rng.integers(0, len(X), 2000)] + rng.normal(scale=0.003, size=(2000, 3)),
                        rng.uniform(-1.5, 1.5, size=(300, 3)),                  # many off the surface, some off the grid
                        np.array([[np.nan, 0, 0], [np.inf, 0, 0]])]).astype(np.float32)
    for k in (8, 32):
        for r in (None, np.float32(0.02)):
            G = ctx.estimate_at(Q, k, r)
            C = cpu.normals(X, k, r, queries=Q, threads=16)
            assert np.array_equal(NH.bits(G), NH.bits(C)), (k, r)
            assert not G[-2:].any()
    # queries that are the cloud's own points give estimate()'s answer
    idx = rng.integers(0, len(X), 1000)
    assert np.array_equal(NH.bits(ctx.estimate_at(X[idx], 16)), NH.bits(ctx.estimate(16)[idx]))


def test_two_calls_and_numpy_torch_agree(nrm, clouds, contexts):
    import torch
    X = clouds["lidar"]
    ctx = contexts["lidar"]
    a = ctx.estimate(16)
    assert np.array_equal(NH.bits(a), NH.bits(ctx.estimate(16)))
    Xt = S.to_device(X)
    t = nrm.estimate_normals(Xt, k=16)
    assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (len(X), 3)
    assert np.array_equal(NH.bits(S.to_host(t)), NH.bits(a))
    assert np.array_equal(NH.bits(nrm.estimate_normals(X, k=16)), NH.bits(a))
    Q = X[:777] + np.float32(0.01)
    qn = nrm.estimate_normals(X, k=8, radius=0.5, queries=Q)
    qt = nrm.estimate_normals(Xt, k=8, radius=0.5, queries=S.to_device(Q))
    assert np.array_equal(NH.bits(S.to_host(qt)), NH.bits(qn))


def test_plane_sphere_and_zero_normals(nrm):
    rng = np.random.default_rng(2)
    P = np.column_stack([rng.uniform(-1, 1, 20000), rng.uniform(-1, 1, 20000), np.full(20000, 0.25)]).astype(np.float32)
    N = nrm.estimate_normals(P, k=16)
    assert np.array_equal(N, np.tile(np.array([0, 0, 1], np.float32), (len(P), 1)))      # +e_z: the sign rule
    d = rng.normal(size=(200_000, 3))                    # dense enough that the kNN patch's curvature tilt stays < 1 deg
    S = (d / np.linalg.norm(d, axis=1, keepdims=True) * 2.0 + np.array([10.0, -5.0, 3.0])).astype(np.float32)
    N = nrm.estimate_normals(S, k=16).astype(np.float64)
    radial = S.astype(np.float64) - np.array([10.0, -5.0, 3.0])
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    ang = np.degrees(np.arccos(np.clip(np.abs((N * radial).sum(1)), 0, 1)))
    print("sphere: max angle %.4f deg" % ang.max())
    assert ang.max() < 1.0
    # fewer than 3 points, nothing within r, coincident neighbours
    assert not nrm.estimate_normals(np.array([[0, 0, 0], [1, 0, 0]], np.float32), k=3).any()
    far = np.array([[0, 0, 0], [0, 1, 0], [1, 0, 0], [5, 5, 5]], np.float32)
    assert not nrm.estimate_normals(far, k=3, radius=0.5).any()
    assert not nrm.estimate_normals(np.ones((10, 3), np.float32), k=8).any()
    assert np.array_equal(nrm.estimate_normals(far, k=3)[:3], np.tile(np.array([0, 0, 1], np.float32), (3, 1)))


def test_bad_arguments(nrm):
    X = np.random.default_rng(1).uniform(size=(100, 3)).astype(np.float32)
    for k in (2, 33):
        with pytest.raises(nrm.NormalsError) as e:
            nrm.estimate_normals(X, k=k)
        assert e.value.code == -1
    with pytest.raises(nrm.NormalsError) as e:
        nrm.estimate_normals(X, k=8, radius=float("nan"))
    assert e.value.code == -1
    Xn = X.copy(); Xn[5, 1] = np.nan
    with pytest.raises(nrm.NormalsError) as e:
        nrm.estimate_normals(Xn)
    assert e.value.code == -1
    ctx = nrm.Normals(0)
    with pytest.raises(nrm.NormalsError) as e:
        ctx.estimate(16)
    assert e.value.code == -7
    ctx.close()


def test_registration_parity_with_estimated_normals(nrm, oracle_mod, s4p_lib_built):
    """The H.small_pair case of test_attribute_filters_on_gpu_match_oracle with estimated normals instead of radial ones:
    the device matcher and the oracle see the same normals and agree on every count and on the result."""
    from super4pcs_amd import capi
    O = oracle_mod
    delta, overlap, n_s = 0.01, 0.6, 200
    P, Q, T_gt = H.small_pair(20000, delta=delta, seed=31)
    Pn = nrm.estimate_normals(P, k=16)
    Qn = nrm.estimate_normals(Q, k=16)
    assert Pn.any(1).all() and Qn.any(1).all()
    opts = dict(max_normal_difference=20.0)
    om = O.Matcher(O.make_options(delta, overlap, n_s, **opts))
    o_lcp, o_M, o_Q = om.compute_transformation(P, Q, Pn, None, Qn, None)
    gm = capi.Matcher(capi.make_options(delta, overlap, n_s, **opts))
    g_lcp, g_M, g_Q = gm.compute_transformation(P, Q, Pn, None, Qn, None)
    gi, os_ = gm.info(), om.stats()
    assert gi.pairs_total == os_.n_pairs and gi.quads_total == os_.n_quads and gi.candidates_verified == os_.n_verified
    assert g_lcp == o_lcp and np.array_equal(g_M, o_M)
    gm0 = capi.Matcher(capi.make_options(delta, overlap, n_s))
    gm0.compute_transformation(P, Q)
    print("pairs %d (unfiltered %d), quads %d (%d), candidates %d (%d), lcp %.4f (%.4f)"
          % (gi.pairs_total, gm0.info().pairs_total, gi.quads_total, gm0.info().quads_total, gi.candidates_verified,
             gm0.info().candidates_verified, g_lcp, gm0.info().best_lcp))
    assert gi.pairs_total < gm0.info().pairs_total



def test_cli_estimate_normals_matches_the_python_path(nrm, s4p_lib_built, tmp_path):
    from super4pcs_amd import build as B, capi
    delta, overlap, n_s = 0.01, 0.6, 200
    P, Q, _ = H.small_pair(8000, delta=delta, seed=33)
    apps.write_obj(tmp_path / "P.obj", P); apps.write_obj(tmp_path / "Q.obj", Q)
    Pr = np.loadtxt(tmp_path / "P.obj", comments="#", usecols=(1, 2, 3), dtype=np.float32)      # the file's float values
    Qr = np.loadtxt(tmp_path / "Q.obj", comments="#", usecols=(1, 2, 3), dtype=np.float32)
    assert np.array_equal(Pr, P) and np.array_equal(Qr, Q)
    cli = B.build_cli()
    common = [cli, "-i", str(tmp_path / "P.obj"), str(tmp_path / "Q.obj"), "-o", str(overlap), "-d", str(delta), "-n", str(n_s),
              "-t", "1000", "-a", "20"]
    r = subprocess.run(common + ["--estimate-normals", "16", "-m", str(tmp_path / "mat.txt"), "-r", str(tmp_path / "reg.obj")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.array([[float(v) for v in ln.split()] for ln in (tmp_path / "mat.txt").read_text().splitlines()[2:6]])
    # the Python path: the same normals, renormalised as Point3D::set_normal does, into the device matcher
    Pn = NH.point3d_normalise(nrm.estimate_normals(P, k=16))
    Qn = NH.point3d_normalise(nrm.estimate_normals(Q, k=16))
    gm = capi.Matcher(capi.make_options(delta, overlap, n_s, max_normal_difference=20.0))
    _, M, gQ = gm.compute_transformation(P, Q, Pn, None, Qn, None)
    print("cli:\n%s\npython:\n%s" % (got, M))
    assert np.max(np.abs(got - np.asarray(M, np.float64))) <= 1e-5
    # -r: Q moved by that transform, without normals (the file had none): the bytes the path without the flag writes
    head, body = (tmp_path / "reg.ply").read_bytes().split(b"end_header\n", 1)
    assert b"property float nx" not in head
    assert np.array_equal(np.frombuffer(body, "<f4").reshape(-1, 3), gQ)
    # without the flag, -a has no normals to filter on: the run differs (and is the one it was before this feature)
    r0 = subprocess.run(common + ["-m", str(tmp_path / "mat0.txt"), "-r", str(tmp_path / "reg0.obj")], capture_output=True, text=True,
                        timeout=300)
    assert r0.returncode == 0, r0.stderr
